"""Savings construction restated in numpy + a Python loop.  TEST INFRASTRUCTURE ONLY.

A literal restatement of the reference's hub_position + sorted_edges_by_savings + savings::solve (src/tsp/savings.rs:34-163) on
top of _greedy_oracle's select_edges / cycle_to_path, with this project's two ordering rules:
  * equal savings go in (i, j) ascending order (the reference's sort_unstable_by leaves that order open);
  * a NaN saving of any sign or payload is ONE value that ranks below every number, after -inf (ties by (i, j)) — applied
    explicitly (`s != s`), never inherited from the platform's default NaN.
Key of the edge (i < j): (inverted total-order key of s) << 32 | i << 16 | j, ascending; s = (dh[i] + dh[j]) - d(i, j) in two f32
operations, dh[k] = d(hub, k), dh[hub] = +0.0.  Distances are the pinned oracle's bits (_oracle.dm_build_packed for EUC_2D, or the
packed matrix of a GEO / EXPLICIT problem); the hub always comes from the coordinates; the cost is _oracle.tour_length.
"""
import numpy as np

import _oracle as O
from _greedy_oracle import cycle_to_path, packed_of, route_sha256, select_edges, total_keys  # noqa: F401

NAN_KEY = np.uint32(0xFF800001)  # just after -inf's inverted key (0xFF800000)
F32_MAX = np.float32(3.4028234663852886e38)


def hub_position(xy):
    """savings.rs:94-117 in f32: sequential left-to-right sums, each divided by n as f32, d2 = dx*dx + dy*dy unfused, the first
    i with d2 < best_d2 from best = 0, best_d2 = f32::MAX (so NaN / inf coordinates give 0)."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    n = len(xy)
    if n == 0:
        return 0
    with np.errstate(all="ignore"):
        # cumsum is a sequential recurrence (no pairwise blocks); the leading +0.0 is the accumulator's start
        cx = np.cumsum(np.concatenate([np.zeros(1, np.float32), xy[:, 0]]), dtype=np.float32)[-1] / np.float32(n)
        cy = np.cumsum(np.concatenate([np.zeros(1, np.float32), xy[:, 1]]), dtype=np.float32)[-1] / np.float32(n)
        dx, dy = xy[:, 0] - cx, xy[:, 1] - cy
        d2 = dx * dx + dy * dy
        ok = d2 < F32_MAX
    if not ok.any():
        return 0
    return int(np.argmin(np.where(ok, d2, np.float32(np.inf))))  # the first occurrence of the minimum


def hub_distances(packed, n, hub):
    """dh[k] = d(hub, k) from the packed strict lower triangle; dh[hub] = +0.0 (distance_by_pos's diagonal rule)."""
    dh = np.zeros(n, dtype=np.float32)
    if hub > 0:
        dh[:hub] = packed[hub * (hub - 1) // 2: hub * (hub - 1) // 2 + hub]
    k = np.arange(hub + 1, n, dtype=np.int64)
    dh[hub + 1:] = packed[k * (k - 1) // 2 + hub]
    return dh


def savings_key32(s, nan_rule=True):
    """Descending f32::total_cmp of s as an ascending unsigned order, NaN (any sign, any payload) after -inf."""
    k = ~total_keys(s)
    if nan_rule:
        s = np.asarray(s, dtype=np.float32)
        k = np.where(s != s, NAN_KEY, k).astype(np.uint32)
    return k


def sorted_savings_keys(packed, n, hub, tie="ij", nan_rule=True, order="sum_first"):
    """Every edge i < j as one u64 key, ascending.  tie="ji", nan_rule=False and order="diff_first" (dh[i] + (dh[j] - d)) are
    the deliberately wrong variants the tests use to show that each rule matters."""
    assert n <= 65535
    m = n * (n - 1) // 2
    dh = hub_distances(packed, n, hub)
    keys = np.empty(m, dtype=np.uint64)
    off = 0
    with np.errstate(all="ignore"):
        for j in range(1, n):
            d = packed[off:off + j]
            s = (dh[:j] + dh[j]) - d if order == "sum_first" else dh[:j] + (dh[j] - d)
            i = np.arange(j, dtype=np.uint64)
            low = (i << np.uint64(16)) | np.uint64(j)
            if tie != "ij":
                low = np.uint64(0xFFFFFFFF) - low
            keys[off:off + j] = (savings_key32(s, nan_rule).astype(np.uint64) << np.uint64(32)) | low
            off += j
    keys.sort()
    if tie != "ij":
        keys = (keys & ~np.uint64(0xFFFFFFFF)) | (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF)))
    return keys


def savings(xy, packed=None, n=None, hub=None, tie="ij", chunk=0, with_stats=False, nan_rule=True, order="sum_first"):
    """savings::solve on positions: returns (route positions uint32, cost float32, hub[, stats]).  hub None: hub_position(xy)."""
    n = len(xy) if n is None else n
    if hub is None:
        hub = hub_position(np.asarray(xy, dtype=np.float32).reshape(-1, 2)[:n])
    if n <= 2:
        route = np.arange(n, dtype=np.uint32)
        cost = np.float32(0.0) if n < 2 else O.tour_length(xy if packed is None else None, packed, route)
        return (route, cost, hub, {"examined": 0}) if with_stats else (route, cost, hub)
    pk = packed_of(xy, packed)
    keys = sorted_savings_keys(pk, n, hub, tie, nan_rule, order)
    edges, examined = select_edges(n, keys, chunk)
    route = np.asarray(cycle_to_path(n, edges), dtype=np.uint32)
    cost = O.tour_length(xy if packed is None else None, packed, route)
    return (route, cost, hub, {"examined": examined, "edges": edges}) if with_stats else (route, cost, hub)
