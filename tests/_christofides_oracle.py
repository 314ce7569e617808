"""Christofides construction restated in numpy + Python loops.  TEST INFRASTRUCTURE ONLY.

A literal restatement of the reference's prim_mst + odd_degree_nodes + greedy_matching + build_multigraph + hierholzer + shortcut
(src/tsp/christofides.rs:12-241) on positions, with the orders this project pins:
  * Prim takes the FIRST minimum in position order (Iterator::min_by), -0.0 equal to +0.0 (partial_cmp), and lowers a key only
    where d < key strictly;
  * the matching sorts by partial_cmp of the length, stably: equal lengths (and -0.0 / +0.0) go in (i, j) ascending order;
  * a NaN length between two odd vertices — the reference's comparator is inconsistent there, its order unspecified — is ONE value
    after +inf, ties by (i, j);
  * a vertex other than 0 that joins the tree without a parent raises NotSpanning (the reference's result is then not a tour).
Distances are the pinned oracle's bits (_oracle.dm_build_packed for EUC_2D, or the packed matrix of a GEO / EXPLICIT problem), the
cost is _oracle.tour_length of the route.

The switches prim="last", tie="ji", zero="total_cmp" and euler="all" are the deliberately wrong variants that
tests/test_christofides_oracle.py uses to show that each pinned rule decides a tour.
"""
import numpy as np

import _oracle as O
from _greedy_oracle import packed_of, route_sha256, total_keys  # noqa: F401

F32_MAX = np.float32(3.4028234663852886e38)
NAN_KEY = np.uint32(0xFF800001)  # just after +inf's key (0xFF800000)


class NotSpanning(ValueError):
    def __init__(self, position):
        super().__init__(f"no distance below f32::MAX reaches position {position}")
        self.position = position


def row(packed, n, u):
    """d(u, v) for every v from the packed strict lower triangle (row j holds d(j, 0..j-1)); +0.0 at v == u."""
    d = np.zeros(n, dtype=np.float32)
    if u > 0:
        d[:u] = packed[u * (u - 1) // 2: u * (u - 1) // 2 + u]
    v = np.arange(u + 1, n, dtype=np.int64)
    d[u + 1:] = packed[v * (v - 1) // 2 + u]
    return d


def canon_zero(d):
    d = np.asarray(d, dtype=np.float32)
    return np.where(d == 0, np.float32(0.0), d).astype(np.float32)


def prim(packed, n, prim="first", zero="partial_cmp"):
    """prim_mst (christofides.rs:75-114): returns (parent[n] with -1 = none, order[n] = the vertex that joined in round r)."""
    in_tree = np.zeros(n, dtype=bool)
    key = np.full(n, F32_MAX, dtype=np.float32)
    key[0] = np.float32(0.0)
    parent = np.full(n, -1, dtype=np.int64)
    order = np.empty(n, dtype=np.int64)
    for r in range(n):
        if zero == "partial_cmp":
            k = np.where(in_tree, np.float32(np.inf), key)   # -0.0 == +0.0 under numpy's comparison as under partial_cmp
        else:
            k = np.where(in_tree, np.uint32(0xFFFFFFFF), total_keys(key))
        u = int(np.argmin(k)) if prim == "first" else n - 1 - int(np.argmin(k[::-1]))
        in_tree[u] = True
        order[r] = u
        if r > 0 and parent[u] < 0:
            raise NotSpanning(u)
        d = row(packed, n, u)
        with np.errstate(invalid="ignore"):
            upd = ~in_tree & (d < key)                       # a NaN distance never lowers a key
        key[upd] = d[upd]
        parent[upd] = u
    return parent, order


def odd_vertices(parent, n):
    deg = np.zeros(n, dtype=np.int64)
    child = np.nonzero(parent >= 0)[0]
    np.add.at(deg, child, 1)
    np.add.at(deg, parent[child], 1)
    return np.nonzero(deg & 1)[0]


def matching_key32(d, zero="partial_cmp"):
    d = np.asarray(d, dtype=np.float32)
    k = total_keys(canon_zero(d) if zero == "partial_cmp" else d)
    return np.where(d != d, NAN_KEY, k).astype(np.uint32)


def sorted_pair_keys(packed, odd, tie="ij", zero="partial_cmp"):
    """Every pair i < j of odd vertices as one u64 key (matching_key32 of d) << 32 | i << 16 | j, ascending."""
    odd = np.asarray(odd, dtype=np.int64)
    chunks = []
    for b in range(1, len(odd)):
        j = int(odd[b])
        i = odd[:b]
        d = packed[j * (j - 1) // 2 + i]
        low = (i.astype(np.uint64) << np.uint64(16)) | np.uint64(j)
        if tie != "ij":
            low = np.uint64(0xFFFFFFFF) - low
        chunks.append((matching_key32(d, zero).astype(np.uint64) << np.uint64(32)) | low)
    keys = np.sort(np.concatenate(chunks)) if chunks else np.empty(0, dtype=np.uint64)
    if tie != "ij":
        keys = (keys & ~np.uint64(0xFFFFFFFF)) | (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF)))
    return keys


def greedy_matching(n, keys, target, chunk=4096):
    """christofides.rs:156-165 over the sorted keys: a pair is taken iff both ends are unmatched.  Every chunk is first filtered
    in bulk against the state at its start (a matched vertex stays matched).  Returns (pairs in acceptance order, examined)."""
    matched = np.zeros(n, dtype=bool)
    pairs, examined = [], 0
    for s in range(0, len(keys), chunk):
        if len(pairs) == target:
            break
        kk = keys[s:s + chunk]
        us = ((kk >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64)
        vs = (kk & np.uint64(0xFFFF)).astype(np.int64)
        keep = np.nonzero(~matched[us] & ~matched[vs])[0]
        for t in keep.tolist():
            u, v = int(us[t]), int(vs[t])
            if matched[u] or matched[v]:
                continue
            matched[u] = matched[v] = True
            pairs.append((u, v))
            examined = s + t + 1
            if len(pairs) == target:
                break
    assert len(pairs) == target, f"greedy_matching placed {len(pairs)} of {target} pairs"
    return pairs, examined


def euler_shortcut(n, parent, order, pairs, euler="one"):
    """build_multigraph + hierholzer from 0 + shortcut (christofides.rs:172-241).  euler="all" removes every occurrence of v from
    adj[u] instead of the first one (the wrong variant)."""
    adj = [[] for _ in range(n)]
    for r in range(1, n):
        u = int(order[r])
        v = int(parent[u])
        adj[u].append(v)
        adj[v].append(u)
    for u, v in pairs:
        adj[u].append(v)
        adj[v].append(u)
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if adj[v]:
            u = adj[v].pop()
            a = adj[u]
            if euler == "one":
                if v in a:
                    pos = a.index(v)
                    a[pos] = a[-1]  # swap_remove
                    a.pop()
            else:
                adj[u] = [x for x in a if x != v]
            stack.append(u)
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    seen, route = [False] * n, []
    for v in circuit:
        if not seen[v]:
            seen[v] = True
            route.append(v)
    return route


def christofides(xy, packed=None, n=None, prim_rule="first", tie="ij", zero="partial_cmp", euler="one", with_stats=False, want_cost=True):
    """christofides::solve on positions: returns (route positions uint32, cost float32[, stats])."""
    n = len(xy) if n is None else n
    if n < 4:
        route = np.arange(n, dtype=np.uint32)
        cost = np.float32(0.0) if n < 2 else O.tour_length(xy if packed is None else None, packed, route)
        return (route, cost, {"examined": 0, "k": 0, "pairs": [], "mst_edges": 0}) if with_stats else (route, cost)
    pk = packed_of(xy, packed)
    parent, order = prim(pk, n, prim_rule, zero)
    odd = odd_vertices(parent, n)
    assert len(odd) % 2 == 0
    keys = sorted_pair_keys(pk, odd, tie, zero)
    pairs, examined = greedy_matching(n, keys, len(odd) // 2)
    route = np.asarray(euler_shortcut(n, parent, order, pairs, euler), dtype=np.uint32)
    cost = None
    if want_cost and len(route) == n:
        cost = O.tour_length(xy if packed is None else None, packed, route)
    st = {"examined": examined, "k": len(odd), "pairs": pairs, "mst_edges": int((parent >= 0).sum()), "parent": parent, "order": order}
    return (route, cost, st) if with_stats else (route, cost)
