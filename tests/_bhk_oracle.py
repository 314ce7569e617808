"""Bellman-Held-Karp exact solver restated in numpy.  TEST INFRASTRUCTURE ONLY.

A restatement of the reference's bellman_karp::solve (src/tsp/bellman_karp.rs:24-165) on positions, layer by layer (all subsets
of one size at once) instead of the reference's memoised recursion.  k = n - 1, last = k; the table is mask-major, T[S][c]:
  * init (:39-47)   T = f32::MAX everywhere, T[1 << i][i] = d(i, last);
  * fill (:89-120)  for S with >= 2 bits and c in S, R = S & ~(1 << c): T[S][c] = the minimum over i in R, in ascending i, of
                    T[R][i] + d(i, c), started at f32::MAX and replaced under a strict `<` (a NaN term, or one that rounds to
                    MAX / inf, is never taken; the memo test of :98 only saves work);
  * optimum (:65-75) the f32::min fold from f32::MAX over i of T[full][i] + d(i, last), terms with both operands < f32::MAX only;
  * walk (:122-156) route[0] = last, left = optimal; per step the first j in `unread` with approx(left, T[unread][j] +
                    d(j, route[i - 1])), then left -= d(j, route[i - 1]); stops altogether once left <= 0.0; where no j
                    qualifies route[i] stays 0 — so the result need not be a tour;
  * approx (:158-165) |a - b| <= max(|a|, |b|, 1) * 1e-4, all in f32;
  * total (:86)     tour_length of the route as given (closing edge first, sequential f32, d(p, p) = 0), NOT `optimal`.
exact_walk() is this project's own second walk (TL_FLAG_BHK_EXACT_WALK, no counterpart in the reference): the first j in `unread`
with T[unread][j] + d(j, prev) == rem exactly, then rem = T[unread][j]; rem starts at `optimal`.  It cannot fail while
optimal < f32::MAX; otherwise the reference walk's result is returned unchanged.

All arithmetic is np.float32.  Distances are the pinned oracle's bits (_oracle.dm_build_packed for EUC_2D) or the packed matrix
of a GEO / EXPLICIT problem.
"""
import numpy as np

import _oracle as O

F32_MAX = np.float32(3.4028234663852886e38)
TOL = np.float32(1e-4)


def full_matrix(xy, packed, n):
    """d(p, q) for all positions as an n x n f32 array with a +0.0 diagonal (distance_by_pos, distance_matrix.rs:177-191)."""
    if n < 2:
        return np.zeros((n, n), dtype=np.float32)
    if packed is None:
        packed = O.dm_build_packed(np.ascontiguousarray(xy, dtype=np.float32)[:n])
    d = O.dm_expand_full(np.ascontiguousarray(packed, dtype=np.float32), n).astype(np.float32)
    d[np.arange(n), np.arange(n)] = np.float32(0.0)
    return d


def table(d, n):
    """Steps 1 and 2: T[2^k][k] (for k = 0 a single empty row)."""
    k = n - 1
    T = np.full((1 << k, max(k, 1)), F32_MAX, dtype=np.float32)
    for i in range(k):
        T[1 << i, i] = d[i, k]                                      # :44-46
    if k < 2:
        return T
    masks = np.arange(1 << k, dtype=np.int64)
    pop = np.zeros(1 << k, dtype=np.uint8)
    for b in range(k):
        pop += ((masks >> b) & 1).astype(np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(2, k + 1):
            layer = masks[pop == p]
            for c in range(k):
                S = layer[(layer >> c) & 1 == 1]
                R = S ^ (1 << c)
                best = np.full(len(S), F32_MAX, dtype=np.float32)   # :95
                for i in range(k):                                  # :104-116, ascending i
                    if i == c:
                        continue
                    sel = np.nonzero((R >> i) & 1)[0]
                    t = T[R[sel], i] + d[i, c]                      # f32 + f32
                    b = best[sel]
                    best[sel] = np.where(t < b, t, b)               # strict <: NaN, MAX and inf never replace
                T[S, c] = best                                      # :118
    return T


def optimum(T, d, n):
    """Step 3 (:65-75)."""
    k = n - 1
    full = (1 << k) - 1
    opt = F32_MAX
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            sub, ret = T[full, i], d[i, k]
            if sub < F32_MAX and ret < F32_MAX:
                t = np.float32(sub + ret)
                opt = t if t < opt else opt                         # f32::min of two non-NaN values
    return np.float32(opt)


def approx(a, b):
    """:158-165.  A NaN on either side makes diff NaN and the answer False, whatever f32::max does with it."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.abs(np.float32(a) - np.float32(b))
        scale = np.float32(max(np.float32(max(np.abs(np.float32(a)), np.abs(np.float32(b)))), np.float32(1.0)))
        if np.isnan(diff):
            return False
        return bool(diff <= np.float32(scale * TOL))


def tolerance_walk(T, d, n, optimal):
    """Step 4 (read_optimal_route, :122-156)."""
    k = n - 1
    route = np.zeros(n, dtype=np.int64)
    route[0] = k
    unread = (1 << k) - 1
    left = np.float32(optimal)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n):
            if left <= np.float32(0.0):                             # :129
                break
            prev = int(route[i - 1])
            for j in range(k):
                step = d[j, prev]
                cur = np.float32(T[unread, j] + step)
                if (unread >> j) & 1 and approx(left, cur):
                    left = np.float32(left - step)
                    route[i] = j
                    unread &= ~(1 << j)
                    break
    return route


def _exact_walk(T, d, n, optimal):
    k = n - 1
    route = np.zeros(n, dtype=np.int64)
    route[0] = k
    unread = (1 << k) - 1
    rem = np.float32(optimal)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n):
            prev = int(route[i - 1])
            for j in range(k):
                if not (unread >> j) & 1:
                    continue
                sub, step = T[unread, j], d[j, prev]
                if i == 1 and not (sub < F32_MAX and step < F32_MAX):   # the fold's own admission test
                    continue
                if np.float32(sub + step) == rem:
                    rem = np.float32(sub)
                    route[i] = j
                    unread &= ~(1 << j)
                    break
            else:
                raise AssertionError("exact walk: no successor reproduces the remaining optimum")
    return route


def tour_length(d, route):
    """distance_matrix.rs:235-245 on a route that need not be a permutation: the closing edge first, then sequential f32."""
    n = len(route)
    if n == 0:
        return np.float32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.float32(d[route[n - 1], route[0]])
        for a in range(n - 1):
            total = np.float32(total + d[route[a], route[a + 1]])
    return total


def is_tour(route):
    return int(sorted(int(v) for v in route) == list(range(len(route))))


def _solve(xy, packed, n, walk):
    if n is None:
        n = len(xy)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.float32(0.0), np.float32(0.0), 1
    d = full_matrix(xy, packed, n)
    T = table(d, n)
    optimal = optimum(T, d, n)
    if walk == "exact" and optimal < F32_MAX:
        route = _exact_walk(T, d, n, optimal)
    else:
        route = tolerance_walk(T, d, n, optimal)
    return route, tour_length(d, route), optimal, is_tour(route)


def bellman_karp(xy, packed=None, n=None):
    """(route positions, total, optimal, is_tour) as the reference returns them."""
    return _solve(xy, packed, n, "tolerance")


def exact_walk(xy, packed=None, n=None):
    """The same table and optimum, read back by the walk of TL_FLAG_BHK_EXACT_WALK."""
    return _solve(xy, packed, n, "exact")


def both(xy, packed=None, n=None):
    """Both walks over ONE table: ((route, total, optimal, is_tour) of the reference's walk, the same of the exact walk)."""
    if n is None:
        n = len(xy)
    if n == 0:
        z = (np.zeros(0, dtype=np.int64), np.float32(0.0), np.float32(0.0), 1)
        return z, z
    d = full_matrix(xy, packed, n)
    T = table(d, n)
    optimal = optimum(T, d, n)
    r = tolerance_walk(T, d, n, optimal)
    ref = (r, tour_length(d, r), optimal, is_tour(r))
    if not optimal < F32_MAX:
        return ref, ref
    x = _exact_walk(T, d, n, optimal)
    return ref, (x, tour_length(d, x), optimal, is_tour(x))


def campaign():
    """The issue's seeded campaign: 200 instances of 4..12 random points."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(4, 13))
        yield (rng.random((n, 2)) * 100).astype(np.float32)
