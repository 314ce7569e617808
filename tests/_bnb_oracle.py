"""The branch and bound's contract (include/teeline_gpu.h) in numpy and plain Python:

  brute()    every (n - 1)! sequence from `start` for n <= 9: L as tl_tour_length sums it (the closing edge first, sequential f32),
             the restriction rule of n_nearest, the argmin of (L, p).  No bound, no prune: what the search must find.
  dfs()      the depth-first search with the specified prune, child order and counts: what tl_branch_and_bound_host does node for
             node (Python's float is the f64 of the C text).
"""
import itertools

import numpy as np

F32_MAX = np.finfo(np.float32).max


def dist_matrix(xy=None, packed=None, n=None):
    """D as the library builds it: fl(sqrt(fl(fl(dx dx) + fl(dy dy)))) or the packed strict lower triangle; +0.0 on the diagonal."""
    if packed is not None:
        packed = np.asarray(packed, dtype=np.float32)
        D = np.zeros((n, n), dtype=np.float32)
        for a in range(1, n):
            for b in range(a):
                D[a, b] = D[b, a] = packed[a * (a - 1) // 2 + b]
        return D
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    dx = xy[:, None, 0] - xy[None, :, 0]
    dy = xy[:, None, 1] - xy[None, :, 1]
    D = np.sqrt(dx * dx + dy * dy).astype(np.float32)  # float32 throughout: one rounding per operation
    np.fill_diagonal(D, 0.0)
    return D


def packed_of(D):
    n = len(D)
    return np.ascontiguousarray([D[a, b] for a in range(1, n) for b in range(a)], dtype=np.float32)


def tour_length(D, p):
    total = D[p[-1], p[0]]
    for a in range(len(p) - 1):
        total = np.float32(total + D[p[a], p[a + 1]])
    return np.float32(total)


def bits(v):
    return int(np.float32(v).view(np.uint32))


def nk_masks(D, K):
    """N_K(c): c itself and the K - 1 positions j != c with the least (D(c, j), j); every position where K does not restrict."""
    n = len(D)
    full = (1 << n) - 1
    if not 0 < K < n:
        return [full] * n
    out = []
    for c in range(n):
        order = sorted((bits(D[c, j]), j) for j in range(n) if j != c)
        m = 1 << c
        for _, j in order[:K - 1]:
            m |= 1 << j
        out.append(m)
    return out


def brute(D, start=0, K=0, init=None):
    """(route, L, improved): the contract's result by enumeration."""
    n = len(D)
    assert 2 <= n <= 9
    others = [c for c in range(n) if c != start]
    P = np.array([(start,) + q for q in itertools.permutations(others)], dtype=np.int64)  # lexicographic order
    NK = np.array(nk_masks(D, K), dtype=np.uint64)
    full = np.uint64((1 << n) - 1)
    ok = np.ones(len(P), dtype=bool)
    visited = np.full(len(P), np.uint64(1 << start), dtype=np.uint64)
    for k in range(1, n):
        r = NK[P[:, k - 1]] & (full & ~visited)
        bit = np.uint64(1) << P[:, k].astype(np.uint64)
        ok &= (r == 0) | ((r & bit) != 0)
        visited |= bit
    L = D[P[:, -1], P[:, 0]].astype(np.float32)
    for a in range(n - 1):
        L = (L + D[P[:, a], P[:, a + 1]]).astype(np.float32)
    L = np.where(ok, L, np.float32(np.inf))
    best = int(np.argmin(L))  # the first minimum: the lexicographically least among equal lengths
    route, length = [int(v) for v in P[best]], np.float32(L[best])
    if init is not None:
        ub0 = tour_length(D, list(init))
        if not length < ub0:
            return [int(v) for v in init], ub0, 0
    return route, length, 1


def dfs(D, start=0, K=0, init=None):
    """(route, L, improved, nodes, leaves) of the sequential search with the specified prune."""
    n = len(D)
    full = (1 << n) - 1
    NK = nk_masks(D, K)
    factor = 1.0 + (n + 1) * 2.0 ** -23
    Db = [[bits(D[a, b]) for b in range(n)] for a in range(n)]
    Df = [[float(D[a, b]) for b in range(n)] for a in range(n)]
    ub0 = bits(tour_length(D, list(init))) if init is not None else None
    state = {"ub": ub0 if init is not None else bits(F32_MAX), "best": None, "nodes": 0, "leaves": 0}

    def prim(unv):
        key = {v: Db[start][v] for v in range(n) if unv >> v & 1}
        total = 0.0
        while key:
            u = min(key, key=lambda v: (key[v], v))
            total += float(np.uint32(key.pop(u)).view(np.float32))
            for v in key:
                if Db[u][v] < key[v]:
                    key[v] = Db[u][v]
        return total

    path = [start]

    def node(V, cost):
        state["nodes"] += 1
        unv = full & ~V
        mst = prim(unv)
        cand = NK[path[-1]] & unv or unv
        prev = path[-1]
        for _, c in sorted((Db[prev][c], c) for c in range(n) if cand >> c & 1):
            nc = cost + Df[prev][c]
            if nc + mst > float(np.uint32(state["ub"]).view(np.float32)) * factor:
                break
            path.append(c)
            if len(path) == n:
                state["leaves"] += 1
                Lb = bits(tour_length(D, path))
                if Lb <= state["ub"]:
                    state["ub"] = Lb
                    if (ub0 is None or Lb < ub0) and (state["best"] is None or (Lb, path) < state["best"]):
                        state["best"] = (Lb, list(path))
            else:
                node(V | 1 << c, nc)
            path.pop()

    node(1 << start, 0.0)
    if state["best"] is None:
        return [int(v) for v in init], tour_length(D, list(init)), 0, state["nodes"], state["leaves"]
    Lb, route = state["best"]
    return route, np.uint32(Lb).view(np.float32), 1, state["nodes"], state["leaves"]
