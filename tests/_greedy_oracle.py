"""Greedy-edge construction restated in numpy + a Python loop.  TEST INFRASTRUCTURE ONLY.

A literal restatement of the reference's sorted_edges + select_edges + hamiltonian_cycle_to_path (src/tsp/graph.rs:54-196)
and greedy_edge::solve (src/tsp/greedy_edge.rs:21-65), with this project's tie rule: equal lengths in (i, j) ascending order
(the reference's sort_unstable_by leaves that order open).  Distances are the pinned oracle's bits (_oracle.dm_build_packed for
EUC_2D, or the packed matrix of a GEO / EXPLICIT problem), the cost is _oracle.tour_length of the path.
"""
import numpy as np

import _oracle as O


def total_keys(d):
    """f32::total_cmp as an unsigned order: flip every bit of a negative pattern, set the sign bit of a positive one."""
    b = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def sorted_edge_keys(packed, n, tie="ij"):
    """Every edge i < j as one u64 key (total-order key of d) << 32 | i << 16 | j, ascending.  packed: the strict lower
    triangle, row j holding d(j, 0..j-1).  tie="ji" reverses the order among equal lengths (for the tie-rule test only)."""
    assert n <= 65535
    m = n * (n - 1) // 2
    keys = np.empty(m, dtype=np.uint64)
    k32 = total_keys(packed[:m]).astype(np.uint64) << np.uint64(32)
    off = 0
    for j in range(1, n):
        i = np.arange(j, dtype=np.uint64)
        if tie == "ij":
            low = (i << np.uint64(16)) | np.uint64(j)
        else:  # reversed (i, j) order among ties
            low = np.uint64(0xFFFFFFFF) - ((i << np.uint64(16)) | np.uint64(j))
        keys[off:off + j] = k32[off:off + j] | low
        off += j
    keys.sort()
    if tie != "ij":
        low = np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))
        keys = (keys & ~np.uint64(0xFFFFFFFF)) | low
    return keys


def _ij(keys):
    return ((keys >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64), (keys & np.uint64(0xFFFF)).astype(np.int64)


class _UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, a):
        p = self.parent
        while p[a] != a:
            p[a] = p[p[a]]
            a = p[a]
        return a

    def union(self, a, b):
        self.parent[self.find(a)] = self.find(b)


def select_edges(n, keys, chunk=0):
    """graph.rs:98-126 over the sorted keys.  Returns (accepted [(u, v)] in acceptance order, edges examined).
    chunk > 0: the same walk, but every chunk of keys is first filtered in bulk against the degrees at the chunk's start
    (rejections are final: degrees never fall); tests/test_greedy_edge_oracle.py shows it equal to the literal walk."""
    uf, degree, accepted = _UnionFind(n), [0] * n, []
    examined = 0

    def walk(us, vs, first):
        nonlocal examined
        for t, (u, v) in enumerate(zip(us, vs)):
            if len(accepted) == n:
                return True
            if degree[u] >= 2 or degree[v] >= 2:
                continue
            if uf.find(u) == uf.find(v) and len(accepted) != n - 1:
                continue
            uf.union(u, v)
            degree[u] += 1
            degree[v] += 1
            accepted.append((u, v))
            if len(accepted) == n:
                examined = first[t] + 1
                return True
        return False

    if chunk <= 0:
        us, vs = _ij(keys)
        walk(us.tolist(), vs.tolist(), list(range(len(keys))))
    else:
        deg = np.zeros(n, dtype=np.int8)
        for s in range(0, len(keys), chunk):
            us, vs = _ij(keys[s:s + chunk])
            deg[:] = degree
            keep = np.nonzero((deg[us] < 2) & (deg[vs] < 2))[0]
            if walk(us[keep].tolist(), vs[keep].tolist(), (keep + s).tolist()):
                break
    assert len(accepted) == n, f"select_edges placed {len(accepted)} of {n} edges"
    return accepted, examined


def cycle_to_path(n, edges):
    """hamiltonian_cycle_to_path (graph.rs:140-196): from position 0, first along adj[0][0], then never back."""
    adj = [[] for _ in range(n)]
    for u, v in edges:
        adj[u].append(v)
        adj[v].append(u)
    assert all(len(a) == 2 for a in adj)
    path, seen, prev, cur = [], [False] * n, -1, 0
    for _ in range(n):
        assert not seen[cur]
        seen[cur] = True
        path.append(cur)
        nxt = next(x for x in adj[cur] if x != prev)
        prev, cur = cur, nxt
    return path


def packed_of(xy, packed=None):
    return O.dm_build_packed(xy) if packed is None else np.ascontiguousarray(packed, dtype=np.float32)


def greedy_edge(xy, packed=None, n=None, tie="ij", chunk=0, with_stats=False):
    """greedy_edge::solve on positions: returns (route positions uint32, cost float32[, stats])."""
    n = len(xy) if n is None else n
    if n <= 2:
        route = np.arange(n, dtype=np.uint32)
        cost = np.float32(0.0) if n < 2 else O.tour_length(xy if packed is None else None, packed, route)
        return (route, cost, {"examined": 0}) if with_stats else (route, cost)
    pk = packed_of(xy, packed)
    keys = sorted_edge_keys(pk, n, tie)
    edges, examined = select_edges(n, keys, chunk)
    route = np.asarray(cycle_to_path(n, edges), dtype=np.uint32)
    cost = O.tour_length(xy if packed is None else None, packed, route)
    return (route, cost, {"examined": examined, "edges": edges}) if with_stats else (route, cost)


def route_sha256(route):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(route, dtype=np.uint32).tobytes()).hexdigest()
