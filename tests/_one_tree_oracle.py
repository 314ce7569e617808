"""The Held-Karp lower bound's specification in numpy and plain Python: the statement of record.

  one_tree()  the minimum 1-tree under penalties pi with special position s: Prim over the other positions by prim_mst's rule (the
              smallest key, the first in position order among equals; a key is lowered only where w is strictly smaller), the
              root's two smallest edges (the lower position among equals), L and the degrees.
  ascent()    the subgradient ascent; every figure tl_one_tree_bound reports.

w(i, j) = (double)d(i, j) + (pi_i + pi_j) in f64 (numpy's float64 and Python's float are the f64 of the C text; every operation
here is one rounding, none is contracted).  Sums are sequential.
"""
import numpy as np

NONE = 0xFFFFFFFF
STOP_TOUR, STOP_LAMBDA, STOP_UPPER, STOP_ITERATIONS = 1, 2, 3, 4
LAMBDA_FLOOR = 2.0 ** -20


def rows_of(xy=None, packed=None, n=None):
    """row(u) -> d(u, .) as f32, the library's bits: fl(sqrt(fl(fl(dx dx) + fl(dy dy)))) or the packed strict lower triangle."""
    if packed is not None:
        packed = np.asarray(packed, dtype=np.float32)
        D = np.zeros((n, n), dtype=np.float32)
        il = np.tril_indices(n, -1)
        D[il] = packed  # row-major strict lower triangle: (1,0), (2,0), (2,1), ..
        D = D + D.T
        return lambda u: D[u]
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)

    def row(u):
        dx = xy[u, 0] - xy[:, 0]
        dy = xy[u, 1] - xy[:, 1]
        return np.sqrt(dx * dx + dy * dy)  # float32 throughout
    return row


def seq_sum(values):
    total = 0.0
    for x in values:
        total = total + x
    return total


def one_tree(row, n, pi, s):
    """(L, degrees, parents, (a, b)) of the minimum 1-tree under pi with special position s."""
    start = 1 if s == 0 else 0
    key = np.full(n, np.inf)
    key[start] = 0.0
    par = np.full(n, NONE, dtype=np.uint32)
    intree = np.zeros(n, dtype=bool)
    intree[s] = True
    deg = np.zeros(n, dtype=np.int64)
    total = 0.0
    for _ in range(n - 1):
        u = int(np.argmin(np.where(intree, np.inf, key)))  # the first minimum
        assert not intree[u]
        intree[u] = True
        total = total + float(key[u])
        if par[u] != NONE:
            deg[u] += 1
            deg[par[u]] += 1
        w = row(u).astype(np.float64) + (pi[u] + pi)
        lower = ~intree & (w < key)
        key[lower] = w[lower]
        par[lower] = u
    ws = row(s).astype(np.float64) + (pi[s] + pi)
    ws[s] = np.inf
    a = int(np.argmin(ws))
    total = total + float(ws[a])
    ws[a] = np.inf
    b = int(np.argmin(ws))
    total = total + float(ws[b])
    deg[a] += 1
    deg[b] += 1
    deg[s] = 2
    L = total - 2.0 * seq_sum(pi.tolist())
    return L, deg, par, (a, b)


def tour_of(par, nb, s, n):
    """The tour a 1-tree of degrees 2 is: from the root towards its first chosen neighbour."""
    adj = [[] for _ in range(n)]
    for v in range(n):
        if v != s and par[v] != NONE:
            adj[v].append(int(par[v]))
            adj[int(par[v])].append(v)
    tour, prev, cur = [s], None, nb[0]
    for _ in range(n - 1):
        tour.append(cur)
        nxt = [x for x in adj[cur] if x != prev]
        prev, cur = cur, (nxt[0] if nxt else None)
    return tour


def ascent(xy=None, packed=None, n=None, *, upper, root=0, iterations=1000, lambda0=2.0, patience=10):
    """dict: bound, best_iter, iterations_run, stop, is_tour, tour, pi, parent, root_nb, tour_nb, lam, log (rows L_k, sum g^2, lambda)."""
    if n is None:
        n = len(xy)
    row = rows_of(xy, packed, n)
    if n <= 2:
        bound = 0.0 if n <= 1 else 2.0 * float(row(0)[1])
        return dict(bound=bound, best_iter=0, iterations_run=0, stop=0, is_tour=1, tour=list(range(n)), pi=np.zeros(n),
                    parent=np.full(n, NONE, dtype=np.uint32), root_nb=(NONE, NONE), tour_nb=(NONE, NONE), lam=0.0, log=[])
    pi = np.zeros(n)
    lam, stall, best, best_iter = float(lambda0), 0, -np.inf, 0
    best_pi, best_par, best_nb, tour, tour_nb = pi.copy(), np.full(n, NONE, dtype=np.uint32), (NONE, NONE), None, (NONE, NONE)
    stop, is_tour, log, k = 0, 0, [], 0
    while stop == 0:
        L, deg, par, nb = one_tree(row, n, pi, root)
        g = deg - 2
        g2 = int((g * g).sum())
        if L > best:
            best, best_iter, stall = L, k, 0
            best_pi, best_par, best_nb = pi.copy(), par.copy(), nb
        else:
            stall += 1
            if stall == patience:
                lam = lam * 0.5
                stall = 0
        log.append((L, float(g2), lam))
        k += 1
        if g2 == 0:
            stop, is_tour, tour, tour_nb = STOP_TOUR, 1, tour_of(par, nb, root, n), nb
        elif lam < LAMBDA_FLOOR:
            stop = STOP_LAMBDA
        elif upper - L <= 0.0:
            stop = STOP_UPPER
        else:
            t = lam * (upper - L) / float(g2)
            pi = pi + t * g.astype(np.float64)
            if k == iterations:
                stop = STOP_ITERATIONS
    return dict(bound=best, best_iter=best_iter, iterations_run=k, stop=stop, is_tour=is_tour, tour=tour, pi=best_pi, parent=best_par,
                root_nb=best_nb, tour_nb=tour_nb, lam=lam, log=log)


def tour_length_f64(row, tour):
    """The tour's length as the exact-enough f64 sum of its f32 edges."""
    return seq_sum(float(row(tour[i])[tour[(i + 1) % len(tour)]]) for i in range(len(tour)))
