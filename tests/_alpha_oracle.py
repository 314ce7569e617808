"""Alpha-nearness as this project specifies it in numpy: the statement of record.

  table()       alpha(i, j) and w(i, j) of every pair under penalties pi, with the 1-tree they come from
  candidates()  every figure tl_alpha_candidates reports: the rows, their alphas, the tree's parents and the root's neighbours

The 1-tree is _one_tree_oracle.one_tree's (§4.29).  For i != j, both != root: beta(i, j) is the largest w on the tree path between
i and j and alpha(i, j) = w(i, j) - beta(i, j).  For the root r with its neighbours a (chosen first) and b: alpha(r, a) = alpha(r, b)
= 0, else alpha(r, j) = w(r, j) - w(r, b); alpha(j, r) = alpha(r, j).  beta is a maximum and therefore exact; alpha is one f64
subtraction per pair.  Row i: the min(k, n - 1) positions j != i smallest by (alpha, w, j), the doubles compared as numbers.

beta is filled in a topological order of the tree (a position after its parent): a new position v with parent p takes
beta(v, u) = max(beta(p, u), w(v, p)) against every position u already placed.
"""
import numpy as np

import _one_tree_oracle as H

NONE = H.NONE


def ordered(x):
    """one_tree_ordered on an array: -0.0 is +0.0, then the total-order bits as uint64."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).copy()
    b[b == np.uint64(0x8000000000000000)] = np.uint64(0)
    neg = (b >> np.uint64(63)) == np.uint64(1)
    return np.where(neg, ~b, b | np.uint64(0x8000000000000000))


def weights(row, n, pi):
    W = np.empty((n, n))
    for i in range(n):
        W[i] = row(i).astype(np.float64) + (pi[i] + pi)
    return W


def topological(par, root, n):
    """The positions other than the root, every one after its parent: by depth, position order within a depth."""
    depth = np.full(n, -1, dtype=np.int64)
    for v in range(n):
        if v == root:
            continue
        chain, u = [], v
        while depth[u] < 0 and par[u] != NONE:
            chain.append(u)
            u = int(par[u])
        if depth[u] < 0:
            depth[u] = 0  # Prim's start
        for t in reversed(chain):
            depth[t] = depth[int(par[t])] + 1
    order = [v for v in np.argsort(depth, kind="stable") if v != root]
    return order, depth


def table(xy=None, packed=None, n=None, pi=None, root=0):
    """(alpha n x n, w n x n, parents, (a, b)); the diagonals mean nothing.  n >= 3."""
    if n is None:
        n = len(xy)
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    row = H.rows_of(xy, packed, n)
    _, _, par, nb = H.one_tree(row, n, pi, root)
    W = weights(row, n, pi)
    order, _ = topological(par, root, n)
    beta = np.full((n, n), -np.inf)
    placed = []
    for v in order:
        if par[v] != NONE:
            p = int(par[v])
            idx = np.asarray(placed, dtype=np.int64)
            b = np.maximum(beta[p, idx], W[v, p])
            beta[v, idx] = b
            beta[idx, v] = b
        placed.append(v)
    A = W - beta
    a, b = nb
    ar = W[root] - W[root, b]
    ar[a] = 0.0
    ar[b] = 0.0
    A[root, :] = ar
    A[:, root] = ar
    return A, W, par, nb


def candidates(xy=None, packed=None, n=None, pi=None, root=0, k=5):
    """dict: cand (n x k' uint32), alpha (n x k' f64), parent (n uint32), root_nb."""
    if n is None:
        n = len(xy)
    if n <= 2:
        kk = n - 1 if n else 0
        cand = np.array([[1], [0]], dtype=np.uint32) if n == 2 else np.zeros((n, kk), dtype=np.uint32)
        return dict(cand=cand, alpha=np.zeros((n, kk)), parent=np.full(n, NONE, dtype=np.uint32), root_nb=(NONE, NONE))
    kk = min(k, n - 1)
    A, W, par, nb = table(xy, packed, n, pi, root)
    cand = np.empty((n, kk), dtype=np.uint32)
    alpha = np.empty((n, kk))
    pos = np.arange(n)
    for i in range(n):
        oa, ow = ordered(A[i]), ordered(W[i])
        oa[i] = ow[i] = np.uint64(0xFFFFFFFFFFFFFFFF)  # i itself is no candidate (no real key is all ones: that is a NaN's)
        first = np.lexsort((pos, ow, oa))[:kk]
        cand[i] = first
        alpha[i] = A[i, first]
    return dict(cand=cand, alpha=alpha, parent=par.copy(), root_nb=(int(nb[0]), int(nb[1])))


def brute_table(xy=None, packed=None, n=None, pi=None, root=0):
    """The same table with beta by a walk along every tree path: the oracle's own check for small n."""
    if n is None:
        n = len(xy)
    pi = np.zeros(n) if pi is None else np.asarray(pi, dtype=np.float64)
    row = H.rows_of(xy, packed, n)
    _, _, par, nb = H.one_tree(row, n, pi, root)
    W = weights(row, n, pi)
    adj = [[] for _ in range(n)]
    for v in range(n):
        if v != root and par[v] != NONE:
            adj[v].append(int(par[v]))
            adj[int(par[v])].append(v)
    A = np.zeros((n, n))
    for i in range(n):
        if i == root:
            continue
        best = {i: -np.inf}
        todo = [i]
        while todo:
            u = todo.pop()
            for v in adj[u]:
                if v not in best:
                    best[v] = max(best[u], float(W[u, v]))
                    todo.append(v)
        for j, b in best.items():
            if j != i:
                A[i, j] = W[i, j] - b
    a, b = nb
    for j in range(n):
        if j != root:
            A[root, j] = A[j, root] = 0.0 if j in (a, b) else W[root, j] - W[root, b]
    return A, W, par, nb
