"""The instances of the alpha-nearness tests, the call into the C ABI and the bit-for-bit comparison with tests/_alpha_oracle.py."""
import ctypes as C
import functools

import numpy as np

import _alpha_oracle as A
import _one_tree_cases as K
import _one_tree_oracle as H
import _oracle as O
import _tsplib as T

TL_ERR_BADARG, TL_ERR_UNSUPPORTED, TL_ERR_BUSY = K.TL_ERR_BADARG, K.TL_ERR_UNSUPPORTED, -8
NONE = A.NONE


def collinear(n):
    """A path: the tree's depth is n - 2 from Prim's start."""
    return np.array([[3.0 * i, 7.0] for i in range(n)], dtype=np.float32)


def star(ring):
    """One centre and a far ring whose points are further from each other than from the centre: every tree edge is a spoke."""
    assert ring <= 5
    pts = [[0.0, 0.0]] + [[1000.0 * np.cos(2 * np.pi * q / ring), 1000.0 * np.sin(2 * np.pi * q / ring)] for q in range(ring)]
    return np.array(pts, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def ascent_pi(name, iterations=20):
    xy, pk, n = instance(name)[:3]
    return H.ascent(xy, pk, n, upper=K.nn_upper(xy, pk, n), iterations=iterations)["pi"]


@functools.lru_cache(maxsize=None)
def instance(name):
    """(xy, packed, n)."""
    kind, _, arg = name.partition(":")
    if kind == "rand":
        return K.random_xy(int(arg), 1), None, int(arg)
    if kind == "line":
        return collinear(int(arg)), None, int(arg)
    if kind == "star":
        return star(int(arg)), None, int(arg) + 1
    if kind == "twins":
        return K.duplicated(int(arg), 3), None, int(arg)
    if kind == "grid":
        c, r = (int(v) for v in arg.split("x"))
        return K.unit_grid(c, r), None, c * r
    if kind == "synth":
        return O.synth_xy(int(arg), seed=9), None, int(arg)
    if kind == "ulysses22":  # GEO: the packed matrix of the library's own rule
        e = T.parse_tsplib(K.HERE + "/golden/tsplib/ulysses22.tsp")
        return None, O.dm_build_packed(e["xy"], geo=True), e["n"]
    return K.tsp(kind)


# name, root, pi ("zero" or "ascent"), k
CASES = [
    ("rand:3", 0, "zero", 5), ("rand:3", 2, "zero", 1), ("rand:4", 1, "zero", 5), ("rand:5", 0, "zero", 4), ("rand:8", 3, "zero", 5),
    ("line:65", 0, "zero", 5), ("line:65", 64, "zero", 5), ("line:65", 30, "zero", 64),
    ("star:5", 0, "zero", 5), ("star:5", 3, "zero", 2),                          # the root interior (the centre), the root a leaf
    ("rand:20", 0, "zero", 1), ("rand:20", 19, "zero", 5), ("rand:20", 7, "zero", 19), ("rand:20", 7, "zero", 40),  # k = 1, 5, n - 1, clipped
    ("twins:12", 0, "zero", 5), ("twins:12", 5, "zero", 11),
    ("grid:5x4", 0, "zero", 5), ("grid:5x4", 19, "zero", 8),
    ("rand:30", 0, "ascent", 5), ("rand:30", 29, "ascent", 7),
    ("ulysses22", 0, "zero", 5), ("ulysses22", 0, "ascent", 5), ("ring6_explicit", 0, "zero", 5), ("ring6_explicit", 4, "zero", 3),
]


def pi_of(name, kind):
    return None if kind == "zero" else ascent_pi(name)


@functools.lru_cache(maxsize=None)
def want(name, root, pi_kind, k):
    xy, pk, n = instance(name)
    return A.candidates(xy, pk, n, pi_of(name, pi_kind), root, k)


def call(ctx, xy, packed, n, pi, root, k, threads=0, outputs=True):
    """tl_alpha_candidates (ctx given) or tl_alpha_candidates_host (ctx None): (rc, dict like the oracle's, TlStats or None)."""
    from teeline_amd import _capi
    lib = _capi.load()
    if xy is not None:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    if packed is not None:
        packed = np.ascontiguousarray(packed, dtype=np.float32)
    if pi is not None:
        pi = np.ascontiguousarray(pi, dtype=np.float64)
    kk = max(min(k, 64, max(n - 1, 0)), 1)
    cand = np.full((max(n, 1), kk), 0xABABABAB, dtype=np.uint32)
    alpha = np.full((max(n, 1), kk), np.nan)
    par = np.full(max(n, 1), 0xABABABAB, dtype=np.uint32)
    nb = np.full(2, 0xABABABAB, dtype=np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    st = None
    if ctx is None:
        rc = lib.tl_alpha_candidates_host(p(xy), p(packed), n, p(pi), root, k, p(cand), p(alpha) if outputs else None, p(par) if outputs else None,
                                          p(nb) if outputs else None)
    else:
        st = _capi.TlStats()
        rc = lib.tl_alpha_candidates(ctx.handle, p(xy), p(packed), n, p(pi), root, k, threads, p(cand), p(alpha) if outputs else None,
                                     p(par) if outputs else None, p(nb) if outputs else None, C.byref(st))
    kk = min(k, max(n - 1, 0))
    return rc, dict(cand=cand[:n, :kk], alpha=alpha[:n, :kk], parent=par[:n], root_nb=(int(nb[0]), int(nb[1]))), st


def assert_same(got, want_, what=""):
    """Rows, alphas, parents and root neighbours, bit for bit."""
    assert got["cand"].shape == want_["cand"].shape, (what, got["cand"].shape, want_["cand"].shape)
    assert np.array_equal(got["parent"], want_["parent"]), (what, "parents")
    assert tuple(got["root_nb"]) == tuple(want_["root_nb"]), (what, "root neighbours", got["root_nb"], want_["root_nb"])
    bad = np.nonzero((got["cand"] != want_["cand"]).any(axis=1))[0]
    assert bad.size == 0, (what, "row", int(bad[0]), got["cand"][bad[0]].tolist(), want_["cand"][bad[0]].tolist())
    ga, wa = np.ascontiguousarray(got["alpha"]).view(np.uint64), np.ascontiguousarray(want_["alpha"]).view(np.uint64)
    bad = np.nonzero((ga != wa).any(axis=1))[0]
    assert bad.size == 0, (what, "alphas of row", int(bad[0]), got["alpha"][bad[0]].tolist(), want_["alpha"][bad[0]].tolist())


def assert_properties(res, n, root, what=""):
    """alpha >= +0.0 (never -0.0); tree edges and both root edges have alpha +0.0 wherever they are output; alpha(i, j) and alpha(j, i)
    are equal bitwise wherever both are output."""
    cand, alpha, par, nb = res["cand"], res["alpha"], res["parent"], res["root_nb"]
    bits = np.ascontiguousarray(alpha).view(np.uint64)
    assert (bits >> np.uint64(63) == 0).all() and not np.isnan(alpha).any(), (what, "a negative alpha, a -0.0 or a NaN")
    seen = {}
    for i in range(n):
        for q, j in enumerate(cand[i]):
            seen[(i, int(j))] = int(bits[i, q])
    for (i, j), b in seen.items():
        if (j, i) in seen:
            assert seen[(j, i)] == b, (what, "alpha is not symmetric", i, j)
    tree = {(v, int(par[v])) for v in range(n) if par[v] != NONE} | {(root, int(nb[0])), (root, int(nb[1]))} if n > 2 else set()
    for u, v in tree:
        for e in ((u, v), (v, u)):
            if e in seen:
                assert seen[e] == 0, (what, "a tree edge's alpha is not +0.0", e)
    if n > 2:
        for i in range(n):  # every tree neighbour has alpha 0 and alpha >= 0: a row of k >= degree holds them all before any positive alpha
            assert (np.diff(alpha[i]) >= 0).all(), (what, "a row is not ascending in alpha", i)
