"""The instances of the Held-Karp bound's tests, the call into the C ABI and the bit-for-bit comparison with the oracle."""
import ctypes as C
import os

import numpy as np

import _one_tree_oracle as H
import _tsplib as T

HERE = os.path.dirname(os.path.abspath(__file__))
TL_ERR_BADARG, TL_ERR_UNSUPPORTED = -1, -6
LDS_BYTES = 160 * 1024  # what an MI355X workgroup may take


def tsp(name):
    e = T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))
    pk = None if e["packed"] is None else np.ascontiguousarray(e["packed"], dtype=np.float32)
    return (None if pk is not None else e["xy"]), pk, e["n"]


def opt_tour_positions(name):
    e = T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))
    pos = {int(v): p for p, v in enumerate(e["ids"])}
    return [pos[i] for i in T.parse_opt_tour(os.path.join(HERE, "golden", "tsplib", f"{name}.opt.tour"))]


def random_xy(n, seed):
    """Uniform integer coordinates in [0, 1000)^2."""
    return np.random.default_rng(7000 * n + seed).integers(0, 1000, size=(n, 2)).astype(np.float32)


def unit_grid(cols, rows):
    """Many equal distances: the position rule decides."""
    return np.array([[c, r] for r in range(rows) for c in range(cols)], dtype=np.float32)


def duplicated(n, seed):
    """Every city twice (d = 0 between the twins), interleaved."""
    xy = random_xy((n + 1) // 2, seed)
    return np.concatenate([xy, xy])[np.random.default_rng(seed).permutation(2 * len(xy))][:n].copy()


def random_matrix(n, seed):
    """A symmetric matrix that is no metric: the packed triangle of uniform f32 weights."""
    return np.random.default_rng(900 + seed).uniform(1.0, 100.0, size=n * (n - 1) // 2).astype(np.float32)


def nn_upper(xy, packed, n):
    """An upper bound without a solver: the nearest-neighbour tour's f64 length from position 0 (ties: the lowest position)."""
    row = H.rows_of(xy, packed, n)
    seen, cur, total = np.zeros(n, dtype=bool), 0, 0.0
    seen[0] = True
    for _ in range(n - 1):
        d = np.where(seen, np.inf, row(cur).astype(np.float64))
        nxt = int(np.argmin(d))
        total += float(d[nxt])
        seen[nxt] = True
        cur = nxt
    return total + float(row(cur)[0])


def call(ctx, xy, packed, n, *, upper, root=0, iterations=1000, lambda0=2.0, patience=10, iters_per_launch=0, log_cap=None, reserved=0):
    """tl_one_tree_bound (ctx given) or tl_one_tree_bound_host (ctx None): (rc, dict like the oracle's)."""
    return call_batch(ctx, xy, packed, n, [dict(upper=upper, root=root, iterations=iterations, lambda0=lambda0, patience=patience,
                                                iters_per_launch=iters_per_launch, reserved=reserved)], log_cap=log_cap, single=True)


def call_batch(ctx, xy, packed, n, sets, *, log_cap=None, single=False):
    """tl_one_tree_bound_batch: (rc, [dict per job], best_index); single: the one-job entries, (rc, dict)."""
    from teeline_amd import _capi
    lib = _capi.load()
    if xy is not None:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    if packed is not None:
        packed = np.ascontiguousarray(packed, dtype=np.float32)
    J = len(sets)
    if log_cap is None:
        log_cap = max(int(s.get("iterations", 1000)) for s in sets)
    arr = (_capi.TlOneTreeOpts * J)(*[_capi.TlOneTreeOpts(int(s.get("root", 0)), int(s.get("iterations", 1000)), int(s.get("patience", 10)),
                                                          int(s.get("iters_per_launch", 0)), float(s.get("lambda0", 2.0)), float(s["upper"]),
                                                          int(s.get("reserved", 0))) for s in sets])
    res = (_capi.TlOneTreeResult * J)()
    m = max(n, 1)
    pi, par, tour = np.full((J, m), np.nan), np.full((J, m), 0xABABABAB, dtype=np.uint32), np.full((J, m), 0xABABABAB, dtype=np.uint32)
    log = np.full((J, max(log_cap, 1), 3), np.nan)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    best = C.c_uint32(0xFFFFFFFF)
    if ctx is None:
        assert single
        rc = lib.tl_one_tree_bound_host(p(xy), p(packed), n, arr, res, p(pi), p(par), p(tour), p(log), log_cap)
    elif single:
        rc = lib.tl_one_tree_bound(ctx.handle, p(xy), p(packed), n, arr, res, p(pi), p(par), p(tour), p(log), log_cap, None)
    else:
        rc = lib.tl_one_tree_bound_batch(ctx.handle, p(xy), p(packed), n, arr, J, res, p(pi), p(par), p(tour), p(log), log_cap, C.byref(best), None)
    out = []
    for j in range(J):
        r = res[j].as_dict()
        r["pi"], r["parent"] = pi[j, :n].copy(), par[j, :n].copy()
        r["tour"] = [int(v) for v in tour[j, :n]] if r["is_tour"] else None
        r["log"] = [tuple(float(v) for v in log[j, k]) for k in range(min(r["iterations_run"], log_cap))]
        out.append(r)
    if single:
        return rc, out[0]
    return rc, out, int(best.value)


def bits(x):
    return np.float64(x).tobytes()


def assert_same(got, want, what=""):
    """Every figure the issue lists, bit for bit: bound, best_iter, iterations run, stop reason, is_tour and tour, pi, parents, every log row."""
    for k in ("best_iter", "iterations_run", "stop", "is_tour"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert bits(got["bound"]) == bits(want["bound"]), (what, got["bound"], want["bound"])
    assert bits(got["lam"]) == bits(want["lam"]), (what, "lambda", got["lam"], want["lam"])
    assert got["tour"] == want["tour"], (what, "tour")
    assert tuple(got["root_nb"]) == tuple(want["root_nb"]) and tuple(got["tour_nb"]) == tuple(want["tour_nb"]), (what, "root neighbours")
    assert np.asarray(got["pi"], dtype=np.float64).tobytes() == np.asarray(want["pi"], dtype=np.float64).tobytes(), (what, "pi")
    assert np.array_equal(np.asarray(got["parent"], dtype=np.uint32), np.asarray(want["parent"], dtype=np.uint32)), (what, "parents")
    assert len(got["log"]) == len(want["log"]), (what, "log rows")
    for k, (a, b) in enumerate(zip(got["log"], want["log"])):
        assert np.asarray(a).tobytes() == np.asarray(b, dtype=np.float64).tobytes(), (what, "log row", k, a, b)
