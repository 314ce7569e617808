"""Lin-Kernighan on supplied candidate lists (-m gpu): tl_lk_candidates, then tl_lk / tl_lk_trace / tl_lk_population against the oracle's
lin_kernighan(cand=rows, n_nearest=k), where rows are the supplied lists put into ascending f32 distance by a STABLE numpy sort on the
oracle's dist — alpha chooses the set, distance orders it.  Tour, cost bits and counters.

The reference's lk_pass can cycle and the oracle does not return from such a pass: every oracle run listed here
was computed on the CPU under a time limit before it went in; all of them returned."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _alpha_oracle as A
import _lk_population_cases as P
import _oracle as O
import _tsplib as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TL_ERR_BADARG = -1


@functools.lru_cache(maxsize=None)
def points(name):
    if name in ("berlin52", "a280"):
        return T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))["xy"]
    if name == "synth1002":
        return O.synth_xy(1002, seed=9)
    if name == "lattice10":
        return P.lattice(10, 2)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def lists(name, kind, k):
    """The rows as they are SUPPLIED.  alpha: tests/_alpha_oracle.py's under zero penalties, in (alpha, w, position) order — not in
    distance order; skip2: each city's 3rd .. (k + 2)th nearest, a set the kd-tree's k nearest never is; reversed: the kd-tree's own
    set, farthest first."""
    xy = points(name)
    if kind == "alpha":
        rows = A.candidates(xy, None, len(xy), None, 0, k)["cand"]
    elif kind == "skip2":
        rows = O.build_candidates(xy, k + 2)[:, 2:]
    elif kind == "reversed":
        rows = O.build_candidates_kdtree(xy, k)[0][:, ::-1]
    else:
        raise KeyError(kind)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    rows.setflags(write=False)
    return rows


def by_distance(xy, rows):
    """Every row in ascending oracle dist, stably: equal distances keep the supplied order."""
    out = np.empty_like(rows)
    for i in range(len(rows)):
        d = np.array([O.dist(xy[i, 0], xy[i, 1], xy[j, 0], xy[j, 1]) for j in rows[i]], dtype=np.float32)
        out[i] = rows[i][np.argsort(d, kind="stable")]
    return out


@functools.lru_cache(maxsize=None)
def want(name, kind, k, seed, epochs, init_seed=None):
    xy = points(name)
    rows = by_distance(xy, lists(name, kind, k))
    init = None if init_seed is None else O.restart_perm(len(xy), init_seed, 0)
    rc, route, cost, st = O.lin_kernighan(xy, init=init, epochs=epochs, n_nearest=k, seed=seed, cand=rows)
    assert rc == 0
    return rc, route, cost, st


def prob(xy):
    import teeline_amd as TA
    return TA.TspProblem(np.arange(len(xy)), xy)


def gpu_lk(ctx, xy, rows, seed, epochs, init=None, n_nearest=5):
    import teeline_amd as TA
    h = TA.HeuristicOptions(epochs=epochs, platoo_epochs=10, n_nearest=n_nearest)
    sol = TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, 5), None, None if init is None else [int(v) for v in init], ctx=ctx, seed=seed,
                                 candidates=rows)
    return np.asarray(sol.route(), dtype=np.uint32), sol.total, sol.stats


def assert_same(g, o, what=""):
    route, cost, st = g
    rc, oroute, ocost, ost = o
    assert rc == 0 and route.tolist() == oroute.tolist(), f"{what}: tour differs from the oracle"
    assert np.float32(cost).tobytes() == np.float32(ocost).tobytes(), what
    assert (st["sweeps"], st["candidates"], st["moves"], st["reversed"]) == (ost["sweeps"], ost["candidates"], ost["moves"], ost["reversed"]), what


# (instance, lists, k, seed, epochs): n <= 700 takes the LDS form by default
SMALL = [("berlin52", "alpha", 5, 1, 100), ("berlin52", "alpha", 1, 2, 100), ("berlin52", "alpha", 8, 3, 100), ("berlin52", "skip2", 5, 1, 100),
         ("a280", "alpha", 5, 7, 30), ("a280", "skip2", 8, 7, 30), ("a280", "alpha", 1, 7, 30), ("lattice10", "alpha", 5, 11, 40),
         ("lattice10", "reversed", 5, 11, 40)]


@pytest.mark.parametrize("name,kind,k,seed,epochs", SMALL)
def test_default_form(ctx, name, kind, k, seed, epochs):
    xy = points(name)
    # n_nearest is ignored while lists are set: 3 here, the lists are k wide
    assert_same(gpu_lk(ctx, xy, lists(name, kind, k), seed, epochs, n_nearest=3), want(name, kind, k, seed, epochs), f"{name} {kind} k={k}")


def test_the_supplied_order_is_not_the_searched_order():
    """The alpha rows are NOT ascending in distance, and the lattice's rows hold equal distances: the cases above pin the stable reorder."""
    xy = points("berlin52")
    rows = lists("berlin52", "alpha", 5)
    assert (by_distance(xy, rows) != rows).any()
    lat, lrows = points("lattice10"), lists("lattice10", "alpha", 5)
    d = np.sqrt(((lat[:, None, :] - lat[lrows]) ** 2).sum(-1))
    assert (np.sort(d, axis=1)[:, 1:] == np.sort(d, axis=1)[:, :-1]).any()
    assert (lists("berlin52", "skip2", 5) != O.build_candidates_kdtree(xy, 5)[0]).any()


@pytest.mark.parametrize("flag", ["TL_FLAG_LK_NO_SPECULATION", "TL_FLAG_LK_CHIP_WIDE", "TL_FLAG_LK_ONE_WORKGROUP"])
def test_the_other_forms(flag):
    import teeline_amd as TA
    with TA.Context(0, getattr(TA, flag)) as c:
        for name, kind, k, seed, epochs in (("berlin52", "alpha", 5, 1, 100), ("berlin52", "skip2", 5, 1, 100), ("a280", "alpha", 5, 7, 30),
                                            ("lattice10", "alpha", 5, 11, 40), ("berlin52", "alpha", 1, 2, 100), ("berlin52", "alpha", 8, 3, 100)):
            assert_same(gpu_lk(c, points(name), lists(name, kind, k), seed, epochs), want(name, kind, k, seed, epochs), f"{flag} {name} {kind} k={k}")


@pytest.mark.parametrize("kind,k", [("alpha", 5), ("skip2", 8)])
def test_chip_wide_by_default_at_1002(ctx, kind, k):
    xy = points("synth1002")
    assert_same(gpu_lk(ctx, xy, lists("synth1002", kind, k), 3, 6), want("synth1002", kind, k, 3, 6), f"synth1002 {kind}")


def test_a_start_tour_and_the_untouched_nn_seed(ctx):
    xy = points("a280")
    init = O.restart_perm(len(xy), 5, 0)
    assert_same(gpu_lk(ctx, xy, lists("a280", "alpha", 5), 2, 5, init=init), want("a280", "alpha", 5, 2, 5, init_seed=5), "a280 from a random start")


def raw_trace(ctx, xy, seed, epochs, k=5, cap=64):
    from teeline_amd import _capi
    n = len(xy)
    out, snaps, dists = np.empty(n, dtype=np.uint32), np.zeros((cap, n), dtype=np.uint32), np.zeros(cap, dtype=np.float32)
    c, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
    o = _capi.TlLkOpts(epochs, 10, k, 5)
    ctx.check(ctx.lib.tl_lk_trace(ctx.handle, xy.ctypes.data_as(C.c_void_p), n, None, None, C.byref(o), seed, out.ctypes.data_as(C.c_void_p), C.byref(c),
                                  C.byref(st), snaps.ctypes.data_as(C.c_void_p), dists.ctypes.data_as(C.c_void_p), cap, C.byref(ln)))
    return out, np.float32(c.value), st.as_dict(), snaps[:min(ln.value, cap)], dists[:min(ln.value, cap)], ln.value


def test_trace_snapshots(ctx):
    """tl_lk_trace on the kd-tree's own lists, supplied: the oracle's messages.  The oracle's trace entry (tlo_lin_kernighan_trace)
    takes no candidate lists, and oracle/ stays as it is, so on alpha lists there is no message list to compare with: there the
    oracle's result (tour, cost, counters), every snapshot a tour, their distances descending, the last one the returned tour."""
    xy = points("berlin52")
    rc, oroute, ocost, ost, osnaps = O.lin_kernighan_trace(xy, epochs=60, seed=1)
    try:
        ctx.lk_candidates(O.build_candidates_kdtree(xy, 5)[0])
        out, cost, st, snaps, dists, ln = raw_trace(ctx, xy, 1, 60)
        assert ln == len(osnaps) and out.tolist() == oroute.tolist()
        for m, (spos, sdist) in enumerate(osnaps):
            assert snaps[m].tolist() == spos.tolist() and dists[m].tobytes() == np.float32(sdist).tobytes()
        ctx.lk_candidates(lists("berlin52", "alpha", 5))
        out, cost, st, snaps, dists, ln = raw_trace(ctx, xy, 1, 100)
        assert_same((out, cost, st), want("berlin52", "alpha", 5, 1, 100), "trace on alpha lists")
        assert ln == len(snaps) >= 1 and snaps[-1].tolist() == out.tolist() and (np.diff(dists) < 0).all()
        assert all(sorted(s.tolist()) == list(range(len(xy))) for s in snaps)
    finally:
        ctx.lk_candidates(None)


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("name,kind,k,epochs", [("berlin52", "alpha", 5, 30), ("berlin52", "skip2", 8, 30), ("a280", "alpha", 5, 10), ("berlin52", "alpha", 1, 30)])
def test_population_of_three(form, name, kind, k, epochs):
    import teeline_amd as TA
    xy = points(name)
    rows = lists(name, kind, k)
    srows = by_distance(xy, rows)
    with TA.Context(0) as c:
        c.lk_population_setting(form, 0)
        h = TA.HeuristicOptions(epochs=epochs, platoo_epochs=10, n_nearest=3)
        sols, best = TA.lin_kernighan.solve_population(prob(xy), TA.LKOptions(h, 5), None, seed=4, runs=3, ctx=c, candidates=rows)
        for r, s in enumerate(sols):
            o = O.lin_kernighan(xy, epochs=epochs, n_nearest=k, seed=P.run_seed(4, r), cand=srows)
            assert_same((np.asarray(s.route(), dtype=np.uint32), s.total, s.stats), o, f"{name} {kind} form {form} run {r}")
        assert best == min(range(3), key=lambda i: (np.float32(sols[i].total), i))


def test_the_kd_trees_own_lists_change_nothing_and_clearing_restores(tsplib_dir):
    import teeline_amd as TA
    xy = points("berlin52")
    h = TA.HeuristicOptions(epochs=100, platoo_epochs=10, n_nearest=5)
    with TA.Context(0) as c:
        solve = lambda **kw: TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, 5), None, None, ctx=c, seed=2, **kw)  # noqa: E731
        key = lambda s: (list(s.route()), np.float32(s.total).tobytes(), s.stats["sweeps"], s.stats["candidates"], s.stats["moves"], s.stats["reversed"])  # noqa: E731
        plain = key(solve())
        own = TA.lin_kernighan.build_candidates(prob(xy), 5, ctx=c)
        assert key(solve(candidates=own)) == plain
        c.lk_candidates(lists("berlin52", "skip2", 5))
        other = key(solve())
        assert other != plain and other[0] == want("berlin52", "skip2", 5, 2, 100)[1].tolist()
        c.lk_candidates(None)
        assert key(solve()) == plain
        # the width the population's LDS form is sized by follows the lists
        wide = c.lk_population_max_n(None)
        c.lk_candidates(lists("berlin52", "alpha", 1))
        assert c.lk_population_max_n(None) > wide
        c.lk_candidates(None)
        assert c.lk_population_max_n(None) == wide


def test_a_context_without_the_setting_is_as_before(tsplib_dir):
    """What the suite pins for tl_lk without lists (the kd-tree's lists through the oracle; berlin52's published optimum with the CLI's
    options) on a fresh context that never had the setting."""
    import teeline_amd as TA
    xy = points("berlin52")
    with TA.Context(0) as c:
        for seed in (1, 4):
            h = TA.HeuristicOptions(epochs=100, platoo_epochs=10, n_nearest=5)
            s = TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, 5), None, None, ctx=c, seed=seed)
            assert_same((np.asarray(s.route(), dtype=np.uint32), s.total, s.stats), O.lin_kernighan(xy, seed=seed), f"seed {seed}")
        h = TA.HeuristicOptions(epochs=10000, platoo_epochs=500, n_nearest=3)
        s = TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, 5), None, None, ctx=c, seed=1)
        assert f"{float(np.float32(s.total)):.5f}" == "7544.36572"


def test_errors(ctx):
    err = lambda: ctx.lib.tl_last_error(ctx.handle)  # noqa: E731
    setting = lambda rows, n, k: ctx.lib.tl_lk_candidates(ctx.handle, None if rows is None else rows.ctypes.data_as(C.c_void_p), n, k)  # noqa: E731
    xy = points("berlin52")
    n = len(xy)
    good = np.array(lists("berlin52", "alpha", 5))
    try:
        for row, col, value, word in ((7, 2, 7, b"own position"), (9, 4, int(good[9, 0]), b"twice"), (51, 0, n, b"no position"), (0, 3, 0xFFFFFFFF, b"no position")):
            bad = good.copy()
            bad[row, col] = value
            assert setting(bad, n, 5) == TL_ERR_BADARG and word in err() and f"row {row} ".encode() in err(), err()
        wide = np.ascontiguousarray(np.tile(np.arange(1, 66, dtype=np.uint32), (100, 1)))
        assert setting(wide, 100, 65) == TL_ERR_BADARG and b"64" in err()
        assert setting(good, 5, 5) == TL_ERR_BADARG and b"n - 1" in err()
        # a refused setting leaves the context without lists
        h_plain = gpu_lk(ctx, xy, None, 1, 20)
        assert setting(good, n, 5) == 0
        other = points("a280")
        out = np.empty(len(other), dtype=np.uint32)
        from teeline_amd import _capi
        o = _capi.TlLkOpts(5, 5, 5, 5)
        rc = ctx.lib.tl_lk(ctx.handle, other.ctypes.data_as(C.c_void_p), len(other), None, None, C.byref(o), 1, out.ctypes.data_as(C.c_void_p), None, None)
        assert rc == TL_ERR_BADARG and b"tl_lk_candidates" in err() and b"n=52" in err()
        cost = np.empty(2, dtype=np.float32)
        outs = np.empty((2, len(other)), dtype=np.uint32)
        rc = ctx.lib.tl_lk_population(ctx.handle, other.ctypes.data_as(C.c_void_p), len(other), None, None, 0, 0, 2, C.byref(o), 1, outs.ctypes.data_as(C.c_void_p),
                                      cost.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == TL_ERR_BADARG and b"tl_lk_candidates" in err()
        assert setting(None, 0, 0) == 0 and setting(good, n, 0) == 0  # NULL or k = 0 clears
        assert gpu_lk(ctx, xy, None, 1, 20)[0].tolist() == h_plain[0].tolist()
    finally:
        ctx.lk_candidates(None)
