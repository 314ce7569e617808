"""Simulated annealing on the GPU (tl_sim_anneal*, csrc/sim_anneal.hip) against the numpy statement of its specification
(tests/_sa_oracle.py): the tour element for element, the cost bit for bit and the whole accept trace (epoch, from, to, cost), in both
input forms, both window forms and for the chains of a population."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from _raw_context import _vp, jitter_context
import _sa_cases as K
import _sa_oracle as SA
from _swarm_oracle import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_opts(o):
    from teeline_amd import _capi
    return _capi.TlSaOpts(o["epochs"], o["cooling_rate"], o["min_temperature"], o["max_temperature"])


def gpu_trace(ctx, xy, packed, n, init, opts, seed, chain=0, cap=None):
    from teeline_amd import _capi
    cap = cap if cap is not None else len(SA.schedule(**opts)) + 1
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.zeros((max(cap, 1), 4), dtype=np.uint32)
    cost, ln, st, o = C.c_float(-1.0), C.c_uint32(), _capi.TlStats(), c_opts(opts)
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_sim_anneal_trace_chain(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), C.byref(o), seed, chain, _vp(out), C.byref(cost), C.byref(st),
                                           _vp(log), cap, C.byref(ln))
    return rc, out[:n], np.float32(cost.value), log[:min(ln.value, cap)], ln.value, st.as_dict()


def gpu_population(ctx, xy, packed, n, init, init_count, first, count, opts, seed):
    from teeline_amd import _capi
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    moves = np.full(count, 0xFFFFFFFF, dtype=np.uint32)
    best, st, o = C.c_uint32(0xFFFFFFFF), _capi.TlStats(), c_opts(opts)
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_sim_anneal_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), init_count, first, count, C.byref(o), seed, _vp(out), _vp(costs),
                                          _vp(moves), C.byref(best), C.byref(st))
    return rc, out, costs, moves, best.value, st.as_dict()


def check_chain(ctx, key, xy, packed, n, init, opts, seed, chain=0):
    """one chain against the oracle: tour, cost, trace, stats"""
    want_tour, want_cost, want_trace = SA.solve_cached((key, seed, chain), xy, packed, n, init, seed=seed, chain=chain, **opts)
    rc, out, cost, log, ln, st = gpu_trace(ctx, xy, packed, n, init, opts, seed, chain)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert ln == len(want_trace), (key, ln, len(want_trace))
    assert [tuple(int(v) for v in r) for r in log] == [(e, f, t, bits(c)) for e, f, t, c in want_trace], key
    assert out.tolist() == want_tour.tolist(), key
    assert bits(cost) == bits(want_cost), (key, cost, want_cost)
    epochs = len(SA.schedule(**opts))
    assert st["sweeps"] == st["candidates"] == epochs and st["moves"] == len(want_trace)
    assert st["reversed"] == sum(t - f + 1 for _e, f, t, _c in want_trace)
    return want_trace


def plan(ctx, n, count=1):
    info = ctx.device_info()
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    assert ctx.lib.tl_sim_anneal_plan(n, count, info["cus"], info["lds_bytes"], ctx.flags, C.byref(w), C.byref(t), C.byref(per)) == 0
    return w.value, t.value, per.value, info["cus"]


@pytest.fixture(scope="module")
def nospec():
    import teeline_amd as TA
    c = TA.Context(0, TA.TL_FLAG_SA_NO_SPECULATION)
    yield c
    c.close()


def geo_packed(ctx, xy):
    from teeline_amd import _capi
    n = len(xy)
    out = np.empty(n * (n - 1) // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), n, _capi.TL_DIST_GEO, _capi.TL_DM_PACKED_LOWER, _vp(out), None))
    return out


MIXED = dict(epochs=3000, cooling_rate=3e-3, min_temperature=50.0, max_temperature=100.0)


def size_cases():
    b = K.tsplib("berlin52")
    cases = {}
    for n in (2, 3, 4, 5):  # from = 0 and to = n - 1 are frequent: the closing-edge paths
        cases[f"small{n}_hot"] = (K.small(n), None, n, None, dict(K.HOT, epochs=120), 5)
        cases[f"small{n}_short"] = (K.small(n), None, n, None, dict(K.SHORT, max_temperature=100000.0), 6)
    cases["berlin52_short"] = (b["xy"], None, 52, None, K.SHORT, 1)
    cases["berlin52_hot"] = (b["xy"], None, 52, None, K.HOT, 2)
    cases["berlin52_cold"] = (b["xy"], None, 52, None, K.COLD, 3)
    cases["berlin52_init"] = (b["xy"], None, 52, np.roll(np.arange(52), 7)[::-1].copy(), K.SHORT, 8)
    for n in (64, 65, 257):
        cases[f"synth{n}_short"] = (K.synth(n, n), None, n, None, K.SHORT, n)
    cases["synth65_hot"] = (K.synth(65, 65), None, 65, None, K.HOT, 66)
    cases["synth1000_mixed"] = (K.synth(1000, 9), None, 1000, None, MIXED, 10)
    cases["one_point"] = (np.full((20, 2), 3.5, dtype=np.float32), None, 20, None, K.HOT, 11)  # every candidate equal: nothing accepted
    cases["grid6x5_short"] = (K.grid(6, 5), None, 30, None, K.SHORT, 12)
    g = K.tsplib("gr17")
    cases["gr17_matrix_short"] = (g["xy"], g["packed"], 17, None, K.SHORT, 4)
    cases["gr17_matrix_hot"] = (g["xy"], g["packed"], 17, None, K.HOT, 13)
    return cases


CASES = size_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_equals_oracle(ctx, name):
    xy, packed, n, init, opts, seed = CASES[name]
    trace = check_chain(ctx, name, xy, packed, n, init, opts, seed)
    if name == "one_point":
        assert len(trace) == 0
    if name.endswith("_hot") and n >= 17:  # (with a handful of cities most pairs are equal, adjacent or the whole path: equal costs)
        assert len(trace) > 0.5 * opts["epochs"]


@pytest.mark.parametrize("name", ["small3_hot", "small5_short", "berlin52_short", "berlin52_hot", "berlin52_cold", "synth65_hot", "gr17_matrix_short"])
def test_no_speculation_gives_the_same_chain(nospec, name):
    assert plan(nospec, 52)[0] == 1
    xy, packed, n, init, opts, seed = CASES[name]
    check_chain(nospec, name, xy, packed, n, init, opts, seed)


def test_window_edges(ctx, nospec):
    """schedule lengths 0, 1, W - 1, W, W + 1 and one that is no multiple of W; two accepts inside one window"""
    b = K.tsplib("berlin52")
    W = plan(ctx, 52)[0]
    assert W >= 64
    for k in (0, 1, W - 1, W, W + 1, 2 * W + 37):
        trace = check_chain(ctx, f"berlin52_len{k}", b["xy"], None, 52, None, K.with_epochs(k), 21)
        assert len(SA.schedule(**K.with_epochs(k))) == k
        if k >= W - 1:
            assert sum(e < W for e, *_x in trace) >= 2, "two accepted epochs inside the first window"
    check_chain(nospec, "berlin52_len1", b["xy"], None, 52, None, K.with_epochs(1), 21)
    check_chain(nospec, "berlin52_len0", b["xy"], None, 52, None, K.with_epochs(0), 21)


def test_matrix_forms(ctx):
    u = K.tsplib("ulysses22")
    packed = geo_packed(ctx, u["xy"])
    check_chain(ctx, "ulysses22_geo", u["xy"], packed, 22, None, K.SHORT, 14)
    # on a EUC_2D instance the coordinate form and the matrix form give the same chain
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    pk = np.empty(52 * 51 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(b["xy"]), 52, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    want = SA.solve_cached(("berlin52_short", 1, 0), b["xy"], None, 52, None, seed=1, **K.SHORT)
    rc, out, cost, log, ln, _st = gpu_trace(ctx, None, pk, 52, None, K.SHORT, 1)
    assert rc == 0 and out.tolist() == want[0].tolist() and bits(cost) == bits(want[1]) and ln == len(want[2])
    assert [tuple(int(v) for v in r) for r in log] == [(e, f, t, bits(c)) for e, f, t, c in want[2]]


def test_plain_entry_and_truncated_trace(ctx):
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    want = SA.solve_cached(("berlin52_short", 1, 0), b["xy"], None, 52, None, seed=1, **K.SHORT)
    out, cost, st, o = np.zeros(52, dtype=np.uint32), C.c_float(), _capi.TlStats(), c_opts(K.SHORT)
    assert ctx.lib.tl_sim_anneal(ctx.handle, _vp(b["xy"]), 52, None, None, C.byref(o), 1, _vp(out), C.byref(cost), C.byref(st)) == 0
    assert out.tolist() == want[0].tolist() and bits(cost.value) == bits(want[1]) and st.moves == len(want[2])
    rc, out2, cost2, log, ln, _ = gpu_trace(ctx, b["xy"], None, 52, None, K.SHORT, 1, cap=5)  # truncation is reported
    assert rc == 0 and ln == len(want[2]) > 5 and len(log) == 5 and out2.tolist() == want[0].tolist()
    assert [tuple(int(v) for v in r) for r in log] == [(e, f, t, bits(c)) for e, f, t, c in want[2][:5]]
    log1, ln1 = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()  # tl_sim_anneal_trace is chain 0
    assert ctx.lib.tl_sim_anneal_trace(ctx.handle, _vp(b["xy"]), 52, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None, _vp(log1), 4, C.byref(ln1)) == 0
    assert ln1.value == ln and log1.tolist() == log[:4].tolist()


# ---------------------------------------------------------------- population
POP = dict(epochs=40, cooling_rate=0.5, min_temperature=400.0, max_temperature=500.0)


def check_population(ctx, xy, n, init, init_count, first, count, sample):
    rc, out, costs, moves, best, st = gpu_population(ctx, xy, None, n, init, init_count, first, count, POP, 31)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        start = None if init_count == 0 else init if init_count == 1 else init[r]
        key = ("pop", n, first + r, None if start is None else tuple(int(v) for v in start))
        tour, cost, trace = SA.solve_cached(key, xy, None, n, start, seed=31, chain=first + r, **POP)
        assert out[r].tolist() == tour.tolist() and bits(costs[r]) == bits(cost) and moves[r] == len(trace), (count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == 40 * count and st["moves"] == int(moves.sum())
    return out, costs, moves


def test_population_counts(ctx):
    n = 5
    xy = K.small(n)
    _w, _t, per, cus = plan(ctx, n, 10 ** 6)
    assert per >= cus
    check_population(ctx, xy, n, None, 0, 0, 1, [0])
    check_population(ctx, xy, n, None, 0, 0, 2 * cus + 3, range(2 * cus + 3))
    for count in (per, per + 1):  # what one launch holds, and one more: a second launch
        edge = sorted({0, 1, cus, per - 2, per - 1, count - 1})
        out, costs, moves = check_population(ctx, xy, n, None, 0, 0, count, edge)
        # first_chain = c, count = 1 equals chain c of the larger population
        for c in (per - 1, count - 1):
            rc, o1, c1, m1, b1, _ = gpu_population(ctx, xy, None, n, None, 0, c, 1, POP, 31)
            assert rc == 0 and b1 == 0 and o1[0].tolist() == out[c].tolist() and bits(c1[0]) == bits(costs[c]) and m1[0] == moves[c]


def test_population_start_tours_and_chain_ids(ctx):
    b = K.tsplib("berlin52")
    rng = np.random.default_rng(5)
    count = 6
    one = rng.permutation(52).astype(np.uint32)
    own = np.stack([rng.permutation(52) for _ in range(count)]).astype(np.uint32)
    check_population(ctx, b["xy"], 52, None, 0, 3, count, range(count))
    check_population(ctx, b["xy"], 52, one, 1, 0, count, range(count))
    check_population(ctx, b["xy"], 52, own, count, 100, count, range(count))
    rc, *_ = gpu_population(ctx, b["xy"], None, 52, own, 2, 0, count, POP, 31)
    assert rc == -1 and ctx.lib.tl_last_error(ctx.handle).decode() == "tl_sim_anneal_population: init_count is 2: 0 (city order), 1 (one start tour) or count (6)"
    assert gpu_population(ctx, b["xy"], None, 52, None, 1, 0, count, POP, 31)[0] == -1  # init_count 1 without a tour
    assert ctx.lib.tl_last_error(ctx.handle).decode() == "tl_sim_anneal_population: NULL argument"
    assert gpu_population(ctx, b["xy"], None, 52, None, 0, 2 ** 32 - 3, count, POP, 31)[0] == -1
    assert ctx.lib.tl_last_error(ctx.handle).decode() == "tl_sim_anneal_population: chain ids beyond 2^32 - 1"
    bad = own.copy()
    bad[4, 0] = bad[4, 1]
    rc, *_ = gpu_population(ctx, b["xy"], None, 52, bad, count, 0, count, POP, 31)
    assert rc == -1 and "start tour 4" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_best_index_and_its_tie_rule(ctx):
    b = K.tsplib("berlin52")
    d = SA.dist_fn(b["xy"], None, 52)
    ident = np.arange(52, dtype=np.uint32)
    other = np.roll(ident, 1)[::-1].copy()  # the same cycle: equal edges in another order
    better = np.array(SA.solve_cached(("berlin52_short", 1, 0), b["xy"], None, 52, None, seed=1, **K.SHORT)[0], dtype=np.uint32)
    # two chains forced equal by a zero-epoch schedule go to the lower chain
    rc, out, costs, moves, best, _ = gpu_population(ctx, b["xy"], None, 52, ident, 1, 0, 3, K.EMPTY, 1)
    assert rc == 0 and best == 0 and len(set(bits(c) for c in costs)) == 1 and (out == ident).all() and (moves == 0).all()
    assert bits(costs[0]) == bits(SA.tour_length(d, ident.astype(np.int64)))
    init = np.stack([ident, better, better, other])
    rc, out, costs, moves, best, _ = gpu_population(ctx, b["xy"], None, 52, init, 4, 0, 4, K.EMPTY, 1)
    assert rc == 0 and best == 1 and (out == init).all() and bits(costs[1]) == bits(costs[2]) < bits(costs[0])
    assert [bits(c) for c in costs] == [bits(SA.tour_length(d, t.astype(np.int64))) for t in init]


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller(ctx):
    import teeline_amd as TA
    g = K.tsplib("gr17")
    with TA.Context(0) as c:
        for name in ("synth257_short", "small4_hot", "gr17_matrix_short", "berlin52_hot", "small2_hot"):
            xy, packed, n, init, opts, seed = CASES[name]
            check_chain(c, name, xy, packed, n, init, opts, seed)
        assert g["packed"] is not None


def test_errors(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    err = lambda: ctx.lib.tl_last_error(ctx.handle).decode()  # noqa: E731
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 52
    assert gpu_trace(ctx, b["xy"], None, 52, bad, K.SHORT, 1)[0] == _capi.TL_ERR_BADARG and "permutation" in err()
    for kw, msg in ((dict(cooling_rate=0.0), "cooling_rate must be > 0"), (dict(cooling_rate=1.0), "cooling_rate must be < 1"),
                    (dict(max_temperature=-1.0), "max_temperature must be > 0"), (dict(min_temperature=-1.0), "min_temperature must be >= 0"),
                    (dict(min_temperature=2000.0), "min_temperature must be < max_temperature")):
        assert gpu_trace(ctx, b["xy"], None, 52, None, dict(SA.DEFAULTS, **kw), 1, cap=4)[0] == _capi.TL_ERR_BADARG and msg in err()
    # the reference test's own combination is run: the start tour comes back (simulated_annealing.rs:90-113)
    xy5 = np.array([[0, 0], [0, 0.5], [0, 1], [1, 1], [1, 0]], dtype=np.float32)
    rc, out, cost, log, ln, st = gpu_trace(ctx, xy5, None, 5, np.arange(5), K.EMPTY, 1)
    assert rc == 0 and out.tolist() == [0, 1, 2, 3, 4] and cost == np.float32(4.0) and ln == 0 and st["sweeps"] == 0
    # one city with a non-empty schedule: the reference panics; with an empty one it returns the city
    assert gpu_trace(ctx, xy5, None, 1, None, K.with_epochs(3), 1)[0] == _capi.TL_ERR_REF_PANICS
    rc, out, cost, *_ = gpu_trace(ctx, xy5, None, 1, None, K.EMPTY, 1)
    assert rc == 0 and out.tolist() == [0] and cost == 0
    # a schedule that never ends
    assert gpu_trace(ctx, b["xy"], None, 52, None, dict(epochs=0, cooling_rate=1e-12, min_temperature=1e-3, max_temperature=1000.0), 1, cap=4)[0] == _capi.TL_ERR_UNSUPPORTED
    # just above the LDS-resident limit: refused before anything of size n is read (the arrays passed hold 52 cities)
    top = ctx.lib.tl_sim_anneal_lds_max_n(ctx.handle)
    assert top == (ctx.device_info()["lds_bytes"] - 32) // 12 and plan(ctx, top)[0] > 0 and plan(ctx, top + 1)[0] == 0
    out, cost, o = np.zeros(52, dtype=np.uint32), C.c_float(), c_opts(K.with_epochs(1))
    rc = ctx.lib.tl_sim_anneal(ctx.handle, _vp(b["xy"]), top + 1, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "LDS-resident limit" in err()
    assert ctx.lib.tl_sim_anneal(ctx.handle, None, 52, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_BADARG
    assert err() == "tl_sim_anneal: NULL argument"
    assert TA.TL_FLAG_SA_NO_SPECULATION == 1 << 29


def test_busy(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    xy, small = K.synth(1000, 9), K.small(5)
    want = SA.solve_cached(("small5_hot", 5, 0), small, None, 5, None, seed=5, **dict(K.HOT, epochs=120))
    with TA.Context(0) as c:
        res = {}

        def long_call():
            out, cost, o = np.zeros(1000, dtype=np.uint32), C.c_float(), c_opts(SA.DEFAULTS)
            res["rc"] = c.lib.tl_sim_anneal(c.handle, _vp(xy), 1000, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None)
            res["out"] = out

        t = threading.Thread(target=long_call)
        t.start()
        busy = 0
        while t.is_alive():
            rc, out, cost, *_ = gpu_trace(c, small, None, 5, None, dict(K.HOT, epochs=120), 5)
            assert rc in (0, _capi.TL_ERR_BUSY)
            if rc == 0:
                assert out.tolist() == want[0].tolist() and bits(cost) == bits(want[1])
            busy += rc == _capi.TL_ERR_BUSY
        t.join()
        assert res["rc"] in (0, _capi.TL_ERR_BUSY)
        busy += res["rc"] == _capi.TL_ERR_BUSY
        assert busy >= 1, "the two threads never met inside the context"
        if res["rc"] == 0:
            assert sorted(res["out"].tolist()) == list(range(1000))
        rc, out, cost, *_ = gpu_trace(c, small, None, 5, None, dict(K.HOT, epochs=120), 5)  # the context works afterwards
        assert rc == 0 and out.tolist() == want[0].tolist()


# ---------------------------------------------------------------- the acceptance rule on the device
def test_selftest_accept(ctx):
    eps = np.float32(1.1920929e-07)
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))  # noqa: E731
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))  # noqa: E731
    rows = []
    one = np.float32(1.0)
    for T in (1.0, 1e-3, 1e30, 1e-30, 1000.0):
        for p in (0.0, 1 - 2.0 ** -24, 0.5):
            rows += [(T, 0.0, dn(eps), p), (T, 0.0, eps, p), (T, 0.0, up(eps), p), (T, one, up(one), p), (T, one, one, p), (T, one, dn(one), p),
                     (T, 100.0, 50.0, p), (T, 10.0, 10.001, p), (T, 10.0, 20.0, p)]
    for x in (-86.9, -87.0, -87.1, dn(-87.0), up(-87.0), -1e-7, -50.0):  # new - old = -x at T = 1
        rows += [(1.0, 0.0, np.float32(-x), p) for p in (0.0, 1e-38, 0.5, 1 - 2.0 ** -24)]
    rng = np.random.default_rng(7)
    m = 4000
    T = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), m))
    old = rng.uniform(1, 1e4, m).astype(np.float32)
    new = (old + np.float32(1) * rng.normal(0, 1, m).astype(np.float32) * T.astype(np.float32) * 3).astype(np.float32)
    rows += list(zip(T, old, new, (rng.integers(0, 1 << 24, m) / float(1 << 24))))
    a = np.array(rows, dtype=np.float32)
    Tt, oo, nn, pp = (np.ascontiguousarray(a[:, k]) for k in range(4))
    acc, crit = np.zeros(len(a), dtype=np.uint32), np.zeros(len(a), dtype=np.float32)
    assert ctx.lib.tl_sa_selftest_accept(ctx.handle, _vp(Tt), _vp(oo), _vp(nn), _vp(pp), len(a), _vp(acc), _vp(crit)) == 0
    want_acc = [SA.is_acceptable(*r) for r in a]
    want_crit = [SA.metropolis(r[0], r[1], r[2]) for r in a]
    assert acc.tolist() == [int(v) for v in want_acc]
    assert crit.view(np.uint32).tolist() == [bits(v) for v in want_crit]
    assert 0.2 < np.mean(want_acc) < 0.9


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_and_chains(ctx):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    opts = TA.SAOptions(TA.HeuristicOptions(epochs=0), cooling_rate=1e-2)
    want = SA.solve_cached(("berlin52_short", 1, 0), prob.xy, None, 52, None, seed=1, **K.SHORT)
    msgs = []
    sol = TA.simulated_annealing.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    assert [k for k, _ in msgs] == ["PathUpdate"] * (len(want[2]) + 1) + ["Done"]
    d = SA.dist_fn(prob.xy, None, 52)
    assert msgs[0][1] == (prob.ids.tolist(), float(SA.tour_length(d, np.arange(52))))
    assert [bits(m[1][1]) for m in msgs[1:-1]] == [bits(c) for *_x, c in want[2]]
    assert msgs[-2][1][0] == sol.route() == prob.ids[want[0]].tolist() and bits(sol.total) == bits(want[1])
    plain = TA.simulated_annealing.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == len(want[2])
    # chains > 1: the best chain, and its own replay
    msgs2 = []
    best = TA.simulated_annealing.solve(prob, opts, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, chains=5)
    singles = [SA.solve_cached(("berlin52_short", 1, c), prob.xy, None, 52, None, seed=1, chain=c, **K.SHORT) for c in range(5)]
    c = int(np.argmin([(bits(s[1]) << 32) | k for k, s in enumerate(singles)]))
    assert best.stats["chain"] == c and best.route() == prob.ids[singles[c][0]].tolist() and bits(best.total) == bits(singles[c][1])
    assert len(msgs2) == len(singles[c][2]) + 2 and msgs2[-2][1][0] == best.route()
    # presets end to end
    for preset in ("classic", "thorough"):
        steps = TA.pipeline.steps_for_solve(preset)
        outs = TA.pipeline.run_pipeline_stages(prob, steps, {"simulated_annealing": opts}, ctx=ctx)
        assert [o.name for o in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
        seeded = SA.solve(prob.xy, None, 52, prob.positions_of(outs[-2].solution.route()), seed=1, **K.SHORT)
        assert outs[-1].solution.route() == prob.ids[seeded[0]].tolist() and bits(outs[-1].solution.total) == bits(seeded[1])
    outs = TA.pipeline.run_pipeline_stages(prob, TA.pipeline.steps_for_solve("simulated_annealing"), {"simulated_annealing": opts}, ctx=ctx)
    assert [o.name for o in outs] == ["shuffle", "simulated_annealing"]


def test_cli_equals_python_mirror(ctx):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    opts = TA.SAOptions(TA.HeuristicOptions(epochs=0), cooling_rate=1e-2)
    sa_args = ["--epochs", "0", "--cooling-rate", "0.01", "--seed", "1"]
    for args, steps in ((["solve", "simulated_annealing"], ["shuffle", "simulated_annealing"]), (["pipeline", "--steps=nn,2opt,simulated_annealing"], ["nn", "2opt", "simulated_annealing"]),
                        (["solve", "classic"], ["nn", "2opt", "simulated_annealing"])):
        r = subprocess.run([cli] + args + ["-i", tsp] + sa_args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs = TA.pipeline.run_pipeline_stages(prob, steps, {"simulated_annealing": opts}, ctx=ctx, lk_seed=1)
        assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(outs[-1].solution).splitlines(), args
    r = subprocess.run([cli, "solve", "simulated_annealing", "-i", tsp, "--chains", "4"] + sa_args, capture_output=True, text=True, timeout=120)
    best = TA.simulated_annealing.solve(prob, opts, None, TA.pipeline.random_shuffle(prob, 1, ctx=ctx).route(), ctx=ctx, seed=1, chains=4)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(best).splitlines()
    r = subprocess.run([cli, "solve", "simulated_annealing", "-i", tsp, "--cooling-rate", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cooling_rate must be < 1" in r.stderr


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """The berlin52 traces on the race-stress build (-DTL_JITTER: waves leave every barrier far apart)."""
    from teeline_amd import _capi
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    jctx = jitter_context({"tl_sim_anneal_trace_chain": [vp, vp, u32, vp, vp, C.POINTER(_capi.TlSaOpts), u64, u32, vp, C.POINTER(C.c_float), C.POINTER(_capi.TlStats), vp, u32,
                                                         C.POINTER(u32)],
                           "tl_sim_anneal_population": [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(_capi.TlSaOpts), u64, vp, vp, vp, C.POINTER(u32),
                                                        C.POINTER(_capi.TlStats)]})
    try:
        for name in ("berlin52_hot", "berlin52_cold", "small3_hot"):
            xy, packed, n, init, opts, seed = CASES[name]
            check_chain(jctx, name, xy, packed, n, init, opts, seed)
        n = 200  # the one-wave population chain with a reversal past one trip
        seed, mid = K.LONG_POP[n]
        traces, _st = check_population_chains(jctx, f"long{n}", K.synth(n, n), None, n, None, 0, jctx.cus + 1, K.long_opts(), seed, (0, mid, jctx.cus))
        K.check_long_reversals(traces[mid], n, 64)
    finally:
        jctx.close()


# ---------------------------------------------------------------- past one pass of a workgroup's loops
def check_population_chains(ctx, key, xy, packed, n, init, init_count, count, opts, seed, sample, oracle_xy=None):
    """chains `sample` of a population against the oracle: tour, cost, accepted moves.  key: the name the oracle's chains are cached
    under (check_chain's); oracle_xy: the coordinates behind a matrix"""
    rc, out, costs, moves, best, st = gpu_population(ctx, xy, packed, n, init, init_count, 0, count, opts, seed)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    traces = {}
    for r in sample:
        start = None if init_count == 0 else init if init_count == 1 else init[r]
        tour, cost, trace = SA.solve_cached((key, seed, r), xy if oracle_xy is None else oracle_xy, None, n, start, seed=seed, chain=r, **opts)
        assert out[r].tolist() == tour.tolist() and bits(costs[r]) == bits(cost) and moves[r] == len(trace), (key, count, r)
        traces[r] = trace
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == len(SA.schedule(**opts)) * count and st["moves"] == int(moves.sum())
    return traces, st


@pytest.mark.parametrize("n", sorted(K.LONG_POP))
def test_one_wave_chains_reverse_past_one_trip(ctx, nospec, n):
    """cus + 1 chains of one wave each at n = 130 and 200: loops over the tour take a second and a third trip, and the chain between the
    first and the last accepts a reversal of more than 128 elements (a second trip of the reversal loops on 64 threads) and a move that
    rebuilds the closing edge (K.check_long_reversals on the oracle's trace).  The same chain alone without speculation."""
    seed, mid = K.LONG_POP[n]
    cus = ctx.device_info()["cus"]
    _w, nt, _per, _cus = plan(ctx, n, cus + 1)
    assert nt == 64 and 0 < mid < cus
    xy, opts = K.synth(n, n), K.long_opts()
    traces, _st = check_population_chains(ctx, f"long{n}", xy, None, n, None, 0, cus + 1, opts, seed, (0, mid, cus))
    assert any(t - f + 1 > 128 for _e, f, t, _c in traces[mid])
    K.check_long_reversals(traces[mid], n, nt)
    assert plan(nospec, n)[:2] == (1, 64)
    check_chain(nospec, f"long{n}", xy, None, n, None, opts, seed, mid)


def test_four_wave_chain_reverses_past_one_trip(ctx):
    """n = 1500 on 256 threads: accepted reversals of more than 512 elements, one of them with from = 0 or to = n - 1"""
    n, seed = K.LONG_SINGLE
    assert plan(ctx, n)[1] == 256
    trace = check_chain(ctx, f"long{n}", K.synth(n, n), None, n, None, K.long_opts(), seed)
    assert any(t - f + 1 > 512 for _e, f, t, _c in trace)
    K.check_long_reversals(trace, n, 256, same_move=True)


TOP_EPOCHS = 40


def test_at_the_lds_limit(ctx):
    """n = tl_sim_anneal_lds_max_n: the verdict slots are the last 32 bytes of the LDS allocation.  One chain with its trace, nothing
    written behind the n output positions, and a population of two."""
    from teeline_amd import _capi
    top = ctx.lib.tl_sim_anneal_lds_max_n(ctx.handle)
    assert top == (ctx.device_info()["lds_bytes"] - 32) // 12 and plan(ctx, top)[0] > 0 and plan(ctx, top + 1)[0] == 0
    xy, opts = K.synth(top, 77), K.long_opts(TOP_EPOCHS)
    tour, cost, trace = SA.solve_cached(("top", 9, 0), xy, None, top, None, seed=9, chain=0, **opts)
    assert len(trace) > TOP_EPOCHS // 2
    pad = 4096
    out = np.full(top + pad, 0xA5A5A5A5, dtype=np.uint32)
    log = np.zeros((TOP_EPOCHS + 1, 4), dtype=np.uint32)
    gcost, ln, st, o = C.c_float(-1.0), C.c_uint32(), _capi.TlStats(), c_opts(opts)
    rc = ctx.lib.tl_sim_anneal_trace_chain(ctx.handle, _vp(xy), top, None, None, C.byref(o), 9, 0, _vp(out), C.byref(gcost), C.byref(st), _vp(log), len(log),
                                           C.byref(ln))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (out[top:] == 0xA5A5A5A5).all(), "written behind the tour"
    assert ln.value == len(trace) and [tuple(int(v) for v in r) for r in log[:ln.value]] == [(e, f, t, bits(c)) for e, f, t, c in trace]
    assert out[:top].tolist() == tour.tolist() and bits(gcost.value) == bits(cost)
    assert st.sweeps == TOP_EPOCHS and st.moves == len(trace) and st.reversed == sum(t - f + 1 for _e, f, t, _c in trace)
    check_population_chains(ctx, "top", xy, None, top, None, 0, 2, opts, 9, (0, 1))


def test_matrix_form_past_one_trip(ctx):
    """n = 257 as a packed EUC_2D matrix: the chain of the coordinate form, alone and as chain 0 of cus + 1 one-wave chains"""
    from teeline_amd import _capi
    xy, _packed, n, _init, opts, seed = CASES["synth257_short"]
    pk = np.empty(n * (n - 1) // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), n, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    tour, cost, trace = SA.solve_cached(("synth257_short", seed, 0), xy, None, n, None, seed=seed, chain=0, **opts)
    rc, out, gcost, log, ln, st = gpu_trace(ctx, None, pk, n, None, opts, seed)
    assert rc == 0 and out.tolist() == tour.tolist() and bits(gcost) == bits(cost) and ln == len(trace) == st["moves"]
    assert [tuple(int(v) for v in r) for r in log] == [(e, f, t, bits(c)) for e, f, t, c in trace]
    cus = ctx.device_info()["cus"]
    assert plan(ctx, n, cus + 1)[1] == 64
    check_population_chains(ctx, "synth257_short", None, pk, n, None, 0, cus + 1, opts, seed, (0, cus), oracle_xy=xy)


# ---------------------------------------------------------------- schedules longer than one piece (the tuning build's TL_SA_CHUNK)
def _on_tune_build():
    import teeline_amd as TA
    return TA._capi.load().tl_version().decode().endswith("+tune")


TUNE_ONLY = pytest.mark.skipif("not _on_tune_build()", reason="TL_SA_CHUNK is read by libteeline_gpu_tune.so only "
                                                              "(test_schedules_in_pieces_on_the_tune_build runs these in a child process)")


@TUNE_ONLY
@pytest.mark.parametrize("piece", K.PIECES)
def test_schedule_in_pieces(ctx, monkeypatch, piece):
    """From the second piece on the chains restart from out_pos with a stride of n, the temperature table is re-based, the trace index
    and the counters continue: the whole trace, the tour, the cost and the stats of chains whose schedule takes several launches."""
    monkeypatch.setenv("TL_SA_CHUNK", str(piece))
    for name, (xy, n, init, opts, seed) in K.piece_cases(piece).items():
        trace = check_chain(ctx, name, xy, None, n, init, opts, seed)
        assert len(SA.schedule(**opts)) > piece and sum(piece <= e < 2 * piece for e, *_x in trace) >= 2
    # a trace that ends inside the second piece
    xy, n, init, opts, seed = K.piece_cases(piece)["berlin52_hot"]
    tour, cost, trace = SA.solve_cached(("berlin52_hot", seed, 0), xy, None, n, init, seed=seed, **opts)
    cap = sum(e < piece for e, *_x in trace) + 1
    assert cap < len(trace) and piece <= trace[cap - 1][0] < 2 * piece
    rc, out, gcost, log, ln, _st = gpu_trace(ctx, xy, None, n, init, opts, seed, cap=cap)
    assert rc == 0 and ln == len(trace) and len(log) == cap and out.tolist() == tour.tolist() and bits(gcost) == bits(cost)
    assert [tuple(int(v) for v in r) for r in log] == [(e, f, t, bits(c)) for e, f, t, c in trace[:cap]]
    # three chains, from a start tour each (stride n from the first piece on) and from city order (stride 0, then n)
    own = K.piece_start_tours()
    for key, init, init_count in (("piece_own", own, 3), ("piece_city", None, 0)):
        traces, st = check_population_chains(ctx, key, xy, None, n, init, init_count, 3, K.SHORT, K.PIECE_POP_SEED, (0, 1, 2))
        assert st["reversed"] == sum(t - f + 1 for tr in traces.values() for _e, f, t, _c in tr)
        assert len({len(tr) for tr in traces.values()}) > 1  # per-chain counts that differ


def test_schedules_in_pieces_on_the_tune_build(ctx, monkeypatch):
    """test_schedule_in_pieces in ONE child process bound to libteeline_gpu_tune.so (a process binds one library).  With TL_SA_CHUNK set the
    product library's chain on a short schedule is the oracle's as before.  (That cannot show whether the variable was read, a schedule
    in pieces being the same chain; that the product library does not read it is the `#ifdef TL_TUNE` around the getenv in tl_api_sa.hip.)"""
    import sys
    if _on_tune_build():
        pytest.skip("already the child")
    tune = os.path.join(ROOT, "teeline_amd", "libteeline_gpu_tune.so")
    assert os.path.exists(tune), "built by __graft_entry__.build() / python -m teeline_amd.build"
    monkeypatch.setenv("TL_SA_CHUNK", "100")
    xy, packed, n, init, opts, seed = CASES["berlin52_short"]
    check_chain(ctx, "berlin52_short", xy, packed, n, init, opts, seed)
    env = dict(os.environ, TEELINE_GPU_LIB=tune)
    env.pop("TL_SA_CHUNK")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "test_schedule_in_pieces"], env=env,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.splitlines()[-1].startswith(f"{len(K.PIECES)} passed") and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-500:]
