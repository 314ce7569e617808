"""The stochastic hill climb on the GPU (tl_hill_climb*, csrc/hill_climb.hip) against the numpy statement of its specification
(tests/_hill_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every record of the
event log and the stats against the oracle's counters — at the plan's window, at window = 1 and window = 64, in both input forms and
for the chains of a population."""
import ctypes as C
import threading

import numpy as np
import pytest

import _hill_cases as HC
import _hill_oracle as HO
from _raw_context import _vp, jitter_context
import _sa_cases as K

pytestmark = pytest.mark.gpu

CASES = HC.cases()
bits = HO.bits


def hopts(epochs, platoo, window=0, reserved=0):
    from teeline_amd import _capi
    return _capi.TlHillOpts(epochs, platoo, window, reserved)


def gpu_trace(ctx, xy, packed, n, init, epochs, platoo, seed, chain=0, window=0, cap=None, reserved=0):
    from teeline_amd import _capi
    cap = cap if cap is not None else epochs + 1
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.zeros((max(cap, 1), 4), dtype=np.uint32)
    cost, ln, st = C.c_float(-1.0), C.c_uint32(), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    o = hopts(epochs, platoo, window, reserved)
    rc = ctx.lib.tl_hill_climb_trace_chain(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), C.byref(o), seed, chain, _vp(out), C.byref(cost), C.byref(st),
                                           _vp(log), cap, C.byref(ln))
    return rc, out[:n], np.float32(cost.value), log[:min(ln.value, cap)], ln.value, st.as_dict()


def gpu_population(ctx, xy, packed, n, init, init_count, first, count, epochs, platoo, seed, window=0):
    from teeline_amd import _capi
    out = np.full((max(count, 1), n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(max(count, 1), -1.0, dtype=np.float32)
    moves = np.full(max(count, 1), 0xFFFFFFFF, dtype=np.uint32)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    o = hopts(epochs, platoo, window)
    rc = ctx.lib.tl_hill_climb_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), init_count, first, count, C.byref(o), seed, _vp(out), _vp(costs),
                                          _vp(moves), C.byref(best), C.byref(st))
    return rc, out, costs, moves, best.value, st.as_dict()


def oracle(key, xy, packed, n, init, epochs, platoo, seed, chain=0):
    return HO.solve_cached((key, epochs, platoo, seed, chain), xy, packed, n, init, epochs=epochs, platoo_epochs=platoo, seed=seed, chain=chain)


def check_chain(ctx, key, xy, packed, n, init, epochs, platoo, seed, chain=0, windows=(0,), res=None):
    """one chain against the oracle, at each of the windows: tour, cost, every log record, stats"""
    res = res or oracle(key, xy, packed, n, init, epochs, platoo, seed, chain)
    want = HO.log_words(res).tolist()
    c = res["counters"]
    for w in windows:
        rc, out, gcost, glog, ln, st = gpu_trace(ctx, xy, packed, n, init, epochs, platoo, seed, chain, window=w)
        assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
        got = glog.tolist()
        first_diff = next((i for i, (g, x) in enumerate(zip(got, want)) if g != x), None)
        assert first_diff is None, (key, w, first_diff, got[first_diff], want[first_diff])
        assert ln == len(want) == c["accepts"] + c["restarts"], (key, w, ln, len(want))
        assert out.tolist() == res["tour"].tolist(), (key, w)
        assert bits(gcost) == bits(res["cost"]), (key, w, gcost, res["cost"])
        assert st["sweeps"] == st["candidates"] == epochs + 1 and st["moves"] == c["accepts"] and st["reversed"] == c["reversed"], (key, w, st, c)
    return res


def plan(ctx, n, count=1, window=0):
    info = ctx.device_info()
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    assert ctx.lib.tl_hill_climb_plan(n, count, info["cus"], info["lds_bytes"], window, C.byref(w), C.byref(t), C.byref(per)) == 0
    return w.value, t.value, per.value, info["cus"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_cases_at_three_windows(ctx, name):
    xy, packed, n, init, o, _want = CASES[name]
    assert plan(ctx, n)[0] == 256
    HC.check_conditions(name, CASES[name])
    check_chain(ctx, name, xy, packed, n, init, o["epochs"], o["platoo_epochs"], o["seed"], o["chain"], windows=(0, 1, 64), res=HC.run(name, CASES[name]))


@pytest.mark.parametrize("n", [62, 63, 64, 65, 254, 255, 256, 257, 258])
def test_size_edges(ctx, n):
    xy = K.synth(n, 300 + n)
    res = check_chain(ctx, f"synth{n}", xy, None, n, HC.start(n, n), 120, 3, 40 + n, windows=(0, 64))
    assert res["counters"]["accepts"] >= 2 and res["counters"]["restarts"] >= 1


def test_matrix_form_equals_coordinate_form(ctx):
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    pk = np.empty(52 * 51 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(b["xy"]), 52, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    xy, _p, n, init, o, _w = CASES["berlin52_p7"]
    res = HC.run("berlin52_p7", CASES["berlin52_p7"])
    for w in (0, 1):
        rc, out, gcost, glog, ln, _st = gpu_trace(ctx, None, pk, 52, init, o["epochs"], o["platoo_epochs"], o["seed"], window=w)
        assert rc == 0 and out.tolist() == res["tour"].tolist() and bits(gcost) == bits(res["cost"]) and glog.tolist() == HO.log_words(res).tolist()


def test_plain_entry_and_truncated_trace(ctx):
    from teeline_amd import _capi
    xy, _p, n, init, o, _w = CASES["berlin52_p7"]
    res = HC.run("berlin52_p7", CASES["berlin52_p7"])
    want, c = HO.log_words(res).tolist(), res["counters"]
    ini = np.ascontiguousarray(init, dtype=np.uint32)
    oo = hopts(o["epochs"], o["platoo_epochs"])
    out, gcost, st = np.zeros(52, dtype=np.uint32), C.c_float(), _capi.TlStats()
    assert ctx.lib.tl_hill_climb(ctx.handle, _vp(xy), 52, None, _vp(ini), C.byref(oo), o["seed"], _vp(out), C.byref(gcost), C.byref(st)) == 0
    assert out.tolist() == res["tour"].tolist() and bits(gcost.value) == bits(res["cost"])
    assert (st.sweeps, st.candidates, st.moves, st.reversed) == (601, 601, c["accepts"], c["reversed"])
    rc, out2, _c, glog, ln, _ = gpu_trace(ctx, xy, None, 52, init, o["epochs"], o["platoo_epochs"], o["seed"], cap=5)  # truncation is reported
    assert rc == 0 and ln == len(want) > 5 and len(glog) == 5 and out2.tolist() == res["tour"].tolist() and glog.tolist() == want[:5]
    log1, ln1 = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()  # tl_hill_climb_trace is chain 0
    assert ctx.lib.tl_hill_climb_trace(ctx.handle, _vp(xy), 52, None, _vp(ini), C.byref(oo), o["seed"], _vp(out), C.byref(gcost), None, _vp(log1), 4,
                                       C.byref(ln1)) == 0
    assert ln1.value == len(want) and log1.tolist() == want[:4]
    # opts NULL: the defaults (10 000 epochs, plateau 500) from city order
    assert ctx.lib.tl_hill_climb(ctx.handle, _vp(xy), 52, None, None, None, 3, _vp(out), C.byref(gcost), C.byref(st)) == 0
    d = oracle("berlin52_defaults", xy, None, 52, None, 10000, 500, 3)
    assert out.tolist() == d["tour"].tolist() and bits(gcost.value) == bits(d["cost"]) and st.sweeps == 10001 and st.moves == d["counters"]["accepts"]


def test_same_call_twice(ctx):
    xy, _p, n, init, o, _w = CASES["berlin52_p7"]
    a = gpu_trace(ctx, xy, None, n, init, o["epochs"], o["platoo_epochs"], o["seed"])
    b = gpu_trace(ctx, xy, None, n, init, o["epochs"], o["platoo_epochs"], o["seed"])
    assert a[0] == b[0] == 0 and a[1].tolist() == b[1].tolist() and bits(a[2]) == bits(b[2]) and a[3].tolist() == b[3].tolist() and a[4] == b[4]


# ---------------------------------------------------------------- population
POP_EPOCHS, POP_PLATOO, POP_SEED = 200, 3, 31


def check_population(ctx, xy, n, init, init_count, first, count, sample, window=0):
    rc, out, costs, moves, best, st = gpu_population(ctx, xy, None, n, init, init_count, first, count, POP_EPOCHS, POP_PLATOO, POP_SEED, window)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        start = None if init_count == 0 else init if init_count == 1 else init[r]
        key = ("pop", n, None if start is None else tuple(int(v) for v in start))
        res = oracle(key, xy, None, n, start, POP_EPOCHS, POP_PLATOO, POP_SEED, first + r)
        assert out[r].tolist() == res["tour"].tolist() and bits(costs[r]) == bits(res["cost"]) and moves[r] == res["counters"]["accepts"], (count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == st["candidates"] == (POP_EPOCHS + 1) * count and st["moves"] == int(moves.sum())
    return out, costs, moves


def test_population_counts_around_the_cus_and_past_one_launch(ctx):
    n = 5
    xy = K.small(n)
    _w, t, per, cus = plan(ctx, n, 10 ** 6)
    assert per >= cus and t == 64
    for count in (cus - 1, cus, cus + 1):
        assert plan(ctx, n, count)[1] == (256 if count <= cus else 64)
        check_population(ctx, xy, n, None, 0, 0, count, sorted({0, 1, count - 2, count - 1}))
    count = per + 1  # one more than a launch holds: a second launch
    out, costs, moves = check_population(ctx, xy, n, None, 0, 0, count, sorted({0, 1, cus, per - 1, per}))
    for c in (per - 1, per):  # first_chain = c, count = 1 equals chain c of the larger population
        rc, o1, c1, m1, b1, _ = gpu_population(ctx, xy, None, n, None, 0, c, 1, POP_EPOCHS, POP_PLATOO, POP_SEED)
        assert rc == 0 and b1 == 0 and o1[0].tolist() == out[c].tolist() and bits(c1[0]) == bits(costs[c]) and m1[0] == moves[c]
    assert gpu_population(ctx, xy, None, n, None, 0, 0, 0, POP_EPOCHS, POP_PLATOO, POP_SEED)[0] == 0  # count == 0: TL_OK, nothing written


def test_population_start_tours_and_chain_ids(ctx):
    b = K.tsplib("berlin52")
    rng = np.random.default_rng(5)
    count = 6
    one = rng.permutation(52).astype(np.uint32)
    own = np.stack([rng.permutation(52) for _ in range(count)]).astype(np.uint32)
    check_population(ctx, b["xy"], 52, None, 0, 3, count, range(count))
    check_population(ctx, b["xy"], 52, one, 1, 0, count, range(count))
    check_population(ctx, b["xy"], 52, own, count, 100, count, range(count))
    check_population(ctx, b["xy"], 52, own, count, 100, count, range(count), window=1)
    rc, *_ = gpu_population(ctx, b["xy"], None, 52, own, 2, 0, count, POP_EPOCHS, POP_PLATOO, POP_SEED)
    assert rc == -1 and ctx.lib.tl_last_error(ctx.handle).decode() == "tl_hill_climb_population: init_count is 2: 0 (city order), 1 (one start tour) or count (6)"
    assert gpu_population(ctx, b["xy"], None, 52, None, 1, 0, count, POP_EPOCHS, POP_PLATOO, POP_SEED)[0] == -1  # init_count 1 without a tour
    assert ctx.lib.tl_last_error(ctx.handle).decode() == "tl_hill_climb_population: NULL argument"
    assert gpu_population(ctx, b["xy"], None, 52, None, 0, 2 ** 32 - 3, count, POP_EPOCHS, POP_PLATOO, POP_SEED)[0] == -1
    assert ctx.lib.tl_last_error(ctx.handle).decode() == "tl_hill_climb_population: chain ids beyond 2^32 - 1"
    bad = own.copy()
    bad[4, 0] = bad[4, 1]
    rc, *_ = gpu_population(ctx, b["xy"], None, 52, bad, count, 0, count, POP_EPOCHS, POP_PLATOO, POP_SEED)
    assert rc == -1 and "start tour 4" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_best_index_and_its_tie_rule(ctx):
    """Ten cities at (0, 0) and ten at (1, 0): a tour costs its number of crossings, exactly, and two is the least a cycle can have.  A
    chain that starts sorted can never find a shorter candidate and returns its start tour at cost 2; equal costs go to the lower chain.
    (The minimum among unequal costs is asserted for every population of this file by check_population.)"""
    xy = np.ascontiguousarray(np.array([[0, 0]] * 10 + [[1, 0]] * 10, dtype=np.float32))
    srt = np.arange(20, dtype=np.uint32)
    alt = np.ascontiguousarray(np.arange(20, dtype=np.uint32).reshape(2, 10).T.reshape(-1))  # 0 10 1 11 ...: twenty crossings
    rc, out, costs, moves, best, _ = gpu_population(ctx, xy, None, 20, srt, 1, 0, 3, 30, 4, 7)  # (restarts shuffle the current tour, never the best)
    assert rc == 0 and best == 0 and [bits(c) for c in costs] == [bits(2.0)] * 3 and (out == srt).all() and (moves == 0).all()
    init = np.stack([alt, srt, srt, alt])
    rc, out, costs, moves, best, _ = gpu_population(ctx, xy, None, 20, init, 4, 0, 4, 1, 0, 7)  # two epochs: a reversal removes four crossings at the most
    assert rc == 0 and best == 1 and (out[1] == srt).all() and (out[2] == srt).all() and bits(costs[1]) == bits(costs[2]) == bits(2.0)
    assert min(costs[0], costs[3]) >= 12.0
    for r in (0, 3):
        res = oracle("two_points", xy, None, 20, alt, 1, 0, 7, r)
        assert out[r].tolist() == res["tour"].tolist() and bits(costs[r]) == bits(res["cost"]) and moves[r] == res["counters"]["accepts"]


# ---------------------------------------------------------------- limits, context reuse, errors
def test_at_the_lds_limit(ctx):
    """n = tl_hill_climb_lds_max_n from a shuffled start, about 300 epochs, a plateau short enough for restarts that shuffle the whole LDS"""
    top = ctx.lib.tl_hill_climb_lds_max_n(ctx.handle)
    info = ctx.device_info()
    assert top == (info["lds_bytes"] - 32) // 12 and plan(ctx, top)[:2] == (256, 256) and plan(ctx, top + 1)[:3] == (0, 0, 0)
    xy = K.synth(top, 78)
    res = check_chain(ctx, "top", xy, None, top, HC.start(top, 7), 300, 3, 9)
    assert res["counters"]["accepts"] >= 2 and res["counters"]["restarts"] >= 1
    rc, *_ = gpu_trace(ctx, xy, None, top + 1, None, 300, 3, 9)
    assert rc == -6 and "LDS-resident limit" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_context_reuse_larger_then_smaller(ctx):
    import teeline_amd as TA
    with TA.Context(0) as c:
        for name in ("berlin52_p7", "small4", "gr17_matrix", "small8_p1", "small3", "small2"):
            xy, packed, n, init, o, _w = CASES[name]
            check_chain(c, name, xy, packed, n, init, o["epochs"], o["platoo_epochs"], o["seed"], o["chain"], res=HC.run(name, CASES[name]))


def test_errors(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    err = lambda: ctx.lib.tl_last_error(ctx.handle).decode()  # noqa: E731
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 52
    assert gpu_trace(ctx, b["xy"], None, 52, bad, 10, 5, 1)[0] == _capi.TL_ERR_BADARG and "permutation" in err()
    assert gpu_trace(ctx, b["xy"], None, 52, None, 0, 5, 1, cap=4)[0] == _capi.TL_ERR_UNSUPPORTED and "never ends" in err()
    assert gpu_trace(ctx, b["xy"], None, 52, None, 2 ** 32 - 1, 5, 1, cap=4)[0] == _capi.TL_ERR_UNSUPPORTED
    assert gpu_trace(ctx, b["xy"], None, 1, None, 3, 5, 1)[0] == _capi.TL_ERR_REF_PANICS
    assert gpu_trace(ctx, b["xy"], None, 0, None, 3, 5, 1)[0] == _capi.TL_ERR_REF_PANICS
    assert gpu_trace(ctx, b["xy"], None, 52, None, 10, 5, 1, reserved=1)[0] == _capi.TL_ERR_BADARG and "reserved" in err()
    assert gpu_trace(ctx, b["xy"], None, 52, None, 10, 5, 1, window=257)[0] == _capi.TL_ERR_BADARG and "window" in err()
    assert gpu_trace(ctx, b["xy"], None, 52, None, 10, 5, 1, window=256)[0] == 0
    cus = ctx.device_info()["cus"]
    assert gpu_population(ctx, b["xy"], None, 52, None, 0, 0, cus + 1, 10, 5, 1, window=65)[0] == _capi.TL_ERR_BADARG  # one wave per chain
    # just above the LDS-resident limit: refused before anything of size n is read (the arrays passed hold 52 cities)
    top = ctx.lib.tl_hill_climb_lds_max_n(ctx.handle)
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    o = hopts(5, 5)
    rc = ctx.lib.tl_hill_climb(ctx.handle, _vp(b["xy"]), top + 1, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "LDS-resident limit" in err()
    assert ctx.lib.tl_hill_climb(ctx.handle, None, 52, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_BADARG
    assert err() == "tl_hill_climb: NULL argument"
    log, ln = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()
    assert ctx.lib.tl_hill_climb_trace(ctx.handle, _vp(b["xy"]), 52, None, None, C.byref(o), 1, _vp(out), C.byref(cost), None, None, 4,
                                       C.byref(ln)) == _capi.TL_ERR_BADARG
    with TA.Context(0, 1 << 31) as odd:  # a bit no flag has
        assert gpu_trace(odd, b["xy"], None, 52, None, 5, 5, 1)[0] == _capi.TL_ERR_UNSUPPORTED


def test_busy(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    xy = K.synth(1000, 9)
    sxy, _p, sn, sinit, so, _w = CASES["small5_p1"]
    res = HC.run("small5_p1", CASES["small5_p1"])
    with TA.Context(0) as c:
        got = {}

        def long_call():  # one chain epoch after epoch: long enough for the other thread to meet it
            out, gcost = np.zeros(1000, dtype=np.uint32), C.c_float()
            o = hopts(20000, 500, 1)
            got["rc"] = c.lib.tl_hill_climb(c.handle, _vp(xy), 1000, None, None, C.byref(o), 1, _vp(out), C.byref(gcost), None)
            got["out"] = out

        t = threading.Thread(target=long_call)
        t.start()
        busy = 0
        while t.is_alive():
            rc, out, gcost, *_ = gpu_trace(c, sxy, None, sn, sinit, so["epochs"], so["platoo_epochs"], so["seed"])
            assert rc in (0, _capi.TL_ERR_BUSY)
            if rc == 0:
                assert out.tolist() == res["tour"].tolist() and bits(gcost) == bits(res["cost"])
            busy += rc == _capi.TL_ERR_BUSY
        t.join()
        assert got["rc"] in (0, _capi.TL_ERR_BUSY)
        busy += got["rc"] == _capi.TL_ERR_BUSY
        assert busy >= 1, "the two threads never met inside the context"
        if got["rc"] == 0:
            assert sorted(got["out"].tolist()) == list(range(1000))
        rc, out, gcost, *_ = gpu_trace(c, sxy, None, sn, sinit, so["epochs"], so["platoo_epochs"], so["seed"])  # the context works afterwards
        assert rc == 0 and out.tolist() == res["tour"].tolist()


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """Windows with and without an event on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the rotating
    verdict slots, the restart and the commit, four waves a chain and one."""
    from teeline_amd import _capi
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    jctx = jitter_context({"tl_hill_climb_trace_chain": [vp, vp, u32, vp, vp, C.POINTER(_capi.TlHillOpts), u64, u32, vp, C.POINTER(C.c_float), C.POINTER(_capi.TlStats), vp, u32,
                                                         C.POINTER(u32)],
                           "tl_hill_climb_population": [vp, vp, u32, vp, vp, u32, u32, u32, C.POINTER(_capi.TlHillOpts), u64, vp, vp, vp, C.POINTER(u32),
                                                        C.POINTER(_capi.TlStats)]})
    try:
        for name in ("berlin52_p7", "small8_p1", "berlin52_e63"):
            xy, packed, n, init, o, _w = CASES[name]
            check_chain(jctx, name, xy, packed, n, init, o["epochs"], o["platoo_epochs"], o["seed"], o["chain"], windows=(0, 64), res=HC.run(name, CASES[name]))
        xy, _p, n, init, o, _w = CASES["berlin52_p7"]
        rc, out, costs, moves, _best, _st = gpu_population(jctx, xy, None, n, init, 1, 0, jctx.cus + 1, o["epochs"], o["platoo_epochs"], o["seed"])
        res = HC.run("berlin52_p7", CASES["berlin52_p7"])
        assert rc == 0 and out[0].tolist() == res["tour"].tolist() and bits(costs[0]) == bits(res["cost"]) and moves[0] == res["counters"]["accepts"]
    finally:
        jctx.close()
