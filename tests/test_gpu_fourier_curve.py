"""The Fourier-curve solver on the GPU (tl_fourier_curve*, csrc/fourier_curve.hip) against the statement of its specification
(tests/_fourier_oracle.py), by exact equality throughout: the final coefficients as f64 bits, every city's sample index of the logged
steps, the coefficients at the end of every stage, the tour and the f32 cost — for every launch shape (threads, chunk, span), in both
input forms, for the jobs of a batch; and the device's search alone (tl_fourier_selftest_search) on planted ties."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _fourier_cases as FC
import _fourier_oracle as FO
from _raw_context import _vp
import _sa_cases as K

pytestmark = pytest.mark.gpu

CASES = FC.cases()
bits = FO.bits
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goldens_fourier.json")))


def c_opts(o, chunk=0, span=0, threads=0):
    from teeline_amd import _capi
    return _capi.TlFourierOpts(o["k_max"], o["m"], o["epochs"], chunk, o["lam"], o["lambda_decay"], o["lr"], span, threads)


def gpu_batch(ctx, xy, packed, n, opts, chunk=0, span=0, threads=0, log_cap=0, stages=False):
    """-> rc, tours [J, n], costs, coefficient words per job, best, log [log_cap, n], stage words, stats"""
    from teeline_amd import _capi
    J = len(opts)
    arr = (_capi.TlFourierOpts * J)(*[c_opts(o, chunk, span, threads) for o in opts])
    stride = 2 * (2 * max(o["k_max"] for o in opts) + 1)
    out = np.full((J, max(n, 1)), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(J, -1.0, dtype=np.float32)
    coeffs = np.full((J, stride), np.nan)
    log = np.full((max(log_cap, 1), max(n, 1)), 0xFFFFFFFF, dtype=np.uint32)
    L2 = 2 * (2 * opts[0]["k_max"] + 1)
    stage = np.full((opts[0]["k_max"], L2), np.nan)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    rc = ctx.lib.tl_fourier_curve_batch(ctx.handle, _vp(xy), n, _vp(packed), arr, J, _vp(out), _vp(costs), _vp(coeffs), stride, C.byref(best), C.byref(st),
                                        _vp(log) if log_cap else None, log_cap, _vp(stage) if stages else None)
    words = [coeffs[j, :2 * (2 * opts[j]["k_max"] + 1)].view(np.uint64).tolist() for j in range(J)]
    return rc, out[:, :n], costs, words, best.value, log[:log_cap, :n], stage.view(np.uint64), st.as_dict()


def gpu_single(ctx, xy, packed, n, o, **kw):
    from teeline_amd import _capi
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    coeffs = np.full(2 * (2 * o["k_max"] + 1), np.nan)
    cost, st = C.c_float(-1.0), _capi.TlStats()
    po = c_opts(o, **kw)
    rc = ctx.lib.tl_fourier_curve(ctx.handle, _vp(xy), n, _vp(packed), C.byref(po), _vp(out), C.byref(cost), _vp(coeffs), C.byref(st))
    return rc, out[:n], np.float32(cost.value), coeffs.view(np.uint64).tolist(), st.as_dict()


def err(ctx):
    return ctx.lib.tl_last_error(ctx.handle).decode()


def check_case(ctx, name, **launch):
    """one job against the oracle: logged sample indices, stage-end coefficients, final coefficients, tour, cost, stats"""
    xy, packed, n, o = CASES[name]
    res = FC.oracle(name)
    steps = o["k_max"] * o["epochs"]
    cap = min(steps, FC.LOG_CAP)
    rc, out, costs, words, best, log, stage, st = gpu_batch(ctx, xy, packed, n, [o], log_cap=cap, stages=True, **launch)
    assert rc == 0, err(ctx)
    for t in range(cap):
        assert log[t].tolist() == res["log"][t].tolist(), (name, launch, "step", t)
    assert stage.ravel().tolist() == FO.f64_words(res["stage_c"]).tolist(), (name, launch)
    assert words[0] == FO.f64_words(res["coeffs"]).tolist(), (name, launch)
    assert out[0].tolist() == res["tour"].tolist() and bits(costs[0]) == bits(res["cost"]), (name, launch, costs[0], res["cost"])
    assert best == 0 and (st["sweeps"], st["candidates"]) == (steps, steps * o["m"] * n), (name, st)
    return res


# ---------------------------------------------------------------- every case, the launch shape the plan picks
@pytest.mark.parametrize("name", sorted(CASES))
def test_job_equals_the_oracle(ctx, name):
    res = check_case(ctx, name)
    if name in GOLD["cases"]:
        assert FC.case_record(res) == GOLD["cases"][name], name


def test_trivial_inputs(ctx):
    """n = 1 and n = 0: the trivial tour, cost 0, no launch; zeroed coefficients"""
    for n in (1, 0):
        rc, out, cost, words, st = gpu_single(ctx, K.small(max(n, 1))[:n].copy() if n else np.zeros((1, 2), dtype=np.float32), None, n, FC.o())
        assert rc == 0 and out.tolist() == [0] * n and bits(cost) == 0 and words == [0] * 10 and st["sweeps"] == 0, (n, err(ctx))


def test_stage_boundaries_free_the_modes_in_turn(ctx):
    """k_max 3, epochs 2: at the end of stage s only the modes |k| <= s + 1 have moved off their start values"""
    xy, packed, n, o = CASES["stages_k3_e2"]
    rc, _out, _costs, _words, _best, _log, stage, _st = gpu_batch(ctx, xy, packed, n, [o], stages=True)
    assert rc == 0, err(ctx)
    start = FO.init_coefficients(xy, 3)
    sc = stage.view(np.float64).reshape(3, 7, 2)
    for s in range(3):
        for ki in range(7):
            k = ki - 3
            same = FO.f64_words(sc[s, ki]).tolist() == FO.f64_words(start[ki]).tolist()
            assert same == (abs(k) > s + 1), (s, k)


def test_launch_shapes_give_identical_bits(ctx):
    """threads (n = threads + 1 with 64 lanes, and the plan's), chunk (n = chunk - 1, chunk, chunk + 1, two chunks and a rest; 1, 7, 64
    and the plan's), span (1 step, 7 steps, all) — every shape gives the oracle's bits"""
    check_case(ctx, "n65_past_64_lanes", threads=64)
    check_case(ctx, "n65_past_64_lanes", threads=64, chunk=64)
    for name in ("n63_chunk", "n64_chunk", "n65_past_64_lanes", "n129_two_chunks"):
        for chunk in (64, 7, 1):
            check_case(ctx, name, chunk=chunk)
    for span in (1, 7, 1 << 20):
        check_case(ctx, "stages_k3_e2", span=span)
        check_case(ctx, "circle5", span=span, threads=1024)
    check_case(ctx, "berlin52", span=7 * 97, chunk=5, threads=128)


def test_plan_picks_the_form_and_shrinks_the_chunk(ctx):
    info = ctx.device_info()
    from teeline_amd import _capi

    def plan(n, o, **kw):
        t, f, ch, sp = C.c_int(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        arr = (_capi.TlFourierOpts * 1)(c_opts(o, **kw))
        rc = ctx.lib.tl_fourier_curve_plan(n, arr, 1, info["lds_bytes"], C.byref(t), C.byref(f), C.byref(ch), C.byref(sp))
        return rc, t.value, f.value, ch.value, sp.value
    assert plan(52, FO.DEFAULTS) == (0, 384, 1, 52, 1 << 16)
    assert plan(280, FO.DEFAULTS)[1:4] == (1024, 1, 64)
    rc, t, f, ch, _sp = plan(5, FC.o(32, 4096, 1))  # basis, curve and its copy alone are 160 KiB: the workspace form, a smaller chunk
    assert (rc, f) == (0, 2) and 1 <= ch <= 5
    assert ctx.lib.tl_fourier_curve_work_bytes(52, None, 1, 0) > 0 and ctx.lib.tl_fourier_curve_work_bytes(1, None, 1, 0) == 0


# ---------------------------------------------------------------- the search alone, on a planted curve
def _selftest(ctx, gamma, xy, threads=0):
    out = np.full(len(xy), 0xFFFFFFFF, dtype=np.uint32)
    g = np.ascontiguousarray(gamma, dtype=np.float64)
    rc = ctx.lib.tl_fourier_selftest_search(ctx.handle, _vp(g), len(g), _vp(xy), len(xy), threads, _vp(out))
    assert rc == 0, err(ctx)
    want = FO.nearest(g[:, 0], g[:, 1], xy)
    host = np.full(len(xy), 0xFFFFFFFF, dtype=np.uint32)
    assert ctx.lib.tl_fourier_nearest(_vp(g), len(g), _vp(xy), len(xy), _vp(host)) == 0 and host.tolist() == want.tolist()
    return out.tolist(), want.tolist()


def _tied_root_samples():
    """(a, b): two points whose f32 squared distances from the origin differ while the f32 roots are equal, |a|^2 > |b|^2"""
    origin = np.zeros((1, 2), dtype=np.float32)
    for dx in np.arange(1.05, 1.4, 0.01, dtype=np.float32):
        S = np.float32(dx * dx)
        up = np.nextafter(S, np.float32(4.0))
        for scale in (1.0, 1.2, 0.8, 1.4):
            dy = np.float32(np.sqrt(np.float64(up) - np.float64(S)) * scale)
            sq = np.float32(S + np.float32(dy * dy))
            if sq != S and np.sqrt(sq, dtype=np.float32) == np.sqrt(S, dtype=np.float32):
                a, b = (float(dx), float(dy)), (float(dx), 0.0)
                r = FO.roots(np.array([a[0], b[0]]), np.array([a[1], b[1]]), origin)[0]
                assert r[0] == r[1]
                return a, b
    raise AssertionError("no pair found")


@pytest.mark.parametrize("threads", (0, 64, 256, 1024))
def test_search_on_planted_ties(ctx, threads):
    city = np.zeros((1, 2), dtype=np.float32)
    for m in (2, 5, 64, 65, 200, 4096):
        far = np.full((m, 2), 9.0)
        plant = {}
        g = far.copy()
        g[[0, m - 1]] = (1.0, 0.0), (1.0, 0.0)                       # two identical samples: the lower index
        plant["identical_first_last"] = (g, 0)
        if m > 2:
            g = far.copy()
            g[[m - 2, m - 1]] = (0.0, 1.0), (1.0, 0.0)               # different points at one distance
            plant["equal_distance_last_two"] = (g, m - 2)
        a, b = _tied_root_samples()
        lo, hi = (0, m - 1) if m < 4 else (m // 2 - 1, m // 2 + 1)
        g = far.copy()
        g[lo], g[hi] = a, b                                          # the LARGER square at the lower index: equal roots, it still wins
        plant["equal_roots_unequal_squares"] = (g, lo)
        g = far.copy()
        g[0] = (0.5, 0.0)
        plant["best_at_0"] = (g, 0)
        g = far.copy()
        g[m - 1] = (0.5, 0.0)
        plant["best_at_last"] = (g, m - 1)
        g = np.full((m, 2), np.nan)
        plant["all_nan"] = (g, 0)
        g = np.full((m, 2), np.nan)
        g[m - 1] = (np.inf, 0.0)
        plant["nan_is_never_nearer"] = (g, m - 1)
        for name, (gamma, want) in plant.items():
            got, oracle = _selftest(ctx, gamma, city, threads)
            assert got == oracle == [want], (m, threads, name, got, oracle)


def test_search_many_cities_against_the_oracle(ctx):
    """more cities than lanes (one lane a city), fewer (several lanes a city), cities on samples, duplicates"""
    E = FO.basis_table(97)
    gamma = 300.0 * E + 500.0
    for n, threads in ((65, 64), (300, 256), (7, 1024), (1025, 1024)):
        xy = K.small(n).copy()
        xy[: min(n, 5)] = gamma[:: 20][: min(n, 5)].astype(np.float32)
        got, want = _selftest(ctx, gamma, np.ascontiguousarray(xy), threads)
        assert got == want, (n, threads)


# ---------------------------------------------------------------- decode
def test_decode_keeps_city_order_on_one_sample_and_prices_by_the_matrix(ctx):
    xy, packed, n, o = CASES["stacked"]
    res = FC.oracle("stacked")
    assert len(set(res["sidx"].tolist())) < n  # several cities share a sample
    for a in range(n):
        for b in range(a + 1, n):
            if res["sidx"][a] == res["sidx"][b]:
                assert res["tour"].tolist().index(a) < res["tour"].tolist().index(b)
    check_case(ctx, "stacked")
    # the matrix only prices: the same tour and coefficients as from the coordinates alone, the cost from the matrix
    g = K.tsplib("gr17")
    o = CASES["gr17_matrix"][3]
    _rc, t_xy, _c_xy, w_xy, _st = gpu_single(ctx, g["xy"], None, 17, o)
    rc, t_dm, c_dm, w_dm, _st = gpu_single(ctx, g["xy"], g["packed"], 17, o)
    res = FC.oracle("gr17_matrix")
    assert rc == 0 and t_dm.tolist() == t_xy.tolist() == res["tour"].tolist() and w_dm == w_xy and bits(c_dm) == bits(res["cost"])


# ---------------------------------------------------------------- batches
def _grid(J):
    return [FC.o(k_max=1 + j % 3, m=(9, 17, 64, 33)[j % 4], epochs=2, lam=0.05 * (1 + j % 5), lr=0.05 + 0.01 * (j % 7)) for j in range(J)]


@pytest.mark.parametrize("J", (1, 3, 300))
def test_every_job_of_a_batch_equals_its_single_call(ctx, J):
    """differing k_max and m in one batch, more jobs than CUs"""
    xy, n = K.small(6), 6
    opts = _grid(J)
    rc, out, costs, words, best, _log, _stage, st = gpu_batch(ctx, xy, None, n, opts)
    assert rc == 0, err(ctx)
    for j in range(J):
        rc1, o1, c1, w1, _st = gpu_single(ctx, xy, None, n, opts[j])
        assert rc1 == 0 and out[j].tolist() == o1.tolist() and bits(costs[j]) == bits(c1) and words[j] == w1, j
    for j in (0, J // 2, J - 1):
        res = FO.solve(xy, None, n, **opts[j])
        assert out[j].tolist() == res["tour"].tolist() and words[j] == FO.f64_words(res["coeffs"]).tolist() and bits(costs[j]) == bits(res["cost"]), j
    assert best == int(np.argmin([(bits(c) << 32) | j for j, c in enumerate(costs)]))
    assert st["sweeps"] == sum(o["k_max"] * o["epochs"] for o in opts)


def test_best_index_is_the_lowest_among_equal_costs(ctx):
    xy, n = K.tsplib("berlin52")["xy"], 52
    a, b = FC.o(1, 9, 2), FC.o(3, 60, 30)
    ca, cb = (FO.solve(xy, None, n, **o)["cost"] for o in (a, b))
    assert bits(ca) != bits(cb)  # two option sets whose tours cost differently
    lo, hi = (a, b) if ca < cb else (b, a)
    rc, _out, costs, _w, best, _l, _s, _st = gpu_batch(ctx, xy, None, n, [hi, lo, hi, lo, lo])
    assert rc == 0 and best == 1 and bits(costs[1]) == bits(costs[3]) == bits(costs[4]) == bits(min(ca, cb)), (costs, best)
    rc, _out, costs, _w, best, _l, _s, _st = gpu_batch(ctx, xy, None, n, [hi, hi, hi])
    assert rc == 0 and best == 0


# ---------------------------------------------------------------- refusals
def test_refusals(ctx):
    from teeline_amd import _capi
    xy, n = K.small(6), 6
    BADARG, UNSUPPORTED, BUSY = -1, -6, -8

    def rc_of(o, nn=n, pts=xy, **kw):
        return gpu_single(ctx, pts, None, nn, o, **kw)[0]
    for bad in (FC.o(k_max=0), FC.o(m=1), FC.o(lam=0.0), FC.o(lam=-1.0), FC.o(lambda_decay=0.0), FC.o(lambda_decay=1.0), FC.o(lr=0.0), FC.o(epochs=0),
                FC.o(lam=float("nan"))):
        assert rc_of(bad) == BADARG, bad
    assert rc_of(FC.o(k_max=33)) == UNSUPPORTED and "k_max" in err(ctx)
    assert rc_of(FC.o(m=4097)) == UNSUPPORTED and "4096" in err(ctx)
    assert rc_of(FC.o(k_max=32, epochs=1 << 27)) == UNSUPPORTED and "2^32" in err(ctx)
    big = np.zeros((65537, 2), dtype=np.float32)
    assert rc_of(FC.o(), nn=65537, pts=big) == UNSUPPORTED and "65536" in err(ctx)
    assert rc_of(FC.o(k_max=32), threads=64) == BADARG and rc_of(FC.o(), threads=100) == BADARG
    out, cost = np.zeros(n, dtype=np.uint32), C.c_float()
    po = c_opts(FC.o())
    assert ctx.lib.tl_fourier_curve(ctx.handle, None, n, None, C.byref(po), _vp(out), C.byref(cost), None, None) == BADARG and "xy is NULL" in err(ctx)
    nan = xy.copy()
    nan[3, 1] = np.inf
    assert rc_of(FC.o(), pts=nan) == BADARG and "not finite" in err(ctx)
    two = (_capi.TlFourierOpts * 2)(c_opts(FC.o(), chunk=8), c_opts(FC.o(), chunk=9))
    outs = np.zeros((2, n), dtype=np.uint32)
    assert ctx.lib.tl_fourier_curve_batch(ctx.handle, _vp(xy), n, None, two, 2, _vp(outs), None, None, 0, None, None, None, 0, None) == BADARG


def test_busy(ctx):
    """two threads on one context: every call gives the right result or TL_ERR_BUSY, never anything else"""
    import threading
    import teeline_amd as TA
    BUSY = -8
    big, small = K.synth(1000, 9), K.small(6)
    o = FC.o()
    want = FO.solve(small, None, 6, **o)
    with TA.Context(0) as c:
        res = {}

        def long_call():
            r = gpu_single(c, big, None, 1000, dict(FO.DEFAULTS, epochs=100))
            res["rc"], res["out"] = r[0], r[1]

        t = threading.Thread(target=long_call)
        t.start()
        busy = 0
        while t.is_alive():
            rc, out, cost, words, _st = gpu_single(c, small, None, 6, o)
            assert rc in (0, BUSY)
            if rc == 0:
                assert out.tolist() == want["tour"].tolist() and words == FO.f64_words(want["coeffs"]).tolist()
            busy += rc == BUSY
        t.join()
        assert res["rc"] in (0, BUSY)
        busy += res["rc"] == BUSY
        assert busy >= 1, "the two threads never met inside the context"
        if res["rc"] == 0:
            assert sorted(res["out"].tolist()) == list(range(1000))
        rc, out, _cost, _words, _st = gpu_single(c, small, None, 6, o)  # the context works afterwards
        assert rc == 0 and out.tolist() == want["tour"].tolist()


# ---------------------------------------------------------------- instances
def test_berlin52_defaults_equal_the_golden(ctx):
    b = K.tsplib("berlin52")
    rc, out, cost, words, _st = gpu_single(ctx, b["xy"], None, 52, dict(FO.DEFAULTS))
    gold = GOLD["cases"]["berlin52"]
    assert rc == 0 and out.tolist() == gold["tour"] and bits(cost) == gold["cost_bits"] and [str(w) for w in words] == gold["coeffs"]
    # opts NULL: the defaults
    out2, c2 = np.zeros(52, dtype=np.uint32), C.c_float()
    assert ctx.lib.tl_fourier_curve(ctx.handle, _vp(b["xy"]), 52, None, None, _vp(out2), C.byref(c2), None, None) == 0
    assert out2.tolist() == gold["tour"] and bits(np.float32(c2.value)) == gold["cost_bits"]
