"""The Kohonen map solver on the GPU (tl_kohonen_som*, csrc/kohonen_som.hip) against the statement of its specification
(tests/_som_oracle.py), by exact equality throughout: the (city, bmu) log of every epoch, the final ring bit for bit, every checkpoint
record (epoch, tour, cost bits) in the reference's message order, the result — in both forms of the ring, in both input forms, for the
runs of a batch; and the device's BMU and extraction alone (tl_som_selftest_bmu) on planted exact ties."""
import ctypes as C

import numpy as np
import pytest

from _raw_context import _vp
import _som_cases as SC
import _som_oracle as SO

pytestmark = pytest.mark.gpu

CASES = SC.cases()
bits = SO.bits


def _opts(o, form=0, work=0):
    from teeline_amd import _capi
    return _capi.TlSomOpts(o["epochs"], o["neuron_multiplier"], o["learning_rate"], o["radius_fraction"], form, 0, work)


def gpu_trace(ctx, xy, packed, n, o, form=0, cp_cap=20):
    from teeline_amd import _capi
    M = n * o["neuron_multiplier"]
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.full((o["epochs"], 2), 0xFFFFFFFF, dtype=np.uint32)
    ring = np.full(2 * M, np.nan)
    ep, tours, cb = np.full(cp_cap, 7, dtype=np.uint32), np.full((cp_cap, max(n, 1)), 0xFFFFFFFF, dtype=np.uint32), np.full(cp_cap, 7, dtype=np.uint32)
    cost, ln, st = C.c_float(-1.0), C.c_uint32(), _capi.TlStats()
    po = _opts(o, form)
    rc = ctx.lib.tl_kohonen_som_trace(ctx.handle, _vp(xy), n, _vp(packed), C.byref(po), o["seed"], o.get("run", 0), _vp(out), C.byref(cost), C.byref(st), _vp(log),
                                      len(log), _vp(ring), _vp(ep), _vp(tours), _vp(cb), cp_cap, C.byref(ln))
    k = min(ln.value, cp_cap)
    return rc, out[:n], np.float32(cost.value), log, ring.view(np.uint64), [(int(ep[i]), tours[i, :n].tolist(), int(cb[i])) for i in range(k)], ln.value, st.as_dict()


def gpu_population(ctx, xy, packed, n, first, count, o, form=0, work=0):
    from teeline_amd import _capi
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    po = _opts(o, form, work)
    rc = ctx.lib.tl_kohonen_som_population(ctx.handle, _vp(xy), n, _vp(packed), first, count, C.byref(po), o["seed"], _vp(out), _vp(costs), C.byref(best), C.byref(st))
    return rc, out, costs, best.value, st.as_dict()


def oracle(key, xy, packed, n, o):
    return SO.solve_cached((key, n, tuple(sorted(o.items()))), xy, packed, n, **o)


def check_run(ctx, key, xy, packed, n, o, form=0):
    """one run against the oracle: log, final ring, every checkpoint record, the result, stats"""
    res = oracle(key, xy, packed, n, o)
    rc, out, cost, log, ring, cps, ln, st = gpu_trace(ctx, xy, packed, n, o, form)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    want = SO.log_words(res)
    for t in range(o["epochs"]):
        assert log[t].tolist() == want[t].tolist(), (key, "epoch", t + 1)
    assert ring.tolist() == SO.ring_words(res).tolist(), key
    assert ln == len(res["checkpoints"]) and cps == [(t, list(tour), bits(c)) for t, tour, c in res["checkpoints"]], key
    assert out.tolist() == res["tour"].tolist() and bits(cost) == bits(res["cost"]), (key, cost, res["cost"])
    assert (st["sweeps"], st["candidates"]) == (o["epochs"], o["epochs"] * res["neurons"]), (key, st)
    return res


def plan(ctx, n, mult, form=0, work=8 << 30):
    info = ctx.device_info()
    M, t, f, per = C.c_uint32(), C.c_int(), C.c_uint32(), C.c_uint32()
    rc = ctx.lib.tl_kohonen_som_plan(n, mult, form, 1, info["cus"], info["lds_bytes"], work, 0, C.byref(M), C.byref(t), C.byref(f), C.byref(per))
    return rc, M.value, t.value, f.value, per.value


# ---------------------------------------------------------------- every case, the form the plan picks
@pytest.mark.parametrize("name", sorted(CASES))
def test_run_equals_the_oracle(ctx, name):
    xy, packed, n, o, want = CASES[name]
    res = check_run(ctx, name, xy, packed, n, o)
    SC.check_conditions(name, res, o, want)
    M = n * o["neuron_multiplier"]
    assert plan(ctx, n, o["neuron_multiplier"])[1:4] == (M, SC.threads_of(M), 1)


def test_cases_cover_the_sizes(ctx):
    """M below, at and one past a wave and the workgroup (64 lanes up to M = 512), 2 T + 1, and rings of two and three waves"""
    Ms = {n * o["neuron_multiplier"] for _xy, _p, n, o, _w in CASES.values()}
    assert {2, 3, 5, 7, 63, 64, 65, 129, 416, 513, 1025, 20, 21} <= Ms
    assert [SC.threads_of(M) for M in (63, 64, 65, 129, 416, 512, 513, 1025, 8016, 10208)] == [64, 64, 64, 64, 64, 64, 128, 192, 1024, 1024]
    assert {o["epochs"] for _xy, _p, _n, o, _w in CASES.values()} >= {1, 9, 10, 11, 25}


# ---------------------------------------------------------------- the two forms
@pytest.mark.parametrize("name", ["M65", "berlin52", "M1025_three_waves", "rf1_even"])
def test_workspace_form_equals_the_lds_form(ctx, name):
    xy, packed, n, o, _want = CASES[name]
    for form in (1, 2):
        check_run(ctx, name, xy, packed, n, o, form)
    assert plan(ctx, n, o["neuron_multiplier"], 2)[3] == 2


def test_forms_at_the_lds_limit(ctx):
    """the LDS form at its largest n and the workspace form one above, 20 epochs each, multiplier 8"""
    from teeline_amd import _capi
    import _sa_cases as K
    info = ctx.device_info()
    top = ctx.lib.tl_kohonen_som_max_n(ctx.handle, 8, 1)
    assert top == (info["lds_bytes"] - 512) // 16 // 8 and ctx.lib.tl_kohonen_som_max_n(ctx.handle, 8, 0) == 65536 // 8 == ctx.lib.tl_kohonen_som_max_n(ctx.handle, 8, 2)
    for n, form in ((top, 1), (top + 1, 2)):
        o = SC.o(20, 8, seed=n)
        assert plan(ctx, n, 8)[1:4] == (8 * n, 1024, form)
        xy = K.synth(n, n)
        check_run(ctx, f"limit{n}", xy, None, n, o)
    o = SC.o(20, 8, seed=top + 1)
    rc, *_ = gpu_trace(ctx, K.synth(top + 1, top + 1), None, top + 1, o, form=1)
    assert rc == _capi.TL_ERR_UNSUPPORTED


# ---------------------------------------------------------------- runs
def test_runs_of_a_batch_equal_the_single_calls(ctx):
    xy, packed, n, o, _want = CASES["M65"]
    rc, outs, costs, best, st = gpu_population(ctx, xy, packed, n, 3, 5, o)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    singles = [oracle("M65", xy, packed, n, dict(o, run=3 + c)) for c in range(5)]
    for c in range(5):
        assert outs[c].tolist() == singles[c]["tour"].tolist() and bits(costs[c]) == bits(singles[c]["cost"]), c
        rc1, out1, cost1, *_ = gpu_trace(ctx, xy, packed, n, dict(o, run=3 + c))
        assert rc1 == 0 and out1.tolist() == outs[c].tolist() and bits(cost1) == bits(costs[c])
    assert best == int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))  # lowest cost, then lowest index
    assert len({bits(s["cost"]) for s in singles}) > 1 and st["sweeps"] == 5 * o["epochs"]
    # more runs than one launch sequence holds: a workspace of two runs' blocks
    run_bytes = 16 * 65 + 16 * n
    assert plan(ctx, n, o["neuron_multiplier"], 0, 2 * run_bytes + 5 * 256)[4] == 2
    for form in (0, 2):
        rc, outs2, costs2, best2, _st = gpu_population(ctx, xy, packed, n, 3, 5, o, form=form, work=2 * run_bytes + 5 * 256)
        assert rc == 0 and outs2.tolist() == outs.tolist() and costs2.tolist() == costs.tolist() and best2 == best
    rc, *_ = gpu_population(ctx, xy, packed, n, 3, 5, o, work=run_bytes)  # not one run
    from teeline_amd import _capi
    assert rc == _capi.TL_ERR_UNSUPPORTED


def test_matrix_prices_the_tour_and_coordinates_are_required(ctx):
    from teeline_amd import _capi
    xy, packed, n, o, _want = CASES["gr17_matrix"]
    with_m, without = oracle("gr17_matrix", xy, packed, n, o), oracle("gr17_xy", xy, None, n, o)
    assert with_m["tour"].tolist() == without["tour"].tolist() and bits(with_m["cost"]) != bits(without["cost"])  # the matrix only prices
    rc, *_ = gpu_trace(ctx, None, packed, n, o)
    assert rc == _capi.TL_ERR_BADARG and b"trains on the coordinates" in ctx.lib.tl_last_error(ctx.handle)
    for bad in (np.nan, np.inf, -np.inf):
        x = np.array(xy, copy=True)
        x[5, 1] = bad
        assert gpu_trace(ctx, x, None, n, o)[0] == _capi.TL_ERR_BADARG
    for k, v in (("epochs", 0), ("learning_rate", 0.0), ("learning_rate", 1.5), ("radius_fraction", 0.0), ("radius_fraction", float("nan")), ("neuron_multiplier", 0)):
        assert gpu_trace(ctx, xy, None, n, dict(o, **{k: v}) if k != "epochs" else dict(o, epochs=0))[0] == _capi.TL_ERR_BADARG, (k, v)
    assert gpu_population(ctx, xy, None, n, 0, 1, dict(o, epochs=2 ** 32 - 1))[0] == _capi.TL_ERR_UNSUPPORTED
    assert gpu_population(ctx, xy, None, n, 0, 1, dict(o, neuron_multiplier=65536 // 17 + 1))[0] == _capi.TL_ERR_UNSUPPORTED
    assert gpu_population(ctx, xy, None, n, 0, 1, o, form=3)[0] == _capi.TL_ERR_BADARG
    # n < 2: the trivial route
    rc, out, cost, _log, _ring, cps, ln, _st = gpu_trace(ctx, xy[:1].copy(), None, 1, SC.o(5))
    assert rc == 0 and out.tolist() == [0] and cost == 0 and ln == 0 and cps == []


# ---------------------------------------------------------------- planted exact ties
def device_bmu(ctx, ring, cities, threads=0, form=0):
    M, n = len(ring), len(cities)
    r = np.ascontiguousarray(np.asarray(ring, dtype=np.float64).T).reshape(-1)
    c = np.ascontiguousarray(np.asarray(cities, dtype=np.float64).T).reshape(-1)
    a, b, t = (np.full(n, 0xFFFFFFFF, dtype=np.uint32) for _ in range(3))
    rc = ctx.lib.tl_som_selftest_bmu(ctx.handle, _vp(r), M, _vp(c), n, threads, form, _vp(a), _vp(b), _vp(t))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    return a.tolist(), b.tolist(), t.tolist()


@pytest.mark.parametrize("M,threads", [(2, 64), (65, 64), (130, 64), (200, 128), (1025, 192), (2049, 1024)])
def test_planted_ties_go_to_the_first_minimum(ctx, M, threads):
    """equal minima astride a lane, a wave and an ownership seam, at index 0 and M - 1: the lowest index wins, in both forms"""
    for name, (ring, city, first) in SC.planted_ties(M, threads).items():
        cities = np.concatenate([city, city])  # (the self-test takes n >= 2: the same city twice, both parities of the slots)
        assert SO.first_min(ring, city[0])[0] == first, name
        for form in (1, 2):
            train, ext, _tour = device_bmu(ctx, ring, cities, threads, form)
            assert train == [first, first] == ext, (name, form)


def test_ranking_ties_go_by_the_city_index(ctx):
    ring, cities = SC.ranking_ties()
    tour, bm = SO.extract(cities, ring)
    keys = [(b, d) for b, d in bm]
    assert len(set(keys)) < len(keys) - 3  # several cities share (neuron, distance)
    train, ext, got = device_bmu(ctx, ring, cities)
    assert train == [b for b, _d in bm] == ext and got == tour
