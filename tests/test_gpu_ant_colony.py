"""The ant colony solver on the GPU (tl_ant_colony*, csrc/ant_colony.hip) against the numpy statement of its specification
(tests/_aco_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every word of the
per-epoch trace (every ant's cost bits — which pin the sequential sums, the power and the deposits of the epochs before —, its start
city and its count of fallback selections), every row of the route log and the stats against the oracle's counters — in both input
forms and for the runs of a batch; and the device's selection alone on given rows (tl_aco_selftest_select)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _aco_cases as AC
import _aco_oracle as ACO
from _raw_context import _vp, jitter_context
import _sa_cases as K
from _swarm_harness import okey
from _swarm_oracle import bits

pytestmark = pytest.mark.gpu

WORK = 8 << 30  # the workspace the entries plan with (include/teeline_gpu.h)
CH = AC.CHUNK


def par(o):
    return o["epochs"], o["alpha"], o["beta"], o["evaporation_rate"], o["num_ants"], o["seed"]


def gpu_trace(ctx, xy, packed, n, init, o, cap=None, route_cap=4096):
    from teeline_amd import _capi
    epochs, ants = o["epochs"], o["num_ants"]
    cap = epochs if cap is None else cap
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.zeros((max(cap, 1), 3 * ants), dtype=np.uint32)
    routes = np.full((max(route_cap, 1), n + 3), 0xFFFFFFFF, dtype=np.uint32)
    cost, ln, rows, st = C.c_float(-1.0), C.c_uint32(), C.c_uint32(), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_ant_colony_trace_run(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), *par(o), o.get("run", 0), _vp(out), C.byref(cost), C.byref(st), _vp(log), cap,
                                         C.byref(ln), _vp(routes), route_cap, C.byref(rows))
    return rc, out[:n], np.float32(cost.value), log[:min(ln.value, cap)], ln.value, st.as_dict(), routes[:min(rows.value, route_cap)], rows.value


def gpu_population(ctx, xy, packed, n, init, init_count, first, count, o):
    from teeline_amd import _capi
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_ant_colony_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), init_count, first, count, *par(o), _vp(out), _vp(costs), C.byref(best),
                                          C.byref(st))
    return rc, out, costs, best.value, st.as_dict()


def check_run(ctx, key, xy, packed, n, init, o, keep=False):
    """one run against the oracle: tour, cost, every trace word, every route row, stats"""
    res = ACO.solve_cached(okey(key, n, init, o), xy, packed, n, init, keep=keep, **o)
    rc, out, gcost, glog, ln, st, routes, rows = gpu_trace(ctx, xy, packed, n, init, o)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert ln == o["epochs"] == len(res["epochs"]), (key, ln)
    want = ACO.log_words(res, o["num_ants"])
    for g in range(ln):
        assert glog[g].tolist() == want[g].tolist(), (key, "epoch", g)
    assert rows == len(res["routes"]) and routes.tolist() == ACO.route_words(res, n).tolist(), key
    assert out.tolist() == res["tour"].tolist(), key
    assert bits(gcost) == bits(res["cost"]), (key, gcost, res["cost"])
    c = res["counters"]
    assert (st["sweeps"], st["candidates"], st["moves"], st["reversed"]) == (o["epochs"], c["tours"], c["improved"], c["fallbacks"]), (key, st, c)
    return res


def plan(ctx, n, ants=25, count=1, work=WORK):
    info = ctx.device_info()
    per, t, need = C.c_uint32(), C.c_int(), C.c_uint64()
    assert ctx.lib.tl_ant_colony_plan(n, ants, count, info["cus"], info["lds_bytes"], work, C.byref(per), C.byref(t), C.byref(need)) == 0
    return per.value, t.value, need.value


# ---------------------------------------------------------------- the device's selection
def device_select(ctx, w, e, vis, r1, r2):
    w, e = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(e, dtype=np.float32)
    vis = np.ascontiguousarray(vis, dtype=np.uint32)
    out = np.full(4, 0xFFFFFFFF, dtype=np.uint32)
    rc = ctx.lib.tl_aco_selftest_select(ctx.handle, _vp(w), _vp(e), _vp(vis), len(w), r1, r2, _vp(out))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    return int(out[0]), int(out[1]), int(out[2]), int(out[3])


def check_select(ctx, w, e, vis, r1, r2, what):
    city, path, t1, t2 = ACO.select_compacted(w, e, vis, np.float32(r1), np.float32(r2))
    got = device_select(ctx, w, e, vis, r1, r2)
    assert got[:2] == (city, path), (len(w), what, r1, r2, got, (city, path, bits(t1), bits(t2)))
    for g, t in zip(got[2:], (t1, t2)):  # the totals bit for bit (a NaN total as a NaN: its payload is the platform's)
        assert g == bits(t) or (np.isnan(t) and np.isnan(np.array([g], dtype=np.uint32).view(np.float32)[0])), (len(w), what, g, bits(t))
    return city, path


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 1, 1002])
def test_selftest_select(ctx, n):
    """n around the wave and the tile (one chunk, its edge, two chunks and a city, many); the rows of AC.selection_rows"""
    seen = set()
    for w, e, vis, r1, r2, what in AC.selection_rows(n, n):
        seen.add(check_select(ctx, w, e, vis, r1, r2, what)[1])
    assert seen == {0, 1, 2}
    if n > CH:  # a target in the first chunk and one in the last, nothing visited
        w = np.ones(n, dtype=np.float32)
        e = np.ones(n, dtype=np.float32)
        none = np.zeros(n, dtype=np.uint32)
        assert check_select(ctx, w, e, none, 1.0 / n, 0.5, "first chunk")[0] < CH
        assert check_select(ctx, w, e, none, (n - 0.5) / n, 0.5, "last chunk")[0] == n - 1 >= (n - 1) // CH * CH
        last = np.ones(n, dtype=np.uint32)  # the only candidate sits in the last chunk, and the walk is exhausted
        last[n - 2] = 0
        assert check_select(ctx, w, e, last, 1.0, 0.5, "exhausted, last chunk") == (n - 2, 0)


def test_selftest_select_reference_vectors(ctx):
    from teeline_amd import _capi
    for primary, fallback, r1, r2, want in AC.REFERENCE_SELECT:
        assert device_select(ctx, primary, fallback, [0, 0], r1, r2)[0] == want
    assert device_select(ctx, [0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0, 0, 0], 0.0, 0.5)[:2] == (2, 0)  # roulette_select: strict acc > target
    out = np.zeros(4, dtype=np.uint32)
    one = np.ones(2, dtype=np.float32)
    assert ctx.lib.tl_aco_selftest_select(ctx.handle, _vp(one), _vp(one), _vp(np.ones(2, dtype=np.uint32)), 2, 0.5, 0.5, _vp(out)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_aco_selftest_select(ctx.handle, _vp(one), _vp(one), None, 2, 0.5, 0.5, _vp(out)) == _capi.TL_ERR_BADARG


# ---------------------------------------------------------------- whole runs
GOLDEN = AC.golden_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    xy, packed, n, init, o = GOLDEN[name]
    res = check_run(ctx, name, xy, packed, n, init, o)
    AC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("n", [3, 4, 5, 8, 65, 2 * CH + 1])
def test_sizes(ctx, n):
    xy = AC.instance(n)
    o = dict(AC.OPT, epochs=3, num_ants=7, seed=11 + n, run=0)
    check_run(ctx, "size", xy, None, n, None, o)
    check_run(ctx, "size_init", xy, None, n, AC.start_tour(n, n), dict(o, run=1))


@pytest.mark.parametrize("ants", [1, 25, 63, 64, 65, 129])
def test_num_ants(ctx, ants):
    """one lane, part of a wave, a full chain wave and its edges, three groups"""
    check_run(ctx, "ants", AC.instance(40), None, 40, AC.start_tour(40, 4), dict(AC.OPT, epochs=2, num_ants=ants, seed=40, run=0))


@pytest.mark.parametrize("epochs", [0, 1, 2, 20])
def test_epochs(ctx, epochs):
    xy = K.small(8)
    check_run(ctx, "epochs", xy, None, 8, None, dict(AC.OPT, epochs=epochs, num_ants=5, seed=5, run=0))
    res = check_run(ctx, "epochs_init", xy, None, 8, AC.start_tour(8, 2), dict(AC.OPT, epochs=epochs, num_ants=5, seed=5, run=0))
    if epochs == 0:
        assert res["tour"].tolist() == AC.start_tour(8, 2).tolist()


@pytest.mark.parametrize("alpha,beta", [(0.0, 2.0), (1.0, 0.0), (0.0, 0.0), (1.3, 2.7), (0.5, 5.5), (2.0, 1.0), (3.0, 3.0)])
def test_exponents(ctx, alpha, beta):
    """the exact exponents 0, 1 and 2 and the f64 path of aco_pow"""
    check_run(ctx, "exp", AC.instance(52), None, 52, AC.start_tour(52, 1), dict(AC.OPT, epochs=3, num_ants=10, alpha=alpha, beta=beta, seed=6, run=0))


def _packed(ctx, xy):
    from teeline_amd import _capi
    n = len(xy)
    pk = np.empty(n * (n - 1) // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), n, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    return pk


def test_matrix_form_equals_coordinate_form(ctx):
    o = dict(AC.OPT, epochs=2, num_ants=9, seed=70, run=0)
    xy = AC.instance(70)
    res = check_run(ctx, "m70", xy, None, 70, None, o)
    rc, out, gcost, glog, ln, _st, _routes, _rows = gpu_trace(ctx, None, _packed(ctx, xy), 70, None, o)
    assert rc == 0 and out.tolist() == res["tour"].tolist() and bits(gcost) == bits(res["cost"]) and glog.tolist() == ACO.log_words(res, 9).tolist()
    xy = AC.instance(257)
    o = dict(AC.OPT, epochs=1, num_ants=5, seed=257, run=0)
    check_run(ctx, "m257", None, _packed(ctx, xy), 257, None, o)


def test_alpha_20_every_selection_takes_the_eta_path(ctx):
    b = K.tsplib("berlin52")
    o = AC.UNDERFLOW
    res = check_run(ctx, "underflow", b["xy"], None, 52, np.arange(52, dtype=np.uint32), o, keep=True)
    assert res["counters"]["fallbacks"] == o["epochs"] * o["num_ants"] * 51
    assert all(p == 1 and t1 == 0 for ep in res["paths"] for ant in ep for p, t1, _t2 in ant)


def test_coincident_cities_take_the_first_candidate(ctx):
    n, o = AC.COINCIDENT_N, AC.COINCIDENT
    xy = np.full((n, 2), 3.0, dtype=np.float32)
    res = check_run(ctx, "coincident", xy, None, n, None, o, keep=True)
    assert res["cost"] == 0 and all(c == 0 for e in res["epochs"] for c in e["costs"]) and res["counters"]["improved"] == 0
    first = res["paths"][0][0]
    assert [p for p, _a, _b in first[:n - 341]] == [2] * (n - 341) and first[-1][0] == 0 and {p for p, _a, _b in first} == {0, 2}
    assert all(np.isinf(t2) for p, _t1, t2 in first if p == 2)


def test_n_1002(ctx):
    check_run(ctx, "n1002", AC.instance(1002), None, 1002, None, dict(AC.OPT, epochs=1, seed=1002, run=0))


def test_largest_n(ctx):
    """n = tl_ant_colony_max_n, two ants, one epoch (the oracle takes about 7 s for it): the construct workgroup's LDS to its last
    byte — 169 prefix chunks, 338 visited words per ant on 160 KiB.  n = 4 097 is the first size past 64 chunks.  One city more is
    refused before anything of size n is read (the arrays passed hold 52 cities)."""
    from teeline_amd import _capi
    top = ctx.lib.tl_ant_colony_max_n(ctx.handle)
    assert 4097 < top <= 65535 and plan(ctx, top, 2)[0] >= 1 and plan(ctx, top + 1, 2) == (0, 0, 0)
    for n in (4097, top):
        check_run(ctx, "largest", AC.instance(n), None, n, None, dict(AC.OPT, epochs=1, num_ants=2, seed=n, run=0))
    b = K.tsplib("berlin52")
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    rc = ctx.lib.tl_ant_colony(ctx.handle, _vp(b["xy"]), top + 1, None, None, 1, 1.0, 2.0, 0.5, 2, 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "exceeds the limit" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_small_n_needs_no_device(ctx):
    for n in (0, 1, 2):
        xy = K.small(3)[:n]
        o = dict(AC.OPT, epochs=3, seed=1, run=0)
        res = ACO.solve(xy, None, n, None, **o)
        rc, out, gcost, glog, ln, _st, routes, rows = gpu_trace(ctx, xy if n else K.small(3), None, n, None, o)
        assert rc == 0 and out.tolist() == list(range(n)) and bits(gcost) == bits(res["cost"]) and rows == 0 and ln == 0


def test_plain_entry_and_truncated_trace(ctx):
    from teeline_amd import _capi
    xy, _packed_, n, init, o = GOLDEN["berlin52"]
    res = ACO.solve_cached(okey("berlin52", n, init, o), xy, None, n, init, **o)
    out, gcost, st = np.zeros(52, dtype=np.uint32), C.c_float(), _capi.TlStats()
    assert ctx.lib.tl_ant_colony(ctx.handle, _vp(xy), 52, None, None, *par(o), _vp(out), C.byref(gcost), C.byref(st)) == 0
    assert out.tolist() == res["tour"].tolist() and bits(gcost.value) == bits(res["cost"])
    assert (st.sweeps, st.candidates, st.moves, st.reversed) == (o["epochs"], res["counters"]["tours"], res["counters"]["improved"], 0)
    rc, out2, _c, glog, ln, _st, routes, rows = gpu_trace(ctx, xy, None, 52, None, o, cap=5, route_cap=2)  # truncation is reported
    assert rc == 0 and ln == o["epochs"] and len(glog) == 5 and len(routes) == 2 and rows == len(res["routes"]) > 2 and out2.tolist() == res["tour"].tolist()
    assert glog.tolist() == ACO.log_words(res, 25)[:5].tolist() and routes.tolist() == ACO.route_words(res, 52)[:2].tolist()
    log1, ln1 = np.zeros((4, 75), dtype=np.uint32), C.c_uint32()  # tl_ant_colony_trace is run 0, the route log optional
    assert ctx.lib.tl_ant_colony_trace(ctx.handle, _vp(xy), 52, None, None, *par(o), _vp(out), C.byref(gcost), None, _vp(log1), 4, C.byref(ln1), None, 0, None) == 0
    assert ln1.value == o["epochs"] and log1.tolist() == glog[:4].tolist()


# ---------------------------------------------------------------- batches
POP = dict(AC.OPT, epochs=2, num_ants=6, seed=31)


def check_population(ctx, xy, n, init, init_count, first, count, sample, o=POP):
    rc, out, costs, best, st = gpu_population(ctx, xy, None, n, init, init_count, first, count, o)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        ini = None if init is None else np.asarray(init).reshape(-1, n)[r if init_count > 1 else 0]
        res = ACO.solve_cached(okey("pop", n, ini, dict(o, run=first + r)), xy, None, n, ini, **dict(o, run=first + r))
        assert out[r].tolist() == res["tour"].tolist() and bits(costs[r]) == bits(res["cost"]), (count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == o["epochs"] * count and st["candidates"] == o["epochs"] * count * o["num_ants"]
    return out, costs


def test_batches(ctx):
    n = 60
    xy = AC.instance(n)
    cus = ctx.device_info()["cus"]
    count = cus + 1
    out, costs = check_population(ctx, xy, n, None, 0, 0, count, [0, 7, cus])
    rc, o1, c1, b1, _ = gpu_population(ctx, xy, None, n, None, 0, 7, 1, POP)  # first_run = 7, count = 1 equals run 7 of the batch
    assert rc == 0 and b1 == 0 and o1[0].tolist() == out[7].tolist() and bits(c1[0]) == bits(costs[7])
    one = AC.start_tour(n, 3)
    check_population(ctx, xy, n, one, 1, 100, 3, [0, 1, 2])
    each = np.stack([AC.start_tour(n, 50 + r) for r in range(3)])
    check_population(ctx, xy, n, each, 3, 5, 3, [0, 1, 2])
    assert gpu_population(ctx, xy, None, n, None, 0, 0, 0, POP)[0] == 0  # count == 0: TL_OK, nothing written


def test_more_runs_than_one_launch_sequence(ctx):
    """the run is the grid's y: a sequence holds at most 65535 runs; at n = 3 with one ant a 65536th run goes in a second one"""
    n = 3
    xy = K.small(3)
    o = dict(AC.OPT, epochs=1, num_ants=1, seed=3)
    per = plan(ctx, n, 1, 10 ** 6)[0]
    assert per == 65535 and plan(ctx, 60, 6, 10, 3 * 60 * 60 * 4 * 2 + 8192)[0] == 2  # a small workspace bounds it, too
    out, costs = check_population(ctx, xy, n, None, 0, 0, per + 1, [0, per - 1, per], o)
    rc, o1, c1, _b, _ = gpu_population(ctx, xy, None, n, None, 0, per, 1, o)
    assert rc == 0 and o1[0].tolist() == out[per].tolist() and bits(c1[0]) == bits(costs[per])


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller():
    """stale matrices, tables and visited bits must not leak: the larger instance leaves its arrays where the smaller one's begin"""
    import teeline_amd as TA
    with TA.Context(0) as c:
        check_run(c, "m257x", AC.instance(257), None, 257, None, dict(AC.OPT, epochs=1, num_ants=70, seed=257, run=0))
        check_run(c, "epochs", K.small(8), None, 8, None, dict(AC.OPT, epochs=20, num_ants=5, seed=5, run=0))
        xy, packed, n, init, o = GOLDEN["gr17_matrix"]
        check_run(c, "gr17_matrix", xy, packed, n, init, o)


def test_errors(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    err = lambda: ctx.lib.tl_last_error(ctx.handle).decode()  # noqa: E731
    good = dict(AC.OPT, epochs=2, seed=1)
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 52
    assert gpu_trace(ctx, b["xy"], None, 52, bad, good)[0] == _capi.TL_ERR_BADARG and "permutation" in err()
    for key, values in (("alpha", (-0.5, float("nan"), float("inf"))), ("beta", (-0.1, 6.5, float("nan"))),
                        ("evaporation_rate", (0.0, 1.0, -1.0, 1.5, float("nan"))), ("num_ants", (0,))):
        for v in values:
            assert gpu_trace(ctx, b["xy"], None, 52, None, dict(good, **{key: v}))[0] == _capi.TL_ERR_BADARG and key in err(), (key, v)
    assert gpu_trace(ctx, b["xy"], None, 52, None, dict(good, num_ants=4097))[0] == _capi.TL_ERR_UNSUPPORTED and "num_ants" in err()
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    assert ctx.lib.tl_ant_colony(ctx.handle, None, 52, None, None, 2, 1.0, 2.0, 0.5, 25, 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_BADARG
    assert err() == "tl_ant_colony: NULL argument"
    assert gpu_population(ctx, b["xy"], None, 52, None, 0, 2 ** 32 - 3, 6, good)[0] == _capi.TL_ERR_BADARG
    assert err() == "tl_ant_colony_population: run ids beyond 2^32 - 1"
    assert gpu_population(ctx, b["xy"], None, 52, np.arange(104, dtype=np.uint32) % 52, 2, 0, 6, good)[0] == _capi.TL_ERR_BADARG and "init_count" in err()
    log, ln = np.zeros((4, 75), dtype=np.uint32), C.c_uint32()
    assert ctx.lib.tl_ant_colony_trace(ctx.handle, _vp(b["xy"]), 52, None, None, 2, 1.0, 2.0, 0.5, 25, 1, _vp(out), C.byref(cost), None, None, 4, C.byref(ln),
                                       None, 0, None) == _capi.TL_ERR_BADARG
    with TA.Context(0, 1 << 31) as odd:  # a bit no flag has
        assert gpu_trace(odd, b["xy"], None, 52, None, good)[0] == _capi.TL_ERR_UNSUPPORTED


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    AcoOptions = TA.ant_colony.AcoOptions
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    xy, _pk, n, init, o = GOLDEN["berlin52"]
    opts = AcoOptions(TA.HeuristicOptions(epochs=o["epochs"]))
    res = ACO.solve_cached(okey("berlin52", n, init, o), prob.xy, None, 52, None, **o)
    msgs = []
    sol = TA.ant_colony.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    want = ACO.messages(res, prob.ids)
    assert [k for k, _ in msgs] == [k for k, _ in want]
    for (k, p), (_k, w) in zip(msgs, want):
        if k == "PathUpdate":
            assert p[0] == w[0] and bits(p[1]) == bits(w[1])
        else:
            assert p == w
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    plain = TA.ant_colony.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == res["counters"]["improved"]
    short = AcoOptions(TA.HeuristicOptions(epochs=3), num_ants=10)
    so = dict(AC.OPT, epochs=3, num_ants=10, seed=1)
    msgs2 = []
    bestsol = TA.ant_colony.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [ACO.solve_cached(okey("mirror", 52, None, dict(so, run=r)), prob.xy, None, 52, None, **dict(so, run=r)) for r in range(4)]
    r = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r]["tour"]].tolist() and bits(bestsol.total) == bits(singles[r]["cost"])
    assert [k for k, _ in msgs2] == [k for k, _ in ACO.messages(singles[r])]
    steps = TA.pipeline.steps_for_solve("ant_colony")
    assert steps == ["shuffle", "ant_colony"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"ant_colony": short}, ctx=ctx, lk_seed=3)
    assert [x.name for x in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = ACO.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), **dict(so, seed=3))
    assert outs[-1].solution.route() == prob.ids[seeded["tour"]].tolist() and bits(outs[-1].solution.total) == bits(seeded["cost"])


def test_cli_equals_the_oracle(ctx):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "3", "--seed", "3", "--alpha", "1.5", "--beta", "2.5", "--evaporation-rate", "0.25", "--num-ants", "10"]
    o = dict(epochs=3, alpha=1.5, beta=2.5, evaporation_rate=0.25, num_ants=10, seed=3)
    r = subprocess.run([cli, "solve", "ant_colony", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    shuffled = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=3)[0].solution
    res = ACO.solve(prob.xy, None, 52, prob.positions_of(shuffled.route()), **o)
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()
    r = subprocess.run([cli, "solve", "ant_colony", "--no-seed", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    res = ACO.solve(prob.xy, None, 52, None, **o)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()
    r = subprocess.run([cli, "solve", "aco", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "ant_colony" in r.stderr
    # the C++ mirror's messages: PathUpdate(start) and one per improving ant, EpochUpdate per epoch, Done
    import re
    r = subprocess.run([cli, "solve", "ant_colony", "--no-seed", "--progress-digest", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=[0-9a-f]{16} epoch_updates=(\d+)", r.stderr)
    assert r.returncode == 0 and m, r.stderr
    assert [int(v) for v in m.groups()] == [len(res["routes"]), 0, 1, o["epochs"]]
    r = subprocess.run([cli, "solve", "ant_colony", "--no-seed", "--runs", "3", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    three = [ACO.solve(prob.xy, None, 52, None, **dict(o, run=k)) for k in range(3)]
    best = three[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(three)]))]
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(TA.Solution(best["cost"], prob.ids[best["tour"]], prob)).splitlines()


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """n = 130 with 65 ants on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the double-buffered tiles,
    the per-ant chunk of the second walk, two groups of ants"""
    from teeline_amd import _capi
    vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
    jctx = jitter_context({"tl_ant_colony_trace_run": [vp, vp, u32, vp, vp, u32, f32, f32, f32, u32, u64, u32, vp, C.POINTER(f32), C.POINTER(_capi.TlStats), vp, u32, C.POINTER(u32),
                                                       vp, u32, C.POINTER(u32)]})
    try:
        check_run(jctx, "jitter", AC.instance(130), None, 130, None, dict(AC.OPT, epochs=2, num_ants=65, seed=130, run=0))
    finally:
        jctx.close()
