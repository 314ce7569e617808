"""The genetic algorithm on the GPU (tl_genetic_algorithm*, csrc/genetic.hip) against the numpy statement of its specification
(tests/_ga_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every entry of the
per-generation trace (best index, fitness bits — which pin the sequential sums and the division —, recomputed tour_length bits,
population length), the route log and the stats against the oracle's counters — in both input forms and for the runs of a batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _ga_cases as GC
import _ga_oracle as GA
from _raw_context import _vp, jitter_context
import _sa_cases as K
from _swarm_oracle import bits
from test_ga_oracle import PINS

pytestmark = pytest.mark.gpu

WORK = 8 << 30  # the workspace the entries plan with (include/teeline_gpu.h)


def gpu_trace(ctx, xy, packed, n, init, epochs, p, e, seed, run=0, cap=None, route_cap=None):
    from teeline_amd import _capi
    cap = epochs if cap is None else cap
    route_cap = epochs if route_cap is None else route_cap
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.zeros((max(cap, 1), 4), dtype=np.uint32)
    routes = np.full((max(route_cap, 1), max(n, 1)), 0xFFFFFFFF, dtype=np.uint32)
    cost, ln, st = C.c_float(-1.0), C.c_uint32(), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_genetic_algorithm_trace_run(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), epochs, p, e, seed, run, _vp(out), C.byref(cost), C.byref(st),
                                                _vp(log), cap, C.byref(ln), _vp(routes), route_cap)
    return rc, out[:n], np.float32(cost.value), log[:min(ln.value, cap)], ln.value, st.as_dict(), routes[:min(ln.value, route_cap)]


def gpu_population(ctx, xy, packed, n, init, first, count, epochs, p, e, seed):
    from teeline_amd import _capi
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_genetic_algorithm_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), first, count, epochs, p, e, seed, _vp(out), _vp(costs),
                                                 C.byref(best), C.byref(st))
    return rc, out, costs, best.value, st.as_dict()


def want_trace(trace):
    return [(b, bits(f), bits(c), ln) for b, f, c, ln in trace]


def check_run(ctx, key, xy, packed, n, init, epochs, p, e, seed, run=0):
    """one run against the oracle: tour, cost, every trace entry, every logged route, stats"""
    tour, cost, trace, cnt, pops = GA.solve_cached((key, n, epochs, p, e, seed, run), xy, packed, n, init, epochs=epochs, mutation_probability=p, n_elite=e,
                                                   seed=seed, run=run, keep=True)
    rc, out, gcost, glog, ln, st, routes = gpu_trace(ctx, xy, packed, n, init, epochs, p, e, seed, run)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert ln == epochs == len(trace), (key, ln)
    got = [tuple(int(v) for v in r) for r in glog]
    first_diff = next((i for i, (g, w) in enumerate(zip(got, want_trace(trace))) if g != w), None)
    assert first_diff is None, (key, first_diff, got[first_diff], want_trace(trace)[first_diff])
    for g, (b, _f, _c, _l) in enumerate(trace):
        assert routes[g].tolist() == pops[g + 1][b][1], (key, g)
    assert out.tolist() == tour.tolist(), key
    assert bits(gcost) == bits(cost), (key, gcost, cost)
    assert (st["sweeps"], st["candidates"], st["moves"], st["reversed"]) == (epochs, cnt["children"], cnt["improved"], cnt["mutations"]), (key, st, cnt)
    return trace, cnt


def plan(ctx, n, count=1):
    info = ctx.device_info()
    per, t, need = C.c_uint32(), C.c_int(), C.c_uint64()
    assert ctx.lib.tl_genetic_algorithm_plan(n, count, info["cus"], info["lds_bytes"], WORK, C.byref(per), C.byref(t), C.byref(need)) == 0
    return per.value, t.value, need.value


# ---------------------------------------------------------------- the device crossover
def device_crossover(ctx, p1, p2, lo, hi):
    n = len(p1)
    a, b = np.ascontiguousarray(p1, dtype=np.uint32), np.ascontiguousarray(p2, dtype=np.uint32)
    o1, o2 = np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    rc = ctx.lib.tl_ga_selftest_crossover(ctx.handle, _vp(a), _vp(b), n, lo, hi, _vp(o1), _vp(o2))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    return o1.tolist(), o2.tolist()


def test_selftest_crossover_recorded_examples(ctx):
    for p1, p2, lo, hi, c1, c2 in PINS:
        z = min(p1)
        g1, g2 = device_crossover(ctx, [v - z for v in p1], [v - z for v in p2], lo, hi)
        assert [v + z for v in g1] == c1 and [v + z for v in g2] == c2


def _random_parents(n):
    rng = np.random.default_rng(n)
    return [int(v) for v in rng.permutation(n)], [int(v) for v in rng.permutation(n)]


@pytest.mark.parametrize("n", [2, 3, 8, 63, 64, 65, 129, 257])
def test_selftest_crossover_random_parents(ctx, n):
    """n = 63 .. 65, 129, 257: the wave and workgroup edges of the compaction"""
    p1, p2 = _random_parents(n)
    if n <= 8:
        pairs = [(lo, hi) for lo in range(n) for hi in range(lo, n)]
    else:
        pairs = [(0, n - 1), (0, 0), (n - 1, n - 1), (0, 1), (n - 2, n - 1), (0, n - 2), (1, n - 1), (n // 2, n // 2), (1, n - 2), (62, 64), (63, 63), (0, 63)]
        pairs = [(lo, hi) for lo, hi in pairs if hi < n]
    for lo, hi in pairs:
        want = GA.crossover(p1, p2, lo, hi)
        assert device_crossover(ctx, p1, p2, lo, hi) == want, (n, lo, hi)
    from teeline_amd import _capi
    o = np.zeros(n, dtype=np.uint32)
    a = np.ascontiguousarray(p1, dtype=np.uint32)
    assert ctx.lib.tl_ga_selftest_crossover(ctx.handle, _vp(a), _vp(a), n, 1, 0, _vp(o), _vp(o)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_ga_selftest_crossover(ctx.handle, _vp(a), _vp(a), n, 0, n, _vp(o), _vp(o)) == _capi.TL_ERR_BADARG


@pytest.mark.parametrize("n", GC.CROSS_SIZES + ("top",))
def test_selftest_crossover_past_two_rounds(ctx, n):
    """n > 512 on 256 threads: the compaction's third and later rounds use the first set of wave counts again; n = 511 .. 513 its edge;
    the largest n the algorithm takes.  Segments on the workgroup's widths (GC.crossover_segments)."""
    if n == "top":
        n = ctx.lib.tl_genetic_algorithm_max_n(ctx.handle)
        assert 4097 < n <= 65535
    assert plan(ctx, n)[1] == 256
    p1, p2 = _random_parents(n)
    for lo, hi in GC.crossover_segments(n):
        assert device_crossover(ctx, p1, p2, lo, hi) == GA.crossover(p1, p2, lo, hi), (n, lo, hi)


# ---------------------------------------------------------------- whole runs
GOLDEN = GC.golden_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    xy, packed, n, init, epochs, p, e, seed, run = GOLDEN[name]
    trace, cnt = check_run(ctx, name, xy, packed, n, init, epochs, p, e, seed, run)
    GC.check_conditions(name, n, epochs, trace, cnt)


def instance(n):
    return K.tsplib("berlin52")["xy"] if n == 52 else K.small(n) if n <= 8 else K.synth(n, 700 + n)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 7, 8, 52, 65])
def test_sizes_elites_and_probabilities(ctx, n):
    xy = instance(n)
    for e in sorted({0, 3, n // 2, n + 1}):
        for p in (0.0, 0.5, 1.0):
            for init in (None, GC.start_tour(n, n)):
                check_run(ctx, ("size", init is not None), xy, None, n, init, 2 if n >= 52 else 6, p, e, 11 + n)


@pytest.mark.parametrize("n,epochs", [(257, 3), (280, 3)])
def test_beyond_one_workgroup_width(ctx, n, epochs):
    xy = instance(n)
    check_run(ctx, "wide", xy, None, n, None, epochs, 0.5, 3, n)
    check_run(ctx, "wide_init", xy, None, n, GC.start_tour(n, n), epochs, 0.5, 0, n)


def test_whole_runs_past_two_compaction_rounds(ctx):
    """n = 520: three compaction rounds per child; with and without a start tour, and once as a packed matrix"""
    from teeline_amd import _capi
    w = GC.WIDE
    n, xy = w["n"], GC.instance(w["n"])
    assert GC.rounds(n, plan(ctx, n)[1]) >= 3
    for init in (None, GC.start_tour(n, n)):
        want = GA.solve_cached(("wide", init is not None), xy, None, n, init, epochs=w["epochs"], mutation_probability=w["p"], n_elite=w["e"], seed=w["seed"])
        rc, out, gcost, glog, ln, st, _routes = gpu_trace(ctx, xy, None, n, init, w["epochs"], w["p"], w["e"], w["seed"])
        assert rc == 0 and ln == w["epochs"] and [tuple(int(v) for v in r) for r in glog] == want_trace(want[2]), init is not None
        assert out.tolist() == want[0].tolist() and bits(gcost) == bits(want[1])
        assert (st["candidates"], st["moves"], st["reversed"]) == (want[3]["children"], want[3]["improved"], want[3]["mutations"])
    check_run(ctx, "wide_routes", xy, None, n, None, w["epochs"], w["p"], w["e"], w["seed"])  # and every logged route
    pk = np.empty(n * (n - 1) // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), n, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    want = GA.solve_cached(("wide", False), xy, None, n, None, epochs=w["epochs"], mutation_probability=w["p"], n_elite=w["e"], seed=w["seed"])
    rc, out, gcost, glog, ln, _st, _routes = gpu_trace(ctx, None, pk, n, None, w["epochs"], w["p"], w["e"], w["seed"])
    assert rc == 0 and out.tolist() == want[0].tolist() and bits(gcost) == bits(want[1]) and [tuple(int(v) for v in r) for r in glog] == want_trace(want[2])


def test_rank_past_one_thread_per_individual(ctx):
    """n = 1030, one generation, three elites: 1030 individuals ranked by 1024 threads, then the 1027 of the next generation"""
    r = GC.RANK
    n, xy = r["n"], GC.instance(r["n"])
    want = GA.solve_cached("rank", xy, None, n, None, epochs=r["epochs"], mutation_probability=r["p"], n_elite=r["e"], seed=r["seed"])
    rc, out, gcost, glog, ln, st, _routes = gpu_trace(ctx, xy, None, n, None, r["epochs"], r["p"], r["e"], r["seed"])
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert ln == 1 and [tuple(int(v) for v in x) for x in glog] == want_trace(want[2]) and want[2][0][3] == n - 3 > 1024
    assert out.tolist() == want[0].tolist() and bits(gcost) == bits(want[1])
    assert (st["sweeps"], st["candidates"], st["moves"], st["reversed"]) == (1, want[3]["children"], want[3]["improved"], want[3]["mutations"])


@pytest.mark.parametrize("epochs", [0, 1, 2, 50])
def test_epochs(ctx, epochs):
    xy = K.small(8)
    check_run(ctx, "epochs", xy, None, 8, None, epochs, 0.5, 3, 5)
    check_run(ctx, "epochs_init", xy, None, 8, GC.start_tour(8, 2), epochs, 0.5, 0, 5)


def test_one_city(ctx):
    from teeline_amd import _capi
    one = np.zeros((1, 2), dtype=np.float32)
    for epochs, e in ((0, 0), (0, 3), (3, 1), (3, 7)):
        check_run(ctx, "one", one, None, 1, None, epochs, 0.5, e, 1)
    assert gpu_trace(ctx, one, None, 1, None, 1, 0.5, 0, 1)[0] == _capi.TL_ERR_REF_PANICS and "empty population" in ctx.lib.tl_last_error(ctx.handle).decode()
    assert gpu_trace(ctx, one, None, 0, None, 1, 0.5, 3, 1)[0] == _capi.TL_ERR_REF_PANICS
    zero = np.zeros((4, 2), dtype=np.float32)  # every city in one place: total fitness 0, the roulette's range is empty
    assert gpu_trace(ctx, zero, None, 4, None, 2, 0.5, 0, 1)[0] == _capi.TL_ERR_REF_PANICS and "empty range" in ctx.lib.tl_last_error(ctx.handle).decode()
    assert gpu_trace(ctx, zero, None, 4, None, 2, 0.5, 2, 1)[0] == 0  # elites only: no roulette, as in the reference


def test_matrix_form_equals_coordinate_form(ctx):
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    pk = np.empty(52 * 51 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(b["xy"]), 52, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    xy, _packed, n, init, epochs, p, e, seed, run = GOLDEN["berlin52"]
    tour, cost, trace, _cnt = GA.solve_cached(("berlin52_plain", seed, run), xy, None, n, init, epochs=epochs, mutation_probability=p, n_elite=e, seed=seed, run=run)
    rc, out, gcost, glog, ln, _st, _routes = gpu_trace(ctx, None, pk, 52, None, epochs, p, e, seed)
    assert rc == 0 and out.tolist() == tour.tolist() and bits(gcost) == bits(cost) and ln == epochs
    assert [tuple(int(v) for v in r) for r in glog] == want_trace(trace)


def test_all_distances_equal_pins_the_stable_rank_and_the_last_of_equals(ctx):
    for n, e in ((6, 1), (17, 3), (66, 3)):
        pk = GC.equal_matrix(n)
        trace, _cnt = check_run(ctx, "equal", None, pk, n, None, 4, 0.5, e, n)
        assert all(b == ln - 1 and c == np.float32(n) for b, _f, c, ln in trace)


def test_ring6_explicit(ctx):
    import _tsplib
    inst = _tsplib.parse_tsplib(os.path.join(K.TSPLIB, "ring6_explicit.tsp"))
    assert inst["n"] == 6
    check_run(ctx, "ring6", None, inst["packed"], 6, None, 20, 0.5, 1, 6)


def test_plain_entry_and_truncated_trace(ctx):
    from teeline_amd import _capi
    xy, _packed, n, init, epochs, p, e, seed, run = GOLDEN["berlin52"]
    tour, cost, trace, cnt, pops = GA.solve_cached(("berlin52", n, epochs, p, e, seed, run), xy, None, n, init, epochs=epochs, mutation_probability=p, n_elite=e,
                                                   seed=seed, run=run, keep=True)
    out, gcost, st = np.zeros(52, dtype=np.uint32), C.c_float(), _capi.TlStats()
    assert ctx.lib.tl_genetic_algorithm(ctx.handle, _vp(xy), 52, None, None, epochs, p, e, seed, _vp(out), C.byref(gcost), C.byref(st)) == 0
    assert out.tolist() == tour.tolist() and bits(gcost.value) == bits(cost)
    assert (st.sweeps, st.candidates, st.moves, st.reversed) == (epochs, cnt["children"], cnt["improved"], cnt["mutations"])
    rc, out2, _c, glog, ln, _st, routes = gpu_trace(ctx, xy, None, 52, None, epochs, p, e, seed, cap=5, route_cap=2)  # truncation is reported
    assert rc == 0 and ln == epochs and len(glog) == 5 and len(routes) == 2 and out2.tolist() == tour.tolist()
    assert [tuple(int(v) for v in r) for r in glog] == want_trace(trace)[:5] and routes[1].tolist() == pops[2][trace[1][0]][1]
    log1, ln1 = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()  # tl_genetic_algorithm_trace is run 0, the route log optional
    assert ctx.lib.tl_genetic_algorithm_trace(ctx.handle, _vp(xy), 52, None, None, epochs, p, e, seed, _vp(out), C.byref(gcost), None, _vp(log1), 4,
                                              C.byref(ln1), None, 0) == 0
    assert ln1.value == epochs and log1.tolist() == glog[:4].tolist()


# ---------------------------------------------------------------- batches
POP = dict(epochs=3, p=0.5, e=1, seed=31)


def check_population(ctx, xy, n, init, first, count, sample):
    rc, out, costs, best, st = gpu_population(ctx, xy, None, n, init, first, count, POP["epochs"], POP["p"], POP["e"], POP["seed"])
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        tour, cost, _trace, _cnt = GA.solve_cached(("pop", n, None if init is None else tuple(int(v) for v in init), first + r), xy, None, n, init,
                                                   epochs=POP["epochs"], mutation_probability=POP["p"], n_elite=POP["e"], seed=POP["seed"], run=first + r)
        assert out[r].tolist() == tour.tolist() and bits(costs[r]) == bits(cost), (count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == POP["epochs"] * count and st["candidates"] == 2 * (n // 2 - POP["e"]) * POP["epochs"] * count
    return out, costs


def test_batches(ctx):
    b = K.tsplib("berlin52")
    check_population(ctx, b["xy"], 52, None, 0, 1, [0])
    check_population(ctx, b["xy"], 52, None, 0, 3, [0, 1, 2])
    check_population(ctx, b["xy"], 52, GC.start_tour(52, 9), 100, 3, [0, 1, 2])
    n = 4
    xy = K.small(n)
    per, _t, _need = plan(ctx, n, 10 ** 6)
    assert 1 <= per <= 65535
    count = per + 1  # one more than a launch sequence holds: a second sequence
    out, costs = check_population(ctx, xy, n, None, 0, count, [0, 1, per - 1, per])
    for c in (per - 1, per):  # first_run = c, count = 1 equals run c of the batch
        rc, o1, c1, b1, _ = gpu_population(ctx, xy, None, n, None, c, 1, POP["epochs"], POP["p"], POP["e"], POP["seed"])
        assert rc == 0 and b1 == 0 and o1[0].tolist() == out[c].tolist() and bits(c1[0]) == bits(costs[c])
    assert gpu_population(ctx, xy, None, n, None, 0, 0, 3, 0.5, 1, 31)[0] == 0  # count == 0: TL_OK, nothing written


def test_best_index_tie_rule(ctx):
    """all distances 1: every run costs n exactly, and equal costs go to the lower run"""
    from teeline_amd import _capi
    n, count = 6, 5
    pk = GC.equal_matrix(n)
    out = np.zeros((count, n), dtype=np.uint32)
    costs, best = np.zeros(count, dtype=np.float32), C.c_uint32(99)
    assert ctx.lib.tl_genetic_algorithm_population(ctx.handle, None, n, _vp(pk), None, 0, count, 2, 0.5, 1, 3, _vp(out), _vp(costs), C.byref(best), None) == 0
    assert best.value == 0 and [bits(c) for c in costs] == [bits(6.0)] * count and _capi.TL_OK == 0


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller():
    """stale populations, orders and prefixes must not leak: the larger instance leaves its arrays where the smaller one's begin"""
    import teeline_amd as TA
    with TA.Context(0) as c:
        check_run(c, "wide", instance(257), None, 257, None, 3, 0.5, 3, 257)
        check_run(c, "epochs", K.small(8), None, 8, None, 50, 0.5, 3, 5)
        xy, packed, n, init, epochs, p, e, seed, run = GOLDEN["gr17_matrix"]
        check_run(c, "gr17_matrix", xy, packed, n, init, epochs, p, e, seed, run)


def test_errors(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    err = lambda: ctx.lib.tl_last_error(ctx.handle).decode()  # noqa: E731
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 52
    assert gpu_trace(ctx, b["xy"], None, 52, bad, 3, 0.5, 3, 1)[0] == _capi.TL_ERR_BADARG and "permutation" in err()
    for p in (-0.25, 1.5, float("nan"), float("inf")):
        assert gpu_trace(ctx, b["xy"], None, 52, None, 3, p, 3, 1)[0] == _capi.TL_ERR_BADARG and "mutation_probability" in err()
    # just above the limit: refused before anything of size n is read (the arrays passed hold 52 cities)
    top = ctx.lib.tl_genetic_algorithm_max_n(ctx.handle)
    assert 0 < top <= 65535 and plan(ctx, top)[0] >= 1 and plan(ctx, top + 1) == (0, 0, 0)
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    rc = ctx.lib.tl_genetic_algorithm(ctx.handle, _vp(b["xy"]), top + 1, None, None, 5, 0.5, 3, 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "exceeds the limit" in err()
    assert ctx.lib.tl_genetic_algorithm(ctx.handle, None, 52, None, None, 5, 0.5, 3, 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_BADARG
    assert err() == "tl_genetic_algorithm: NULL argument"
    assert gpu_population(ctx, b["xy"], None, 52, None, 2 ** 32 - 3, 6, 3, 0.5, 3, 1)[0] == _capi.TL_ERR_BADARG
    assert err() == "tl_genetic_algorithm_population: run ids beyond 2^32 - 1"
    log, ln = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()
    assert ctx.lib.tl_genetic_algorithm_trace(ctx.handle, _vp(b["xy"]), 52, None, None, 5, 0.5, 3, 1, _vp(out), C.byref(cost), None, None, 4, C.byref(ln), None,
                                              0) == _capi.TL_ERR_BADARG
    with TA.Context(0, 1 << 31) as odd:  # a bit no flag has
        assert gpu_trace(odd, b["xy"], None, 52, None, 5, 0.5, 3, 1)[0] == _capi.TL_ERR_UNSUPPORTED


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    GAOptions = TA.genetic_algorithm.GAOptions
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    opts = GAOptions(TA.HeuristicOptions(epochs=50), mutation_probability=0.5, n_elite=3)
    tour, cost, trace, cnt, pops = GA.solve_cached(("berlin52", 52, 50, 0.5, 3, 1, 0), prob.xy, None, 52, None, epochs=50, mutation_probability=0.5, n_elite=3,
                                                   seed=1, run=0, keep=True)
    msgs = []
    sol = TA.genetic_algorithm.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    assert [k for k, _ in msgs] == ["PathUpdate"] * 51 + ["Done"]  # one per generation, then the final one, then Done
    for g, (b, _f, c, _l) in enumerate(trace):
        assert msgs[g][1][0] == prob.ids[np.asarray(pops[g + 1][b][1])].tolist() and bits(msgs[g][1][1]) == bits(c)
    assert msgs[-2][1][0] == sol.route() == prob.ids[tour].tolist() and bits(msgs[-2][1][1]) == bits(sol.total) == bits(cost)
    plain = TA.genetic_algorithm.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == cnt["improved"] and plain.stats["reversed"] == cnt["mutations"]
    # runs > 1: the best run, and its own replay
    short = GAOptions(TA.HeuristicOptions(epochs=5), mutation_probability=0.5, n_elite=3)
    msgs2 = []
    bestsol = TA.genetic_algorithm.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [GA.solve_cached(("berlin52", 52, 5, 0.5, 3, 1, r), prob.xy, None, 52, None, epochs=5, mutation_probability=0.5, n_elite=3, seed=1, run=r, keep=True)
               for r in range(4)]
    r = int(np.argmin([(bits(s[1]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r][0]].tolist() and bits(bestsol.total) == bits(singles[r][1])
    assert len(msgs2) == 5 + 2 and msgs2[-2][1][0] == bestsol.route()
    # the pipeline: `solve genetic_algorithm` is shuffle -> genetic_algorithm, the stage draws from the pipeline's one seed
    steps = TA.pipeline.steps_for_solve("genetic_algorithm")
    assert steps == ["shuffle", "genetic_algorithm"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"genetic_algorithm": short}, ctx=ctx, lk_seed=3)
    assert [o.name for o in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = GA.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), epochs=5, mutation_probability=0.5, n_elite=3, seed=3)
    assert outs[-1].solution.route() == prob.ids[seeded[0]].tolist() and bits(outs[-1].solution.total) == bits(seeded[1])
    outs3 = TA.pipeline.run_pipeline_stages(prob, ["shuffle", "genetic_algorithm", "2opt"], {"genetic_algorithm": short}, ctx=ctx, lk_seed=3)
    assert outs3[-1].solution.total <= outs[-1].solution.total and TA.validate_tour(outs3[-1].solution.route(), prob)


def test_cli_equals_the_oracle(ctx):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "5", "--seed", "3", "--mutation-probability", "0.5", "--n-elite", "3"]
    r = subprocess.run([cli, "solve", "genetic_algorithm", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    shuffled = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=3)[0].solution
    tour, cost, _trace, _cnt = GA.solve(prob.xy, None, 52, prob.positions_of(shuffled.route()), epochs=5, mutation_probability=0.5, n_elite=3, seed=3)
    want = TA.pipeline.format_solution(TA.Solution(cost, prob.ids[tour], prob))
    assert r.stdout.splitlines()[-2:] == want.splitlines()
    r = subprocess.run([cli, "solve", "genetic_algorithm", "--no-seed", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    tour, cost, _trace, _cnt = GA.solve(prob.xy, None, 52, None, epochs=5, mutation_probability=0.5, n_elite=3, seed=3)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(TA.Solution(cost, prob.ids[tour], prob)).splitlines()
    r = subprocess.run([cli, "pipeline", "--steps=shuffle,genetic_algorithm,2opt", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    outs = TA.pipeline.run_pipeline_stages(prob, ["shuffle", "genetic_algorithm", "2opt"],
                                           {"genetic_algorithm": TA.genetic_algorithm.GAOptions(TA.HeuristicOptions(epochs=5), 0.5, 3)}, ctx=ctx, lk_seed=3)
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(outs[-1].solution).splitlines()
    r = subprocess.run([cli, "solve", "ga", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "genetic_algorithm" in r.stderr


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """Runs on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the compaction's double-buffered wave counts"""
    from teeline_amd import _capi
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    jctx = jitter_context({"tl_genetic_algorithm_trace_run": [vp, vp, u32, vp, vp, u32, C.c_float, u32, u64, u32, vp, C.POINTER(C.c_float), C.POINTER(_capi.TlStats), vp, u32,
                                                              C.POINTER(u32), vp, u32]})
    try:
        check_run(jctx, "wide", instance(257), None, 257, None, 3, 0.5, 3, 257)
        check_run(jctx, "epochs", K.small(8), None, 8, None, 50, 0.5, 3, 5)
        xy, packed, n, init, epochs, p, e, seed, run = GOLDEN["synth65_init"]
        check_run(jctx, "synth65_init", xy, packed, n, init, epochs, p, e, seed, run)
        w = GC.WIDE  # three compaction rounds per child: the first set of wave counts is used again
        check_run(jctx, "wide_routes", GC.instance(w["n"]), None, w["n"], None, w["epochs"], w["p"], w["e"], w["seed"])
    finally:
        jctx.close()
