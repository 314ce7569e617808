"""The genetic algorithm without a GPU: the numpy statement of the specification (tests/_ga_oracle.py) against the stand-alone C++
restatement (tests/probes/ga_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the crossover's recorded
examples, the roulette's two forms, the population-length sequence, the stale fitness of a mutated child; pipeline names."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _ga_cases as GC
import _ga_oracle as GA
import _sa_cases as K
import _sa_oracle as SA
from _swarm_oracle import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_ga.json")))
CASES = GC.golden_cases()


def trace_words(trace):
    return np.array([[b, bits(f), bits(c), ln] for b, f, c, ln in trace], dtype=np.uint32).reshape(-1, 4)


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ga") / "ga_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "ga_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, epochs, p, e, seed, run = CASES[name]
    return GA.solve_cached((name, seed, run), xy, packed, n, init, epochs=epochs, mutation_probability=p, n_elite=e, seed=seed, run=run)


def run_baseline(exe, tmp_path, xy, init, epochs, p, e, seed, run):
    tsp = str(tmp_path / "case.tsp")
    write_tsp(tsp, xy)
    args = [exe, tsp, "--trace", "--epochs", str(epochs), "--seed", str(seed), "--run", str(run), "--mutation-probability", repr(float(p)), "--n-elite", str(e)]
    if init is not None:
        ini = str(tmp_path / "case.init")
        open(ini, "w").write(" ".join(str(int(v)) for v in init) + "\n")
        args += ["--init", ini]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    head = [int(v) for v in lines[0].split()[:5]]
    return head, [int(v) for v in lines[1].split()], [[int(v) for v in ln.split()] for ln in lines[2:]]


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_oracle_equals_goldens(name):
    _xy, _packed, n, _init, epochs, _p, _e, _seed, _run = CASES[name]
    tour, cost, trace, cnt = oracle(name)
    want = GOLD["cases"][name]
    assert tour.tolist() == want["tour"] and bits(cost) == want["cost_bits"] and cnt == want["counters"]
    assert hashlib.sha256(trace_words(trace).astype("<u4").tobytes()).hexdigest() == want["trace_sha256"]
    assert trace_words(trace)[:8].tolist() == want["trace_head"]
    GC.check_conditions(name, n, epochs, trace, cnt)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, _n, init, epochs, p, e, seed, run = CASES[name]
    head, route, log = run_baseline(baseline, tmp_path, xy, init, epochs, p, e, seed, run)
    tour, cost, trace, cnt = oracle(name)
    want = GOLD["cases"][name]
    assert head == [epochs, cnt["children"], cnt["mutations"], cnt["improved"], bits(cost)] and bits(cost) == want["cost_bits"]
    assert route == tour.tolist() == want["tour"]
    assert log == trace_words(trace).tolist()


@pytest.mark.parametrize("n", [7, 8, 65])
@pytest.mark.parametrize("with_init", [False, True])
def test_cpp_restatement_on_random_instances(baseline, tmp_path, n, with_init):
    xy = K.synth(n, 500 + n)
    init = GC.start_tour(n, n) if with_init else None
    tour, cost, trace, cnt = GA.solve(xy, None, n, init, epochs=12, mutation_probability=0.3, n_elite=2, seed=n, run=3)
    head, route, log = run_baseline(baseline, tmp_path, xy, init, 12, 0.3, 2, n, 3)
    assert head == [12, cnt["children"], cnt["mutations"], cnt["improved"], bits(cost)] and route == tour.tolist() and log == trace_words(trace).tolist()


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--run", "5"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [GA.draw(77, 5, base + e, s) for base in (0, GA.INIT_EVENT) for e in range(8) for s in range(28)]


# ---------------------------------------------------------------- draws
def test_draws_are_the_annealing_stream_indexed_by_the_event():
    for seed, run, event, slot in ((1, 0, 0, 0), (9, 3, 12345, 21), (2 ** 64 - 1, 7, GA.init_event(1002, 1001, 1001), 26)):
        assert GA.draw(seed, run, event, slot) == SA.mix(SA.chain_key(seed, run) + SA.G * (32 * event + slot + 1))
        if event < 2 ** 32:
            assert GA.draw(seed, run, event, slot) == SA.draw(seed, run, event, slot)
    assert GA.pair_event(3, 52, 7, 2) == 4 * (3 * 52 + 7) + 2 and GA.init_event(52, 5, 9) == 2 ** 58 + 5 * 52 + 9
    # the largest generation event stays below the start population's range, whose 32-fold does not wrap
    assert GA.pair_event(2 ** 32 - 1, 65535, 32767, 3) < GA.INIT_EVENT and 32 * (GA.init_event(65535, 65534, 65534) + 1) < 2 ** 64


def test_draws_match_goldens_and_library(lib):
    for seed, run, event, slot, want in GOLD["draws"]:
        assert GA.draw(int(seed), run, int(event), slot) == int(want)
        assert lib.tl_ga_draw(int(seed), run, int(event), slot) == int(want)
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, run, event, slot = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 59)), int(rng.integers(0, 32))
        assert lib.tl_ga_draw(seed, run, event, slot) == GA.draw(seed, run, event, slot)
    assert lib.tl_sa_draw(1, 3, 138148, 21) == SA.draw(1, 3, 138148, 21)  # sa_spec.h's functions keep their results


@pytest.mark.parametrize("n,e,seeded", [(2, 0, False), (3, 0, False), (4, 1, False), (7, 0, False), (10, 3, True), (11, 2, True), (16, 20, True)])
def test_no_two_roles_share_an_event_and_slot(n, e, seeded):
    roles = GA.roles(n, e, 3, seeded)
    seen = {}
    for event, slot, role in roles:
        assert slot < 32 and seen.setdefault((event, slot), role) == role, (event, slot, role, seen[(event, slot)])
    assert len(seen) == len(set((ev, s) for ev, s, _ in roles))
    assert len({(ev, s) for ev, s, r in roles}) == len({(ev, s, r) for ev, s, r in roles})


# ---------------------------------------------------------------- crossover
PINS = [  # the reference's own unit tests' recorded examples, relabelled 0-based
    ([1, 2, 5, 3, 6, 4], [5, 1, 4, 3, 6, 2], 2, 4, [2, 5, 4, 3, 6, 1], [1, 4, 5, 3, 6, 2]),
    ([9, 8, 4, 5, 6, 7, 1, 3, 2, 0], [8, 7, 1, 2, 3, 0, 9, 5, 4, 6], 3, 5, [5, 6, 7, 2, 3, 0, 1, 9, 8, 4], [2, 3, 0, 5, 6, 7, 9, 4, 8, 1]),
]


def test_crossover_recorded_examples():
    for p1, p2, lo, hi, c1, c2 in PINS:
        z = min(p1)  # the first example is 1-based as recorded: relabel
        g1, g2 = GA.crossover([v - z for v in p1], [v - z for v in p2], lo, hi)
        assert [v + z for v in g1] == c1 and [v + z for v in g2] == c2


def test_crossover_edges():
    rng = np.random.default_rng(3)
    for n in (2, 3, 6, 9):
        p1, p2 = [int(v) for v in rng.permutation(n)], [int(v) for v in rng.permutation(n)]
        for lo in range(n):
            for hi in range(lo, n):
                g1, g2 = GA.crossover(p1, p2, lo, hi)
                assert sorted(g1) == sorted(g2) == list(range(n))
                assert g1[lo:hi + 1] == p2[lo:hi + 1] and g2[lo:hi + 1] == p1[lo:hi + 1]
                seg = set(p2[lo:hi + 1])
                rot = [p1[(hi + 1 + t) % n] for t in range(n)]
                assert [g1[(hi + 1 + t) % n] for t in range(n - (hi - lo + 1))] == [v for v in rot if v not in seg]
        assert GA.crossover(p1, p2, 0, n - 1) == (p2, p1)  # the whole route: the parents change places


# ---------------------------------------------------------------- roulette
def test_binary_search_equals_the_linear_roulette():
    cases = [[0.5, 0.25, 0.25, 0.0, 0.0, 0.125], [0.0, 0.0, 1.0], [1.0], [0.0, 0.0], [3e-5] * 40, [1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 0.5]]
    rng = np.random.default_rng(5)
    cases.append(sorted((np.float32(1.0) / rng.uniform(7000, 30000, size=300).astype(np.float32)).tolist(), reverse=True))
    for fits in cases:
        fits = [np.float32(f) for f in fits]
        prefix = GA.prefix_of(fits)
        assert (np.diff(prefix) >= 0).all()
        probes = set(float(v) for v in prefix) | {float(np.nextafter(v, np.float32(np.inf))) for v in prefix} | {
            float(np.nextafter(v, np.float32(-np.inf))) for v in prefix[1:]} | {float(prefix[-1]) * 2 + 1.0, float("inf")}
        probes |= {float(np.float32(u) * prefix[-1]) for u in rng.uniform(0, 1, size=50)}
        for r in sorted(probes):
            r = np.float32(r)
            assert GA.select_search(prefix, r) == GA.select_linear(fits, r), (fits[:6], r)
        assert GA.select_linear(fits, prefix[-1]) == len(fits) - 1 == GA.select_search(prefix, prefix[-1])  # r at the total: the last one


# ---------------------------------------------------------------- the generation loop
@pytest.mark.parametrize("n,e", [(8, 0), (8, 3), (9, 3), (9, 0), (8, 4), (9, 4), (8, 9), (3, 0), (2, 0), (10, 100)])
def test_population_lengths_and_permutations(n, e):
    xy = K.small(n) if n <= 8 else K.synth(n, 40 + n)
    tour, cost, trace, cnt, pops = GA.solve(xy, None, n, None, epochs=4, mutation_probability=0.5, n_elite=e, seed=2, keep=True)
    half = n // 2
    after = min(e, n) if e >= half else (n - e if n % 2 == 0 else n - 1 - e)
    assert [len(p) for p in pops] == [n] + [after] * 4 and [t[3] for t in trace] == [after] * 4
    for pop in pops:
        for _f, r in pop:
            assert sorted(r) == list(range(n))
    assert sorted(tour.tolist()) == list(range(n)) and cnt["children"] == 4 * 2 * max(0, half - e)
    if e >= half:  # elites only: nothing is drawn, the best stays
        assert cnt["mutations"] == 0 and len({t[1] for t in trace}) == 1


def test_a_mutated_child_keeps_its_stale_fitness():
    n = 8
    xy = K.small(n)
    d = GA.dist_fn(xy, None, n)
    _t, _c, _trace, cnt, pops = GA.solve(xy, None, n, None, epochs=3, mutation_probability=1.0, n_elite=0, seed=7, keep=True)
    assert cnt["mutations"] == cnt["children"] == 24
    stale = 0
    for pop in pops[1:]:
        for f, r in pop:
            stale += bits(f) != bits(GA.fitness_of(GA.tour_length(d, np.asarray(r))))
    assert stale >= 12, "most mutations change the length, and none may change the fitness"
    # without mutation every fitness is its route's
    _t, _c, _trace, _cnt, pops = GA.solve(xy, None, n, None, epochs=3, mutation_probability=0.0, n_elite=0, seed=7, keep=True)
    assert all(bits(f) == bits(GA.fitness_of(GA.tour_length(d, np.asarray(r)))) for pop in pops for f, r in pop)


def test_best_is_the_last_of_equals_and_epochs_zero():
    n = 6
    pk = GC.equal_matrix(n)
    tour, cost, trace, _cnt, pops = GA.solve(None, pk, n, None, epochs=2, mutation_probability=0.5, n_elite=1, seed=3, keep=True)
    assert cost == np.float32(n) and [t[0] for t in trace] == [len(pops[1]) - 1] * 2 and tour.tolist() == pops[-1][-1][1]
    assert GA.best_of([(1.0, []), (2.0, []), (2.0, []), (0.5, [])]) == 2
    tour0, cost0, trace0, cnt0, pops0 = GA.solve(K.small(8), None, 8, None, epochs=0, seed=3, keep=True)
    assert trace0 == [] and cnt0["children"] == 0 and tour0.tolist() == pops0[0][GA.best_of(pops0[0])][1]


def test_small_n_as_the_reference_behaves():
    one = np.zeros((1, 2), dtype=np.float32)
    tour, cost, trace, _ = GA.solve(one, None, 1, None, epochs=3, n_elite=3, seed=1)
    assert tour.tolist() == [0] and cost == 0 and [t[3] for t in trace] == [1, 1, 1]
    assert GA.solve(one, None, 1, None, epochs=0, n_elite=0, seed=1)[0].tolist() == [0]
    with pytest.raises(ValueError, match="empty population"):
        GA.solve(one, None, 1, None, epochs=1, n_elite=0, seed=1)
    with pytest.raises(ValueError, match="empty population"):
        GA.solve(one[:0], None, 0, None, epochs=1, seed=1)
    with pytest.raises(ValueError, match="empty range"):  # every city in one place: total fitness 0
        GA.solve(np.zeros((4, 2), dtype=np.float32), None, 4, None, epochs=1, n_elite=0, seed=1)
    for n in (2, 3):
        tour, _cost, trace, cnt = GA.solve(K.small(n), None, n, None, epochs=3, n_elite=0, mutation_probability=0.5, seed=1)
        assert sorted(tour.tolist()) == list(range(n)) and [t[3] for t in trace] == [2, 2, 2] and cnt["children"] == 6


def test_start_population_with_an_initial_tour():
    n = 20
    xy = K.synth(n, 20)
    init = GC.start_tour(n, 1)
    pop = GA.start_population(GA.dist_fn(xy, None, n), GA.chain_key(5, 0), n, init)
    assert len(pop) == n and pop[0][1] == init.tolist()
    for i in range(1, 4):  # n / 5 = 4 seeded individuals: the tour after 2 .. 4 reversals
        want = init.tolist()
        for m in range(2 + GA.position(GA.draw(5, 0, GA.init_event(n, i, 0), GA.SLOT_COUNT), 3)):
            lo, hi = SA.pair_from_key(GA.chain_key(5, 0), GA.init_event(n, i, 1 + m), n)
            want[lo:hi + 1] = want[lo:hi + 1][::-1]
        assert pop[i][1] == want != init.tolist()
    assert all(sorted(r) == list(range(n)) for _f, r in pop)
    counts = {2 + GA.position(GA.draw(5, 0, GA.init_event(n, i, 0), GA.SLOT_COUNT), 3) for i in range(1, 200)}
    assert counts == {2, 3, 4}


# ---------------------------------------------------------------- plan, limits, names
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    per, t, need = C.c_uint32(), C.c_int(), C.c_uint64()
    lds, work = 163840, 8 << 30
    assert lib.tl_genetic_algorithm_plan(52, 1, 256, lds, work, C.byref(per), C.byref(t), C.byref(need)) == 0
    assert per.value == 65535 and t.value == 128 and 4 * 52 * 52 <= need.value <= 4 * 52 * 52 + 4096
    assert lib.tl_genetic_algorithm_plan(1002, 64, 256, lds, work, C.byref(per), C.byref(t), C.byref(need)) == 0
    assert t.value == 256 and 2000 <= per.value <= work // (4 * 1002 * 1002) and 64 * 4 * 1002 * 1002 <= need.value <= 64 * 4 * 1002 * 1002 * 1.01
    # the workspace bounds what one launch sequence holds: a run's populations are 4 n^2 bytes
    assert lib.tl_genetic_algorithm_plan(1000, 10 ** 6, 256, lds, 10 * 4_100_000, C.byref(per), C.byref(t), C.byref(need)) == 0 and 9 <= per.value <= 10
    top = (lds - 480) // 14
    assert lib.tl_genetic_algorithm_plan(top, 1, 256, lds, 1 << 40, C.byref(per), C.byref(t), C.byref(need)) == 0 and per.value >= 1 and t.value == 256
    for n, w in ((top + 1, 1 << 40), (0, work), (1000, 1000)):
        assert lib.tl_genetic_algorithm_plan(n, 1, 256, lds, w, C.byref(per), C.byref(t), C.byref(need)) == 0
        assert (per.value, t.value, need.value) == (0, 0, 0)
    assert lib.tl_genetic_algorithm_plan(52, 1, 0, lds, work, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_genetic_algorithm_max_n(None) == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["genetic_algorithm"] == "genetic_algorithm" and "ga" not in P.SOLVER_NAMES
    assert P.steps_for_solve("genetic_algorithm") == ["shuffle", "genetic_algorithm"] and P.steps_for_solve("Genetic_Algorithm", no_seed=True) == ["genetic_algorithm"]
    with pytest.raises(ValueError, match="the seeded genetic algorithm of this build is `genetic_algorithm`"):
        P.steps_for_solve("ga")
    with pytest.raises(ValueError, match="the seeded genetic algorithm of this build is `genetic_algorithm`"):
        P.run_pipeline_stages(None, ["ga"])
    assert P.steps_for_solve("tabu_search") == ["nn", "tabu_search"] and P.steps_for_solve("simulated_annealing") == ["shuffle", "simulated_annealing"]


def test_options_validate():
    from teeline_amd.host.genetic_algorithm import GAOptions
    assert (GAOptions().epochs, GAOptions().mutation_probability, GAOptions().n_elite) == (10_000, 0.001, 3)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mutation_probability"):
            GAOptions(mutation_probability=bad).validate()
    GAOptions(mutation_probability=1.0).validate()


def test_header_and_bindings_agree_on_the_symbols(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_genetic_algorithm", "tl_genetic_algorithm_trace", "tl_genetic_algorithm_trace_run", "tl_genetic_algorithm_population",
                "tl_genetic_algorithm_max_n", "tl_genetic_algorithm_plan", "tl_ga_draw", "tl_ga_selftest_crossover"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)


# ---------------------------------------------------------------- the conditions of the cases past two rounds / one thread each
def test_wide_and_rank_cases_are_what_they_claim(lib):
    per, t, need = C.c_uint32(), C.c_int(), C.c_uint64()
    w, r = GC.WIDE, GC.RANK
    assert lib.tl_genetic_algorithm_plan(w["n"], 1, GC.CUS, GC.LDS_BYTES, GC.WORK, C.byref(per), C.byref(t), C.byref(need)) == 0
    assert GC.rounds(w["n"], t.value) >= 3 and all(GC.rounds(n, t.value) >= 2 for n in GC.CROSS_SIZES) and GC.rounds(GC.CROSS_SIZES[2], t.value) == 3
    for n in GC.CROSS_SIZES:  # every boundary the segments are meant to sit on is there
        segs = GC.crossover_segments(n)
        assert {(0, n - 1), (0, 0), (n - 1, n - 1)} <= set(segs) and all(0 <= lo <= hi < n for lo, hi in segs)
        for v in (255, 256, 257, 511, 512):
            if v < n:
                assert any(lo == v for lo, _hi in segs) and any(hi == v for _lo, hi in segs), (n, v)
    for init in (None, GC.start_tour(w["n"], w["n"])):
        _tour, _cost, trace, cnt = GA.solve_cached(("wide", init is not None), GC.instance(w["n"]), None, w["n"], init, epochs=w["epochs"],
                                                   mutation_probability=w["p"], n_elite=w["e"], seed=w["seed"])
        assert cnt["children"] == 2 * (w["n"] // 2 - w["e"]) * w["epochs"] and 0 < cnt["mutations"] < cnt["children"]
        assert [ln for *_x, ln in trace] == [w["e"] + 2 * (w["n"] // 2 - w["e"])] * w["epochs"]
    # the first rank sees n > 1024 individuals, the second the next generation's n - 3
    _tour, _cost, trace, cnt = GA.solve_cached("rank", GC.instance(r["n"]), None, r["n"], None, epochs=r["epochs"], mutation_probability=r["p"],
                                               n_elite=r["e"], seed=r["seed"])
    assert r["n"] > 1024 and [ln for *_x, ln in trace] == [r["n"] - 3] and r["n"] - 3 > 1024 and cnt["children"] == r["n"] - 6
