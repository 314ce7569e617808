"""Tabu search without a GPU: the numpy statement of the specification (tests/_tabu_oracle.py) against the stand-alone C++
restatement (tests/probes/tabu_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the list's FIFO semantics
and the reference's own unit tests of it (tabu_search.rs:128-160); pipeline names of the Python mirror; the new flag's value."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _sa_cases as K
import _sa_oracle as SA
from _swarm_oracle import bits
import _tabu_cases as TC
import _tabu_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_tabu.json")))
CASES = TC.golden_cases()


def log_words(log):
    return np.array([[a, f, t, bits(c)] for a, f, t, c in log], dtype=np.uint32).reshape(-1, 4)


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tabu") / "tabu_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "tabu_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, epochs, seed, chain = CASES[name]
    return TO.solve_cached((name, seed, chain), xy, packed, n, init, epochs=epochs, seed=seed, chain=chain)


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_oracle_equals_goldens(name):
    _xy, _packed, n, _init, epochs, _seed, _chain = CASES[name]
    tour, cost, log, cnt = oracle(name)
    want = GOLD["cases"][name]
    assert tour.tolist() == want["tour"] and bits(cost) == want["cost_bits"] and cnt == want["counters"]
    assert hashlib.sha256(log_words(log).astype("<u4").tobytes()).hexdigest() == want["log_sha256"]
    assert log_words(log)[:8].tolist() == want["log_head"]
    TC.check_conditions(name, n, epochs, log, cnt)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, n, _init, epochs, seed, chain = CASES[name]
    tsp = str(tmp_path / "case.tsp")
    write_tsp(tsp, xy)
    lines = subprocess.run([baseline, tsp, "--trace", "--epochs", str(epochs), "--seed", str(seed), "--chain", str(chain)], capture_output=True, text=True,
                           check=True).stdout.splitlines()
    ran, hits, forced, bests, candidates, cost_bits, _sec = lines[0].split()
    tour, cost, log, cnt = oracle(name)
    want = GOLD["cases"][name]
    assert int(ran) == epochs + 1 and (int(hits), int(forced), int(bests), int(candidates)) == (cnt["hits"], cnt["forced"], cnt["bests"], cnt["candidates"])
    assert [int(v) for v in lines[1].split()] == tour.tolist() == want["tour"] and int(cost_bits) == bits(cost) == want["cost_bits"]
    assert [[int(v) for v in ln.split()] for ln in lines[2:]] == log_words(log).tolist()


def test_cpp_restatement_start_tour_and_draws(baseline, tmp_path):
    xy = K.small(8)
    tsp, ini = str(tmp_path / "s8.tsp"), str(tmp_path / "s8.init")
    write_tsp(tsp, xy)
    start = [3, 1, 4, 0, 7, 5, 2, 6]
    open(ini, "w").write(" ".join(str(v) for v in start) + "\n")
    lines = subprocess.run([baseline, tsp, "--trace", "--epochs", "50", "--seed", "9", "--chain", "2", "--init", ini], capture_output=True, text=True,
                           check=True).stdout.splitlines()
    tour, cost, log, _cnt = TO.solve(xy, None, 8, start, epochs=50, seed=9, chain=2)
    assert [int(v) for v in lines[1].split()] == tour.tolist() and int(lines[0].split()[5]) == bits(cost)
    assert [[int(v) for v in ln.split()] for ln in lines[2:]] == log_words(log).tolist()
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--chain", "5"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [TO.draw(77, 5, 7, e, a, s) for e in range(2) for a in range(8) for s in range(22)]


# ---------------------------------------------------------------- draws
def test_draws_are_the_annealing_stream_indexed_by_the_event():
    for seed, chain, n, epoch, attempt, slot in ((1, 0, 52, 0, 0, 0), (9, 3, 17, 5, 17, 21), (2 ** 64 - 1, 7, 1002, 77, 1002, 3)):
        ev = epoch * (n + 1) + attempt
        assert TO.event(epoch, n, attempt) == ev
        assert TO.draw(seed, chain, n, epoch, attempt, slot) == SA.mix(SA.chain_key(seed, chain) + SA.G * (32 * ev + slot + 1))
        if ev < 2 ** 32:  # where the event fits an epoch, the value is the annealing draw of that epoch
            assert TO.draw(seed, chain, n, epoch, attempt, slot) == SA.draw(seed, chain, ev, slot)
        assert TO.pair(seed, chain, n, epoch, attempt) == SA.pair_from_key(SA.chain_key(seed, chain), ev, n)


def test_draws_match_goldens_and_library(lib):
    for seed, chain, n, epoch, attempt, slot, want in GOLD["draws"]:
        assert TO.draw(int(seed), chain, n, epoch, attempt, slot) == int(want)
        assert lib.tl_tabu_draw(int(seed), chain, n, epoch, attempt, slot) == int(want)
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, chain, n, epoch = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32)), int(rng.integers(2, 2 ** 16)), int(rng.integers(0, 2 ** 32))
        attempt, slot = int(rng.integers(0, n + 1)), int(rng.integers(0, 32))
        assert lib.tl_tabu_draw(seed, chain, n, epoch, attempt, slot) == TO.draw(seed, chain, n, epoch, attempt, slot)
    # sa_spec.h's functions keep their results
    assert lib.tl_sa_draw(1, 3, 138148, 21) == SA.draw(1, 3, 138148, 21)


# ---------------------------------------------------------------- the list
def test_reference_unit_tests_of_the_list():
    # tabu_search.rs:128-160
    assert not TO.TabuList(5).contains([0, 1, 2])
    t = TO.TabuList(5)
    t.add([0, 1, 2])
    assert t.contains([0, 1, 2])
    t = TO.TabuList(2)
    for r in ([0, 1, 2], [1, 0, 2], [2, 1, 0]):
        t.add(r)
    assert not t.contains([0, 1, 2]) and t.contains([1, 0, 2]) and t.contains([2, 1, 0])
    assert TO.TabuList(7).capacity == 7


def test_ring_fifo_semantics():
    """the start tour listed twice, eviction of the oldest, and an evicted route admissible again"""
    start, r1, r2, r3 = [0, 1, 2], [1, 0, 2], [2, 1, 0], [0, 2, 1]
    as_lists = lambda t: [np.frombuffer(b, dtype=np.int64).tolist() for b in t.items]  # noqa: E731
    t = TO.TabuList(3)
    t.add(start)   # before the first epoch
    t.add(start)   # the old u of epoch 0
    assert as_lists(t) == [start, start]
    t.add(r1)
    assert as_lists(t) == [r1, start, start]
    t.add(r2)      # full: the oldest copy of the start tour goes, the other stays
    assert as_lists(t) == [r2, r1, start] and t.contains(start)
    t.add(r3)
    assert as_lists(t) == [r3, r2, r1] and not t.contains(start)  # evicted: admissible again


def test_the_chain_uses_the_list_that_way():
    """replaying a chain's log: the list a candidate met was [the old u of the last n - 1 epochs ..., the start tour twice while it
    lasts]; every checked taken candidate is outside it, and on three cities (six routes, a list of three) a route that was listed
    and evicted is taken again"""
    for name in ("small3", "small5", "gr17_matrix"):
        xy, packed, n, _init, _epochs, _seed, _chain = CASES[name]
        _tour, _cost, log, cnt = oracle(name)
        u = list(range(n))
        listed = [tuple(u)]           # oldest first
        ever, readmitted = {tuple(u)}, 0
        for e, (a, lo, hi, _c) in enumerate(log):
            cand = u[:lo] + u[lo:hi + 1][::-1] + u[hi + 1:]
            if e == 1:
                assert listed == [tuple(range(n))] * 2
            assert len(listed) == min(e + 1, n)
            if a < n:
                assert tuple(cand) not in listed, (name, e)
                readmitted += tuple(cand) in ever
            listed = (listed + [tuple(u)])[-n:]
            ever.add(tuple(u))
            u = cand
        if name == "small3":
            assert readmitted >= 1
        assert cnt["hits"] >= 1


def test_epochs_plus_one_epochs_run_and_the_best_is_returned():
    xy = K.small(8)
    for epochs in (1, 2, 7):
        tour, cost, log, cnt = TO.solve(xy, None, 8, None, epochs=epochs, seed=5)
        assert len(log) == epochs + 1
        d = TO.dist_fn(xy, None, 8)
        costs = [TO.tour_length(d, np.arange(8))] + [c for *_x, c in log]
        assert bits(cost) == bits(min(costs)) == bits(TO.tour_length(d, tour.astype(np.int64))) and cnt["bests"] == sum(
            c < min(costs[:k + 1]) for k, c in enumerate(costs[1:]))
    with pytest.raises(ValueError):
        TO.solve(xy, None, 8, None, epochs=0, seed=5)
    with pytest.raises(ValueError):
        TO.solve(xy[:1], None, 1, None, epochs=3, seed=5)


def test_reference_test_respects_initial_tour():
    # test_tabu_respects_initial_tour (tabu_search.rs:162-175): the best route is never longer than the start tour
    xy = np.array([[0, 0], [0, 0.5], [0, 1], [1, 1], [1, 0]], dtype=np.float32)
    tour, cost, _log, _cnt = TO.solve(xy, None, 5, [0, 1, 2, 3, 4], epochs=1, seed=1)
    assert cost == np.float32(4.0) and sorted(tour.tolist()) == [0, 1, 2, 3, 4]


def test_candidate_costs_equal_tour_length():
    xy = K.synth(30, 3)
    d = TO.dist_fn(xy, None, 30)
    tour = np.random.default_rng(2).permutation(30).astype(np.int64)
    pairs = [(0, 29), (0, 0), (5, 5), (3, 4), (0, 7), (11, 29), (1, 28), (29, 29)]
    cands, costs = TO.candidate_costs(d, tour, pairs)
    for (lo, hi), c, cost in zip(pairs, cands, costs):
        want = tour.copy()
        want[lo:hi + 1] = tour[lo:hi + 1][::-1]
        assert c.tolist() == want.tolist() and bits(cost) == bits(TO.tour_length(d, want))


# ---------------------------------------------------------------- plan, limits, names, flag
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    lds, work = 163840, 8 << 30
    assert lib.tl_tabu_search_plan(52, 1, 256, lds, work, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
    assert w.value == t.value and t.value % 64 == 0 and 64 <= t.value <= 1024 and per.value >= 256
    wide = t.value
    assert lib.tl_tabu_search_plan(52, 257, 256, lds, work, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
    assert w.value == t.value and 64 <= t.value <= wide and per.value >= 257
    # the flag changes no width
    assert lib.tl_tabu_search_plan(52, 1, 256, lds, work, _capi.TL_FLAG_TABU_FULL_COMPARE, C.byref(w), C.byref(t), C.byref(per)) == 0 and t.value == wide
    # the workspace bounds what one launch holds: a chain's ring is 2 n^2 bytes (and n hashes)
    assert lib.tl_tabu_search_plan(1000, 10 ** 6, 256, lds, 10 * 2_100_000, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
    assert 9 <= per.value <= 10
    assert lib.tl_tabu_search_plan(1000, 1, 256, lds, 1000, 0, C.byref(w), C.byref(t), C.byref(per)) == 0 and per.value == 0
    # beyond the LDS-resident limit, and below two cities: no plan
    top = (lds - 288) // 12
    assert lib.tl_tabu_search_plan(top, 1, 256, lds, 1 << 40, 0, C.byref(w), C.byref(t), C.byref(per)) == 0 and w.value > 0 and per.value >= 1
    for n in (top + 1, 1, 0):
        assert lib.tl_tabu_search_plan(n, 1, 256, lds, 1 << 40, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
        assert (w.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_tabu_search_plan(52, 1, 0, lds, work, 0, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_tabu_search_plan(52, 1, 256, lds, work, 1 << 31, None, None, None) == _capi.TL_ERR_UNSUPPORTED  # a bit no flag has
    assert lib.tl_tabu_search_lds_max_n(None) == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["tabu_search"] == "tabu_search" and "tabu" not in P.SOLVER_NAMES
    assert P.steps_for_solve("tabu_search") == ["nn", "tabu_search"] and P.steps_for_solve("Tabu_Search", no_seed=True) == ["tabu_search"]
    assert "tabu_search" in P.AUTO_EXPAND_WITH_NN
    with pytest.raises(ValueError, match="the seeded tabu search of this build is `tabu_search`"):
        P.steps_for_solve("tabu")
    with pytest.raises(ValueError, match="the seeded tabu search of this build is `tabu_search`"):
        P.run_pipeline_stages(None, ["tabu"])
    # `sa` is refused as before, with the hint it had
    with pytest.raises(ValueError, match="; the seeded annealing of this build is `simulated_annealing`$"):
        P.steps_for_solve("sa")
    assert P.steps_for_solve("simulated_annealing") == ["shuffle", "simulated_annealing"] and P.steps_for_solve("2opt") == ["nn", "2opt"]
    for other in ("stochastic_hill", "hill"):
        with pytest.raises(ValueError, match="unknown solver"):
            P.steps_for_solve(other)


def test_header_and_bindings_agree_on_the_new_flag_and_symbols(lib):
    import teeline_amd as TA
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (TL_FLAG_\w+) \(1u << (\d+)\)", text)}
    assert flags["TL_FLAG_TABU_FULL_COMPARE"] == 30 and TA.TL_FLAG_TABU_FULL_COMPARE == _capi.TL_FLAG_TABU_FULL_COMPARE == 1 << 30
    assert [k for k, v in flags.items() if v == 30] == ["TL_FLAG_TABU_FULL_COMPARE"]
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_tabu_search", "tl_tabu_search_trace", "tl_tabu_search_trace_chain", "tl_tabu_search_population", "tl_tabu_search_lds_max_n",
                "tl_tabu_search_plan", "tl_tabu_draw"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)


# ---------------------------------------------------------------- the list's record, and the cases chosen with it
def test_the_record_agrees_with_the_counters_and_the_replayed_list():
    """solve's record: one list length and one look-up count per epoch, one entry per refusal, and the ring indices are where a ring
    that writes its k-th route to slot k mod n holds the refused candidate"""
    for name in TC.HIT_CASES:
        xy, packed, n, _init, epochs, seed, chain = CASES[name]
        _tour, _cost, log, cnt = oracle(name)
        rec = TO.record_of((name, seed, chain))
        assert len(rec["list_len"]) == len(rec["checked"]) == epochs + 1 and len(rec["refusals"]) == cnt["hits"] >= 1
        assert rec["list_len"] == [min(e + 1, n) for e in range(epochs + 1)]
        ring, u, k = [None] * n, list(range(n)), 1
        ring[0] = tuple(u)
        by_epoch = {}
        for e, a, idx in rec["refusals"]:
            by_epoch.setdefault(e, []).append((a, idx))
        for e, (a, lo, hi, _c) in enumerate(log):
            for ra, idx in by_epoch.get(e, []):
                plo, phi = TO.pair(seed, chain, n, e, ra)
                cand = tuple(u[:plo] + u[plo:phi + 1][::-1] + u[phi + 1:])
                assert ra < a and idx and list(idx) == [j for j in range(n) if ring[j] == cand], (name, e)
            assert rec["checked"][e] == len(by_epoch.get(e, [])) + (a < n)
            ring[k % n] = tuple(u)
            k += 1
            u = u[:lo] + u[lo:hi + 1][::-1] + u[hi + 1:]


def widths(lib, n):
    """(threads of a chain alone, threads of a chain among more chains than CUs): the look-up takes that many listed routes per round"""
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    out = []
    for count in (1, TC.CUS + 1):
        assert lib.tl_tabu_search_plan(n, count, TC.CUS, TC.LDS_BYTES, TC.WORK, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
        out.append(t.value)
    return tuple(out)


@pytest.mark.parametrize("n", sorted(TC.WRAP_SEEDS))
def test_wrapped_ring_cases_refuse_beyond_one_round(lib, n):
    key, xy, packed, _n, init, epochs, seed = TC.wrap_chain(n)
    _tour, _cost, log, _cnt = TO.solve_cached((key, seed, 0), xy, packed, n, init, epochs=epochs, seed=seed, chain=0)
    assert widths(lib, n)[1] == 64
    TC.check_wrapped_ring(n, widths(lib, n)[1], log, TO.record_of((key, seed, 0)))


def test_long_list_case_looks_up_beyond_one_round(lib):
    """(No seed of 1 .. 13 000 gives this chain a single refusal, at any ring index: from city order improving candidates that the list
    does not hold are plentiful for all 331 epochs.  So the case covers look-ups in a list of more than 256 routes against false hits
    only; a look-up that stops after 256 rows gives the same chain.)"""
    key, xy, packed, n, init, epochs, seed = TC.long_chain()
    _tour, _cost, log, _cnt = TO.solve_cached((key, seed, 0), xy, packed, n, init, epochs=epochs, seed=seed, chain=0)
    assert widths(lib, n)[0] == 256
    TC.check_long_list(n, widths(lib, n)[0], log, TO.record_of((key, seed, 0)))
