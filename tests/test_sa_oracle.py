"""Simulated annealing without a GPU: the numpy statement of the specification (tests/_sa_oracle.py) against the stand-alone C++
restatement (tests/probes/sa_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the reference's own unit
tests (simulated_annealing.rs:90-126); pipeline names, presets and option validation of the Python mirror."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _sa_cases as K
import _sa_oracle as SA
from _swarm_oracle import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_sa.json")))


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sa") / "sa_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "probes", "sa_cpu_baseline.cpp"), "-o", exe])
    return exe


def run_baseline(exe, opts, seed, chain):
    args = [exe, os.path.join(K.TSPLIB, "berlin52.tsp"), "--trace", "--seed", str(seed), "--chain", str(chain), "--epochs", str(opts["epochs"]),
            "--cooling-rate", repr(opts["cooling_rate"]), "--min-temperature", repr(opts["min_temperature"]), "--max-temperature",
            repr(opts["max_temperature"])]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    epochs, accepted, cost_bits, _sec = lines[0].split()
    return int(epochs), int(accepted), int(cost_bits), [int(v) for v in lines[1].split()], [[int(v) for v in ln.split()] for ln in lines[2:]]


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(K.golden_cases()))
def test_numpy_oracle_equals_goldens(name):
    xy, packed, n, init, opts, seed, chain = K.golden_cases()[name]
    tour, cost, trace = SA.solve_cached(name, xy, packed, n, init, seed=seed, chain=chain, **opts)
    want = GOLD["cases"][name]
    assert tour.tolist() == want["tour"] and bits(cost) == want["cost_bits"]
    assert [[e, f, t, bits(c)] for e, f, t, c in trace] == want["trace"]
    assert len(trace) > 0 or n == 2  # (two cities: every candidate is the same cycle, nothing is ever accepted)


@pytest.mark.parametrize("name", ["berlin52_short", "berlin52_hot", "berlin52_cold_chain3"])
def test_cpp_restatement_equals_goldens(baseline, name):
    _xy, _packed, _n, _init, opts, seed, chain = K.golden_cases()[name]
    epochs, accepted, cost_bits, tour, trace = run_baseline(baseline, opts, seed, chain)
    want = GOLD["cases"][name]
    assert epochs == len(SA.schedule(**opts)) and accepted == len(want["trace"])
    assert tour == want["tour"] and cost_bits == want["cost_bits"] and trace == want["trace"]


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--chain", "5"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [SA.draw(77, 5, e, s) for e in range(2) for s in range(23)]


def test_hot_and_cold_cases_are_what_they_claim():
    hot, cold = GOLD["cases"]["berlin52_hot"]["trace"], GOLD["cases"]["berlin52_cold_chain3"]["trace"]
    assert len(hot) > 0.9 * 300                      # nearly every epoch accepted
    costs = [np.array([c], dtype=np.uint32).view(np.float32)[0] for *_x, c in cold]
    assert 0 < len(cold) < 0.1 * 4000 and all(b < a for a, b in zip(costs, costs[1:]))  # improvements only
    gaps = np.diff([e for e, *_x in cold])
    assert gaps.max() > 2 * 256                         # a run of whole windows with nothing accepted


# ---------------------------------------------------------------- schedule
def test_default_schedule_is_138149_epochs():
    assert len(SA.schedule()) == 138149


def test_schedule_lengths_match_goldens_and_library(lib):
    from teeline_amd import _capi
    for o, want in GOLD["schedules"]:
        assert len(SA.schedule(**o)) == want
        n = C.c_uint64()
        co = _capi.TlSaOpts(o["epochs"], o["cooling_rate"], o["min_temperature"], o["max_temperature"])
        assert lib.tl_sa_schedule_epochs(C.byref(co), C.byref(n)) == 0 and n.value == want
    n = C.c_uint64()
    assert lib.tl_sa_schedule_epochs(None, C.byref(n)) == 0 and n.value == 138149
    # never ending (the temperature stops falling above min_temperature) and too long: TL_ERR_UNSUPPORTED
    co = _capi.TlSaOpts(0, 1e-12, 1e-3, 1000.0)
    assert lib.tl_sa_schedule_epochs(C.byref(co), C.byref(n)) == _capi.TL_ERR_UNSUPPORTED
    co = _capi.TlSaOpts(0, 1e-4, 0.0, 1000.0)
    assert lib.tl_sa_schedule_epochs(C.byref(co), C.byref(n)) == _capi.TL_ERR_UNSUPPORTED
    assert lib.tl_sa_schedule_epochs(C.byref(co), None) == _capi.TL_ERR_BADARG


def test_temperature_is_two_roundings():
    T = SA.schedule(epochs=5, cooling_rate=1e-4, min_temperature=1e9, max_temperature=1000.0)
    for a, b in zip(T, T[1:]):
        assert b == np.float32(a - np.float32(np.float32(1e-4) * a))


# ---------------------------------------------------------------- draws
def test_draws_match_goldens_and_library(lib):
    for seed, chain, epoch, slot, want in GOLD["draws"]:
        assert SA.draw(int(seed), chain, epoch, slot) == int(want)
        assert lib.tl_sa_draw(int(seed), chain, epoch, slot) == int(want)
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, chain, epoch, slot = (int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 32)))
        assert lib.tl_sa_draw(seed, chain, epoch, slot) == SA.draw(seed, chain, epoch, slot)


@pytest.mark.parametrize("n", [2, 3, 4, 52])
def test_pair_rule(n):
    adjacent = 0
    for e in range(400):
        lo, hi = SA.pair(9, 0, e, n)
        assert 0 <= lo <= hi < n
        key = SA.chain_key(9, 0)
        attempts = []
        for a in range(11):
            p = sorted((((SA.draw(9, 0, e, 2 * a) >> 32) * n) >> 32, ((SA.draw(9, 0, e, 2 * a + 1) >> 32) * n) >> 32))
            attempts.append(tuple(p))
        good = [p for p in attempts[:10] if p[1] - p[0] > 1]
        assert (lo, hi) == (good[0] if good else attempts[10]) == SA.pair_from_key(key, e, n)
        adjacent += hi - lo <= 1
    if n <= 3:
        assert adjacent > 0  # after 10 redraws the last pair is used even when equal or adjacent
    if n == 2:
        assert adjacent == 400


def test_p_is_a_24_bit_fraction():
    key = SA.chain_key(3, 1)
    ps = [SA.p_from_key(key, e) for e in range(500)]
    assert all(0 <= p < 1 and float(p) * 2 ** 24 == int(float(p) * 2 ** 24) for p in ps) and 0.4 < float(np.mean(ps)) < 0.6


# ---------------------------------------------------------------- criterion and acceptance
def test_criterion_equals_f32_exp_on_a_sweep():
    xs = np.concatenate([np.linspace(-87.0, 0.0, 20001), -np.logspace(-30, 1.9, 2000), [-87.0, -86.99999, -1e-45, -0.0, 0.0]]).astype(np.float32)
    for x in xs:
        assert SA.criteria(x) == np.float32(math.exp(float(x))), x


def test_criterion_edges():
    assert SA.criteria(np.float32(-87.00001)) == 0 and bits(SA.criteria(np.float32(-87.00001))) == 0
    assert SA.criteria(np.float32(-1e30)) == 0 and SA.criteria(np.float32(-np.inf)) == 0
    assert SA.criteria(np.float32(-0.0)) == 1 and SA.criteria(np.float32(0.0)) == 1
    assert SA.criteria(np.float32(-87.0)) > 0
    assert np.isnan(SA.criteria(np.float32(np.nan)))


def test_reference_unit_tests_of_is_acceptable():
    # simulated_annealing.rs:115-126
    for p in (0.0, 0.5, 1 - 2.0 ** -24):
        assert SA.is_acceptable(0.001, 100.0, 50.0, p) and SA.is_acceptable(0.001, 100.0, 99.999, p)
        assert not SA.is_acceptable(1_000_000.0, 10.0, 10.0, p)
    # :128-150, with the seeded p: > 90 % at high T, < 10 % at low T
    key = SA.chain_key(1, 0)
    ps = [SA.p_from_key(key, e) for e in range(1000)]
    assert sum(SA.is_acceptable(1_000_000.0, 10.0, 10.001, p) for p in ps) > 900
    assert sum(SA.is_acceptable(0.0001, 10.0, 20.0, p) for p in ps) < 100


def test_empty_schedule_returns_the_start_tour():
    # test_sa_respects_initial_tour (simulated_annealing.rs:90-113)
    xy = np.array([[0, 0], [0, 0.5], [0, 1], [1, 1], [1, 0]], dtype=np.float32)
    assert len(SA.schedule(**K.EMPTY)) == 0
    tour, cost, trace = SA.solve(xy, None, 5, [0, 1, 2, 3, 4], **K.EMPTY)
    assert tour.tolist() == [0, 1, 2, 3, 4] and cost == np.float32(4.0) and trace == []
    tour, _c, _t = SA.solve(xy, None, 5, [3, 1, 4, 0, 2], **K.EMPTY)
    assert tour.tolist() == [3, 1, 4, 0, 2]
    with pytest.raises(ValueError):
        SA.solve(xy[:1], None, 1, None, **K.with_epochs(1))


def test_accumulate_is_sequential():
    rng = np.random.default_rng(3)
    e = (rng.random(1000) * 1000).astype(np.float32)
    tot = np.float32(0)
    for v in e:
        tot = np.float32(tot + v)
    assert np.add.accumulate(e, dtype=np.float32)[-1] == tot


# ---------------------------------------------------------------- host logic of the mirror
def test_pipeline_names_presets_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["simulated_annealing"] == "simulated_annealing"
    assert P.steps_for_solve("classic") == ["nn", "2opt", "simulated_annealing"] and P.steps_for_solve("thorough") == ["nn", "3opt", "simulated_annealing"]
    assert P.steps_for_solve("fast") == ["nn", "2opt"]
    assert P.steps_for_solve("Simulated_Annealing", no_seed=True) == ["simulated_annealing"]
    with pytest.raises(ValueError, match="simulated_annealing"):  # the short alias stays refused, as before; the message names the long one
        P.steps_for_solve("sa")
    assert P.steps_for_solve("simulated_annealing") == ["shuffle", "simulated_annealing"]
    assert P.steps_for_solve("2opt") == ["nn", "2opt"] and P.steps_for_solve("gec") == ["gec"]


def test_options_validation_messages():
    import teeline_amd as T
    T.SAOptions().validate()
    o = T.SAOptions()
    assert (o.heuristic.epochs, o.cooling_rate, o.min_temperature, o.max_temperature) == (10_000, 0.0001, 0.001, 1000.0)
    for kw, msg in ((dict(cooling_rate=0.0), "cooling_rate must be > 0"), (dict(cooling_rate=1.0), "cooling_rate must be < 1"),
                    (dict(max_temperature=0.0), "max_temperature must be > 0"), (dict(min_temperature=-1.0), "min_temperature must be >= 0"),
                    (dict(min_temperature=2000.0), "min_temperature (2000.0) must be < max_temperature (1000.0)")):
        with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(")", r"\)")):
            T.SAOptions(**kw).validate()
        assert SA.validate(**dict(SA.DEFAULTS, **kw)) is not None
    with pytest.raises(ValueError):  # the option parser refuses the reference test's own combination; solve() runs it
        T.SAOptions.parse(epochs=0, max_temperature=0.0, min_temperature=1e6)
    assert T.SAOptions.parse(epochs=5, cooling_rate=0.5).heuristic.epochs == 5
    assert T.simulated_annealing.schedule_epochs() == 138149


def test_plan_is_host_only(lib):
    from teeline_amd import _capi
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    assert lib.tl_sim_anneal_plan(52, 1, 256, 163840, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
    assert w.value == t.value and t.value % 64 == 0 and 64 <= t.value <= 1024 and per.value >= 256
    assert lib.tl_sim_anneal_plan(52, 1, 256, 163840, _capi.TL_FLAG_SA_NO_SPECULATION, C.byref(w), C.byref(t), C.byref(per)) == 0
    assert w.value == 1 and t.value == 64
    assert lib.tl_sim_anneal_plan(20000, 1, 256, 163840, 0, C.byref(w), C.byref(t), C.byref(per)) == 0
    assert (w.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_sim_anneal_plan(52, 1, 0, 163840, 0, None, None, None) == _capi.TL_ERR_BADARG


# ---------------------------------------------------------------- the conditions of the cases past one workgroup pass
def threads(lib, n, count, flags=0):
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    assert lib.tl_sim_anneal_plan(n, count, K.CUS, K.LDS_BYTES, flags, C.byref(w), C.byref(t), C.byref(per)) == 0
    return t.value


@pytest.mark.parametrize("n", sorted(K.LONG_POP))
def test_long_population_chains_reverse_past_one_trip(lib, n):
    """the chain between the first and the last of cus + 1 one-wave chains: a reversal of more than 128 elements and a closing-edge
    move, accepted; the same chain alone without speculation runs on 64 threads too"""
    from teeline_amd import _capi
    seed, mid = K.LONG_POP[n]
    nt = threads(lib, n, K.CUS + 1)
    assert nt == threads(lib, n, 1, _capi.TL_FLAG_SA_NO_SPECULATION) == 64 and 0 < mid < K.CUS and n > 2 * nt
    key, *args, opts, seed, chain = K.long_chain(n, seed, mid)
    trace = SA.solve_cached(key, *args, seed=seed, chain=chain, **opts)[2]
    assert len(SA.schedule(**opts)) == K.LONG_EPOCHS and len(trace) > K.LONG_EPOCHS // 2
    assert any(t - f + 1 > 128 for _e, f, t, _c in trace)
    K.check_long_reversals(trace, n, nt)


def test_long_single_chain_reverses_past_one_trip(lib):
    n, seed = K.LONG_SINGLE
    nt = threads(lib, n, 1)
    assert nt == 256
    key, *args, opts, seed, chain = K.long_chain(n, seed, 0)
    trace = SA.solve_cached(key, *args, seed=seed, chain=chain, **opts)[2]
    assert any(t - f + 1 > 512 for _e, f, t, _c in trace)
    K.check_long_reversals(trace, n, nt, same_move=True)


@pytest.mark.parametrize("piece", K.PIECES)
def test_piece_cases_reach_a_second_piece(piece):
    """every schedule run in pieces has more than one; the last piece of one epoch is one; accepted epochs fall into the second piece
    (the trace index continues there) and a trace can be cut inside it"""
    for name, (xy, n, init, opts, seed) in K.piece_cases(piece).items():
        epochs = len(SA.schedule(**opts))
        trace = SA.solve_cached((name, seed, 0), xy, None, n, init, seed=seed, **opts)[2]
        assert epochs > piece, name
        if name.startswith("last_piece_of_one"):
            assert epochs % piece == 1 and epochs // piece == 2 and trace[-1][0] == epochs - 1
        first = sum(e < piece for e, *_x in trace)
        second = sum(piece <= e < 2 * piece for e, *_x in trace)
        assert first >= 1 and second >= 2, (name, first, second)  # a cap of first + 1 ends the trace inside the second piece
