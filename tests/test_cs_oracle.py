"""The cuckoo search solver without a GPU: the statement of the specification (tests/_cs_oracle.py) against the stand-alone C++
restatement (tests/probes/cs_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the gather form of the
reversals against the literal loop, the Lévy step (accuracy against libm, edge words, the resample path), the flight length, pa,
the conditions every seeded case is there for, the deliberately wrong variants those cases tell apart; pipeline names."""
import ctypes as C
import hashlib
import itertools
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _cs_cases as CC
import _cs_oracle as CO
import _sa_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_cs.json")))
CASES = CC.golden_cases()
bits = CO.bits
SWEEP = 1 << 20  # seeded draws of the accuracy sweep (>= 10^6)


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cs") / "cs_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "cs_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, o = CASES[name]
    return CO.solve_cached((name,), xy, packed, n, init, **o)


def seeded(name):
    xy, _packed, n, init, o, want = CC.seeded_case(name)
    return CO.solve_cached(("seeded", name), xy, None, n, init, **o), n, want


def run_baseline(exe, tmp_path, xy, init, o):
    tsp = str(tmp_path / "case.tsp")
    write_tsp(tsp, xy)
    args = [exe, tsp, "--trace", "--epochs", str(o["epochs"]), "--seed", str(o["seed"]), "--run", str(o["run"]), "--n-nearest", str(o["n_nearest"]),
            "--mutation-probability", repr(o["mutation_probability"])]
    if init is not None:
        ini = str(tmp_path / "case.init")
        open(ini, "w").write(" ".join(str(int(v)) for v in init) + "\n")
        args += ["--init", ini]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    head = [int(v) for v in lines[0].split()[:4]]
    log = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("I")]
    elog = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("E")]
    return head, [int(v) for v in lines[1].split()], log, elog


def host_levy(lib, words):
    t = C.c_uint32()
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return lib.tl_levy_from_words(w.ctypes.data_as(C.c_void_p), C.byref(t)), t.value


# ---------------------------------------------------------------- the draws
def test_no_two_roles_share_a_draw():
    for n, N, epochs, given in ((2, 25, 4, False), (5, 25, 3, True), (8, 27, 2, False), (13, 64, 2, True)):
        roles = CO.roles(n, N, epochs, given)
        assert len({(e, s) for e, s, _ in roles}) == len(roles) == (N - given) * (n - 1) + epochs * N * (CO.WORDS + 2 + 2 * (n // 2) + n - 1)
        assert max(s for _e, s, _r in roles) < 32
        assert max(e for e, _s, r in roles if r[0] != "shuffle") < CO.init_event(n, 0, 0) <= min(e for e, _s, r in roles if r[0] == "shuffle")
    assert CO.events_fit(10_000, 25, 1002) and CO.events_fit(2 ** 32 - 2, 4096, 16000) and not CO.events_fit(2 ** 32 - 2, 4096, 65535)
    assert CO.base(2 ** 32 - 2, 4096, 4095, 16000) + 16000 < CO.EVENT_LIMIT
    assert CO.uniform(2 ** 64 - 1) == 1.0 - 2.0 ** -53 and CO.uniform(0) == 0.0


def test_draws_and_levy_equal_the_goldens_and_the_library(lib):
    for seed, run, event, slot, want in GOLD["draws"]:
        assert CO.draw(int(seed), run, int(event), slot) == int(want) == lib.tl_cs_draw(int(seed), run, int(event), slot)
    for words, vb, tries, ks in GOLD["levy"]:
        w = [int(x) for x in words]
        v, t = CO.levy_from_words(w)
        hv, ht = host_levy(lib, w)
        assert CO.f64_bits(v) == int(vb) == CO.f64_bits(hv) and t == tries == ht
        assert [CO.flight_length(abs(v), n) for n in (2, 3, 52, 280, 1002)] == ks == [lib.tl_cs_flight_length(abs(hv), n) for n in (2, 3, 52, 280, 1002)]


# ---------------------------------------------------------------- the gather
def test_gather_equals_the_literal_loop_exhaustively():
    """every pair list of length <= 3 at n <= 5"""
    for n in range(2, 6):
        all_pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
        tour = list(range(10, 10 + n))
        for k in range(0, 4):
            for pairs in itertools.product(all_pairs, repeat=k):
                want = CO.reverse_literal(tour, pairs)
                assert CO.reverse_gather(tour, list(pairs)) == want == CO.reverse_gather_np(tour, list(pairs)).tolist(), (n, pairs)


def test_gather_equals_the_literal_loop_on_random_lists():
    rng = np.random.default_rng(7)
    for n, k in [(n, int(rng.integers(1, n // 2 + 1))) for n in list(range(6, 80)) + [257, 513]] + [(600, 300), (600, 257), (1002, 501)]:
        tour = rng.permutation(n).tolist()
        pairs = []
        for _ in range(k):
            i = int(rng.integers(0, n - 1))
            pairs.append((i, int(rng.integers(i + 1, n))))
        pairs[0] = (0, n - 1)  # the whole tour
        pairs[-1] = (n // 2 - 1, n // 2)  # j = i + 1
        want = CO.reverse_literal(tour, pairs)
        assert CO.reverse_gather_np(tour, pairs).tolist() == want, (n, k)
        if n <= 80:
            assert CO.reverse_gather(tour, pairs) == want


# ---------------------------------------------------------------- the Lévy step
def test_levy_accuracy_and_flight_length_against_libm(lib):
    """The measurement of DESIGN.md §4.21: 2^20 seeded draws plus the edge words, the specification's step against numpy's libm
    evaluation of the reference formula.  The bound is twice the maximum measured when the specification was fixed (levy_spec.h:
    kLevyMeasuredRelDiff) because the sweep is finite; k must agree wherever levy 0.1 n is not within that bound of an integer."""
    text = open(os.path.join(ROOT, "teeline_amd", "csrc", "levy_spec.h")).read()
    measured = float(re.search(r"kLevyMeasuredRelDiff = ([0-9.e+-]+);", text).group(1))
    bound = 2.0 * measured
    rng = np.random.default_rng(2026)
    words = rng.integers(0, 2 ** 64, size=(SWEEP, CO.WORDS), dtype=np.uint64)
    edge = np.asarray([[int(x) for x in w] for w, _v, t, _k in GOLD["levy"] if t == 0], dtype=np.uint64)
    words = np.concatenate([words, edge])
    spec, tries = CO.levy_spec(words)
    ref = CO.levy_libm(words)
    # u2 = 1/4 or 3/4 in u: the exact reduction gives a step of exactly 0 where libm's rounded argument 2 pi u2 leaves a residue of
    # 1e-16: no relative difference exists there; the residue is bounded instead
    zero = spec == 0.0
    assert zero.sum() <= 2 and (np.abs(ref[zero]) < 1e-13).all()
    ok = np.isfinite(ref) & (ref != 0.0) & (tries == 0) & ~zero
    assert ok.sum() >= SWEEP
    rel = np.abs(spec[ok] - ref[ok]) / np.abs(ref[ok])
    worst = float(rel.max())
    print(f"levy: max relative difference {worst:.3e} over {int(ok.sum())} draws (recorded {measured:.3e}, bound {bound:.3e}); median {float(np.median(rel)):.3e}")
    assert worst <= bound
    assert worst >= measured / 4.0  # the recorded figure is this sweep's, not a loose guess
    for n in (52, 280, 1002):
        ks, kr = CO.flight_length_np(np.abs(spec[ok]), n), CO.flight_length_np(np.abs(ref[ok]), n)
        x = np.abs(ref[ok]) * (n * 0.1)
        near = np.abs(x - np.rint(x)) <= bound * np.maximum(x, 1.0)
        differ = ks != kr
        print(f"levy: n={n}: k differs from libm's on {int(differ.sum())} draws, {int(near.sum())} lie within the bound of an integer")
        assert not (differ & ~near).any()
    for i in rng.integers(0, SWEEP, size=300):  # the library's host entry is the same statement
        hv, ht = host_levy(lib, words[i])
        assert CO.f64_bits(hv) == CO.f64_bits(spec[i]) and ht == tries[i]


def test_levy_edge_words(lib):
    top, q1, q3, mid = CO.word_of_uniform(2 ** 53 - 1), CO.word_of_uniform(2 ** 51), CO.word_of_uniform(3 * 2 ** 51), CO.word_of_uniform(12345678901234)
    ok = [mid, CO.word_of_uniform(2 ** 50)]
    assert CO.uniform(q1) == 0.25 and CO.uniform(q3) == 0.75 and CO.uniform(top) == 1.0 - 2.0 ** -53
    # the exact reduction: cos(2 pi / 4) and cos(2 pi 3 / 4) are exactly zero (libm's are not), cos(0) = 1, cos(pi) = -1
    c = CO.cos2pi_spec(np.array([0.25, 0.75, 0.0, 0.5, 0.125]))
    assert c[0] == 0.0 and c[1] == 0.0 and c[2] == 1.0 and c[3] == -1.0 and abs(c[4] - math.sqrt(0.5)) < 2e-16 and math.cos(2 * math.pi * 0.25) != 0.0
    # u1 = 0 takes the floor: sqrt(-2 log(MIN_POSITIVE)) = 37.6..
    v, t = CO.levy_from_words([0, 0, mid, mid] + ok * 4)
    assert t == 0 and math.isfinite(v) and v > 0.0 and abs(float(CO.normal_spec(0, 0)) - math.sqrt(-2.0 * math.log(CO.MIN_POSITIVE))) < 1e-12
    # u1 = 1 - 2^-53 in v: |v| <= 2^-26, the step is huge and k saturates at n / 2
    v, t = CO.levy_from_words([mid, mid, top, mid] + ok * 4)
    assert t == 0 and abs(v) > 1e4 and all(CO.flight_length(abs(v), n) == n // 2 == lib.tl_cs_flight_length(abs(v), n) for n in (2, 3, 52, 280, 1002))
    # u2 = 1/4: v is exactly zero and the next pair is taken; after four zero pairs v is 1.0 and the step is u itself
    for row, tries in (([mid, mid, mid, q1] + ok * 4, 1), ([mid, mid, mid, q3] + [mid, q1] + ok * 3, 2), ([mid, mid, mid, q1] + [mid, q3] * 3 + ok, 4),
                       ([mid, mid, mid, q1] + [mid, q3] * 4, 4)):
        v, t = CO.levy_from_words(row)
        hv, ht = host_levy(lib, row)
        assert t == tries == ht and CO.f64_bits(v) == CO.f64_bits(hv) and math.isfinite(v)
    u = float(CO.normal_spec(mid, mid)) * CO.SIGMA_U
    assert CO.levy_from_words([mid, mid, mid, q1] + [mid, q3] * 4)[0] == u  # |v| = 1: exp((1 / 1.5) log 1) = 1
    assert CO.levy_from_words([mid, mid, mid, q1] + ok * 4)[0] == CO.levy_from_words([mid, mid] + ok + ok * 4)[0]
    assert CO.RESAMPLES == 4 and CO.WORDS == 12 and CO.SLOT_LEVY + CO.WORDS <= CO.SLOT_TARGET


def test_flight_length_and_pa(lib):
    fl = lib.tl_cs_flight_length
    assert fl(float("nan"), 52) == 1 == CO.flight_length(float("nan"), 52) and fl(float("inf"), 52) == 26 == CO.flight_length(float("inf"), 52)
    assert fl(1e300, 1002) == 501 and fl(0.0, 52) == 1 and fl(-3.0, 52) == 1 and fl(float("inf"), 1002) == 501
    for n in (2, 3):
        assert [fl(x, n) for x in (0.0, 0.5, 3.0, 1e9, float("inf"), float("nan"))] == [1] * 6 == [CO.flight_length(x, n) for x in (0.0, 0.5, 3.0, 1e9, float("inf"), float("nan"))]
    assert fl(1.0, 0) == 0 and fl(1.0, 1) == 0
    rng = np.random.default_rng(3)
    for x in np.concatenate([rng.uniform(0, 12, 300), np.arange(0, 30) / 5.2]):
        for n in (52, 280, 1002):
            want = min(max(math.ceil(float(x) * (n * 0.1)), 1), n // 2)
            assert fl(float(x), n) == want == CO.flight_length(float(x), n) == int(CO.flight_length_np(np.array([x]), n)[0])
    assert lib.tl_cs_pa(0.0) == 0.01 == CO.pa_of(0.0) and lib.tl_cs_pa(1.0) == 0.99 == CO.pa_of(1.0) and lib.tl_cs_pa(0.001) == 0.01 == CO.pa_of(0.001)
    assert lib.tl_cs_pa(0.5) == 0.5 and lib.tl_cs_pa(0.25) == CO.pa_of(0.25) and lib.tl_cs_pa(0.3) == float(np.float32(0.3)) == CO.pa_of(0.3)
    assert CO.nests(3) == 25 and CO.nests(25) == 25 and CO.nests(26) == 26


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_goldens(name):
    _xy, _packed, n, _init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    assert res["tour"].tolist() == want["tour"] and bits(res["cost"]) == want["cost_bits"] and res["counters"] == want["counters"]
    assert CO.log_words(res).tolist() == want["log"] and sha(CO.route_words(res, n)) == want["routes_sha256"]
    assert sha(CO.epoch_words(res)) == want["epochs_sha256"] and CO.epoch_words(res)[:1].tolist() == want["epochs_head"]
    CC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, _n, init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head == [o["epochs"], res["counters"]["flights"], res["counters"]["improved"], bits(res["cost"])] and bits(res["cost"]) == want["cost_bits"]
    assert route == res["tour"].tolist() == want["tour"]
    assert log == CO.log_words(res)[:, :3].tolist() and elog == CO.epoch_words(res).tolist()


@pytest.mark.parametrize("name", sorted(CC.SEEDED))
def test_cpp_restatement_on_the_seeded_cases(baseline, tmp_path, name):
    xy, _packed, n, init, o, _want = CC.seeded_case(name)
    res, _n, _w = seeded(name)
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head[1:] == [res["counters"]["flights"], res["counters"]["improved"], bits(res["cost"])] and route == res["tour"].tolist()
    assert log == CO.log_words(res)[:, :3].tolist() and elog == CO.epoch_words(res).tolist()


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--run", "5"], capture_output=True, text=True, check=True).stdout.splitlines()
    draws = [CO.draw(77, 5, base + e, s) for base in (0, 1 << 58) for e in range(8) for s in range(28)]
    assert [int(v) for v in out[:len(draws)]] == draws
    for e, line in enumerate(out[len(draws):len(draws) + 64]):
        v, t = CO.levy_from_words([CO.draw(77, 5, e, s) for s in range(CO.WORDS)])
        assert [int(x) for x in line.split()] == [CO.f64_bits(v), t] + [CO.flight_length(abs(v), n) for n in (52, 280, 1002)]


# ---------------------------------------------------------------- what the seeded cases are there for
@pytest.mark.parametrize("name", sorted(CC.SEEDED))
def test_seeded_cases_meet_their_conditions(name):
    res, n, want = seeded(name)
    got = CC.conditions(res, n)
    assert set(want) <= got, (name, set(want) - got)
    assert set(want) <= set(CC.CONDITIONS)
    if name == "synth600_long_flights":
        assert max(max(ep["ks"]) for ep in res["epochs"]) > 256


def test_every_condition_is_met():
    met = set()
    for name in CC.SEEDED:
        res, n, _want = seeded(name)
        met |= CC.conditions(res, n)
    assert met == set(CC.CONDITIONS)


def test_n_2_every_cost_ties_and_the_first_minimum_is_nest_0():
    res = CO.solve(K.small(2), None, 2, None, epochs=6, mutation_probability=0.5, seed=2)
    assert res["improvements"] == [(CO.NONE, 0, res["cost"], res["improvements"][0][3])] and len({bits(c) for ep in res["epochs"] for c in ep["costs"]}) == 1
    assert all(k == 1 for ep in res["epochs"] for k in ep["ks"]) and not any(a for ep in res["epochs"] for a in ep["accepted"])
    assert all(p == [(0, 1)] for ep in res["epochs"] for p in ep["pairs"]) and any(a for ep in res["epochs"] for a in ep["abandoned"])


@pytest.mark.parametrize("mutate", ["epoch_start", "best_is_min", "le"])
def test_the_seeded_cases_tell_the_wrong_variants_apart(mutate):
    """flights from the epoch-start nest, best as the minimum over the nests, the target test <=: each changes a seeded record"""
    differs = 0
    for name in sorted(CC.SEEDED)[:4]:  # (not n = 600: the small cases do it)
        xy, _packed, n, init, o, _want = CC.seeded_case(name)
        res, _n, _w = seeded(name)
        wrong = CO.solve(xy, None, n, init, mutate=mutate, **o)
        differs += (CO.epoch_words(wrong).tolist() != CO.epoch_words(res).tolist() or CO.log_words(wrong).tolist() != CO.log_words(res).tolist()
                    or wrong["tour"].tolist() != res["tour"].tolist() or bits(wrong["cost"]) != bits(res["cost"]))
    assert differs >= 1


def test_small_n_and_epochs_zero():
    for n in (0, 1):
        res = CO.solve(K.small(3)[:n], None, n, None, epochs=0, seed=1)
        assert res["tour"].tolist() == list(range(n)) and res["cost"] == 0 and [m[0] for m in CO.messages(res)] == ["PathUpdate", "Done"]
        with pytest.raises(ValueError, match="panics"):
            CO.solve(K.small(3)[:n], None, n, None, epochs=1, seed=1)
    init = CC.start_tour(8, 2)
    res = CO.solve(K.small(8), None, 8, init, epochs=0, seed=5)
    assert len(res["improvements"]) == 1 and res["epochs"] == [] and [m[0] for m in CO.messages(res)] == ["PathUpdate", "Done"]
    d = CO.dist_fn(K.small(8), None, 8)
    key = CO.chain_key(5, 0)
    starts = [init.tolist()] + [CO.shuffled(key, 8, CO.init_event(8, i, 0), CO.SLOT_SHUFFLE) for i in range(1, 25)]
    costs = [CO.tour_length(d, np.asarray(s)) for s in starts]
    first = min(range(25), key=lambda i: (costs[i], i))  # the FIRST minimum
    assert res["improvements"][0][1] == first and res["tour"].tolist() == starts[first]


# ---------------------------------------------------------------- plan, limits, names
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    N, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    lds, work = 163840, 8 << 30
    out = (C.byref(N), C.byref(t), C.byref(per))
    assert lib.tl_cuckoo_search_plan(52, 3, 1, 256, lds, work, 0, *out) == 0 and (N.value, t.value, per.value) == (25, 64, 65535)
    assert lib.tl_cuckoo_search_plan(130, 26, 1, 256, lds, work, 0, *out) == 0 and (N.value, t.value, per.value) == (26, 192, 65535)
    run_bytes = 6 * 25 * 1002 + 2 * 1002 + 16 * 25
    assert lib.tl_cuckoo_search_plan(1002, 3, 64, 256, lds, 3 * run_bytes + 11 * 256, 0, *out) == 0 and per.value == 3 and t.value == 256
    up = lambda v: (v + 15) & ~15  # noqa: E731
    top = max(n for n in range(lds // 11, lds // 10 + 1) if 576 + up(4 * (n // 2)) + up(4 * n) + 2 * up(2 * n) <= lds)
    assert lib.tl_cuckoo_search_plan(top, 3, 1, 256, lds, 1 << 40, 0, *out) == 0 and per.value >= 1 and t.value == 256
    for n, nn, w in ((top + 1, 3, 1 << 40), (0, 3, work), (1, 3, work), (1000, 3, 1000), (52, 4097, work)):
        assert lib.tl_cuckoo_search_plan(n, nn, 1, 256, lds, w, 0, *out) == 0
        assert (N.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_cuckoo_search_plan(52, 4096, 1, 256, lds, work, 0, *out) == 0 and N.value == 4096 and per.value >= 1
    assert lib.tl_cuckoo_search_plan(52, 3, 1, 0, lds, work, 0, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_cuckoo_search_plan(52, 3, 1, 256, lds, work, 1 << 31, *out) == _capi.TL_ERR_UNSUPPORTED and (N.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_cuckoo_search_max_n(None) == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["cuckoo_search"] == "cuckoo_search" and "cs" not in P.SOLVER_NAMES and "cuckoo_search" in P.AUTO_EXPAND_WITH_SHUFFLE
    assert P.steps_for_solve("cuckoo_search") == ["shuffle", "cuckoo_search"] and P.steps_for_solve("Cuckoo_Search", no_seed=True) == ["cuckoo_search"]
    with pytest.raises(ValueError, match="the seeded cuckoo search of this build is `cuckoo_search`"):
        P.steps_for_solve("cs")
    with pytest.raises(ValueError, match="the seeded cuckoo search of this build is `cuckoo_search`"):
        P.run_pipeline_stages(None, ["cs"])
    assert P.REFUSED_ALIASES["cs"] == "cuckoo_search"
    with pytest.raises(ValueError, match="unknown solver") as info:
        P.steps_for_solve("stochastic_hill")
    assert "of this build is" not in str(info.value)
    assert P.steps_for_solve("particle_swarm") == ["shuffle", "particle_swarm"] and P.steps_for_solve("tabu_search") == ["nn", "tabu_search"]


def test_header_bindings_and_flags_agree(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_cuckoo_search", "tl_cuckoo_search_trace", "tl_cuckoo_search_population", "tl_cuckoo_search_max_n", "tl_cuckoo_search_plan", "tl_cs_draw",
                "tl_levy_from_words", "tl_cs_flight_length", "tl_cs_pa", "tl_cs_selftest_levy", "tl_cs_selftest_reversals"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)
    assert re.search(r"typedef struct tl_cs_opts \{[^}]*uint32_t epochs;[^}]*uint32_t n_nearest;[^}]*float mutation_probability;[^}]*\} tl_cs_opts;", text)
    assert [f for f, _ in _capi.TlCsOpts._fields_] == ["epochs", "n_nearest", "mutation_probability"] and C.sizeof(_capi.TlCsOpts) == 12
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags  # the bit the solver refuses is one no flag has: no new flag was added
