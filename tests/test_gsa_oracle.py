"""The gravitational search solver without a GPU: the statement of the specification (tests/_gsa_oracle.py) against the stand-alone
C++ restatement (tests/probes/gsa_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the seeded draws, g,
the pull length and its bound, the masses and the stable ranking, the conditions every seeded case is there for, the deliberately
wrong variants those cases tell apart; names."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _gsa_cases as GC
import _gsa_oracle as GO
import _pso_oracle as PO
import _sa_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_gsa.json")))
CASES = GC.golden_cases()
bits = GO.bits
FAST = GO.swap_sequence_inverse


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gsa") / "gsa_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "gsa_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, o = CASES[name]
    return GO.solve_cached((name,), xy, packed, n, init, **o)


def seeded(name):
    xy, _packed, n, init, o, want = GC.seeded_case(name)
    return GO.solve_cached(("seeded", name), xy, None, n, init, seq=FAST if n >= 600 else GO.swap_sequence_literal, **o), n, want


def run_baseline(exe, tmp_path, xy, init, o):
    tsp = str(tmp_path / "case.tsp")
    write_tsp(tsp, xy)
    args = [exe, tsp, "--trace", "--epochs", str(o["epochs"]), "--seed", str(o["seed"]), "--run", str(o["run"]), "--n-nearest", str(o["n_nearest"])]
    if init is not None:
        ini = str(tmp_path / "case.init")
        open(ini, "w").write(" ".join(str(int(v)) for v in init) + "\n")
        args += ["--init", ini]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    head = [int(v) for v in lines[0].split()[:4]]
    log = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("I")]
    elog = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("E")]
    return head, [int(v) for v in lines[1].split()], log, elog


def masses_of_lib(lib, costs):
    c = np.asarray(costs, dtype=np.float32)
    m, r = np.zeros(len(c), dtype=np.float64), np.zeros(len(c), dtype=np.uint32)
    rc = lib.tl_gsa_masses(c.ctypes.data, len(c), m.ctypes.data, r.ctypes.data)
    return rc, m, r.tolist()


# ---------------------------------------------------------------- the draws
def test_no_two_roles_share_a_draw():
    for n, N, epochs, given in ((2, 25, 4, False), (5, 25, 3, True), (8, 27, 2, False), (13, 64, 2, True)):
        roles = GO.roles(n, N, epochs, given)
        assert len({(e, s) for e, s, _ in roles}) == len(roles) == (N - given) * (n - 1) + epochs * N * N
        assert max(e for e, _s, r in roles if r[0] != "shuffle") < GO.init_event(n, 0, 0) <= min(e for e, _s, r in roles if r[0] == "shuffle")
    assert GO.event(2 ** 32 - 2, 4096, 4095, 4095) < 2 ** 56 < GO.init_event(2, 0, 0) == 2 ** 58
    assert GO.uniform(2 ** 64 - 1) == 1.0 - 2.0 ** -53 and GO.uniform(0) == 0.0


def test_start_population_equals_the_swarms_for_equal_counts():
    key = GO.chain_key(7, 3)
    assert [GO.shuffled(key, 9, i) for i in range(30)] == [PO.shuffled(key, 9, i) for i in range(30)]


def test_draws_g_pulls_and_masses_equal_the_goldens_and_the_library(lib):
    for seed, run, event, slot, want in GOLD["draws"]:
        assert GO.draw(int(seed), run, int(event), slot) == int(want) == lib.tl_gsa_draw(int(seed), run, int(event), slot)
    for e, total, want in GOLD["g"]:
        assert GO.f64_bits(GO.g_of(e, total)) == int(want) == GO.f64_bits(lib.tl_gsa_g(e, total)), (e, total)
    for r, g, m, want in GOLD["pulls"]:
        assert GO.pull_swaps(r, g, m) == want == lib.tl_gsa_pull_swaps(r, g, m)
    for costs, want_m, want_rank in GOLD["masses"]:
        m, rank, _u = GO.masses_of(costs)
        rc, lm, lrank = masses_of_lib(lib, costs)
        assert rc == 0 and [GO.f64_bits(x) for x in m] == [int(v) for v in want_m] == [GO.f64_bits(x) for x in lm] and rank == want_rank == lrank


def test_g_starts_at_g0_and_never_exceeds_it(lib):
    """levy_exp(0) is exactly 1 and levy_exp of a non-positive argument is at most 1: g <= G0, the argument of kGsaMaxPull"""
    assert GO.g_of(0, 10_000) == 20.0 == lib.tl_gsa_g(0, 10_000) == lib.tl_gsa_g(0, 0) == lib.tl_gsa_g(0, 1)
    for epochs in (1, 2, 3, 7, 100, 10_000, 2 ** 32 - 2):
        es = sorted(e for e in {0, 1, 2, epochs // 3, epochs // 2, epochs - 2, epochs - 1} if 0 <= e < epochs)
        gs = [lib.tl_gsa_g(e, epochs) for e in es]
        assert all(0.0 < g <= 20.0 for g in gs) and gs == sorted(gs, reverse=True) and gs == [GO.g_of(e, epochs) for e in es]
    assert abs(lib.tl_gsa_g(9_999, 10_000) - 20.0 * np.exp(-0.9999)) < 1e-12


def test_pull_length_rounds_half_away_from_zero(lib):
    """x = k + 0.5 rounds up, just below stays; the product is (r g) mass, left to right"""
    for k in range(0, 20):
        x = k + 0.5
        below = float(np.nextafter(x, 0.0))
        for r, g, m, want in ((x / 32.0, 32.0, 1.0, k + 1), (below / 32.0, 32.0, 1.0, k), (1.0, x, 1.0, k + 1), (1.0, 1.0, below, k)):
            assert lib.tl_gsa_pull_swaps(r, g, m) == want == GO.pull_swaps(r, g, m), (r, g, m)
    assert lib.tl_gsa_pull_swaps(float("nan"), 20.0, 1.0) == 0 == lib.tl_gsa_pull_swaps(0.5, 20.0, 0.0) == lib.tl_gsa_pull_swaps(-1.0, 20.0, 1.0)


def test_a_pull_is_at_most_twenty_swaps(lib):
    """kGsaMaxPull: r < 1, g <= 20, mass <= 1 — the largest r there is against the largest g and mass, and a sweep of seeded draws
    against the masses of seeded costs"""
    top = 1.0 - 2.0 ** -53
    assert GO.MAX_PULL == 20 and lib.tl_gsa_pull_swaps(top, 20.0, 1.0) == 20 == GO.pull_swaps(top, 20.0, 1.0)
    assert re.search(r"constexpr uint32_t kGsaMaxPull = 20;", open(os.path.join(ROOT, "teeline_amd", "csrc", "gsa_spec.h")).read())
    rng = np.random.default_rng(11)
    worst_seen = 0
    for trial in range(40):
        N = int(rng.integers(25, 80))
        costs = rng.choice([1.0, 2.0, 3.5, 100.0, 7.25], size=N) if trial % 4 == 0 else rng.uniform(1.0, 1e4, size=N)
        m, _rank, _u = GO.masses_of(np.asarray(costs, dtype=np.float32))
        assert all(0.0 <= x <= 1.0 for x in m)
        key = GO.chain_key(trial, 0)
        for e in (0, 1, 50):
            g = GO.g_of(e, 100)
            for i in range(0, N, 7):
                for j in range(N):
                    k = GO.pull_swaps(GO.uniform(GO.draw_key(key, GO.event(e, N, i, j), 0)), g, m[j])
                    worst_seen = max(worst_seen, k)
    assert 1 <= worst_seen <= 20


# ---------------------------------------------------------------- the masses and the ranking
def test_masses_and_ranking_with_ties(lib):
    for N in (25, 26, 65):
        kb = (N + 1) // 2
        m, rank, uniform = GO.masses_of([7.0] * N)  # every cost equal: uniform masses, kbest = 0 .. k_best - 1
        rc, lm, lrank = masses_of_lib(lib, [7.0] * N)
        assert uniform and rc == 0 and m == [1.0 / N] * N == lm.tolist() and rank == list(range(N)) == lrank and rank[:kb] == list(range(kb))
        # two equal costs straddling the k_best cut: the lower index is inside
        costs = [float(100 + a) for a in range(N)]
        lo, hi = 3, N - 2
        order = sorted(range(N), key=lambda a: costs[a])
        costs[lo] = costs[hi] = costs[order[kb - 1]]  # ties with the agent at the cut
        m, rank, uniform = GO.masses_of(costs)
        rc, lm, lrank = masses_of_lib(lib, costs)
        assert not uniform and rc == 0 and rank == lrank and m == lm.tolist()
        tied = [a for a in range(N) if costs[a] == costs[lo]]
        at = [rank.index(a) for a in tied]
        assert at == sorted(at) and len(tied) == 3 and min(at) < kb <= max(at)  # ascending index among the equal, the cut between them
        assert rank == sorted(range(N), key=lambda a: (-m[a], a)) and abs(sum(m) - 1.0) < 1e-12


def test_sum_fitness_just_below_and_above_epsilon(lib):
    """worst - c is an f32 difference: 2^-53 (below f64::EPSILON = 2^-52) and 2^-51 (above) are both reachable near 2^-30"""
    base = np.float32(2.0 ** -30)
    ulp = float(np.nextafter(base, np.float32(1.0)) - base)
    assert ulp == 2.0 ** -53 and ulp < GO.EPSILON < 4 * ulp
    below = [float(base + np.float32(ulp))] + [float(base)] * 24           # sum_fitness = 24 x 2^-53 > epsilon: not uniform
    m, _r, uniform = GO.masses_of(below)
    assert not uniform and m[0] == 0.0 and m[1] == 1.0 / 24.0
    one = [float(base)] * 24 + [float(base + np.float32(ulp))]              # the worst is last: the same
    assert not GO.masses_of(one)[2]
    single = [float(base + np.float32(ulp))] * 24 + [float(base)]           # sum_fitness = 2^-53 < epsilon: uniform
    m, rank, uniform = GO.masses_of(single)
    assert uniform and m == [1.0 / 25.0] * 25 and rank == list(range(25))
    two = [float(base + np.float32(ulp))] * 23 + [float(base)] * 2          # 2 x 2^-53 = epsilon exactly: not below it
    assert not GO.masses_of(two)[2]
    for costs in (below, one, single, two):
        m, rank, _u = GO.masses_of(costs)
        rc, lm, lrank = masses_of_lib(lib, costs)
        assert rc == 0 and lm.tolist() == m and lrank == rank


def test_where_the_reference_panics(lib):
    from teeline_amd import _capi
    inf = float("inf")
    for costs in ([1.0, inf] + [2.0] * 23, [inf] * 25, [1.0, float("nan")] + [2.0] * 23):
        with pytest.raises(GO.RefPanics):
            GO.masses_of(costs)
        assert masses_of_lib(lib, costs)[0] == _capi.TL_ERR_REF_PANICS
    m = np.zeros(1)
    assert lib.tl_gsa_masses(None, 25, m.ctypes.data, m.ctypes.data) == _capi.TL_ERR_BADARG
    assert masses_of_lib(lib, [1.0] * 4097)[0] == _capi.TL_ERR_BADARG and masses_of_lib(lib, [])[0] == _capi.TL_ERR_BADARG
    g = K.tsplib("gr17")
    packed = np.array(g["packed"], dtype=np.float32)
    packed[:] = inf  # every edge: every start cost is inf, worst - c is NaN
    with pytest.raises(GO.RefPanics):
        GO.solve(g["xy"], packed, 17, None, epochs=1, seed=1)
    assert GO.solve(g["xy"], packed, 17, None, epochs=0, seed=1)["cost"] == inf  # no epoch, no ranking: the reference does not panic


# ---------------------------------------------------------------- the pull
def test_pull_is_a_prefix_of_every_statement_of_swap_sequence():
    rng = np.random.default_rng(3)
    for n in (2, 5, 17, 64, 65, 257, 600):
        for _ in range(4):
            s, t = (rng.permutation(n).tolist() for _ in range(2))
            full = GO.swap_sequence_literal(s, t)
            assert PO.swap_sequence_orbit(s, t) == full == FAST(s, t)  # the orbit rule is the form the device computes a prefix of
            for m in (0, 1, 20, len(full) + 3):
                assert GO.pull(s, t, m) == full[:m] == GO.pull(s, t, m, seq=FAST)


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_goldens(name):
    _xy, _packed, n, _init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    assert res["tour"].tolist() == want["tour"] and bits(res["cost"]) == want["cost_bits"] and res["counters"] == want["counters"]
    assert GO.log_words(res).tolist() == want["log"] and sha(GO.route_words(res, n)) == want["routes_sha256"]
    assert sha(GO.epoch_words(res)) == want["epochs_sha256"] and GO.epoch_words(res)[:1].tolist() == want["epochs_head"]
    GC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, _n, init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head == [o["epochs"], res["counters"]["moves"], res["counters"]["improved"], bits(res["cost"])] and bits(res["cost"]) == want["cost_bits"]
    assert route == res["tour"].tolist() == want["tour"]
    assert log == GO.log_words(res)[:, :3].tolist() and elog == GO.epoch_words(res).tolist()


@pytest.mark.parametrize("name", sorted(GC.SEEDED))
def test_cpp_restatement_on_the_seeded_cases(baseline, tmp_path, name):
    xy, _packed, n, init, o, _want = GC.seeded_case(name)
    res, _n, _w = seeded(name)
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head[1:] == [res["counters"]["moves"], res["counters"]["improved"], bits(res["cost"])] and route == res["tour"].tolist()
    assert log == GO.log_words(res)[:, :3].tolist() and elog == GO.epoch_words(res).tolist()


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--run", "5"], capture_output=True, text=True, check=True).stdout.splitlines()
    draws = [GO.draw(77, 5, GO.event(3, 25, i, j), 0) for i in range(5) for j in range(5)]
    gs = [GO.f64_bits(GO.g_of(e, total)) for total in (8, 10_000) for e in range(8)]
    assert [int(v) for v in out] == draws + gs


# ---------------------------------------------------------------- what the seeded cases are there for
@pytest.mark.parametrize("name", sorted(GC.SEEDED))
def test_seeded_cases_meet_their_conditions(name):
    res, _n, want = seeded(name)
    got = GC.conditions(res)
    assert want and set(want) <= got, (name, set(want) - got)
    assert set(want) <= set(GC.CONDITIONS)


def test_every_condition_is_met():
    """every condition of the scan by a seeded run; prefix_past_64_positions by planted inputs alone (two agents that agree on their
    first 64 positions do not come up in a small seeded run): tests/test_gpu_gravitational_search.py plants them for
    tl_gsa_selftest_pull, and the oracle's statement of them is checked here"""
    met = set()
    for name in GC.SEEDED:
        met |= GC.conditions(seeded(name)[0])
    assert met == set(GC.CONDITIONS) and GC.PLANTED_ONLY == ("prefix_past_64_positions",)
    for name, (src, dst, m) in GC.planted_pairs(600).items():
        pairs = GO.pull(src, dst, m, seq=FAST)
        assert pairs == GO.swap_sequence_literal(src, dst)[:m], name
        if name.startswith("agree_"):
            k = int(name.split("_")[1])
            assert pairs and pairs[0][0] >= k and (k < 64 or pairs[0][0] >= 64), name
    assert any(p[0][0] < 64 <= p[-1][0] for p in (GO.pull(s, d, m, seq=FAST) for s, d, m in GC.planted_pairs(600).values()) if p)  # a prefix across a chunk boundary


def test_initial_tour_and_sizes_are_covered():
    assert {GC.SEEDED[k][1] is not None for k in GC.SEEDED} == {True, False}
    assert {GC.SEEDED[k][0] for k in GC.SEEDED} >= {3, 5, 8, 52, 130, 600}
    assert GO.vmax(5) == 2 and GO.vmax(3) == 2 and GO.vmax(2) == 1


WRONG = {"epoch_start": "berlin52_default", "by_rank": "small8", "unstable": "small5_truncated", "no_cut": "small5_truncated"}


@pytest.mark.parametrize("mutate", sorted(WRONG))
def test_the_seeded_cases_tell_the_wrong_variants_apart(mutate):
    """every pull against the epoch-start positions, r keyed by the rank, ties in descending index, no cut to v_max: each changes the
    record of the seeded case named for it"""
    name = WRONG[mutate]
    xy, _packed, n, init, o, _want = GC.seeded_case(name)
    res, _n, _w = seeded(name)
    wrong = GO.solve(xy, None, n, init, mutate=mutate, **o)
    assert GO.epoch_words(wrong).tolist() != GO.epoch_words(res).tolist()


def test_small_n_and_epochs_zero():
    """n = 0 and n = 1: the reference does not panic — the masses are uniform, every sequence is empty, nothing improves"""
    for n in (0, 1):
        res = GO.solve(K.small(3)[:n], None, n, None, epochs=3, seed=1)
        assert res["tour"].tolist() == list(range(n)) and res["cost"] == 0 and len(res["improvements"]) == 1
        assert [m[0] for m in GO.messages(res)] == ["PathUpdate", "EpochUpdate", "EpochUpdate", "EpochUpdate", "Done"]
        moves = [m for ep in res["epochs"] for m in ep["moves"]]
        assert all(ep["uniform"] for ep in res["epochs"]) and not any(m["velocity"] for m in moves) and any(m["pulls"] for m in moves)
    init = GC.start_tour(8, 2)
    res = GO.solve(K.small(8), None, 8, init, epochs=0, seed=5)
    assert len(res["improvements"]) == 1 and res["epochs"] == [] and [m[0] for m in GO.messages(res)] == ["PathUpdate", "Done"]
    d = GO.dist_fn(K.small(8), None, 8)
    key = GO.chain_key(5, 0)
    starts = [init.tolist()] + [GO.shuffled(key, 8, i) for i in range(1, 25)]
    costs = [GO.tour_length(d, np.asarray(s)) for s in starts]
    first = min(range(25), key=lambda i: (costs[i], i))  # the FIRST minimum
    assert res["improvements"][0][1] == first and res["tour"].tolist() == starts[first]


# ---------------------------------------------------------------- plan, limits, names
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    N, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    lds, work = 163840, 8 << 30
    out = (C.byref(N), C.byref(t), C.byref(per))
    assert lib.tl_gravitational_search_plan(52, 3, 1, 256, lds, work, 0, *out) == 0 and (N.value, t.value, per.value) == (25, 256, 65535)
    assert lib.tl_gravitational_search_plan(130, 26, 1, 256, lds, work, 0, *out) == 0 and (N.value, t.value, per.value) == (26, 256, 65535)
    run_bytes = 2 * 25 * 1002 + 2 * 1002 + 14 * 25
    assert lib.tl_gravitational_search_plan(1002, 3, 64, 256, lds, 3 * run_bytes + 8 * 256, 0, *out) == 0 and per.value == 3
    up = lambda v: (v + 15) & ~15  # noqa: E731
    top = max(n for n in range(lds // 9, lds // 8 + 1) if 1536 + up(4 * n) + 2 * up(2 * n) <= lds)
    assert lib.tl_gravitational_search_plan(top, 3, 1, 256, lds, 1 << 40, 0, *out) == 0 and per.value >= 1
    for n, nn, w in ((top + 1, 3, 1 << 40), (0, 3, work), (1, 3, work), (1000, 3, 1000), (52, 4097, work)):
        assert lib.tl_gravitational_search_plan(n, nn, 1, 256, lds, w, 0, *out) == 0
        assert (N.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_gravitational_search_plan(52, 4096, 1, 256, lds, work, 0, *out) == 0 and N.value == 4096 and per.value >= 1
    assert lib.tl_gravitational_search_plan(52, 3, 1, 0, lds, work, 0, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_gravitational_search_plan(52, 3, 1, 256, lds, work, 1 << 31, *out) == _capi.TL_ERR_UNSUPPORTED and (N.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_gravitational_search_max_n(None) == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["gravitational_search"] == "gravitational_search" and "gsa" not in P.SOLVER_NAMES and "gravitational_search" in P.AUTO_EXPAND_WITH_SHUFFLE
    assert P.steps_for_solve("gravitational_search") == ["shuffle", "gravitational_search"]
    assert P.steps_for_solve("Gravitational_Search", no_seed=True) == ["gravitational_search"]
    with pytest.raises(ValueError, match="the seeded gravitational search of this build is `gravitational_search`"):
        P.steps_for_solve("gsa")
    with pytest.raises(ValueError, match="the seeded gravitational search of this build is `gravitational_search`"):
        P.run_pipeline_stages(None, ["gsa"])
    assert P.REFUSED_ALIASES["gsa"] == "gravitational_search"


def test_header_bindings_and_flags_agree(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_gravitational_search", "tl_gravitational_search_trace", "tl_gravitational_search_population", "tl_gravitational_search_max_n",
                "tl_gravitational_search_plan", "tl_gsa_draw", "tl_gsa_g", "tl_gsa_pull_swaps", "tl_gsa_masses", "tl_gsa_selftest_pull"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)
    assert re.search(r"typedef struct tl_gsa_opts \{[^}]*uint32_t epochs;[^}]*uint32_t n_nearest;[^}]*uint32_t span_epochs;[^}]*\} tl_gsa_opts;", text)
    assert [f for f, _ in _capi.TlGsaOpts._fields_] == ["epochs", "n_nearest", "span_epochs"] and C.sizeof(_capi.TlGsaOpts) == 12
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags and "TL_FLAG_GSA" not in text  # the flag bits are all given out: the span of a launch is an option, not a flag
    rust = open(os.path.join(ROOT, "integration", "teeline-gpu", "src", "lib.rs")).read()
    for sym in ("tl_gravitational_search", "tl_gravitational_search_trace", "tl_gravitational_search_population", "tl_gravitational_search_max_n", "tl_gsa_masses"):
        assert re.search(rf"\bfn {sym}\(", rust), sym
