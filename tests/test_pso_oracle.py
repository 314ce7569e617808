"""The particle swarm solver without a GPU: the statement of the specification (tests/_pso_oracle.py) against the stand-alone C++
restatement (tests/probes/pso_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the rounding, the inertia
weight, the three forms of the swap sequence, the reference's unit vectors, the conditions every seeded case is there for, the
deliberately wrong variants those cases tell apart; pipeline names."""
import ctypes as C
import hashlib
import itertools
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _pso_cases as PC
import _pso_oracle as PO
import _sa_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_pso.json")))
CASES = PC.golden_cases()
bits = PO.bits


def f64_of(text):
    return struct.unpack("<d", struct.pack("<Q", int(text)))[0]


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pso") / "pso_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "pso_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, o = CASES[name]
    return PO.solve_cached((name,), xy, packed, n, init, **o)


def run_baseline(exe, tmp_path, xy, init, o, extra=()):
    tsp = str(tmp_path / "case.tsp")
    write_tsp(tsp, xy)
    args = [exe, tsp, "--trace", "--epochs", str(o["epochs"]), "--seed", str(o["seed"]), "--run", str(o["run"]), "--n-nearest", str(o["n_nearest"])] + list(extra)
    if init is not None:
        ini = str(tmp_path / "case.init")
        open(ini, "w").write(" ".join(str(int(v)) for v in init) + "\n")
        args += ["--init", ini]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    head = [int(v) for v in lines[0].split()[:4]]
    log = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("I")]
    elog = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("E")]
    return head, [int(v) for v in lines[1].split()], log, elog


# ---------------------------------------------------------------- the draws
def test_no_two_roles_share_a_draw():
    for n, P, epochs, seeded in ((2, 30, 4, False), (5, 30, 7, True), (8, 33, 5, False), (13, 64, 3, True)):
        roles = PO.roles(n, P, epochs, seeded)
        assert len({(e, s) for e, s, _ in roles}) == len(roles) == (P - seeded) * (n - 1) + 2 * epochs * P
        assert max(e for e, _s, r in roles if r[0] != "shuffle") < PO.init_event(n, 0, 0) <= min([e for e, _s, r in roles if r[0] == "shuffle"])
    # the largest epoch event of a supported call stays below the first start event
    assert PO.step_event(2 ** 32 - 2, PO.MAX_PARTICLES, PO.MAX_PARTICLES - 1) < PO.init_event(2, 0, 0)
    u = PO.draw(1, 0, 0, 0)
    assert 0.0 <= PO.uniform(u) < 1.0 and PO.uniform(2 ** 64 - 1) == 1.0 - 2.0 ** -53 and PO.uniform(0) == 0.0


def test_draws_keeps_and_weights_equal_the_goldens_and_the_library(lib):
    for seed, run, event, slot, want in GOLD["draws"]:
        assert PO.draw(int(seed), run, int(event), slot) == int(want) == lib.tl_pso_draw(int(seed), run, int(event), slot)
    for xb, want in GOLD["keeps"]:
        assert PO.keep(f64_of(xb)) == want == lib.tl_pso_keep(f64_of(xb)), f64_of(xb)
    for e, of, wb in GOLD["weights"]:
        assert PO.weight(e, of) == f64_of(wb) == lib.tl_pso_weight(e, of)


# ---------------------------------------------------------------- the rounding and the weight
def test_rounding_is_half_away_from_zero(lib):
    for x, want in ((4.5, 5), (2.5, 3), (0.5, 1), (1.5, 2), (0.49999999999999994, 0), (0.9 * 5, 5), (0.0, 0), (2.4999999999999996, 2), (7.0, 7), (-1.0, 0)):
        assert PO.keep(x) == want == lib.tl_pso_keep(x), x
    assert int(np.round(4.5)) == 4 and int(np.round(2.5)) == 2  # what np.round would give: half to even
    assert int(np.floor(0.49999999999999994 + 0.5)) == 1      # what floor(x + 0.5) would give just below .5
    assert lib.tl_pso_keep(float("nan")) == 0 and lib.tl_pso_keep(5e9) == 0xFFFFFFFF
    rng = np.random.default_rng(1)
    for x in np.concatenate([rng.uniform(0, 100, 300), np.arange(0, 60) + 0.5, np.nextafter(np.arange(1, 60) + 0.5, 0)]):
        assert PO.keep(float(x)) == lib.tl_pso_keep(float(x)) == int(np.floor(x)) + (x - np.floor(x) >= 0.5)
    # a keep above its length: 1.5 r can exceed 1, `take` clamps
    assert PO.keep((1.5 * 0.99) * 7) == 10 > 7


def test_weight(lib):
    assert PO.weight(0, 10000) == 0.9 == lib.tl_pso_weight(0, 10000)
    assert PO.weight(9999, 10000) == 0.9 - (0.9 - 0.4) * (9999 / 10000) == lib.tl_pso_weight(9999, 10000) > 0.4
    assert PO.weight(0, 0) == 0.9 == lib.tl_pso_weight(0, 0) and PO.weight(0, 1) == 0.9 == lib.tl_pso_weight(0, 1)
    for e, of in ((1, 3), (2, 3), (5, 7), (39, 40), (123, 1000)):
        assert PO.weight(e, of) == lib.tl_pso_weight(e, of)
    assert PO.vmax(1) == 1 and PO.vmax(2) == 1 and PO.vmax(3) == 2 and PO.vmax(20) == 7 and PO.vmax(52) == 19 and PO.vmax(100) == 35 and PO.vmax(1002) == 351
    assert PO.particles(3) == 30 and PO.particles(30) == 30 and PO.particles(31) == 31


# ---------------------------------------------------------------- the swap sequence
def test_orbit_form_equals_the_literal_loop_exhaustively():
    """every pair of permutations up to n = 5; at n = 6 every target against the identity — which is every pair up to a renaming of
    the cities, and the sequence holds positions only — and against every 37th other start besides"""
    for n in range(0, 7):
        perms = list(itertools.permutations(range(n)))
        for a in perms[:1 if n == 6 else None] + (perms[1::37] if n == 6 else []):
            for b in perms:
                want = PO.swap_sequence_literal(a, b)
                assert want == PO.swap_sequence_orbit(a, b) == PO.swap_sequence_inverse(a, b), (a, b)
                assert PO.apply_swaps(a, want) == list(b) and len(want) == n - len(PO.orbits(a, b)[1])


def test_orbit_form_equals_the_literal_loop_on_random_pairs():
    rng = np.random.default_rng(7)
    for n in list(range(7, 201)) + [257, 600]:
        a, b = rng.permutation(n), rng.permutation(n)
        want = PO.swap_sequence_literal(a, b)
        assert want == PO.swap_sequence_orbit(a, b) == PO.swap_sequence_inverse(a, b), n
        assert all(i < j for i, j in want) and [i for i, _ in want] == sorted(i for i, _ in want)
    n = 300  # one n-cycle: every position but the last has a pair
    a, b = np.arange(n), np.roll(np.arange(n), 1)
    assert len(PO.swap_sequence_orbit(a, b)) == n - 1 and PO.swap_sequence_orbit(a, b) == PO.swap_sequence_literal(a, b)


def test_the_reference_unit_vectors():
    """route.rs tests: swap_sequence([1,2,3,4], [1,3,2,4]) applied gives the target; identity gives the empty sequence"""
    for seq in (PO.swap_sequence_literal, PO.swap_sequence_orbit, PO.swap_sequence_inverse):
        s = seq([0, 1, 2, 3], [0, 2, 1, 3])
        assert s == [(1, 2)] and PO.apply_swaps([1, 2, 3, 4], s) == [1, 3, 2, 4]
        assert seq([0, 1, 2, 3], [0, 1, 2, 3]) == [] and seq([], []) == [] and seq([0], [0]) == []
    assert PO.apply_swaps([1, 2, 3], [(0, 1), (1, 2)]) == [2, 3, 1] and PO.apply_swaps([1, 2, 3], []) == [1, 2, 3]


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_goldens(name):
    _xy, _packed, n, _init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    assert res["tour"].tolist() == want["tour"] and bits(res["cost"]) == want["cost_bits"] and res["counters"] == want["counters"]
    assert PO.log_words(res).tolist() == want["log"] and sha(PO.route_words(res, n)) == want["routes_sha256"]
    assert sha(PO.epoch_words(res)) == want["epochs_sha256"] and PO.epoch_words(res)[:1].tolist() == want["epochs_head"]
    PC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, _n, init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    for extra in ((), ("--inverse-table",)):
        head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o, extra)
        assert head == [o["epochs"], res["counters"]["steps"], res["counters"]["improved"], bits(res["cost"])] and bits(res["cost"]) == want["cost_bits"]
        assert route == res["tour"].tolist() == want["tour"]
        assert log == PO.log_words(res)[:, :3].tolist() and elog == PO.epoch_words(res).tolist()


@pytest.mark.parametrize("name", sorted(PC.SEEDED))
def test_cpp_restatement_on_the_seeded_cases(baseline, tmp_path, name):
    xy, _packed, n, init, o, _want = PC.seeded_case(name)
    res = PO.solve_cached(("seeded", name), xy, None, n, init, **o)
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head[1:] == [res["counters"]["steps"], res["counters"]["improved"], bits(res["cost"])] and route == res["tour"].tolist()
    assert log == PO.log_words(res)[:, :3].tolist() and elog == PO.epoch_words(res).tolist()


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--run", "5"], capture_output=True, text=True, check=True).stdout.split()
    draws = [PO.draw(77, 5, base + e, s) for base in (0, 1 << 58) for e in range(8) for s in range(28)]
    assert [int(v) for v in out[:len(draws)]] == draws
    keeps = [PO.keep(x) for x in (0.0, 0.49999999999999994, 0.5, 1.5, 2.5, 4.5, 0.9 * 5.0, 2.4999999999999996, 1e9 + 0.5)] + [0, 0xFFFFFFFF]
    assert [int(v) for v in out[len(draws):len(draws) + 11]] == keeps
    assert [float(v) for v in out[len(draws) + 11:]] == [PO.weight(e, of) for e in (0, 1, 7, 9999) for of in (0, 1, 8, 10000)]


# ---------------------------------------------------------------- what the seeded cases are there for
@pytest.mark.parametrize("name", sorted(PC.SEEDED))
def test_seeded_cases_meet_their_conditions(name):
    xy, _packed, n, init, o, want = PC.seeded_case(name)
    res = PO.solve_cached(("seeded", name), xy, None, n, init, **o)
    got = PC.conditions(res)
    assert set(want) <= got, (name, set(want) - got)
    assert set(want) <= set(PC.CONDITIONS)


def test_every_condition_is_met_and_a_cut_inside_inertia_cannot_happen():
    met = set()
    for name in PC.SEEDED:
        xy, _packed, n, init, o, _want = PC.seeded_case(name)
        res = PO.solve_cached(("seeded", name), xy, None, n, init, **o)
        met |= PC.conditions(res)  # (asserts parts[0] <= len(v) <= v_max on every step)
        assert all(s["vlen"] <= res["vmax"] for ep in res["epochs"] for s in ep["steps"])
    assert met == set(PC.CONDITIONS)


@pytest.mark.parametrize("mutate", ["no_redo", "half_even", "truncate_first"])
def test_the_seeded_cases_tell_the_wrong_variants_apart(mutate):
    """the redo dropped, half-to-even rounding, truncation before concatenation: each changes the per-epoch record of a seeded case"""
    differs = 0
    for name in sorted(PC.SEEDED):
        xy, _packed, n, init, o, _want = PC.seeded_case(name)
        res = PO.solve_cached(("seeded", name), xy, None, n, init, **o)
        wrong = PO.solve(xy, None, n, init, mutate=mutate, **o)
        differs += PO.epoch_words(wrong).tolist() != PO.epoch_words(res).tolist()
    assert differs >= 1


def test_small_n_and_epochs_zero():
    for n in (0, 1):
        res = PO.solve(K.small(3)[:n], None, n, None, epochs=3, seed=1)
        assert res["tour"].tolist() == list(range(n)) and res["cost"] == 0 and len(res["improvements"]) == 1 and [m[0] for m in PO.messages(res)] == [
            "PathUpdate", "EpochUpdate", "EpochUpdate", "EpochUpdate", "Done"]
    init = PC.start_tour(8, 2)
    res = PO.solve(K.small(8), None, 8, init, epochs=0, seed=5)
    assert len(res["improvements"]) == 1 and res["epochs"] == [] and [m[0] for m in PO.messages(res)] == ["PathUpdate", "Done"]
    d = PO.dist_fn(K.small(8), None, 8)
    starts = [init.tolist()] + [PO.shuffled(PO.chain_key(5, 0), 8, i) for i in range(1, 30)]
    costs = [PO.tour_length(d, np.asarray(s)) for s in starts]
    first = min(range(30), key=lambda i: (costs[i], i))  # the FIRST minimum
    assert res["improvements"][0][1] == first and res["tour"].tolist() == starts[first]
    two = PO.solve(K.small(2), None, 2, None, epochs=4, seed=2)  # n = 2: v_max = 1, sequences of at most one swap
    assert two["vmax"] == 1 and sorted(two["tour"].tolist()) == [0, 1] and all(v <= 1 for ep in two["epochs"] for v in ep["vlens"])


# ---------------------------------------------------------------- plan, limits, names
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    P, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    lds, work = 163840, 8 << 30
    out = (C.byref(P), C.byref(t), C.byref(per))
    assert lib.tl_particle_swarm_plan(52, 3, 1, 256, lds, work, 0, *out) == 0 and (P.value, t.value, per.value) == (30, 64, 65535)
    assert lib.tl_particle_swarm_plan(130, 31, 1, 256, lds, work, 0, *out) == 0 and (P.value, t.value, per.value) == (31, 192, 65535)
    assert lib.tl_particle_swarm_plan(1002, 3, 64, 256, lds, work, 0, *out) == 0 and (P.value, t.value) == (30, 256) and per.value >= 10000
    run_bytes = 6 * 30 * 1002 + 2 * 1002 + 8 * 30 * 351 + 16 * 30  # a small workspace bounds what one launch sequence holds
    assert lib.tl_particle_swarm_plan(1002, 3, 64, 256, lds, 3 * run_bytes + 2560, 0, *out) == 0 and per.value == 3
    top = max(n for n in range(lds // 16, lds // 14 + 1) if 256 + 2 * ((4 * n + 15) & ~15) + ((4 * PO.vmax(n) + 15) & ~15) + 3 * ((2 * n + 15) & ~15) <= lds)
    assert lib.tl_particle_swarm_plan(top, 3, 1, 256, lds, 1 << 40, 0, *out) == 0 and per.value >= 1 and t.value == 256
    for n, nn, w in ((top + 1, 3, 1 << 40), (0, 3, work), (1, 3, work), (1000, 3, 1000), (52, 4097, work)):
        assert lib.tl_particle_swarm_plan(n, nn, 1, 256, lds, w, 0, *out) == 0
        assert (P.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_particle_swarm_plan(52, 4096, 1, 256, lds, work, 0, *out) == 0 and P.value == 4096 and per.value >= 1
    assert lib.tl_particle_swarm_plan(52, 3, 1, 0, lds, work, 0, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_particle_swarm_plan(52, 3, 1, 256, lds, work, 1 << 31, *out) == _capi.TL_ERR_UNSUPPORTED and (P.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_particle_swarm_max_n(None) == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["particle_swarm"] == "particle_swarm" and "pso" not in P.SOLVER_NAMES and "particle_swarm" in P.AUTO_EXPAND_WITH_SHUFFLE
    assert P.steps_for_solve("particle_swarm") == ["shuffle", "particle_swarm"] and P.steps_for_solve("Particle_Swarm", no_seed=True) == ["particle_swarm"]
    with pytest.raises(ValueError, match="the seeded particle swarm of this build is `particle_swarm`"):
        P.steps_for_solve("pso")
    with pytest.raises(ValueError, match="the seeded particle swarm of this build is `particle_swarm`"):
        P.run_pipeline_stages(None, ["pso"])
    assert P.REFUSED_ALIASES["pso"] == "particle_swarm"
    assert P.steps_for_solve("ant_colony") == ["shuffle", "ant_colony"] and P.steps_for_solve("tabu_search") == ["nn", "tabu_search"]


def test_header_bindings_and_flags_agree(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_particle_swarm", "tl_particle_swarm_trace", "tl_particle_swarm_population", "tl_particle_swarm_max_n", "tl_particle_swarm_plan",
                "tl_pso_draw", "tl_pso_weight", "tl_pso_keep", "tl_pso_selftest_swap_sequence"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)
    assert re.search(r"typedef struct tl_pso_opts \{[^}]*uint32_t epochs;[^}]*uint32_t n_nearest;[^}]*\} tl_pso_opts;", text)
    assert [f for f, _ in _capi.TlPsoOpts._fields_] == ["epochs", "n_nearest"] and C.sizeof(_capi.TlPsoOpts) == 8
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags  # the bit the solver refuses is one no flag has: no new flag was added
