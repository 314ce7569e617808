"""The flower pollination solver without a GPU: the statement of the specification (tests/_fpa_oracle.py) against the stand-alone
C++ restatement (tests/probes/fpa_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the seeded draws (j
and k without the rejection loop), the switch probability, both prefix lengths, the oracle's move against a second literal
implementation, the conditions every seeded case is there for, the deliberately wrong variants those cases tell apart; names."""
import ctypes as C
import hashlib
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _fpa_cases as FC
import _fpa_oracle as FO
import _pso_oracle as PO
import _sa_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_fpa.json")))
CASES = FC.golden_cases()
bits = FO.bits
FAST = FO.swap_sequence_inverse


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fpa") / "fpa_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "fpa_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, o = CASES[name]
    return FO.solve_cached((name,), xy, packed, n, init, **o)


def seeded(name):
    xy, _packed, n, init, o, want = FC.seeded_case(name)
    return FO.solve_cached(("seeded", name), xy, None, n, init, seq=FAST if n >= 600 else FO.swap_sequence_literal, **o), n, want


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


# ---------------------------------------------------------------- the draws
def test_no_two_roles_share_a_draw():
    for n, N, epochs, given in ((2, 25, 4, False), (5, 25, 3, True), (8, 27, 2, False), (13, 64, 2, True)):
        roles = FO.roles(n, N, epochs, given)
        assert len({(e, s) for e, s, _ in roles}) == len(roles) == (N - given) * (n - 1) + epochs * N * (FO.WORDS + 4)
        assert max(s for _e, s, _r in roles) < 32
        assert max(e for e, _s, r in roles if r[0] != "shuffle") < FO.init_event(n, 0, 0) <= min(e for e, _s, r in roles if r[0] == "shuffle")
    assert FO.event(2 ** 32 - 2, 4096, 4095) < 2 ** 44 < FO.init_event(2, 0, 0)
    assert FO.uniform(2 ** 64 - 1) == 1.0 - 2.0 ** -53 and FO.uniform(0) == 0.0


def test_start_population_equals_the_swarms_for_equal_counts():
    key = FO.chain_key(7, 3)
    assert [FO.shuffled(key, 9, i) for i in range(30)] == [PO.shuffled(key, 9, i) for i in range(30)]


@pytest.mark.parametrize("N", [25, 26, 64])
def test_partners_step_over_the_excluded_indices(N):
    """over a full enumeration of position's outputs every allowed value is reached exactly once (equal counts: the distribution
    of the rejection loop), j != i and k outside {i, j}, for every i; and the seeded draws obey the same"""
    for i in range(N):
        js = [FO.step_over(r, [i]) for r in range(N - 1)]
        assert sorted(js) == [v for v in range(N) if v != i]
        for j in (js[0], js[N // 2], js[-1]) if N > 26 else js:
            ks = [FO.step_over(r, [i, j]) for r in range(N - 2)]
            assert sorted(ks) == [v for v in range(N) if v not in (i, j)]
    key = FO.chain_key(5, 1)
    seen_j, seen_k = set(), set()
    for e in range(40 * N):
        for i in (0, 1, N // 2, N - 2, N - 1):
            j, k = FO.partners(key, FO.event(e, N, i), i, N)
            assert j != i and k not in (i, j) and 0 <= j < N and 0 <= k < N
            if i == N // 2:
                seen_j.add(j)
                seen_k.add(k)
    assert seen_j == seen_k == set(range(N)) - {N // 2}  # each allowed value is reached
    assert FO.position(2 ** 64 - 1, N - 1) == N - 2 and FO.position(0, N - 1) == 0  # position's outputs are exactly 0 .. m - 1


def test_draws_partners_and_lengths_equal_the_goldens_and_the_library(lib):
    for seed, run, event, slot, want in GOLD["draws"]:
        assert FO.draw(int(seed), run, int(event), slot) == int(want) == lib.tl_fpa_draw(int(seed), run, int(event), slot)
    key = FO.chain_key(77, 5)
    for N, rows in GOLD["partners"]:
        for i, (wj, wk) in enumerate(rows):
            j, k = C.c_uint32(), C.c_uint32()
            assert lib.tl_fpa_partners(77, 5, 3, i, N, C.byref(j), C.byref(k)) == 0
            assert (j.value, k.value) == (wj, wk) == FO.partners(key, FO.event(3, N, i), i, N)
    for x, ln, wg, wl in GOLD["lengths"]:
        assert (lib.tl_fpa_global_swaps(x, ln), lib.tl_fpa_local_swaps(x, ln)) == (wg, wl) == (FO.global_swaps(x, ln), FO.local_swaps(x, ln))


def test_switch_prob(lib):
    below = float(np.nextafter(np.float32(0.01), np.float32(0.0)))  # the largest f32 below 0.01f
    want = {0.0: 0.8, 0.001: 0.8, below: 0.8, 0.01: float(np.float32(0.01)), 0.5: 0.5, 1.0: 1.0}
    for p, w in want.items():
        assert lib.tl_fpa_switch_prob(p) == w == FO.switch_prob(p), p
    assert float(np.float32(0.01)) != 0.01  # (f64) 0.01f is not 0.01: the widening is part of the statement


def test_prefix_lengths(lib):
    """0; a product that is an exact integer; just above one; >= len; NaN; +inf — for both functions"""
    up = float(np.nextafter(0.5, 1.0))
    for x, ln, wg, wl in ((0.0, 8, 1, 1), (0.5, 8, 2, 4), (up, 8, 3, 5), (0.25, 8, 1, 2), (2.0, 8, 8, 8), (2.5, 8, 8, 8), (1.75, 8, 7, 8),
                          (float("nan"), 8, 1, 1), (float("inf"), 8, 8, 8), (0.7, 1, 1, 1), (0.7, 0, 0, 0)):
        assert (FO.global_swaps(x, ln), FO.local_swaps(x, ln)) == (wg, wl), (x, ln)
        assert (lib.tl_fpa_global_swaps(x, ln), lib.tl_fpa_local_swaps(x, ln)) == (wg, wl), (x, ln)


# ---------------------------------------------------------------- the move
def second_move(flower, source, target, prefix):
    """a second, independent literal statement: positions swapped while the working copy of `source` is turned into `target`"""
    work, out, done = list(source), list(flower), 0
    for i in range(len(work) - 1):
        if work[i] == target[i]:
            continue
        j = next(q for q in range(i + 1, len(work)) if work[q] == target[i])
        work[i], work[j] = work[j], work[i]
        if done < prefix:
            out[i], out[j] = out[j], out[i]
        done += 1
    return done, out


def test_move_equals_a_second_literal_statement_exhaustively():
    for n in range(0, 5):
        perms = list(itertools.permutations(range(n)))
        for f, s, t in itertools.product(perms, repeat=3):
            ln = len(FO.swap_sequence_literal(s, t))
            for p in range(ln + 2):
                assert FO.pollinate(f, s, t, p) == second_move(f, s, t, p)
            assert FO.pollinate(f, s, t, ln, seq=FAST) == second_move(f, s, t, ln) and FO.pollinate(f, s, t, ln, seq=PO.swap_sequence_orbit)[1] == second_move(f, s, t, ln)[1]


def test_move_equals_a_second_literal_statement_on_random_tours():
    rng = np.random.default_rng(3)
    for n in (5, 17, 64, 65, 257, 600):
        for _ in range(4):
            f, s, t = (rng.permutation(n).tolist() for _ in range(3))
            ln = len(FO.swap_sequence_literal(s, t))
            for p in (0, 1, ln // 2, ln):
                want = second_move(f, s, t, p)
                assert FO.pollinate(f, s, t, p) == want and FO.pollinate(f, s, t, p, seq=FAST) == want
            assert PO.swap_sequence_orbit(s, t) == FO.swap_sequence_literal(s, t)  # the form the device computes


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_goldens(name):
    _xy, _packed, n, _init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    assert res["tour"].tolist() == want["tour"] and bits(res["cost"]) == want["cost_bits"] and res["counters"] == want["counters"]
    assert FO.log_words(res).tolist() == want["log"] and sha(FO.route_words(res, n)) == want["routes_sha256"]
    assert sha(FO.epoch_words(res)) == want["epochs_sha256"] and FO.epoch_words(res)[:1].tolist() == want["epochs_head"]
    FC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, _n, init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head == [o["epochs"], res["counters"]["moves"], res["counters"]["improved"], bits(res["cost"])] and bits(res["cost"]) == want["cost_bits"]
    assert route == res["tour"].tolist() == want["tour"]
    assert log == FO.log_words(res)[:, :3].tolist() and elog == FO.epoch_words(res).tolist()


@pytest.mark.parametrize("name", sorted(FC.SEEDED))
def test_cpp_restatement_on_the_seeded_cases(baseline, tmp_path, name):
    xy, _packed, n, init, o, _want = FC.seeded_case(name)
    res, _n, _w = seeded(name)
    head, route, log, elog = run_baseline(baseline, tmp_path, xy, init, o)
    assert head[1:] == [res["counters"]["moves"], res["counters"]["improved"], bits(res["cost"])] and route == res["tour"].tolist()
    assert log == FO.log_words(res)[:, :3].tolist() and elog == FO.epoch_words(res).tolist()


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--run", "5"], capture_output=True, text=True, check=True).stdout.splitlines()
    draws = [FO.draw(77, 5, base + e, s) for base in (0, 1 << 58) for e in range(8) for s in range(28)]
    assert [int(v) for v in out[:len(draws)]] == draws
    want = [list(p) for _N, rows in GOLD["partners"] for p in rows]
    assert [[int(v) for v in ln.split()] for ln in out[len(draws):]] == want


# ---------------------------------------------------------------- what the seeded cases are there for
@pytest.mark.parametrize("name", sorted(FC.SEEDED))
def test_seeded_cases_meet_their_conditions(name):
    res, _n, want = seeded(name)
    got = FC.conditions(res)
    assert set(want) <= got, (name, set(want) - got)
    assert set(want) <= set(FC.CONDITIONS)


def test_every_condition_is_met():
    met = set()
    for name in FC.SEEDED:
        met |= FC.conditions(seeded(name)[0])
    assert met == set(FC.CONDITIONS)


def test_initial_tour_and_mutation_probabilities_are_covered():
    inits = {FC.SEEDED[k][1] is not None for k in FC.SEEDED}
    probs = {FC.SEEDED[k][2]["mutation_probability"] for k in FC.SEEDED}
    assert inits == {True, False} and {0.001, 0.01, 1.0} <= probs
    res, _n, _w = seeded("berlin52_all_global")
    assert all(m["glob"] for ep in res["epochs"] for m in ep["moves"])


WRONG = {"epoch_start": "berlin52_default", "le": "small3_empty_local", "no_half": "berlin52_all_global"}


@pytest.mark.parametrize("mutate", sorted(WRONG))
def test_the_seeded_cases_tell_the_wrong_variants_apart(mutate):
    """the second build dropped (every flower moves against the epoch-start state), acceptance with <=, the global length without
    the factor 0.5: each changes the record of the seeded case named for it"""
    name = WRONG[mutate]
    xy, _packed, n, init, o, _want = FC.seeded_case(name)
    res, _n, _w = seeded(name)
    wrong = FO.solve(xy, None, n, init, mutate=mutate, **o)
    assert FO.epoch_words(wrong).tolist() != FO.epoch_words(res).tolist()


def test_small_n_and_epochs_zero():
    """n = 0 and n = 1: the reference does not panic — every sequence is empty, nothing is accepted"""
    for n in (0, 1):
        res = FO.solve(K.small(3)[:n], None, n, None, epochs=3, mutation_probability=0.5, seed=1)
        assert res["tour"].tolist() == list(range(n)) and res["cost"] == 0 and len(res["improvements"]) == 1
        assert [m[0] for m in FO.messages(res)] == ["PathUpdate", "EpochUpdate", "EpochUpdate", "EpochUpdate", "Done"]
        moves = [m for ep in res["epochs"] for m in ep["moves"]]
        assert not any(m["accepted"] or m["again"] or m["len"] or m["prefix"] for m in moves) and {m["glob"] for m in moves} == {True, False}
    init = FC.start_tour(8, 2)
    res = FO.solve(K.small(8), None, 8, init, epochs=0, seed=5)
    assert len(res["improvements"]) == 1 and res["epochs"] == [] and [m[0] for m in FO.messages(res)] == ["PathUpdate", "Done"]
    d = FO.dist_fn(K.small(8), None, 8)
    key = FO.chain_key(5, 0)
    starts = [init.tolist()] + [FO.shuffled(key, 8, i) for i in range(1, 25)]
    costs = [FO.tour_length(d, np.asarray(s)) for s in starts]
    first = min(range(25), key=lambda i: (costs[i], i))  # the FIRST minimum
    assert res["improvements"][0][1] == first and res["tour"].tolist() == starts[first]


# ---------------------------------------------------------------- plan, limits, names
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    N, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    lds, work = 163840, 8 << 30
    out = (C.byref(N), C.byref(t), C.byref(per))
    assert lib.tl_flower_pollination_plan(52, 3, 1, 256, lds, work, 0, *out) == 0 and (N.value, t.value, per.value) == (25, 64, 65535)
    assert lib.tl_flower_pollination_plan(130, 26, 1, 256, lds, work, 0, *out) == 0 and (N.value, t.value, per.value) == (26, 192, 65535)
    run_bytes = 4 * 25 * 1002 + 2 * 1002 + 12 * 25
    assert lib.tl_flower_pollination_plan(1002, 3, 64, 256, lds, 3 * run_bytes + 9 * 256, 0, *out) == 0 and per.value == 3 and t.value == 256
    up = lambda v: (v + 15) & ~15  # noqa: E731
    top = max(n for n in range(lds // 11, lds // 10 + 1) if 768 + up(4 * n) + 3 * up(2 * n) <= lds)
    assert lib.tl_flower_pollination_plan(top, 3, 1, 256, lds, 1 << 40, 0, *out) == 0 and per.value >= 1 and t.value == 256
    for n, nn, w in ((top + 1, 3, 1 << 40), (0, 3, work), (1, 3, work), (1000, 3, 1000), (52, 4097, work)):
        assert lib.tl_flower_pollination_plan(n, nn, 1, 256, lds, w, 0, *out) == 0
        assert (N.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_flower_pollination_plan(52, 4096, 1, 256, lds, work, 0, *out) == 0 and N.value == 4096 and per.value >= 1
    assert lib.tl_flower_pollination_plan(52, 3, 1, 0, lds, work, 0, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_flower_pollination_plan(52, 3, 1, 256, lds, work, 1 << 31, *out) == _capi.TL_ERR_UNSUPPORTED and (N.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_flower_pollination_max_n(None) == 0
    j = C.c_uint32()
    for i, n_fl in ((0, 2), (25, 25), (0, 4097)):
        assert lib.tl_fpa_partners(1, 0, 0, i, n_fl, C.byref(j), C.byref(j)) == _capi.TL_ERR_BADARG
    assert lib.tl_fpa_partners(1, 0, 0, 0, 25, None, C.byref(j)) == _capi.TL_ERR_BADARG


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["flower_pollination"] == "flower_pollination" and "fpa" not in P.SOLVER_NAMES and "flower_pollination" in P.AUTO_EXPAND_WITH_SHUFFLE
    assert P.steps_for_solve("flower_pollination") == ["shuffle", "flower_pollination"] and P.steps_for_solve("Flower_Pollination", no_seed=True) == ["flower_pollination"]
    with pytest.raises(ValueError, match="the seeded flower pollination of this build is `flower_pollination`"):
        P.steps_for_solve("fpa")
    with pytest.raises(ValueError, match="the seeded flower pollination of this build is `flower_pollination`"):
        P.run_pipeline_stages(None, ["fpa"])
    assert P.REFUSED_ALIASES["fpa"] == "flower_pollination"
    from teeline_amd.host import flower_pollination as F
    with pytest.raises(ValueError, match="mutation_probability"):
        F.FPAOptions(mutation_probability=1.5).validate()
    assert F.FPAOptions().mutation_probability == 0.001 and F.FPAOptions().heuristic.epochs == 10_000


def test_header_bindings_and_flags_agree(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_flower_pollination", "tl_flower_pollination_trace", "tl_flower_pollination_population", "tl_flower_pollination_max_n",
                "tl_flower_pollination_plan", "tl_fpa_draw", "tl_fpa_switch_prob", "tl_fpa_global_swaps", "tl_fpa_local_swaps", "tl_fpa_partners",
                "tl_fpa_selftest_pollinate"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)
    assert re.search(r"typedef struct tl_fpa_opts \{[^}]*uint32_t epochs;[^}]*uint32_t n_nearest;[^}]*float mutation_probability;[^}]*\} tl_fpa_opts;", text)
    assert [f for f, _ in _capi.TlFpaOpts._fields_] == ["epochs", "n_nearest", "mutation_probability"] and C.sizeof(_capi.TlFpaOpts) == 12
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags  # the bit the solver refuses is one no flag has: no new flag was added
