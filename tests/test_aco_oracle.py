"""The ant colony solver without a GPU: the numpy statement of the specification (tests/_aco_oracle.py) against the stand-alone C++
restatement (tests/probes/aco_cpu_baseline.cpp), the frozen goldens and the library's host-only queries; the draws, aco_pow, the
masked walk against the compacted one, the reference's own unit vectors, small n, the plan and limits, pipeline names, options."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _aco_cases as AC
import _aco_oracle as ACO
import _sa_cases as K
import _sa_oracle as SA
from _swarm_oracle import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_aco.json")))
CASES = AC.golden_cases()


def f32(b):
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aco") / "aco_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "aco_cpu_baseline.cpp"), "-o", exe])
    return exe


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: t\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def oracle(name):
    xy, packed, n, init, o = CASES[name]
    return ACO.solve_cached(("golden", name), xy, packed, n, init, **o)


def run_baseline(exe, tmp_path, xy, init, o):
    tsp = str(tmp_path / "case.tsp")
    write_tsp(tsp, xy)
    args = [exe, tsp, "--trace", "--epochs", str(o["epochs"]), "--seed", str(o["seed"]), "--run", str(o["run"]), "--alpha", repr(float(o["alpha"])),
            "--beta", repr(float(o["beta"])), "--evaporation-rate", repr(float(o["evaporation_rate"])), "--num-ants", str(o["num_ants"])]
    if init is not None:
        ini = str(tmp_path / "case.init")
        open(ini, "w").write(" ".join(str(int(v)) for v in init) + "\n")
        args += ["--init", ini]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    head = [int(v) for v in lines[0].split()[:5]]
    log = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("E")]
    routes = [[int(v) & 0xFFFFFFFF for v in ln.split()[1:]] for ln in lines[2:] if ln.startswith("R")]
    return head, [int(v) for v in lines[1].split()], log, routes


def same_as_oracle(got, res, o, n):
    head, route, log, routes = got
    c = res["counters"]
    assert head == [o["epochs"], c["tours"], c["improved"], c["fallbacks"], bits(res["cost"])]
    assert route == res["tour"].tolist()
    assert log == ACO.log_words(res, o["num_ants"]).tolist() and routes == ACO.route_words(res, n).tolist()


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_numpy_oracle_equals_goldens(name):
    _xy, _packed, n, _init, o = CASES[name]
    res = oracle(name)
    want = GOLD["cases"][name]
    assert res["tour"].tolist() == want["tour"] and bits(res["cost"]) == want["cost_bits"] and res["counters"] == want["counters"]
    assert sha(ACO.log_words(res, o["num_ants"])) == want["log_sha256"] and sha(ACO.route_words(res, n)) == want["routes_sha256"]
    assert ACO.log_words(res, o["num_ants"])[:2].tolist() == want["log_head"]
    AC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v[1] is None))  # the coordinate cases
def test_cpp_restatement_equals_oracle_and_goldens(baseline, tmp_path, name):
    xy, _packed, n, init, o = CASES[name]
    got = run_baseline(baseline, tmp_path, xy, init, o)
    same_as_oracle(got, oracle(name), o, n)
    assert got[1] == GOLD["cases"][name]["tour"] and got[0][4] == GOLD["cases"][name]["cost_bits"]


@pytest.mark.parametrize("n", [3, 7, 66])
@pytest.mark.parametrize("with_init", [False, True])
def test_cpp_restatement_on_random_instances(baseline, tmp_path, n, with_init):
    xy = K.synth(n, 500 + n)
    init = AC.start_tour(n, n) if with_init else None
    o = dict(epochs=4, alpha=1.3, beta=2.6, evaporation_rate=0.4, num_ants=9, seed=n, run=3)
    same_as_oracle(run_baseline(baseline, tmp_path, xy, init, o), ACO.solve(xy, None, n, init, **o), o, n)


def test_cpp_restatement_takes_the_fallback_paths(baseline, tmp_path):
    b = K.tsplib("berlin52")
    o = AC.UNDERFLOW
    res = ACO.solve(b["xy"], None, 52, np.arange(52), **o)
    assert res["counters"]["fallbacks"] == o["epochs"] * o["num_ants"] * 51
    same_as_oracle(run_baseline(baseline, tmp_path, b["xy"], np.arange(52), o), res, o, 52)


def test_cpp_restatement_draws(baseline):
    out = subprocess.run([baseline, "x", "--draws", "--seed", "77", "--run", "5"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ACO.draw(77, 5, base + e, s) for base in (0, ACO.INIT_EVENT) for e in range(8) for s in range(28)]


# ---------------------------------------------------------------- draws
def test_draws_are_the_annealing_stream_indexed_by_the_event():
    for seed, run, event, slot in ((1, 0, 0, 0), (9, 3, 12345, 2), (2 ** 64 - 1, 7, ACO.shuffle_event(1001), 26)):
        assert ACO.draw(seed, run, event, slot) == SA.mix(SA.chain_key(seed, run) + SA.G * (32 * event + slot + 1))
        if event < 2 ** 32:
            assert ACO.draw(seed, run, event, slot) == SA.draw(seed, run, event, slot)
    assert ACO.event(3, 25, 7, 52, 9) == (3 * 25 + 7) * 52 + 9 and ACO.shuffle_event(5) == 2 ** 58 + 5
    # the largest epoch event of any call the library takes (n below 11 000 on 160 KiB of LDS) stays below the shuffle's range, whose 32-fold does not wrap
    assert ACO.event(2 ** 32 - 1, 4096, 4095, 11000, 10999) < ACO.EVENT_LIMIT and 32 * (ACO.shuffle_event(65534) + 1) < 2 ** 64


def test_draws_match_goldens_and_library(lib):
    for seed, run, event, slot, want in GOLD["draws"]:
        assert ACO.draw(int(seed), run, int(event), slot) == int(want)
        assert lib.tl_aco_draw(int(seed), run, int(event), slot) == int(want) == lib.tl_ga_draw(int(seed), run, int(event), slot)
    rng = np.random.default_rng(1)
    for _ in range(200):
        seed, run, event, slot = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 59)), int(rng.integers(0, 32))
        assert lib.tl_aco_draw(seed, run, event, slot) == ACO.draw(seed, run, event, slot)
    assert lib.tl_sa_draw(1, 3, 138148, 21) == SA.draw(1, 3, 138148, 21)  # sa_spec.h's functions keep their results


@pytest.mark.parametrize("n,ants,seeded", [(3, 1, False), (3, 2, True), (4, 3, False), (7, 5, True), (9, 2, False)])
def test_no_two_roles_share_an_event_and_slot(n, ants, seeded):
    roles = ACO.roles(n, ants, 3, seeded)
    seen = {}
    for event, slot, role in roles:
        assert slot < 32 and seen.setdefault((event, slot), role) == role, (event, slot, role, seen[(event, slot)])
    assert len(seen) == len(roles) == 3 * ants * (1 + 2 * (n - 1)) + (0 if seeded else n - 1)


# ---------------------------------------------------------------- aco_pow
def test_aco_pow_is_exact_at_0_1_2_and_the_special_values(lib):
    x = np.array([0.0, 1e-40, 1e-20, 0.3, 1.0, 2.5, 1e19, 1e30, np.inf, np.nan], dtype=np.float32)
    with np.errstate(all="ignore"):
        assert ACO.aco_pow(x, 0.0).tolist() == [1.0] * len(x)
        assert ACO.aco_pow(x, 1.0).view(np.uint32).tolist() == x.view(np.uint32).tolist()
        assert ACO.aco_pow(x[:-1], 2.0).view(np.uint32).tolist() == (x[:-1] * x[:-1]).view(np.uint32).tolist() and np.isnan(ACO.aco_pow(x, 2.0)[-1])
    for a in (0.5, 1.5, 6.0):
        got = ACO.aco_pow(x, a)
        assert got[0] == 0 and bits(got[0]) == 0 and got[-2] == np.inf and np.isnan(got[-1]) and got[4] == 1
    assert ACO.pow_scalar(1e6, 6.5) == np.inf and ACO.pow_scalar(1e-3, 20.0) == 0 and ACO.pow_scalar(1e6, 6.0) < np.inf
    for v in x:
        for a in (0.0, 1.0, 2.0, 0.5, 6.0):
            g, w = lib.tl_aco_pow(float(v), a), ACO.pow_scalar(v, a)
            assert bits(g) == bits(w) or (np.isnan(g) and np.isnan(w)), (v, a)


def test_aco_pow_within_one_ulp_of_the_f64_power():
    """An f64 evaluation accurate to about 1e-14 relative lands within 1e-14 x 2^24 of an f32 ulp of the true value, so its rounding
    to f32 is the correctly rounded result or its neighbour: at most one ulp from Python's f64 `**` rounded to f32."""
    rng = np.random.default_rng(7)
    x = np.exp(rng.uniform(np.log(1e-30), np.log(1e6), size=40000)).astype(np.float32)
    for a in list(rng.uniform(0.0, 6.0, size=12).astype(np.float32)) + [np.float32(6.0), np.float32(1e-3), np.float32(0.5), np.float32(3.0)]:
        got = ACO.aco_pow(x, a)
        with np.errstate(all="ignore"):
            want = np.array([float(v) ** float(a) for v in x[:2000]] + list(x[2000:].astype(np.float64) ** float(a))).astype(np.float32)
        assert (np.isfinite(got) == np.isfinite(want)).all()
        ok = np.isfinite(want)
        ulps = np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (a, ulps.max())


def test_aco_pow_three_statements_bit_equal(lib, baseline):
    rng = np.random.default_rng(11)
    xs = np.concatenate((np.exp(rng.uniform(np.log(1e-44), np.log(3e38), size=1500)).astype(np.float32), np.array([0.0, np.inf, 1.0, 0.70710677, 0.7071068, 1.4142135], dtype=np.float32)))
    az = rng.uniform(0.0, 6.0, size=len(xs)).astype(np.float32)
    az[::7] = np.float32(2.0)
    az[::11] = np.float32(1.0)
    want = [bits(ACO.pow_scalar(x, a)) for x, a in zip(xs, az)]
    assert [bits(lib.tl_aco_pow(float(x), float(a))) for x, a in zip(xs, az)] == want
    args = [str(v) for x, a in zip(xs, az) for v in (bits(x), bits(a))]
    out = subprocess.run([baseline, "x", "--pow"] + args, capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == want
    for xb, ab, wb in GOLD["pow"]:
        assert bits(ACO.pow_scalar(f32(xb), f32(ab))) == wb == bits(lib.tl_aco_pow(float(f32(xb)), float(f32(ab))))


# ---------------------------------------------------------------- the selection
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 300])
def test_masked_walk_equals_the_compacted_walk(n):
    for w, e, vis, r1, r2, what in AC.selection_rows(n, n) if n > 1 else [(np.ones(1, np.float32), np.ones(1, np.float32), np.zeros(1, np.uint32), 0.5, 0.5, "one")]:
        a = ACO.select_compacted(w, e, vis, np.float32(r1), np.float32(r2))
        b = ACO.select_masked(w, e, vis, np.float32(r1), np.float32(r2))
        assert a[:2] == b[:2] and all(bits(p) == bits(q) or (np.isnan(p) and np.isnan(q)) for p, q in zip(a[2:], b[2:])), (n, what, a, b)
        assert not vis[a[0]]
    rng = np.random.default_rng(n)
    for _ in range(200):
        w = (rng.uniform(size=n) * (rng.uniform(size=n) < 0.7)).astype(np.float32)
        e = rng.uniform(0.1, 3.0, size=n).astype(np.float32)
        vis = (rng.uniform(size=n) < rng.uniform()).astype(np.uint32)
        vis[int(rng.integers(n))] = 0
        r1, r2 = np.float32(rng.choice([0.0, rng.uniform(), 1.0])), np.float32(rng.uniform())
        assert ACO.select_compacted(w, e, vis, r1, r2)[:2] == ACO.select_masked(w, e, vis, r1, r2)[:2]


def test_reference_unit_vectors():
    for primary, fallback, r1, r2, want in AC.REFERENCE_SELECT:  # select_next (ant_colony.rs:336-355)
        assert ACO.select_next(primary, fallback, np.float32(r1), np.float32(r2))[0] == want
    # roulette_select (probability.rs): the strict test skips zero-width buckets at r = 0; the exhausted walk is the last candidate
    assert ACO.roulette_select([0.0, 0.0, 1.0], 1.0, 0.0) == 2 and ACO.roulette_select([1.0, 3.0], 4.0, 0.5) == 1 and ACO.roulette_select([1.0, 1.0], 2.0, 1.0) == 1
    p = np.array([1.0, 1.0], dtype=np.float32)  # evaporate_and_floor (ant_colony.rs:259-275)
    ACO.evaporate_and_floor(p, 0.5, 0.0)
    assert p.tolist() == [0.5, 0.5]
    p = np.array([0.001, 1.0], dtype=np.float32)
    ACO.evaporate_and_floor(p, 0.99, 0.001)
    assert p[0] == np.float32(0.001) and abs(p[1] - 0.01) < 1e-6
    tau = np.zeros((4, 4), dtype=np.float32)  # deposit_tour (ant_colony.rs:297-334)
    ACO.deposit_tour(tau, [0, 1, 2], 10.0)
    want = np.zeros((4, 4), dtype=np.float32)
    for u, v in ((0, 1), (1, 2), (2, 0)):
        want[u, v] = want[v, u] = np.float32(1.0) / np.float32(10.0)
    assert tau.tolist() == want.tolist()
    tau = np.zeros((3, 3), dtype=np.float32)
    ACO.deposit_tour(tau, [0, 1, 2], 0.0)
    assert not tau.any()


def test_small_n_and_epochs_zero():
    for n in (0, 1, 2):  # city order, nothing drawn (ant_colony.rs:109-115)
        res = ACO.solve(K.small(3)[:n], None, n, None, epochs=5, seed=1)
        assert res["tour"].tolist() == list(range(n)) and res["epochs"] == [] and ACO.messages(res) == [("Done", None)]
    assert ACO.solve(K.small(3)[:2], None, 2, None, epochs=5)["cost"] == np.float32(2) * SA.dist_fn(K.small(3), None, 3)(0, 1)
    res = ACO.solve(K.small(3), None, 3, None, epochs=4, num_ants=3, seed=2)
    assert sorted(res["tour"].tolist()) == [0, 1, 2] and len(res["epochs"]) == 4 and all(len(e["costs"]) == 3 for e in res["epochs"])
    init = AC.start_tour(8, 2)
    res = ACO.solve(K.small(8), None, 8, init, epochs=0, seed=3)  # test_aco_respects_initial_tour
    assert res["tour"].tolist() == init.tolist() and ACO.messages(res)[0][0] == "PathUpdate" and len(ACO.messages(res)) == 2
    res = ACO.solve(K.small(8), None, 8, None, epochs=0, seed=3)
    assert res["tour"].tolist() == ACO.start_tour(ACO.chain_key(3, 0), 8).tolist()


# ---------------------------------------------------------------- plan, limits, names
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    per, t, need = C.c_uint32(), C.c_int(), C.c_uint64()
    lds, work = 163840, 8 << 30
    assert lib.tl_ant_colony_plan(52, 25, 1, 256, lds, work, C.byref(per), C.byref(t), C.byref(need)) == 0
    assert per.value == 65535 and t.value == 320 and 12 * 52 * 52 <= need.value <= 12 * 52 * 52 + 6 * 25 * 52 + 8192
    assert lib.tl_ant_colony_plan(1002, 25, 64, 256, lds, work, C.byref(per), C.byref(t), C.byref(need)) == 0
    assert 600 <= per.value <= work // (12 * 1002 * 1002) and 64 * 12 * 1002 * 1002 <= need.value <= 64 * 12 * 1002 * 1002 * 1.02
    assert lib.tl_ant_colony_plan(1000, 25, 10 ** 6, 256, lds, 10 * 12_300_000, C.byref(per), C.byref(t), C.byref(need)) == 0 and 9 <= per.value <= 10
    top = max(n for n in range(10000, 11000) if 768 + 2 * 64 * 65 * 4 + -(-n // 64) * 256 + -(-n // 32) * 256 <= lds)
    assert lib.tl_ant_colony_plan(top, 2, 1, 256, lds, work, C.byref(per), C.byref(t), C.byref(need)) == 0 and per.value >= 1 and t.value == 320
    for n, ants, w in ((top + 1, 2, work), (0, 25, work), (2, 25, work), (1000, 25, 1000), (52, 0, work), (52, 4097, work)):
        assert lib.tl_ant_colony_plan(n, ants, 1, 256, lds, w, C.byref(per), C.byref(t), C.byref(need)) == 0
        assert (per.value, t.value, need.value) == (0, 0, 0)
    assert lib.tl_ant_colony_plan(52, 25, 1, 0, lds, work, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_ant_colony_max_n(None) == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["ant_colony"] == "ant_colony" and "aco" not in P.SOLVER_NAMES
    assert P.steps_for_solve("ant_colony") == ["shuffle", "ant_colony"] and P.steps_for_solve("Ant_Colony", no_seed=True) == ["ant_colony"]
    with pytest.raises(ValueError, match="the seeded ant colony of this build is `ant_colony`"):
        P.steps_for_solve("aco")
    with pytest.raises(ValueError, match="the seeded ant colony of this build is `ant_colony`"):
        P.run_pipeline_stages(None, ["aco"])
    assert P.steps_for_solve("genetic_algorithm") == ["shuffle", "genetic_algorithm"] and P.steps_for_solve("tabu_search") == ["nn", "tabu_search"]


def test_options_validate():
    from teeline_amd.host.ant_colony import AcoOptions
    d = AcoOptions()
    assert (d.epochs, d.alpha, d.beta, d.evaporation_rate, d.num_ants) == (150, 1.0, 2.0, 0.5, 25)
    for kw, msg in ((dict(alpha=-0.1), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"), (dict(beta=6.5), "beta"),
                    (dict(beta=-1.0), "beta"), (dict(beta=float("nan")), "beta"), (dict(evaporation_rate=0.0), "evaporation_rate"),
                    (dict(evaporation_rate=1.0), "evaporation_rate"), (dict(evaporation_rate=float("nan")), "evaporation_rate"), (dict(num_ants=0), "num_ants")):
        with pytest.raises(ValueError, match=msg):
            AcoOptions(**kw).validate()
    AcoOptions(alpha=0.0, beta=6.0, evaporation_rate=0.999, num_ants=1).validate()


def test_header_and_bindings_agree_on_the_symbols(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_ant_colony", "tl_ant_colony_trace", "tl_ant_colony_trace_run", "tl_ant_colony_population", "tl_ant_colony_max_n", "tl_ant_colony_plan",
                "tl_aco_draw", "tl_aco_pow", "tl_aco_selftest_select"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)


# ---------------------------------------------------------------- the GPU cases are what they claim
def test_gpu_cases_are_what_they_claim():
    b = K.tsplib("berlin52")
    o = AC.UNDERFLOW
    res = ACO.solve(b["xy"], None, 52, np.arange(52), keep=True, **o)
    assert res["counters"]["fallbacks"] == o["epochs"] * o["num_ants"] * 51 and all(p == 1 and t1 == 0 and t2 > 0 for ep in res["paths"] for ant in ep for p, t1, t2 in ant)
    n, o = AC.COINCIDENT_N, dict(AC.COINCIDENT, epochs=1, num_ants=1)
    res = ACO.solve(np.full((n, 2), 3.0, dtype=np.float32), None, n, None, keep=True, **o)
    first = res["paths"][0][0]
    assert [p for p, _a, _b in first] == [2] * (n - 341) + [0] * 340 and all(np.isinf(t1) and np.isinf(t2) for p, t1, t2 in first if p == 2)
    assert res["epochs"][0]["costs"] == [0] and res["epochs"][0]["fallbacks"] == [n - 341] and res["counters"]["improved"] == 0
    for w, e, vis, r1, r2, what in AC.selection_rows(129, 129):  # every path of the self-test's rows, and the exhausted walk among them
        assert (np.asarray(vis) == 0).any()
    paths = {ACO.select_compacted(w, e, vis, np.float32(r1), np.float32(r2))[1] for w, e, vis, r1, r2, _ in AC.selection_rows(129, 129)}
    assert paths == {0, 1, 2} and AC.CHUNK == 64
