"""The Kohonen map solver without a GPU: the statement of the specification (tests/_som_oracle.py) against the stand-alone C++
restatement (tests/probes/som_cpu_baseline.cpp, also once under host ASan/UBSan), the frozen goldens and the library's host-only
queries; the fixed exp on the arguments this solver feeds it; the reference's own unit-test properties; plan and limits; names."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _cs_oracle as CO
import _sa_cases as K
import _som_cases as SC
import _som_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_som.json")))
CASES = SC.cases()
bits = SO.bits
LDS, WORK = 163840, 8 << 30
MEASURED_EXP_REL_DIFF = 2.3e-16  # the largest relative difference of exp_spec to numpy's exp seen below; kSomExpMeasuredRelDiff in som_spec.h


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


def _compile(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "probes", "som_cpu_baseline.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("som"), "som_cpu_baseline", [])


def oracle(name):
    xy, packed, n, o, _want = CASES[name]
    return SO.solve_cached((name,), xy, packed, n, **o)


def run_baseline(exe, tmp_path, xy, o):
    path = str(tmp_path / "case.txt")
    with open(path, "w") as fh:
        fh.write(f"{len(xy)}\n" + "".join(f"{float(x)!r} {float(y)!r}\n" for x, y in xy))
    args = [exe, path, "--trace", "--epochs", str(o["epochs"]), "--learning-rate", repr(o["learning_rate"]), "--radius-fraction", repr(o["radius_fraction"]),
            "--neuron-multiplier", str(o["neuron_multiplier"]), "--seed", str(o["seed"]), "--run", str(o["run"])]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    log = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln[0] == "L"]
    cps = [[int(v) for v in ln.split()[1:]] for ln in lines[2:] if ln[0] == "C"]
    ring = [[int(v, 16) for v in ln.split()[1:]] for ln in lines[2:] if ln[0] == "R"]
    return int(lines[0]), [int(v) for v in lines[1].split()], log, cps, [r[0] for r in ring] + [r[1] for r in ring]


def check_baseline(exe, tmp_path, name):
    xy, packed, _n, o, _want = CASES[name]
    res = oracle(name)
    cost_bits, tour, log, cps, ring = run_baseline(exe, tmp_path, xy, o)
    assert log == SO.log_words(res).tolist() and ring == SO.ring_words(res).tolist(), name
    assert tour == res["tour"].tolist() and [c[0] for c in cps] == [t for t, _r, _c in res["checkpoints"]] and [c[2:] for c in cps] == [list(r) for _t, r, _c in res["checkpoints"]]
    if packed is None:  # (the restatement prices by the coordinates)
        assert cost_bits == bits(res["cost"]) and [c[1] for c in cps] == [bits(c) for _t, _r, c in res["checkpoints"]], name


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_cpp_restatement_equals_oracle(baseline, tmp_path, name):
    check_baseline(baseline, tmp_path, name)


def test_cpp_restatement_is_clean_under_host_sanitizers(tmp_path):
    """the stand-alone program (its own main, no GPU code) under ASan and UBSan: the same output, nothing reported"""
    exe = _compile(tmp_path, "som_cpu_baseline_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    for name in ("M65", "rf1_odd", "duplicates"):
        check_baseline(exe, tmp_path, name)
    assert subprocess.run([exe, "x", "--queries"], capture_output=True, text=True).returncode == 0


@pytest.mark.parametrize("name", sorted(SC.GOLDEN))
def test_oracle_equals_goldens(name):
    _xy, _packed, _n, o, want = CASES[name]
    res = oracle(name)
    assert SC.case_record(res) == GOLD["cases"][name]
    SC.check_conditions(name, res, o, want)


def test_literal_loops_equal_the_numpy_statement():
    for name in ("n7_mult1", "M65", "rf1_even", "rf1_odd", "M20_floor_crossed", "duplicates"):
        xy, packed, n, o, _want = CASES[name]
        lit = SO.solve(xy, packed, n, literal=True, **o)
        assert SO.ring_words(lit).tolist() == SO.ring_words(oracle(name)).tolist() and lit["moved"] == oracle(name)["moved"] and lit["log"] == oracle(name)["log"]


def test_cpp_restatement_queries(baseline):
    out = subprocess.run([baseline, "x", "--queries"], capture_output=True, text=True, check=True).stdout.splitlines()
    want = [str(SO.city_of(SO.chain_key(77, 5), t, 52)) for t in range(1, 9)]
    for epochs in (1, 10, 100000):
        for t in (1, max(epochs // 2, 1), epochs):
            eta, sigma, tss, radius = SO.schedule(t, epochs, 416, 0.8, 0.1)
            want.append(f"{SO.f64_bits(eta)} {SO.f64_bits(sigma)} {SO.f64_bits(tss)} {radius}")
    for d in (0.0, 1.0, 3.0, 4.0, 5.0, 6.0, 100.0):
        ok, h = SO.h_of(d, 2.0)
        want.append(f"{int(ok)} {SO.f64_bits(h)}")
    for M in (1, 2, 3, 4, 7, 416):
        want += [f"{SO.f64_bits(x)} {SO.f64_bits(y)}" for x, y in SO.ring_init(0.5, 0.25, M)]
    assert out == want


# ---------------------------------------------------------------- the host-only entries
def lib_schedule(lib, t, epochs, M, lr, rf):
    eta, sigma, tss, radius = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
    rc = lib.tl_som_schedule(t, epochs, M, lr, rf, C.byref(eta), C.byref(sigma), C.byref(tss), C.byref(radius))
    return rc, (eta.value, sigma.value, tss.value, radius.value)


def lib_h(lib, d, tss):
    h = C.c_double(-1.0)
    return bool(lib.tl_som_h(d, tss, C.byref(h))), h.value


def test_draws_schedules_h_and_rings_equal_the_goldens_and_the_library(lib):
    for seed, run, t, n, want in GOLD["draws"]:
        assert SO.city_of(SO.chain_key(int(seed), run), t, n) == want == lib.tl_som_draw(int(seed), run, t, n) and want < n
    for t, epochs, M, lr, rf, eta, sigma, tss, radius in GOLD["schedules"]:
        got = SO.schedule(t, epochs, M, lr, rf)
        rc, lgot = lib_schedule(lib, t, epochs, M, lr, rf)
        assert rc == 0 and [SO.f64_bits(v) for v in got[:3]] == [int(eta), int(sigma), int(tss)] == [SO.f64_bits(v) for v in lgot[:3]] and got[3] == radius == lgot[3]
    for dbits, tss, ok, h in GOLD["h"]:
        d = float(np.array([int(dbits)], dtype=np.uint64).view(np.float64)[0])
        assert SO.h_of(d, tss) == (bool(ok), float(np.array([int(h)], dtype=np.uint64).view(np.float64)[0])) == lib_h(lib, d, tss)
    for M, want in GOLD["rings"]:
        assert [str(SO.f64_bits(v)) for v in SO.ring_init(0.5, 0.25, M).T.reshape(-1)] == want


def test_draw_is_bounded_and_keyed_by_the_epoch(lib):
    key = SO.chain_key(9, 2)
    for n in (1, 2, 3, 52, 65536):
        got = [lib.tl_som_draw(9, 2, t, n) for t in range(1, 200)]
        assert got == [SO.city_of(key, t, n) for t in range(1, 200)] and max(got) < n and (n < 3 or len(set(got)) > 1)
    assert lib.tl_som_draw(9, 2, 5, 0) == 0
    assert SO.city_of(key, 7, 52) == SO.position(SO.draw(9, 2, 7, 0), 52)  # event t, slot 0 of the genetic algorithm's stream


def test_schedule_floor_radius_and_errors(lib):
    from teeline_amd import _capi
    for epochs, M, lr, rf in ((25, 20, 0.8, 0.1), (11, 21, 1.0, 1.0), (100_000, 8016, 0.8, 0.1), (10, 7, 0.3, 0.1)):
        for t in sorted({1, 2, epochs // 2, epochs - 1, epochs} - {0}):
            rc, got = lib_schedule(lib, t, epochs, M, lr, rf)
            eta, sigma, tss, radius = SO.schedule(t, epochs, M, lr, rf)
            assert rc == 0 and got == (eta, sigma, tss, radius) and sigma >= 1.0 and tss == (2.0 * sigma) * sigma
            assert radius == min(M, int(np.floor(np.sqrt(8.0 * tss))) + 2)
            # conservative: the first distance outside the radius is skipped without an exp, and so is everything beyond
            for d in range(radius + 1, min(radius + 4, M // 2 + 1)):
                assert lib_h(lib, float(d), tss) == (False, 0.0), (t, d)
    assert SO.schedule(10, 10, 7, 0.3, 0.1)[1] == 1.0 and abs(SO.schedule(10, 10, 7, 0.3, 0.1)[0] - 0.3 * np.exp(-1.0)) < 1e-15
    for bad in ((0, 10, 7), (11, 10, 7), (1, 0, 7), (1, 10, 0), (1, 10, 65537)):
        assert lib_schedule(lib, *bad, 0.8, 0.1)[0] == _capi.TL_ERR_BADARG


def test_h_on_both_sides_of_the_two_cuts(lib):
    """tss = 2 (the floor): d = 3 is moved (h = 1.1e-2), d = 4 gives y = -8.0 exactly — not below the cut, the exp is taken and
    h = 3.4e-4 falls to the 1e-3 cut —, the next f64 above 4 is below -8 and takes no exp"""
    assert lib_h(lib, 3.0, 2.0) == SO.h_of(3.0, 2.0) and SO.h_of(3.0, 2.0)[0] and abs(SO.h_of(3.0, 2.0)[1] - np.exp(-4.5)) < 1e-17
    ok, h = lib_h(lib, 4.0, 2.0)
    assert not ok and abs(h - np.exp(-8.0)) < 1e-18 and (ok, h) == SO.h_of(4.0, 2.0)
    up = float(np.nextafter(4.0, 5.0))
    assert lib_h(lib, up, 2.0) == (False, 0.0) == SO.h_of(up, 2.0)
    # the 1e-3 cut lies at y = ln 1e-3 = -6.9078: d^2 = 13.8155 on tss = 2
    lo, hi = float(np.sqrt(13.81)), float(np.sqrt(13.82))
    assert lib_h(lib, lo, 2.0)[0] and not lib_h(lib, hi, 2.0)[0] and lib_h(lib, hi, 2.0)[1] > 0.0
    assert lib_h(lib, lo, 2.0) == SO.h_of(lo, 2.0) and lib_h(lib, hi, 2.0) == SO.h_of(hi, 2.0)
    assert lib_h(lib, 0.0, 2.0) == (True, 1.0) and lib_h(lib, 1e7, 2.0) == (False, 0.0)  # far outside levy_exp's domain: never evaluated


def lib_ring(lib, xy, mult):
    xy = np.ascontiguousarray(xy, dtype=np.float32)
    n = len(xy)
    ring, cities = np.full(2 * n * mult, np.nan), np.full(2 * n, np.nan)
    rc = lib.tl_som_ring_init(xy.ctypes.data, n, mult, ring.ctypes.data, cities.ctypes.data)
    return rc, ring, cities


def test_ring_init_and_normalisation(lib):
    from teeline_amd import _capi
    for xy, mult in ((K.small(1), 1), (K.small(2), 1), (K.small(3), 1), (K.small(2), 2), (K.small(7), 1), (K.small(3), 4), (K.tsplib("berlin52")["xy"], 8), (SC.line(9), 6)):
        rc, ring, cities = lib_ring(lib, xy, mult)
        want_c, cx, cy = SO.normalise(xy)
        M = len(xy) * mult
        assert rc == 0 and cities.view(np.uint64).tolist() == np.ascontiguousarray(want_c.T).reshape(-1).view(np.uint64).tolist()
        assert ring.view(np.uint64).tolist() == np.ascontiguousarray(SO.ring_init(cx, cy, M).T).reshape(-1).view(np.uint64).tolist(), (len(xy), mult)
    # neuron 0 is at angle 0, the quarter turns are exact, and the cosine is the Lévy step's
    r = SO.ring_init(0.0, 0.0, 4)
    assert r.tolist() == [[0.1, 0.0], [0.0, 0.1], [-0.1, 0.0], [0.0, -0.1]]
    u = np.arange(416) / 416.0
    c, s = SO.cossin2pi(u)
    # against libm: ITS argument fl(fl(2 pi) u) is off by up to ~9e-16 (pi's rounding times u, and the product's), which moves its
    # result by as much where the slope is 1; a few ulps of evaluation on top: 2e-15
    assert c.tolist() == CO.cos2pi_spec(u).tolist() and np.abs(c - np.cos(2 * np.pi * u)).max() < 2e-15 and np.abs(s - np.sin(2 * np.pi * u)).max() < 2e-15
    assert np.abs(c * c + s * s - 1.0).max() < 5e-16
    line = SO.normalise(SC.line(9))[0]
    assert (line[:, 0] == 0.0).all() and line[:, 1].min() == 0.0 and line[:, 1].max() == 1.0  # span 1e-9: (x - min) / 1e-9 = 0
    bad = np.array(K.small(3), copy=True)
    bad[1, 0] = np.inf
    assert lib_ring(lib, bad, 1)[0] == _capi.TL_ERR_BADARG and lib_ring(lib, K.small(3), 0)[0] == _capi.TL_ERR_BADARG
    assert lib_ring(lib, K.small(3), 65536 // 3 + 1)[0] == _capi.TL_ERR_BADARG


def test_the_quadrant_reduction_is_exact_for_any_u():
    """som_spec.h's claim, checked with exact rational arithmetic on non-dyadic u = i / M"""
    from fractions import Fraction
    for M in (3, 7, 416, 8016, 65535):
        for i in sorted(i for i in {0, 1, M // 4, M // 4 + 1, M // 2, M // 2 + 1, (3 * M) // 4, (3 * M) // 4 + 1, M - 1} if i < M):
            u = float(i) / float(M)
            t = u * 4.0
            q = np.floor(t)
            f = t - q
            g = f if f <= 0.5 else 1.0 - f
            assert Fraction(t) == 4 * Fraction(u) and Fraction(f) == Fraction(t) - Fraction(q) and Fraction(g) == (Fraction(f) if f <= 0.5 else 1 - Fraction(f))
            assert 0.0 <= u < 1.0


def test_exp_on_this_solvers_arguments():
    """levy_exp on the schedule's arguments, -t / epochs in [-1, 0), and on the neighbourhood's, y in [-8, 0], against numpy's exp: the
    largest relative difference is recorded in som_spec.h; the bound is twice that measurement, as levy_spec.h does"""
    rng = np.random.default_rng(24)
    y = np.concatenate([-np.arange(1, 100_001) / 100_000.0, -np.arange(1, 26) / 25.0, -rng.uniform(0.0, 8.0, 200_000), [-8.0, 0.0, -1.0],
                        -(np.arange(0, 120, dtype=np.float64) ** 2) / 3461.12])
    y = y[y >= -8.0]
    got, want = CO.exp_spec(y), np.exp(y)
    rel = float(np.max(np.abs(got - want) / want))
    print(f"exp_spec vs numpy exp on {len(y)} arguments in [-8, 0]: largest relative difference {rel:.3e}")
    text = open(os.path.join(ROOT, "teeline_amd", "csrc", "som_spec.h")).read()
    m = re.search(r"constexpr double kSomExpMeasuredRelDiff = ([0-9.e-]+);", text)
    assert m and float(m.group(1)) == MEASURED_EXP_REL_DIFF
    assert rel <= 2.0 * MEASURED_EXP_REL_DIFF
    assert CO.exp_spec(np.float64(0.0)) == 1.0 and (got <= 1.0).all() and (got > 0.0).all()


# ---------------------------------------------------------------- the reference's own unit-test properties (som.rs:226-300)
def _solve_circle(n, ids=None):
    xy = SC.circle(n)
    res = SO.solve(xy, None, n, epochs=500, seed=n)
    return res, (np.arange(n) if ids is None else np.asarray(ids))[res["tour"]].tolist()


def test_reference_unit_test_properties():
    for n in (3, 10):
        res, route = _solve_circle(n)
        assert sorted(route) == list(range(n)) and len(route) == n
    assert _solve_circle(3)[0]["cost"] > 0
    res = SO.solve(np.array([[0.0, 0.0], [1.0, 0.0]], dtype=np.float32), None, 2, epochs=500)
    assert sorted(res["tour"].tolist()) == [0, 1] and res["cost"] == 2.0
    _res, route = _solve_circle(5, ids=[5, 10, 15, 20, 25])
    assert sorted(route) == [5, 10, 15, 20, 25]  # the ids, not the array positions
    res, _route = _solve_circle(8)
    assert np.isfinite(res["cost"]) and res["cost"] > 0
    # a trained map on a circle finds the circle: the tour is the polygon
    res, route = _solve_circle(10)
    k = route.index(0)
    turned = route[k:] + route[:k]
    assert turned in (list(range(10)), [0] + list(range(9, 0, -1)))
    for n in (0, 1):
        res = SO.solve(K.small(3)[:n], None, n, epochs=5)
        assert res["tour"].tolist() == list(range(n)) and res["cost"] == 0 and SO.messages(res) == []


def test_messages_follow_the_checkpoints():
    for e, kinds in ((1, ["EpochUpdate", "PathUpdate", "Done"]), (9, ["EpochUpdate", "PathUpdate"] * 9 + ["Done"]), (10, ["EpochUpdate", "PathUpdate"] * 10 + ["Done"]),
                     (11, ["EpochUpdate", "PathUpdate"] * 11 + ["Done"]), (25, ["EpochUpdate", "PathUpdate"] * 12 + ["PathUpdate", "Done"])):
        res = oracle(f"epochs{e}")
        msgs = SO.messages(res)
        assert [k for k, _p in msgs] == kinds, e
        cp = max(e // 10, 1)
        assert [p for k, p in msgs if k == "EpochUpdate"] == list(range(cp, e + 1, cp))
        if e % cp:
            assert msgs[-2][1][0] == res["tour"].tolist() and bits(msgs[-2][1][1]) == bits(res["cost"])
    assert max(e // max(e // 10, 1) + (e % max(e // 10, 1) != 0) for e in range(1, 3000)) == 19  # (epochs = 19) what the trace's callers size for


# ---------------------------------------------------------------- plan, limits, names
def plan(lib, n, mult, form=0, lds=LDS, work=WORK, flags=0, cus=256):
    M, t, f, per = C.c_uint32(), C.c_int(), C.c_uint32(), C.c_uint32()
    rc = lib.tl_kohonen_som_plan(n, mult, form, 1, cus, lds, work, flags, C.byref(M), C.byref(t), C.byref(f), C.byref(per))
    return rc, M.value, t.value, f.value, per.value


def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    assert plan(lib, 52, 8) == (0, 416, 64, 1, 65535) and plan(lib, 1002, 8) == (0, 8016, 1024, 1, (WORK - 5 * 256) // (16 * 8016 + 16 * 1002)) and plan(lib, 280, 8)[1:4] == (2240, 320, 1)
    top = (LDS - 512) // 16 // 8  # the largest n of the LDS form at the default multiplier
    assert top == 1276 and SC.LDS_MAX_NEURONS == 10208
    assert plan(lib, top - 1, 8)[1:4] == (10200, 1024, 1) and plan(lib, top, 8)[1:4] == (10208, 1024, 1) and plan(lib, top + 1, 8)[1:4] == (10216, 1024, 2)
    assert plan(lib, 10208, 1)[3] == 1 and plan(lib, 10209, 1)[3] == 2 and plan(lib, 10209, 1, 1) == (0, 0, 0, 0, 0)  # form 1 forced where it does not fit
    assert plan(lib, 52, 8, 2)[1:4] == (416, 64, 2) and plan(lib, 52, 8, 1)[3] == 1  # forced forms at a small size
    assert plan(lib, 65536, 1)[1:4] == (65536, 1024, 2) and plan(lib, 8192, 8)[1] == 65536  # the cap on M
    for n, mult in ((65537, 1), (8193, 8), (0, 8), (1, 8), (52, 0), (2, 2 ** 31)):
        assert plan(lib, n, mult) == (0, 0, 0, 0, 0), (n, mult)
    run_bytes = 16 * 8016 + 16 * 1002
    assert plan(lib, 1002, 8, work=3 * run_bytes + 5 * 256)[4] == 3 and plan(lib, 1002, 8, work=run_bytes)[4] == 0
    assert [SC.threads_of(M) for M in (1, 512, 513, 1024, 1025, 8129, 65536)] == [plan(lib, M, 1)[2] if M > 1 else 64 for M in (1, 512, 513, 1024, 1025, 8129, 65536)]
    assert plan(lib, 52, 8, cus=0)[0] == _capi.TL_ERR_BADARG and plan(lib, 52, 8, form=3)[0] == _capi.TL_ERR_BADARG
    assert plan(lib, 52, 8, flags=1 << 31) == (_capi.TL_ERR_UNSUPPORTED, 0, 0, 0, 0)
    assert lib.tl_kohonen_som_max_n(None, 8, 0) == 0
    text = open(os.path.join(ROOT, "teeline_amd", "csrc", "som_spec.h")).read()
    assert re.search(r"constexpr uint32_t kSomMaxNeurons = 65536;", text) and SO.MAX_NEURONS == 65536


def test_options_validate_as_the_reference_does():
    from teeline_amd.host.kohonen_som import SOMOptions
    d = SOMOptions()
    assert (d.epochs, d.learning_rate, d.radius_fraction, d.neuron_multiplier) == (100_000, 0.8, 0.1, 8) == tuple(SO.DEFAULTS[k] for k in ("epochs", "learning_rate", "radius_fraction", "neuron_multiplier"))
    d.validate()
    SOMOptions(1, 1.0, 1.0, 1).validate()
    for kw, msg in ((dict(epochs=0), "epochs must be >= 1"), (dict(learning_rate=0.0), r"learning_rate must be in \(0, 1\]"), (dict(learning_rate=1.01), "learning_rate"),
                    (dict(radius_fraction=0.0), r"radius_fraction must be in \(0, 1\]"), (dict(radius_fraction=2.0), "radius_fraction"), (dict(neuron_multiplier=0), "neuron_multiplier must be >= 1")):
        with pytest.raises(ValueError, match=msg):
            SOMOptions(**kw).validate()
        assert not SO.validate(**dict(SO.DEFAULTS, **kw))


def test_pipeline_names_and_refusals():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["kohonen_som"] == "kohonen_som" and "som" not in P.SOLVER_NAMES and "kohonen" not in P.SOLVER_NAMES
    # a constructive solver that ignores its start tour runs alone: it is in neither of mod.rs:129-157's lists
    assert "kohonen_som" not in P.AUTO_EXPAND_WITH_SHUFFLE and "kohonen_som" not in P.AUTO_EXPAND_WITH_NN
    assert P.steps_for_solve("kohonen_som") == ["kohonen_som"] == P.steps_for_solve("Kohonen_SOM", no_seed=True)
    for alias in ("som", "kohonen", "SOM"):
        with pytest.raises(ValueError, match="the seeded Kohonen map of this build is `kohonen_som`"):
            P.steps_for_solve(alias)
        with pytest.raises(ValueError, match="the seeded Kohonen map of this build is `kohonen_som`"):
            P.run_pipeline_stages(None, [alias.lower()])
    assert P.REFUSED_ALIASES["som"] == P.REFUSED_ALIASES["kohonen"] == "kohonen_som"
    hpp = open(os.path.join(ROOT, "teeline_amd", "host_cpp", "teeline_gpu.hpp")).read()
    cpu_only = re.search(r"static const char \*cpu_only\[\] = \{([^}]*)\}", hpp).group(1)
    assert '"som"' in cpu_only and '"kohonen"' in cpu_only and '"kohonen_som"' not in cpu_only and "Solvers::KohonenSom" in hpp


def test_header_bindings_and_flags_agree(lib):
    from teeline_amd import _capi
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    syms = ("tl_kohonen_som", "tl_kohonen_som_trace", "tl_kohonen_som_population", "tl_kohonen_som_max_n", "tl_kohonen_som_plan", "tl_som_draw", "tl_som_schedule",
            "tl_som_h", "tl_som_ring_init", "tl_som_selftest_bmu")
    for sym in syms:
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)
    m = re.search(r"typedef struct tl_som_opts \{(.*?)\} tl_som_opts;", text, re.S)
    fields = re.findall(r"^\s*(uint32_t|uint64_t|double) (\w+);", m.group(1), re.M)
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_capi.TlSomOpts._fields_)
    assert [n for _t, n in fields] == ["epochs", "neuron_multiplier", "learning_rate", "radius_fraction", "form", "reserved", "work_bytes"]
    assert C.sizeof(_capi.TlSomOpts) == 40 and _capi.TlSomOpts.learning_rate.offset == 8 and _capi.TlSomOpts.form.offset == 24 and _capi.TlSomOpts.work_bytes.offset == 32
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags and "TL_FLAG_SOM" not in text  # no flag bit is added: the form is an option
    rust = open(os.path.join(ROOT, "integration", "teeline-gpu", "src", "lib.rs")).read()
    for sym in ("tl_kohonen_som", "tl_kohonen_som_trace", "tl_kohonen_som_population", "tl_kohonen_som_max_n", "tl_som_draw", "tl_som_schedule", "tl_som_h", "tl_som_ring_init"):
        assert re.search(rf"\bfn {sym}\(", rust), sym
    from teeline_amd import build
    assert "tl_api_som.hip" in build.SOURCES and "kohonen_som.hip" in build.SOURCES and "som_spec.h" in build.HEADERS


# ---------------------------------------------------------------- informational
def test_share_of_tours_equal_to_a_libm_run():
    """Informational, not a pass criterion: over seeded small instances, the share whose final tour equals that of the
    same oracle run with numpy's libm exp, cos and sin.  Only that the comparison runs is asserted."""
    same = total = 0
    for k in range(200):
        n = 5 + k % 8
        xy = K.synth(n, 1000 + k)
        a = SO.solve(xy, None, n, epochs=60, seed=k)
        b = SO.solve(xy, None, n, epochs=60, seed=k, exp=SO.exp_libm, cossin=SO.cossin_libm)
        same += a["tour"].tolist() == b["tour"].tolist()
        total += 1
    print(f"final tour equal to the libm run's: {same} of {total}")
    assert total == 200 and 0 <= same <= total
