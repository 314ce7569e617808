"""The Fourier-curve solver's specification on the CPU: the numpy statement (tests/_fourier_oracle.py) against the stand-alone C++
restatement (tests/probes/fourier_cpu_baseline.cpp, also once under host ASan/UBSan), its literal-loop form, the frozen goldens and
the library's host-only entry points; option validation, the solver names, the reference's own four unit-test situations, and the
measured sizes of the specification's departures."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _fourier_cases as FC
import _fourier_oracle as FO
from _raw_context import _vp
import _sa_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_fourier.json")))
CASES = FC.cases()
bits = FO.bits


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi
    return _capi.load()


def _compile(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "probes", "fourier_cpu_baseline.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("fourier"), "fourier_cpu_baseline", [])


def run_baseline(exe, tmp_path, xy, o, extra=("--trace",)):
    path = str(tmp_path / "case.txt")
    with open(path, "w") as fh:
        fh.write(f"{len(xy)}\n" + "\n".join(f"{float(a)!r} {float(b)!r}" for a, b in xy) + "\n")
    args = [exe, path, "--k-max", str(o["k_max"]), "--m", str(o["m"]), "--lambda", repr(o["lam"]), "--lambda-decay", repr(o["lambda_decay"]), "--lr", repr(o["lr"]),
            "--epochs", str(o["epochs"]), "--log-cap", str(FC.LOG_CAP)] + list(extra)
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("cost_bits")][0]
    return dict(cost_bits=int(lines[at].split()[1], 16), tour=[int(v) for v in lines[at + 1].split()],
                log=[[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("L")],
                stage=[int(v, 16) for ln in lines if ln.startswith("S ") for v in ln.split()[2:]],
                coeffs=[int(v, 16) for ln in lines if ln.startswith("C") for v in ln.split()[1:]], lines=lines)


def check_baseline(exe, tmp_path, name):
    xy, packed, n, o = CASES[name]
    assert packed is None  # the restatement reads coordinates only
    res = FC.oracle(name)
    got = run_baseline(exe, tmp_path, xy, o)
    assert got["log"] == res["log"][:FC.LOG_CAP].tolist(), name
    assert got["stage"] == FO.f64_words(res["stage_c"]).tolist() and got["coeffs"] == FO.f64_words(res["coeffs"]).tolist(), name
    assert got["tour"] == res["tour"].tolist() and got["cost_bits"] == bits(res["cost"]), name


CPP_CASES = [c for c in FC.GOLDEN if CASES[c][1] is None] + ["m4096_k32", "n129_two_chunks"]


@pytest.mark.parametrize("name", CPP_CASES)
def test_cpp_restatement_equals_oracle(baseline, tmp_path, name):
    check_baseline(baseline, tmp_path, name)


def test_cpp_restatement_is_clean_under_host_sanitizers(tmp_path):
    """a stand-alone program, compiled and run on the host: ASan and UBSan abort on the first finding"""
    exe = _compile(tmp_path, "fourier_cpu_baseline_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    for name in ("n2", "circle5", "m2_k1", "stages_k3_e2", "stacked"):
        check_baseline(exe, tmp_path, name)
    xy, _p, _n, o = CASES["circle5"]
    for form in ("tree", "brute"):  # the timing forms too: the kd-tree is this project's own text
        got = run_baseline(exe, tmp_path, xy, o, extra=("--time", form))
        assert sorted(got["tour"]) == list(range(5)) and any(ln.startswith("ms ") for ln in got["lines"])


def test_tree_form_agrees_where_no_root_is_tied(baseline, tmp_path):
    """a280, 40 steps: no query has tied roots (the oracle counts them), so the kd-tree's answer is the linear search's"""
    xy = K.tsplib("a280")["xy"]
    o = dict(FO.DEFAULTS, epochs=10)
    res = FO.solve(xy, None, 280, count_ties=True, **o)
    assert res["ties"] == 0
    got = run_baseline(baseline, tmp_path, xy, o, extra=("--time", "tree"))
    assert got["tour"] == res["tour"].tolist() and got["cost_bits"] == bits(res["cost"])


@pytest.mark.parametrize("name", FC.GOLDEN)
def test_oracle_equals_goldens(name):
    assert FC.case_record(FC.oracle(name)) == GOLD["cases"][name]


def test_literal_loops_equal_the_numpy_statement():
    for name in ("n2", "n3", "m2_k1", "stages_k3_e2", "stacked"):
        xy, packed, n, o = CASES[name]
        a, b = FC.oracle(name), FO.solve(xy, packed, n, literal=True, **o)
        assert a["log"].tolist() == b["log"].tolist() and FO.f64_words(a["coeffs"]).tolist() == FO.f64_words(b["coeffs"]).tolist(), name
        assert a["tour"].tolist() == b["tour"].tolist() and bits(a["cost"]) == bits(b["cost"]), name


def test_host_entry_points_equal_the_oracle(lib):
    for m, words in GOLD["basis"]:
        out = np.zeros(2 * m)
        assert lib.tl_fourier_basis(m, _vp(out)) == 0 and [str(int(v)) for v in out.view(np.uint64)] == words
        assert words == [str(int(v)) for v in FO.f64_words(FO.basis_table(m))]
    for name, k_max, words in GOLD["init"]:
        xy = np.ascontiguousarray(CASES[name][0])
        out = np.full(2 * (2 * k_max + 1), np.nan)
        assert lib.tl_fourier_init(_vp(xy), len(xy), k_max, _vp(out)) == 0 and [str(int(v)) for v in out.view(np.uint64)] == words
    assert lib.tl_fourier_basis(1, _vp(np.zeros(2))) == -1 and lib.tl_fourier_basis(4097, _vp(np.zeros(2))) == -1
    # the nearest sample: the lowest index among equal roots, a NaN never nearer, all NaN: sample 0
    city = np.zeros((1, 2), dtype=np.float32)
    for gamma, want in (([[1, 0], [0, 1], [-1, 0]], 0), ([[2, 0], [0, 1], [1, 0]], 1), ([[np.nan, 0], [np.inf, 0]], 1), ([[np.nan, 0], [0, np.nan]], 0)):
        g, out = np.array(gamma, dtype=np.float64), np.zeros(1, dtype=np.uint32)
        assert lib.tl_fourier_nearest(_vp(g), len(g), _vp(city), 1, _vp(out)) == 0 and out[0] == want == FO.nearest(g[:, 0], g[:, 1], city)[0], gamma


def test_tied_roots_of_unequal_squares_exist_and_go_to_the_lower_index():
    big, small, root = FC.tied_root_pair()
    assert big > small and np.sqrt(big, dtype=np.float32) == np.sqrt(small, dtype=np.float32) == root
    # a search that compared squares alone would take the smaller square at the higher index
    d = np.array([[root, root]], dtype=np.float32)
    key = d.view(np.uint32).astype(np.uint64)
    assert int(((key << np.uint64(32)) | np.arange(2, dtype=np.uint64)).min(axis=1)[0] & np.uint64(0xFFFFFFFF)) == 0


def test_options_validate_as_the_reference_does():
    from teeline_amd.host.fourier_curve import FourierOptions
    d = FourierOptions()
    assert (d.k_max, d.m, d.lam, d.lambda_decay, d.lr, d.epochs) == (4, 200, 0.05, 0.5, 0.05, 400) == tuple(FO.DEFAULTS[k] for k in ("k_max", "m", "lam", "lambda_decay", "lr", "epochs"))
    d.validate()
    FO.validate(**FO.DEFAULTS)
    for bad, msg in ((dict(k_max=0), "k_max"), (dict(m=1), "m must"), (dict(lam=0.0), "lambda must"), (dict(lam=-0.1), "lambda must"), (dict(lambda_decay=0.0), "lambda_decay"),
                     (dict(lambda_decay=1.0), "lambda_decay"), (dict(lr=0.0), "lr must"), (dict(epochs=0), "epochs"), (dict(lam=float("nan")), "lambda must")):
        with pytest.raises(ValueError, match=msg):
            FourierOptions(**bad).validate()
        with pytest.raises(ValueError, match=msg):
            FO.validate(**dict(FO.DEFAULTS, **bad))
    FourierOptions(k_max=1, m=2, lam=1e-300, lambda_decay=0.999, lr=1e-300, epochs=1).validate()


def test_pipeline_names_and_refusals():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["fourier_curve"] == "fourier_curve" and "fourier" not in P.SOLVER_NAMES and "branch_bound" not in P.SOLVER_NAMES
    assert "fourier_curve" not in P.AUTO_EXPAND_WITH_NN and "fourier_curve" not in P.AUTO_EXPAND_WITH_SHUFFLE
    assert P.steps_for_solve("fourier_curve") == ["fourier_curve"] == P.steps_for_solve("fourier_curve", no_seed=True)
    with pytest.raises(ValueError, match="the Fourier-curve solver of this build is `fourier_curve`"):
        P.steps_for_solve("fourier")
    with pytest.raises(ValueError, match="unknown solver `branch_bound`") as e:
        P.steps_for_solve("branch_bound")
    assert "fourier_curve`" not in str(e.value).split("])")[-1]  # no hint for branch_bound
    assert P.REFUSED_ALIASES["fourier"] == "fourier_curve" and "branch_bound" not in P.REFUSED_ALIASES


def test_header_bindings_agree():
    from teeline_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    body = re.search(r"typedef struct tl_fourier_opts \{(.*?)\} tl_fourier_opts;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", body, re.M)
    ctype = {"uint32_t": C.c_uint32, "double": C.c_double}
    assert [(("lam" if nm == "lambda" else nm), ctype[t]) for t, nm in fields] == list(_capi.TlFourierOpts._fields_)
    assert C.sizeof(_capi.TlFourierOpts) == 48
    spec = open(os.path.join(ROOT, "teeline_amd", "csrc", "fourier_spec.h")).read()
    assert float(re.search(r"kFourierBasisMeasuredAbsDiff = ([0-9.e-]+);", spec).group(1)) == FO.BASIS_MEASURED_ABS_DIFF
    for name, tag in (("berlin52", "Berlin52"), ("a280", "A280")):
        assert int(re.search(rf"kFourier{tag}MovedCities = (\d+);", spec).group(1)) == FO.MEASURED[name]["moved"]
        assert int(re.search(rf"kFourier{tag}TiedQueries = (\d+);", spec).group(1)) == FO.MEASURED[name]["ties"]
    for k, v in (("kFourierMaxK", FO.MAX_K), ("kFourierMaxM", FO.MAX_M), ("kFourierMaxN", FO.MAX_N)):
        assert int(re.search(rf"{k} = (\d+);", spec).group(1)) == v


# ---------------------------------------------------------------- the reference's own unit situations (fourier.rs:139-235)
def test_reference_unit_test_properties():
    fast = FC.o(2, 50, 20)
    res = FC.oracle("circle5")
    assert sorted(res["tour"].tolist()) == [0, 1, 2, 3, 4]                      # the 5-city circle gives a permutation
    from teeline_amd.host import TspProblem
    prob = TspProblem([5, 10, 15, 20, 25], FC.circle(5))                         # non-contiguous ids come back as ids
    assert sorted(int(v) for v in prob.ids[res["tour"]]) == [5, 10, 15, 20, 25]
    # one step lowers the energy on the 3-city triangle (k_max 1, m 30, lambda 0.05, lr 0.05)
    tri = FC.circle(3)
    z = tri.astype(np.float64)
    c0 = FO.init_coefficients(tri, 1)
    Br, Bi = FO.basis_spec(1, 30)
    c1, _idx, _t = FO.step_numpy(c0, Br, Bi, z, tri, 1, 1, np.float64(0.05), np.float64(0.05) / np.float64(3))
    assert FO.energy(c1, 1, 30, z, 0.05) < FO.energy(c0, 1, 30, z, 0.05)
    # the initial curve is a circle of radius / 2 around the centroid
    c = np.zeros((3, 2))
    c[1], c[2] = (1.0, 0.0), (0.5, 0.0)
    gr, gi = FO.gamma_of(c, *FO.basis_spec(1, 100))
    assert abs(float(np.max(np.hypot(gr - 1.0, gi))) - 0.5) < 0.05
    assert fast == CASES["circle5"][3]


# ---------------------------------------------------------------- the measured sizes of the departures
def test_basis_departure_is_within_twice_the_measured_size():
    worst = 0.0
    for m in (2, 50, 200, 4096):
        sr, si = FO.basis_spec(32, m)
        lr, li = FO.basis_libm(32, m)
        worst = max(worst, float(np.abs(sr - lr).max()), float(np.abs(si - li).max()))
    print("largest |E - libm| over m in {2, 50, 200, 4096}, |k| <= 32:", worst)
    assert worst <= 2.0 * FO.BASIS_MEASURED_ABS_DIFF
    for m in (2, 3, 50, 200, 4096):  # the reduction of k j is exact: the table is on the unit circle to an ulp, E[0] = 1
        E = FO.basis_table(m)
        assert E[0].tolist() == [1.0, 0.0] and float(np.abs(np.hypot(E[:, 0], E[:, 1]) - 1.0).max()) <= 2.3e-16


def test_berlin52_tour_equals_the_libm_variants():
    """default options: no city's tour position differs between the specification and the libm variant; the tied queries are counted"""
    xy = K.tsplib("berlin52")["xy"]
    spec = FO.solve(xy, None, 52, count_ties=True, log_cap=0, **FO.DEFAULTS)
    libm = FO.solve(xy, None, 52, arith="libm", log_cap=0, **FO.DEFAULTS)
    moved = int((np.argsort(spec["tour"]) != np.argsort(libm["tour"])).sum())
    print("berlin52: moved cities", moved, "tied queries", spec["ties"])
    assert moved == FO.MEASURED["berlin52"]["moved"] and spec["ties"] == FO.MEASURED["berlin52"]["ties"]
    assert spec["tour"].tolist() == FC.oracle("berlin52")["tour"].tolist()
