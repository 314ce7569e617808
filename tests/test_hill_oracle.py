"""The stochastic hill climb without a GPU: the statement of the specification (tests/_hill_oracle.py) against the stand-alone C++
restatement (tests/probes/hill_cpu_baseline.cpp, also once under host ASan/UBSan), the frozen goldens and the library's host-only
queries (tl_hill_draw, tl_hill_climb_plan); the draw roles; header, bindings and names."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _hill_cases as HC
import _hill_oracle as HO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_hill.json")))
CASES = HC.cases()
LDS = 163840


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import _capi, build
    build.build()
    return _capi.load()


def _compile(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc")] + extra +
                          [os.path.join(ROOT, "tests", "probes", "hill_cpu_baseline.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("hill"), "hill_cpu_baseline", [])


def write_case(tmp_path, xy, packed, n, init):
    path = str(tmp_path / "case.txt")
    with open(path, "w") as fh:
        if packed is None:
            fh.write(f"{n} xy\n" + "".join(f"{float(x)!r} {float(y)!r}\n" for x, y in xy))
        else:
            full = np.zeros((n, n), dtype=np.float32)
            full[np.tril_indices(n, -1)] = packed
            full = full + full.T
            fh.write(f"{n} dm\n" + "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in full))
    args = [path]
    if init is not None:
        ipath = str(tmp_path / "init.txt")
        with open(ipath, "w") as fh:
            fh.write(" ".join(str(int(v)) for v in init) + "\n")
        args += ["--init", ipath]
    return args


def check_baseline(exe, tmp_path, name):
    xy, packed, n, init, o, _want = CASES[name]
    res = HC.run(name, CASES[name])
    args = [exe] + write_case(tmp_path, xy, packed, n, init) + ["--trace", "--epochs", str(o["epochs"]), "--platoo", str(o["platoo_epochs"]), "--seed", str(o["seed"]),
                                                                "--chain", str(o["chain"])]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    epochs, accepts, restarts, reversed_, cost_bits = (int(v) for v in lines[0].split()[:5])
    c = res["counters"]
    assert (epochs, accepts, restarts, reversed_, cost_bits) == (o["epochs"] + 1, c["accepts"], c["restarts"], c["reversed"], HO.bits(res["cost"])), name
    assert [int(v) for v in lines[1].split()] == res["tour"].tolist(), name
    assert [[int(v) for v in ln.split()] for ln in lines[2:]] == HO.log_words(res).tolist(), name


# ---------------------------------------------------------------- the three statements agree
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_goldens(name):
    HC.check_conditions(name, CASES[name])
    assert HC.case_record(HC.run(name, CASES[name])) == GOLD["cases"][name]


def test_goldens_hold_every_case():
    assert sorted(GOLD["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpp_restatement_equals_oracle(baseline, tmp_path, name):
    check_baseline(baseline, tmp_path, name)


def test_cpp_restatement_is_clean_under_host_sanitizers(tmp_path):
    """the stand-alone program (its own main, no GPU code) under ASan and UBSan: the same output, nothing reported"""
    exe = _compile(tmp_path, "hill_cpu_baseline_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    for name in ("small2", "small8_p1", "gr17_matrix", "berlin52_p7", "last_epoch_restart"):
        check_baseline(exe, tmp_path, name)
    assert subprocess.run([exe, "x", "--draws"], capture_output=True, text=True).returncode == 0


def test_cpp_restatement_draws(baseline):
    out = [int(v) for v in subprocess.run([baseline, "x", "--draws", "--seed", "9", "--chain", "2"], capture_output=True, text=True, check=True).stdout.split()]
    want = [HO.draw(9, 2, e, s) for e in range(2) for s in range(22)] + [HO.draw(9, 2, HO.shuffle_event(3, 7, j), HO.SLOT_SHUFFLE) for j in range(1, 7)]
    assert out == want


def test_window_resolution_equals_the_epoch_chain():
    """the window rule (lowest accepting lane a, tripping lane r, a <= r) stated in numpy gives the chain of solve() at any width"""
    for name in ("small5_p1", "small8_p2", "berlin52_p7", "last_epoch_restart", "berlin52_e63"):
        for W in (1, 2, 7, 64, 256):
            HC.window_record(name, W, CASES[name])


# ---------------------------------------------------------------- draws
def test_draws_equal_the_goldens_and_the_library(lib):
    for s, c, ev, sl, u in GOLD["draws"]:
        assert HO.draw(int(s), c, int(ev), sl) == int(u) == lib.tl_hill_draw(int(s), c, int(ev), sl)
    rng = np.random.default_rng(3)
    for _ in range(200):
        s, c, ev, sl = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 59)), int(rng.integers(0, 32))
        assert lib.tl_hill_draw(s, c, ev, sl) == HO.draw(s, c, ev, sl)


def test_pair_draws_are_simulated_annealings(lib):
    for e in (0, 1, 77, 0xFFFFFFFE):
        for sl in range(22):
            assert lib.tl_hill_draw(5, 3, e, sl) == lib.tl_sa_draw(5, 3, e, sl)


def test_shuffle_draws_are_the_genetic_algorithms_stream(lib):
    assert lib.tl_hill_draw(5, 3, HO.shuffle_event(2, 9, 4), 26) == lib.tl_ga_draw(5, 3, HO.shuffle_event(2, 9, 4), 26)


@pytest.mark.parametrize("n", range(2, 9))
def test_draw_roles_are_disjoint(n):
    """no two roles share an (event, slot), and no two (event, slot) share the stream's argument 32 event + slot + 1 (mod 2^64)"""
    roles = HO.roles(n, 40)
    keys = [k for k, _role in roles]
    assert len(set(keys)) == len(keys) == 40 * (22 + n - 1)
    args = [(32 * ev + sl + 1) & HO.M64 for ev, sl in keys]
    assert len(set(args)) == len(args)
    assert all(32 * ev + sl + 1 < 1 << 64 for ev, sl in keys)  # nothing wraps
    top = HO.shuffle_event(0xFFFFFFFE, 13650, 13649)  # the last epoch at the LDS limit
    assert 32 * top + HO.SLOT_SHUFFLE + 1 < 1 << 64 and HO.shuffle_event(0, n, 1) > 0xFFFFFFFF


def test_shuffle_is_a_permutation_keyed_by_the_epoch():
    from _sa_oracle import chain_key
    a, b = np.arange(30), np.arange(30)
    HO.shuffle(chain_key(1, 0), 4, 30, a)
    HO.shuffle(chain_key(1, 0), 5, 30, b)
    assert sorted(a) == list(range(30)) and sorted(b) == list(range(30)) and a.tolist() != b.tolist() and a.tolist() != list(range(30))


# ---------------------------------------------------------------- plan and limits
def test_plan_and_limits_are_host_only(lib):
    from teeline_amd import _capi
    w, t, per = C.c_uint32(), C.c_int32(), C.c_uint32()
    out = (C.byref(w), C.byref(t), C.byref(per))
    top = (LDS - 32) // 12
    assert lib.tl_hill_climb_plan(52, 1, 256, LDS, 0, *out) == 0 and (w.value, t.value) == (256, 256) and per.value == 256 * 8
    assert lib.tl_hill_climb_plan(52, 256, 256, LDS, 0, *out) == 0 and (w.value, t.value) == (256, 256)
    assert lib.tl_hill_climb_plan(52, 257, 256, LDS, 0, *out) == 0 and (w.value, t.value) == (64, 64) and per.value == 256 * 32  # more chains than CUs
    assert lib.tl_hill_climb_plan(1002, 1024, 256, LDS, 0, *out) == 0 and per.value == 256 * (LDS // (12 * 1002 + 32))
    assert lib.tl_hill_climb_plan(top, 1, 256, LDS, 0, *out) == 0 and (w.value, t.value, per.value) == (256, 256, 256)
    assert lib.tl_hill_climb_plan(top - 1, 1, 256, LDS, 0, *out) == 0 and per.value == 256
    for n in (top + 1, 0, 1):
        assert lib.tl_hill_climb_plan(n, 1, 256, LDS, 0, *out) == 0 and (w.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_hill_climb_plan(top + 1, 1, 256, LDS, 999, *out) == 0 and (w.value, t.value, per.value) == (0, 0, 0)
    for req, cnt, want in ((1, 1, 1), (64, 1, 64), (256, 1, 256), (1, 1000, 1), (64, 1000, 64)):  # the window request
        assert lib.tl_hill_climb_plan(52, cnt, 256, LDS, req, *out) == 0 and w.value == want and t.value == (256 if cnt <= 256 else 64)
    assert lib.tl_hill_climb_plan(52, 1, 256, LDS, 257, *out) == _capi.TL_ERR_BADARG and (w.value, t.value, per.value) == (0, 0, 0)
    assert lib.tl_hill_climb_plan(52, 1000, 256, LDS, 65, *out) == _capi.TL_ERR_BADARG
    assert lib.tl_hill_climb_plan(52, 1, 0, LDS, 0, *out) == _capi.TL_ERR_BADARG and lib.tl_hill_climb_plan(52, 1, 256, -1, 0, *out) == _capi.TL_ERR_BADARG
    assert lib.tl_hill_climb_plan(52, 1, 256, LDS, 0, None, None, None) == 0
    assert lib.tl_hill_climb_lds_max_n(None) == 0


# ---------------------------------------------------------------- header, bindings, names
def test_header_bindings_and_flags_agree(lib):
    from teeline_amd import _capi, build
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert re.search(r"#define TL_ABI_VERSION 5\b", text) and lib.tl_abi_version() == 5
    for sym in ("tl_hill_climb", "tl_hill_climb_trace", "tl_hill_climb_trace_chain", "tl_hill_climb_population", "tl_hill_climb_lds_max_n", "tl_hill_climb_plan",
                "tl_hill_draw"):
        assert sym in _capi.SYMBOLS and re.search(rf"\b{sym}\(", text) and hasattr(lib, sym)
    assert re.search(r"typedef struct tl_hill_opts \{[^}]*uint32_t epochs;[^}]*uint32_t platoo_epochs;[^}]*uint32_t window;[^}]*uint32_t reserved;[^}]*\} tl_hill_opts;", text)
    assert [f for f, _ in _capi.TlHillOpts._fields_] == ["epochs", "platoo_epochs", "window", "reserved"] and C.sizeof(_capi.TlHillOpts) == 16
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags and len(flags) == len([k for k in dir(_capi) if k.startswith("TL_FLAG_") and getattr(_capi, k)])  # no new flag
    assert not re.search(r"TL_FLAG_HILL", text)
    assert "tl_api_hill.hip" in build.SOURCES and "hill_climb.hip" in build.SOURCES and "hill_spec.h" in build.HEADERS


def test_spec_header_compiles_with_a_plain_host_compiler(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "hill_spec.h"\nint main() { unsigned a[5] = {0, 1, 2, 3, 4}; tl::hill_shuffle(tl::sa_chain_key(1, 0), 0, 5, a); return a[0] > 4; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "teeline_amd", "csrc"), str(src), "-o", str(tmp_path / "t")])
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_pipeline_names_and_expansion():
    from teeline_amd.host import pipeline as P
    assert P.SOLVER_NAMES["hill_climb"] == "hill_climb" and "hill_climb" in P.AUTO_EXPAND_WITH_SHUFFLE
    assert P.steps_for_solve("hill_climb") == ["shuffle", "hill_climb"] and P.steps_for_solve("Hill_Climb", no_seed=True) == ["hill_climb"]
    for name in ("stochastic_hill", "hill"):
        assert name not in P.SOLVER_NAMES and name not in P.REFUSED_ALIASES and name not in P.REFUSED_HINTS
        with pytest.raises(ValueError, match="unknown solver") as info:
            P.steps_for_solve(name)
        assert "of this build is" not in str(info.value)
        with pytest.raises(ValueError, match="unknown solver"):
            P.run_pipeline_stages(None, [name])
    import inspect
    assert inspect.signature(P.run_pipeline_stages).parameters["hill_chains"].default == 1
    import teeline_amd
    sig = inspect.signature(teeline_amd.hill_climb.solve)
    assert [sig.parameters[k].default for k in ("seed", "chains", "window", "ctx")] == [1, 1, 0, None]


def test_messages_of_the_oracle_follow_the_reference():
    """PathUpdate(start, 0.0), PathUpdate(best, cost) per acceptance, PathUpdate(shuffled, 0.0) per restart (also on the last epoch), Done"""
    xy, packed, n, init, o, _w = CASES["last_epoch_restart"]
    res = HC.run("last_epoch_restart", CASES["last_epoch_restart"])
    msgs = HO.replay(np.arange(1, n + 1), init, res)
    assert msgs[0] == ("PathUpdate", ([int(v) + 1 for v in init], 0.0)) and msgs[-1] == ("Done", None)
    assert msgs[-2][1][1] == 0.0 and len(msgs) == 2 + len(res["log"])
    assert sorted(msgs[-2][1][0]) == list(range(1, n + 1))
