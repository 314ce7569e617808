"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads, exports every symbol the
header declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teeline_gpu.h")


def header_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import build
    build.build()
    from teeline_amd import _capi
    return _capi.load()


def test_header_declares_what_the_binding_lists():
    from teeline_amd import _capi
    assert header_symbols() == sorted(_capi.SYMBOLS)


def header_constants(prefix):
    out = {}
    for name, val in re.findall(r"#define\s+(" + prefix + r"[A-Z0-9_]+)\s+\(?([^/\n]*?)\)?\s*(?:/\*|$)", open(HEADER).read(), flags=re.M):
        val = val.strip().replace("u", "")
        out[name] = eval(val, {"__builtins__": {}})  # "1 << 13", "-4", "0"
    return out


def test_flags_modes_and_error_codes_agree_with_the_binding():
    from teeline_amd import _capi
    consts = {}
    for prefix in ("TL_FLAG_", "TL_ERR_", "TL_MODE_", "TL_DM_", "TL_DIST_"):
        consts.update(header_constants(prefix))
    assert len([k for k in consts if k.startswith("TL_FLAG_")]) >= 12
    flags = [v for k, v in consts.items() if k.startswith("TL_FLAG_") and v]
    assert len(set(flags)) == len(flags) and all(v & (v - 1) == 0 for v in flags), "create flags are distinct single bits"
    for name, val in consts.items():
        assert hasattr(_capi, name), f"{name} is in the header but not in teeline_amd/_capi.py"
        assert getattr(_capi, name) == val, f"{name}: header {val}, binding {getattr(_capi, name)}"


def test_library_exports_every_declared_symbol(lib):
    for name in header_symbols():
        assert hasattr(lib, name), f"libteeline_gpu.so does not export {name}"
    assert lib.tl_abi_version() == 5
    assert b"gfx950" in lib.tl_version()


def test_library_contains_gfx950_code_object():
    from teeline_amd import _capi
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-S", _capi.LIB_PATH], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("llvm-readelf unavailable")
    assert ".hip_fatbin" in out.stdout
    blob = open(_capi.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"k_two_opt_ref_lds" in blob


def test_pack_cost_key_orders_by_cost_then_restart(lib):
    k = lib.tl_pack_cost_key
    assert k(1.0, 5) < k(1.5, 0) and k(2.0, 3) < k(2.0, 4) and k(77647.55469, 0) >> 32 == 0x4797A7C7


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    rc = lib.tl_create(0, 0, C.byref(h))
    assert rc == -3 and not h.value  # TL_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.tl_last_error(None)
    import teeline_amd
    with pytest.raises(teeline_amd.TeelineGpuError):
        teeline_amd.Context(0)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "teeline_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "tl_oracle" not in text and "libtl_oracle" not in text, f"{f} references the oracle"
                assert not re.search(r"^\s*(from|import)\s+_?oracle", text, flags=re.M), f"{f} imports the oracle"


def test_host_mirror_tsplib_and_types(tsplib_dir):
    import numpy as np
    import teeline_amd as T
    import _tsplib
    for name in ("berlin52", "a280", "att532", "gr17", "ring6_explicit", "bays29", "burma14", "att48"):
        d = T.tsplib.read_from_file(os.path.join(tsplib_dir, f"{name}.tsp"))
        e = _tsplib.parse_tsplib(os.path.join(tsplib_dir, f"{name}.tsp"))
        assert len(d) == e["n"] and np.array_equal(d.xy, e["xy"]) and np.array_equal(d.ids, e["ids"])
        if e["packed"] is not None:
            assert np.array_equal(d.raw_distances, e["packed"])
    d = T.tsplib.read_from_file(os.path.join(tsplib_dir, "att532.tsp"))
    assert d.distance_type == "euc2d"  # ATT silently becomes EUC_2D (tsplib.rs:199-202)
    with pytest.raises(ValueError):
        T.tsplib.read_from_str("NAME: x\nTYPE: ATSP\nDIMENSION: 2\nNODE_COORD_SECTION\n1 0 0\n2 1 1\nEOF\n")
    p = T.TspProblem([1, 2, 3], [[0, 0], [1, 0], [0, 1]])
    assert p.positions_of([3, 1, 2]).tolist() == [2, 0, 1]
    with pytest.raises(T.ReferencePanics):
        p.positions_of([3, 1, 9])
    assert T.validate_tour([3, 1, 2], p) and not T.validate_tour([3, 1, 1], p)
    with pytest.raises(ValueError):
        T.LKOptions(max_depth=0).validate()


def test_cpp_host_mirror_builds_and_fails_loudly_without_gpu(tsplib_dir):
    import torch
    from teeline_amd import build
    cli = build.build_cli()
    assert os.path.exists(cli)
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([cli, "solve", "2opt", "-i", os.path.join(tsplib_dir, "berlin52.tsp")], capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr and r.stdout == ""
    r = subprocess.run([cli, "bogus"], capture_output=True, text=True)
    assert r.returncode == 2


def _c_arg_count(decl):
    args = decl.strip()
    if args in ("", "void"):
        return 0
    return args.count(",") + 1


def test_rust_binding_matches_the_header():
    """integration/teeline-gpu/src/lib.rs (the FFI crate a maintainer adds to the reference workspace) cannot be compiled
    here (no cargo/rustc): check its `extern "C"` block against the header instead — every bound symbol is declared, with
    the same number of arguments."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    hdr = {m.group(1): _c_arg_count(m.group(2)) for m in re.finditer(r"\b(tl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    rs = open(os.path.join(ROOT, "integration", "teeline-gpu", "src", "lib.rs")).read()
    block = rs[rs.index('unsafe extern "C" {'):]
    block = block[:block.index("\n}\n")]
    bound = {m.group(1): _c_arg_count(m.group(2)) for m in re.finditer(r"fn (tl_[a-z0-9_]+)\(([^)]*)\)", block, flags=re.S)}
    assert {"tl_two_opt", "tl_three_opt", "tl_lk", "tl_or_opt", "tl_nearest_neighbor", "tl_dm_is_euc2d", "tl_create",
            "tl_two_opt_multistart_devices"} <= set(bound)
    for name, argc in bound.items():
        assert name in hdr, f"{name} is not declared in teeline_gpu.h"
        assert hdr[name] == argc, f"{name}: header has {hdr[name]} arguments, lib.rs {argc}"
    m = re.search(r"TL_ABI_VERSION: c_int = (\d+)", rs)
    assert m and f"#define TL_ABI_VERSION {m.group(1)}" in open(HEADER).read()


def test_reference_patch_applies_cleanly(tmp_path):
    """integration/patches/0001-gpu-feature.patch against the reference tree it was cut against, kept as SHA-256 digests in
    tests/golden/reference_patch_targets.json (make_patch_fingerprint.py): every hunk replaces exactly the reference's lines at the
    line numbers it names, and `patch` takes it without offset or fuzz on a tree rebuilt from those lines."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_patch_fingerprint as F
    want = json.load(open(F.OUT))
    got = F.parse(open(F.PATCH).read())
    assert sorted(got) == sorted(want)
    for path, hunks in got.items():
        if want[path] is None:
            assert all(s == 0 and n == 0 for s, n, _ in hunks), f"{path}: not in the reference tree, but the patch edits it"
            continue
        assert [[s, n, F.sha(old)] for s, n, old in hunks] == want[path]["hunks"], f"{path}: a hunk does not fit the reference's lines"
        text = [f"{path}: line {k + 1}\n" for k in range(want[path]["lines"])]
        for s, n, old in hunks:
            text[s - 1:s - 1 + n] = old
        dst = tmp_path / path
        dst.parent.mkdir(parents=True, exist_ok=True)
        dst.write_text("".join(text))
    patch = F.PATCH
    r = subprocess.run(["patch", "-p1", "--dry-run", "-F0", "-d", str(tmp_path), "-i", patch], capture_output=True, text=True)
    assert r.returncode == 0 and "offset" not in r.stdout and "fuzz" not in r.stdout, r.stdout + r.stderr
    # the three arms SURVEY.md §8(b) names are switched, and the module added by the patch is the file kept beside the crate
    text = open(patch).read()
    for arm in ("two_opt_impl::solve(problem, &h, tx, init_tour)", "three_opt_impl::solve(problem, &h, tx, init_tour)",
                "lk_impl::solve(problem, &lk, tx, init_tour)"):
        assert "+" + " " * 8 + "Solvers::" in text and arm in text
    gpu_rs = open(os.path.join(ROOT, "integration", "teeline-gpu", "gpu.rs")).read()
    for sig in ("progress_tx: Option<&mpsc::Sender<ProgressMessage>>", "init_tour: Option<&[usize]>", ") -> Solution {"):
        assert gpu_rs.count(sig) >= 4


def test_reference_patch_carries_the_current_gpu_rs():
    """The new-file hunk `src/tsp/gpu.rs` of the reference patch is integration/teeline-gpu/gpu.rs, line for line
    (scripts/refresh_patch.py rebuilds it)."""
    import subprocess
    import sys
    assert subprocess.call([sys.executable, os.path.join(ROOT, "scripts", "refresh_patch.py"), "--check"]) == 0


def test_rust_side_compiles():
    """scripts/check_rust.sh: `cargo check` of the FFI crate (and of the patched reference where $TEELINE_REFERENCE_DIR names a
    checkout).  Exit 3 = no Rust toolchain on this box: the Rust side is UNCOMPILED — reported as an expected failure so that it
    shows in every summary instead of passing silently."""
    import shutil
    ref = os.environ.get("TEELINE_REFERENCE_DIR")
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "check_rust.sh")] + ([ref] if ref else []), capture_output=True, text=True)
    if r.returncode == 3:
        assert shutil.which("cargo") is None
        pytest.xfail("no cargo / rustc in this image: integration/teeline-gpu (lib.rs, gpu.rs, the reference patch) has never been compiled")
    assert r.returncode == 0, r.stdout + r.stderr


def test_two_opt_plan_is_the_selection_rule(lib):
    # host-only: which form of the LDS descent a batch runs (threads per descent, late phase on neighbour lists) on an MI355X-sized
    # device (256 CUs, 160 KB of LDS).  DESIGN.md §8.
    from teeline_amd import _capi

    def plan(n, count, flags=0):
        t, l = C.c_int(), C.c_int()
        assert lib.tl_two_opt_plan(n, count, 256, 163840, flags, C.byref(t), C.byref(l)) == 0
        return t.value, l.value

    assert plan(10000, 256) == (1024, 1)        # the headline batch: one descent per CU, late phase
    assert plan(10000, 1) == (1024, 1)
    assert plan(10000, 256, _capi.TL_FLAG_2OPT_NO_NL) == (1024, 0)
    assert plan(10000, 256, _capi.TL_FLAG_NO_PRUNE) == (1024, 0)
    assert plan(12416, 256) == (1024, 1) and plan(12417, 256) == (1024, 0)   # the late phase's state no longer fits beside the tour
    assert plan(399, 1) == (1024, 0) and plan(400, 1) == (1024, 1)
    assert plan(26, 1, _capi.TL_FLAG_2OPT_NL_ALWAYS) == (1024, 1) and plan(25, 1, _capi.TL_FLAG_2OPT_NL_ALWAYS) == (1024, 0)
    assert plan(5000, 512) == (512, 1) and plan(5568, 512) == (512, 1) and plan(5569, 512) == (512, 0)   # two descents per CU
    assert plan(6000, 512) == (512, 0)
    assert plan(2000, 1024) == (256, 1) and plan(3000, 1024) == (256, 0)       # four per CU
    assert plan(10000, 512) == (1024, 0) or plan(10000, 512) == (1024, 1)      # (float2: two tours do not fit; the grid form is decided on the device)
    assert plan(20000, 1) == (0, 0)                                             # beyond the LDS-resident limit
    assert plan(4000, 1, _capi.TL_FLAG_2OPT_NT512) == (512, 1)
