"""CPU-side checks of best-sweep 2-opt for batches (tl_two_opt_best_population, tl_two_opt_best_lds_max_n, tl_two_opt_best_plan,
tl_two_opt_best_force_scan): the symbols are bound and exported, forcing the loop is a context setting and no create flag (bit 31
stays unassigned), the plan is the selection rule, nothing computes without a device, and the mirror refuses ragged tours before it
touches a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teeline_gpu.h")


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import build
    build.build()
    from teeline_amd import _capi
    return _capi.load()


def test_symbols_are_bound_and_exported(lib):
    from teeline_amd import _capi
    for name in ("tl_two_opt_best_population", "tl_two_opt_best_lds_max_n", "tl_two_opt_best_plan", "tl_two_opt_best_force_scan"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), f"libteeline_gpu.so does not export {name}"
    assert lib.tl_two_opt_best_lds_max_n.restype is C.c_uint32
    assert len(lib.tl_two_opt_best_population.argtypes) == 9 and len(lib.tl_two_opt_best_plan.argtypes) == 7
    assert lib.tl_abi_version() == 5  # additions: the version stays
    assert lib.tl_two_opt_best_lds_max_n(None) == 0


def test_forcing_the_loop_is_a_setting_not_a_create_flag(lib):
    """All 31 assigned tl_create bits are taken and the seeded solvers refuse bit 31 as `the one bit no flag has` (their tests pin that),
    so the cross-check form is switched by tl_two_opt_best_force_scan(ctx, on)."""
    from teeline_amd import _capi
    text = open(HEADER).read()
    assert "TL_FLAG_2OPT_BEST" not in text and not [k for k in dir(_capi) if k.startswith("TL_FLAG_2OPT_BEST")]
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags
    assert re.search(r"int tl_two_opt_best_force_scan\(tl_ctx \*ctx, int on\);", text) and len(lib.tl_two_opt_best_force_scan.argtypes) == 2
    assert lib.tl_two_opt_best_force_scan(None, 1) == _capi.TL_ERR_BADARG


def test_plan_is_the_selection_rule(lib):
    # host-only, on an MI355X-sized device (256 CUs, 160 KB of LDS); the limit is DESIGN.md §8's formula
    from teeline_amd import _capi

    def plan(n, count, force_scan=0, lds=163840):
        f, t = C.c_int(-1), C.c_int(-1)
        assert lib.tl_two_opt_best_plan(n, count, 256, lds, force_scan, C.byref(f), C.byref(t)) == 0
        return f.value, t.value

    def lds_bytes(n):
        n_pad = (n + 64 + 63) // 64 * 64
        return 18 * n_pad + 20 * (((n_pad >> 6) + 63) // 64 * 64) + 144

    top = max(n for n in range(3, 12000) if lds_bytes(n) <= 163840)
    assert top == 8768
    assert plan(200, 256) == (0, 1024) and plan(top, 256) == (0, 1024)
    assert plan(top + 1, 256) == (1, 0) and plan(10000, 256) == (1, 0) and plan(65535, 1) == (1, 0)
    assert plan(200, 256, 1) == (1, 0)
    assert plan(3, 8)[0] == 0 and plan(5, 8) == (0, 128) and plan(19, 8) == (0, 1024)  # no more waves than rows
    assert plan(64, 515) == (0, 512)  # more descents than CUs: narrower workgroups share a CU
    assert plan(200, 1, lds=65536) == (0, 1024) and plan(4000, 1, lds=65536) == (1, 0)
    f, t = C.c_int(), C.c_int()
    assert lib.tl_two_opt_best_plan(200, 1, 256, 163840, 0, None, C.byref(t)) == _capi.TL_ERR_BADARG
    assert lib.tl_two_opt_best_plan(200, 1, 256, 163840, 0, C.byref(f), None) == _capi.TL_ERR_BADARG
    assert lib.tl_two_opt_best_plan(200, 1, 0, 163840, 0, C.byref(f), C.byref(t)) == _capi.TL_ERR_BADARG


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import teeline_amd as TA
    h = C.c_void_p()
    assert lib.tl_create(0, 0, C.byref(h)) == -3 and not h.value  # TL_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.tl_last_error(None)
    # without a context the entry refuses, whatever else it is given
    xy = np.zeros((5, 2), np.float32)
    init = np.arange(5, dtype=np.uint32)
    out = np.full(5, 77, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tl_two_opt_best_population(None, vp(xy), 5, vp(init), 1, vp(out), None, None, None) == TA._capi.TL_ERR_BADARG
    assert out.tolist() == [77] * 5
    prob = TA.TspProblem(np.arange(5) + 1, xy)
    with pytest.raises(TA.TeelineGpuError):
        TA.two_opt.solve_population(prob, [[1, 2, 3, 4, 5]], mode=TA.TL_MODE_BEST_SWEEP)


class _NoContext:
    """Stands where a context would: any use of it is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name})")


def test_solve_population_checks_tour_lengths_before_any_pointer():
    import teeline_amd as TA
    prob = TA.TspProblem(np.arange(6) + 1, np.zeros((6, 2), np.float32))
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.two_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5]], ctx=_NoContext(), mode=TA.TL_MODE_BEST_SWEEP)
    assert e.value.code == TA._capi.TL_ERR_BADARG and "tour 1" in str(e.value)
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.two_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6, 6]], ctx=_NoContext(), mode=TA.TL_MODE_BEST_SWEEP)
    assert e.value.code == TA._capi.TL_ERR_BADARG
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.two_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6]], ctx=_NoContext(), mode=7)
    assert e.value.code == TA._capi.TL_ERR_BADARG
