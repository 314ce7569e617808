"""CPU-side checks of the Or-opt population entry (tl_or_opt_population, tl_or_opt_lds_max_n): the symbols are bound and exported,
the flag agrees between header and binding, nothing computes without a device, and the host mirrors refuse bad input before they
touch a context."""
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
    for name in ("tl_or_opt_population", "tl_or_opt_lds_max_n"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), f"libteeline_gpu.so does not export {name}"
    assert lib.tl_or_opt_lds_max_n.restype is C.c_uint32 and len(lib.tl_or_opt_population.argtypes) == 10
    assert lib.tl_abi_version() == 5  # an addition: the version stays
    assert lib.tl_or_opt_lds_max_n(None) == 0


def test_flag_value_agrees_with_the_header():
    from teeline_amd import _capi
    import teeline_amd
    m = re.search(r"#define\s+TL_FLAG_OR_OPT_FORCE_SCAN\s+\(1u << (\d+)\)", open(HEADER).read())
    assert m and _capi.TL_FLAG_OR_OPT_FORCE_SCAN == 1 << int(m.group(1)) == teeline_amd.TL_FLAG_OR_OPT_FORCE_SCAN
    others = [getattr(_capi, k) for k in dir(_capi) if k.startswith("TL_FLAG_") and k != "TL_FLAG_OR_OPT_FORCE_SCAN"]
    assert _capi.TL_FLAG_OR_OPT_FORCE_SCAN not in others


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import teeline_amd as TA
    h = C.c_void_p()
    assert lib.tl_create(0, TA.TL_FLAG_OR_OPT_FORCE_SCAN, C.byref(h)) == -3 and not h.value  # TL_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.tl_last_error(None)
    # without a context the entry refuses, whatever else it is given
    xy = np.zeros((5, 2), np.float32)
    init = np.arange(5, dtype=np.uint32)
    out = np.full(5, 77, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tl_or_opt_population(None, vp(xy), 5, None, vp(init), 1, vp(out), None, None, None) == TA._capi.TL_ERR_BADARG
    assert out.tolist() == [77] * 5
    prob = TA.TspProblem(np.arange(5) + 1, xy)
    with pytest.raises(TA.TeelineGpuError):
        TA.or_opt.solve_population(prob, [[1, 2, 3, 4, 5]])
    with pytest.raises(TA.TeelineGpuError):
        TA.pipeline.run_population(prob, ["2opt", "or_opt"], [[1, 2, 3, 4, 5]])


class _NoContext:
    """Stands where a context would: any use of it is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name})")


def test_run_population_rejects_other_steps_before_touching_a_context():
    import teeline_amd as TA
    prob = TA.TspProblem(np.arange(6) + 1, np.zeros((6, 2), np.float32))
    tours = [[1, 2, 3, 4, 5, 6]]
    with pytest.raises(ValueError, match="lk"):
        TA.pipeline.run_population(prob, ["2opt", "lk"], tours, ctx=_NoContext())
    with pytest.raises(ValueError, match="nn"):
        TA.pipeline.run_population(prob, ["nn", "or_opt"], tours, ctx=_NoContext())
    with pytest.raises(ValueError, match="bogus"):
        TA.pipeline.run_population(prob, ["bogus"], tours, ctx=_NoContext())
    assert TA.pipeline.run_population(prob, [], tours, ctx=_NoContext()) == [[]]


def test_solve_population_checks_tour_lengths_before_any_pointer():
    import teeline_amd as TA
    prob = TA.TspProblem(np.arange(6) + 1, np.zeros((6, 2), np.float32))
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.or_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5]], ctx=_NoContext())
    assert e.value.code == TA._capi.TL_ERR_BADARG and "tour 1" in str(e.value)
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.or_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6, 6]], ctx=_NoContext())
    assert e.value.code == TA._capi.TL_ERR_BADARG
