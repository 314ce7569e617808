"""CPU-side checks of the 3-opt population entry (tl_three_opt_population, tl_three_opt_pop_max_n, tl_three_opt_population_plan,
tl_three_opt_population_work_limit): the symbols are bound and exported, the flags agree between header and binding, nothing
computes without a device, the host mirrors refuse bad input before they touch a context, and the plan is the selection rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teeline_gpu.h")
FLAGS = ("TL_FLAG_3OPT_POP_FORCE_SCAN", "TL_FLAG_3OPT_POP_FORCE_WG")
CUS, LDS, GIB8 = 256, 163840, 8 << 30  # an MI355X-sized device and the default workspace limit


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import build
    build.build()
    from teeline_amd import _capi
    return _capi.load()


def test_symbols_are_bound_and_exported(lib):
    from teeline_amd import _capi
    for name in ("tl_three_opt_population", "tl_three_opt_pop_max_n", "tl_three_opt_population_plan", "tl_three_opt_population_work_limit"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), f"libteeline_gpu.so does not export {name}"
    assert lib.tl_three_opt_pop_max_n.restype is C.c_uint32 and len(lib.tl_three_opt_population.argtypes) == 10
    assert len(lib.tl_three_opt_population_plan.argtypes) == 9 and len(lib.tl_three_opt_population_work_limit.argtypes) == 2
    assert lib.tl_abi_version() == 5  # an addition: the version stays
    assert lib.tl_three_opt_pop_max_n(None) == 0
    assert lib.tl_three_opt_population_work_limit(None, 0) == _capi.TL_ERR_BADARG


def test_flag_values_agree_with_the_header():
    from teeline_amd import _capi
    import teeline_amd
    text = open(HEADER).read()
    for name in FLAGS:
        m = re.search(r"#define\s+" + name + r"\s+\(1u << (\d+)\)", text)
        assert m and 27 <= int(m.group(1)) <= 31
        assert getattr(_capi, name) == 1 << int(m.group(1)) == getattr(teeline_amd, name)
        others = [getattr(_capi, k) for k in dir(_capi) if k.startswith("TL_FLAG_") and k != name]
        assert getattr(_capi, name) not in others


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import teeline_amd as TA
    h = C.c_void_p()
    assert lib.tl_create(0, TA.TL_FLAG_3OPT_POP_FORCE_WG, C.byref(h)) == -3 and not h.value  # TL_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.tl_last_error(None)
    # without a context the entry refuses, whatever else it is given
    xy = np.zeros((5, 2), np.float32)
    init = np.arange(5, dtype=np.uint32)
    out = np.full(5, 77, np.uint32)
    costs = np.full(1, 77, np.float32)
    moves = np.full(1, 77, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tl_three_opt_population(None, vp(xy), 5, None, vp(init), 1, vp(out), vp(costs), vp(moves), None) == TA._capi.TL_ERR_BADARG
    assert out.tolist() == [77] * 5 and costs.tolist() == [77.0] and moves.tolist() == [77]
    prob = TA.TspProblem(np.arange(5) + 1, xy)
    with pytest.raises(TA.TeelineGpuError):
        TA.three_opt.solve_population(prob, [[1, 2, 3, 4, 5]])
    # "3opt" is a population step now: the pipeline reaches the device layer, which has no device here
    with pytest.raises(TA.TeelineGpuError):
        TA.pipeline.run_population(prob, ["2opt", "3opt", "or_opt"], [[1, 2, 3, 4, 5]])


class _NoContext:
    """Stands where a context would: any use of it is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name})")


def test_run_population_takes_3opt_and_still_rejects_the_rest():
    import teeline_amd as TA
    assert "three_opt" in TA.pipeline.POPULATION_SOLVERS
    prob = TA.TspProblem(np.arange(6) + 1, np.zeros((6, 2), np.float32))
    tours = [[1, 2, 3, 4, 5, 6]]
    for steps, bad in ((["3opt", "lk"], "lk"), (["nn", "three_opt"], "nn"), (["3opt", "bogus"], "bogus")):
        with pytest.raises(ValueError, match=bad):
            TA.pipeline.run_population(prob, steps, tours, ctx=_NoContext())
    # accepted: the step is looked up and run — the first thing it does is use the context
    with pytest.raises(AssertionError, match="the context was touched"):
        TA.pipeline.run_population(prob, ["3opt"], tours, ctx=_NoContext())


def test_solve_population_checks_tour_lengths_before_any_pointer():
    import teeline_amd as TA
    prob = TA.TspProblem(np.arange(6) + 1, np.zeros((6, 2), np.float32))
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.three_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5]], ctx=_NoContext())
    assert e.value.code == TA._capi.TL_ERR_BADARG and "tour 1" in str(e.value)
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.three_opt.solve_population(prob, [[1, 2, 3, 4, 5, 6, 6]], ctx=_NoContext())
    assert e.value.code == TA._capi.TL_ERR_BADARG


def plan(lib, n, count, flags=0, work=GIB8, cus=CUS, lds=LDS):
    f, t, b = C.c_int(-1), C.c_int(-1), C.c_uint32(0xFFFF)
    assert lib.tl_three_opt_population_plan(n, count, cus, lds, work, flags, C.byref(f), C.byref(t), C.byref(b)) == 0
    return f.value, t.value, b.value


def test_plan_is_the_selection_rule(lib):
    from teeline_amd import _capi
    SCAN, WG = _capi.TL_FLAG_3OPT_POP_FORCE_SCAN, _capi.TL_FLAG_3OPT_POP_FORCE_WG
    max_n = (LDS - 264) // 20  # 20 bytes per city, the 8 of Pt[n] and 256 of reduction slots
    # one large tour leaves all CUs but one idle; a CU's worth of small tours pays four launches per move in the loop
    assert plan(lib, 1000, 1)[0] == 0
    assert plan(lib, 64, CUS)[0] == 1
    # either force flag wins over the model (and the loop over the workgroup form where both are set)
    assert plan(lib, 1000, 1, WG)[0] == 1 and plan(lib, 64, CUS, SCAN)[0] == 0 and plan(lib, 64, CUS, SCAN | WG)[0] == 0
    # beyond the LDS fit: the loop, even when forced
    assert plan(lib, max_n, 4, WG, work=1 << 40)[0] == 1 and plan(lib, max_n + 1, 4, WG, work=1 << 40)[0] == 0
    assert plan(lib, 64, CUS, WG, lds=64 * 20 + 264)[0] == 1 and plan(lib, 64, CUS, WG, lds=64 * 20 + 263)[0] == 0
    # batch = floor(work_bytes / Dt bytes), at most count; not even one matrix: the loop
    dt = 200 * 201 * 4
    assert plan(lib, 200, 256, WG)[2] == 256
    assert plan(lib, 200, 256, WG, work=3 * dt + dt - 1)[::2] == (1, 3)
    assert plan(lib, 200, 256, WG, work=dt)[::2] == (1, 1)
    assert plan(lib, 200, 256, WG, work=dt - 1)[::2] == (0, 0)
    assert plan(lib, 1002, 3000, WG)[2] == GIB8 // (1002 * 1003 * 4) == 2136
    # threads: a multiple of 64 in [64, 1024] in the workgroup form (0 in the loop form): no more waves than units of 8 j ...
    for n, count in ((4, 1), (5, 1), (9, 1), (10, 1), (13, 1), (14, 1), (52, 256), (52, 515), (200, 1024), (200, 5000), (1000, 256), (max_n, 2)):
        f, t, b = plan(lib, n, count, WG, work=1 << 40)
        assert f == 1 and t % 64 == 0 and 64 <= t <= 1024, (n, count, t)
    assert [plan(lib, n, 1, WG)[1] for n in (4, 5, 9, 10, 13, 14)] == [128, 128, 256, 512, 512, 1024]
    # ... and no wider than lets a CU hold its share of the batch (2 048 threads a CU)
    assert [plan(lib, 52, c, WG)[1] for c in (256, 512, 515, 1024, 5000)] == [1024, 1024, 512, 512, 64]
    assert plan(lib, 64, CUS, SCAN)[1] == 0
    # the share is of the batch, not of the count: three tours at a time are one per CU
    assert plan(lib, 200, 5000, WG, work=3 * dt)[1:] == (1024, 3)
    # a device that is none
    assert lib.tl_three_opt_population_plan(64, 4, 0, LDS, GIB8, 0, None, None, None) == _capi.TL_ERR_BADARG
    assert lib.tl_three_opt_population_plan(64, 4, CUS, LDS, GIB8, 0, None, None, None) == 0  # every output is optional
