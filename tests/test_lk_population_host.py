"""CPU-side checks of Lin-Kernighan for seeded runs (tl_lk_run_seed, tl_lk_population_plan, tl_lk_population_max_n,
tl_lk_population_setting, tl_lk_population): the run-seed rule against its Python restatement, the plan as the selection rule, the
setting as a setting (no create flag), nothing computes without a device, and the mirror's argument checks come before any context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _lk_population_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teeline_gpu.h")
LDS = 163840


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import build
    build.build()
    from teeline_amd import _capi
    return _capi.load()


def test_symbols_are_bound_and_exported(lib):
    from teeline_amd import _capi
    for name in ("tl_lk_run_seed", "tl_lk_population_max_n", "tl_lk_population_plan", "tl_lk_population_setting", "tl_lk_population"):
        assert name in _capi.SYMBOLS
        assert hasattr(lib, name), f"libteeline_gpu.so does not export {name}"
    assert lib.tl_lk_run_seed.restype is C.c_uint64 and lib.tl_lk_population_max_n.restype is C.c_uint32
    assert len(lib.tl_lk_population.argtypes) == 15 and len(lib.tl_lk_population_plan.argtypes) == 9
    assert lib.tl_abi_version() == 5  # additions: the version stays
    assert lib.tl_lk_population_max_n(None, None) == 0


def test_run_seed_is_the_restated_rule(lib):
    import teeline_amd as TA
    for seed in (0, 1, 2**64 - 1):
        assert lib.tl_lk_run_seed(seed, 0) == seed
        got = [lib.tl_lk_run_seed(seed, r) for r in range(1001)]
        assert got == [P.run_seed(seed, r) for r in range(1001)]
        assert len(set(got)) == 1001
        assert all(got[r] != (seed + r) & P.M64 for r in range(1, 1001))
    assert lib.tl_lk_run_seed(1, 1) != lib.tl_lk_run_seed(2, 0)  # what seed + r would give
    assert P.run_seed(1, 5) == P.splitmix64_at(1, 2**63 + 5) and TA.lin_kernighan.run_seed(1, 5) == P.run_seed(1, 5)


def _plan(lib, n, count, opts=None, force=-1, lds=LDS, cus=256):
    from teeline_amd import _capi
    f, t, p = C.c_int(-1), C.c_int(-1), C.c_uint32(99)
    o = None if opts is None else C.byref(_capi.TlLkOpts(*opts))
    assert lib.tl_lk_population_plan(n, o, count, cus, lds, force, C.byref(f), C.byref(t), C.byref(p)) == 0
    return f.value, t.value, p.value


def test_plan_is_the_selection_rule(lib):
    # host-only, on an MI355X-sized device (256 CUs, 160 KB of LDS); options: (epochs, platoo_epochs, n_nearest, max_depth)
    from teeline_amd import _capi
    cli = (10000, 500, 3, 5)
    assert _plan(lib, 52, 8, cli, force=1) == (1, 256, 2)       # two LDS images of berlin52 share a CU
    assert _plan(lib, 200, 8, cli, force=1)[:2] == (1, 256) and _plan(lib, 201, 8, cli, force=1) == (1, 1024, 1)
    assert _plan(lib, 200, 8, None, force=1)[:2] == (1, 256)    # NULL options: the library defaults (k = 5, depth 5)
    # form 0 where the one-workgroup form does not apply (lk_ils_qcap == 0): a level of 5^7 nodes beyond the queues, n beyond the LDS fit, n < 4
    for force in (-1, 0, 1):
        assert _plan(lib, 150, 8, (15, 10, 5, 8), force=force) == (0, 0, 0)
        assert _plan(lib, 20000, 8, cli, force=force) == (0, 0, 0)
        assert _plan(lib, 3, 8, cli, force=force) == (0, 0, 0)
    assert _plan(lib, 150, 8, (15, 10, 2, 8), force=1)[:2] == (1, 256)  # the deep build's query: 2^7 nodes fit
    assert _plan(lib, 64, 8, cli, force=0) == (0, 0, 0) and _plan(lib, 64, 1, cli, force=1)[0] == 1
    assert _plan(lib, 64, 1, cli)[0] == 0                        # a lone run: tl_lk as it is
    assert _plan(lib, 52, 8, cli, force=1, lds=65536)[0] == 1 and _plan(lib, 3000, 8, cli, force=1, lds=65536)[0] == 0
    f = C.c_int()
    assert lib.tl_lk_population_plan(64, None, 8, 256, LDS, -1, None, None, None) == 0  # every output is optional
    assert lib.tl_lk_population_plan(64, None, 8, 256, LDS, -1, C.byref(f), None, None) == 0 and f.value in (0, 1)
    bad = _capi.TL_ERR_BADARG
    assert lib.tl_lk_population_plan(64, None, 8, 0, LDS, -1, C.byref(f), None, None) == bad
    assert lib.tl_lk_population_plan(64, None, 8, 256, -1, -1, C.byref(f), None, None) == bad
    assert lib.tl_lk_population_plan(64, None, 8, 256, LDS, 2, C.byref(f), None, None) == bad
    for opts in ((10, 10, 0, 5), (10, 10, 65, 5), (10, 10, 5, 0), (10, 10, 5, 17)):
        assert lib.tl_lk_population_plan(64, C.byref(_capi.TlLkOpts(*opts)), 8, 256, LDS, -1, C.byref(f), None, None) == bad


def test_python_plan_mirror(lib):
    import teeline_amd as TA
    h = TA.HeuristicOptions(epochs=10000, platoo_epochs=500, n_nearest=3)
    assert TA.lin_kernighan.population_plan(52, TA.LKOptions(h, 5), 8, force_form=1) == {"form": 1, "threads": 256, "per_cu": 2}
    assert TA.lin_kernighan.population_plan(20000, TA.LKOptions(h, 5), 8)["form"] == 0
    with pytest.raises(TA.TeelineGpuError):
        TA.lin_kernighan.population_plan(52, None, 8, cus=0)


def test_the_setting_is_a_setting_not_a_create_flag(lib):
    from teeline_amd import _capi
    text = open(HEADER).read()
    assert "TL_FLAG_LK_POP" not in text and not [k for k in dir(_capi) if k.startswith("TL_FLAG_LK_POP")]
    flags = {1 if m == "1u" else 1 << int(re.search(r"<<\s*(\d+)", m).group(1)) for m in re.findall(r"#define TL_FLAG_[A-Z0-9_]+ (1u|\(1u << \d+\))", text)}
    assert (1 << 31) not in flags
    assert re.search(r"int tl_lk_population_setting\(tl_ctx \*ctx, int force_form, uint32_t slice_scans\);", text)
    assert lib.tl_lk_population_setting(None, 1, 0) == _capi.TL_ERR_BADARG


def test_no_cpu_fallback_without_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import teeline_amd as TA
    xy = np.zeros((5, 2), np.float32)
    out = np.full(10, 77, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tl_lk_population(None, vp(xy), 5, None, None, 0, 0, 2, None, 1, vp(out), None, None, None, None) == TA._capi.TL_ERR_BADARG
    assert out.tolist() == [77] * 10
    prob = TA.TspProblem(np.arange(5) + 1, xy)
    with pytest.raises(TA.TeelineGpuError):
        TA.lin_kernighan.solve_population(prob, seed=1, runs=2)


class _NoContext:
    """Stands where a context would: any use of it is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was touched ({name})")


def test_solve_population_checks_its_arguments_before_any_context():
    import teeline_amd as TA
    prob = TA.TspProblem(np.arange(6) + 1, np.zeros((6, 2), np.float32))
    t = [1, 2, 3, 4, 5, 6]
    for kw, frag in ((dict(runs=0), "runs=0"), (dict(runs=3, init_tours=[t, t]), "2 start tours for 3 runs"),
                     (dict(runs=2, init_tours=[t, t[:5]]), "tour 1"), (dict(runs=1, init_tours=[]), "0 start tours")):
        init = kw.pop("init_tours", None)
        with pytest.raises(TA.TeelineGpuError) as e:
            TA.lin_kernighan.solve_population(prob, None, init, seed=1, ctx=_NoContext(), **kw)
        assert e.value.code == TA._capi.TL_ERR_BADARG and frag in str(e.value)
