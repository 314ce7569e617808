"""TL_MODE_BEST_SWEEP past one tile group, through its row cache and at the limits of its packed key (-m gpu): tl_two_opt against
tlo_two_opt_best, bit for bit, on the case table of tests/_best_sweep_cases.py (tests/test_best_sweep_cases.py shows which seam of
two_opt_best.hip each case reaches and which planted defect it would expose), the n = 65 535 golden, the refusal at 65 536, and the
forced-HBM REF_ORDER form (two_opt_large.hip) on the same perturbed starts against the first-improvement oracle."""
import json
import os

import numpy as np
import pytest

import _best_sweep_cases as B
import _oracle as O
from test_gpu_two_opt import assert_same, gpu_two_opt

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in B.case_table()}


@pytest.mark.parametrize("cid", list(CASES))
def test_case_matches_the_oracle_bit_for_bit(ctx, cid):
    xy, tour = CASES[cid].build()
    n = len(tour)
    want = O.two_opt(xy, None, n, init=tour, best=True)
    assert want[3]["moves"] >= 2
    assert_same(gpu_two_opt(ctx, xy, None, n, tour, mode=1), want, n)


def test_snake_65535_golden(ctx, golden_dir):
    import sys
    sys.path.insert(0, golden_dir)
    import make_goldens_best_sweep as MG
    with open(os.path.join(golden_dir, "goldens_best_sweep.json")) as fh:
        g = json.load(fh)["snake65535_best_sweep"]
    xy, init = B.GOLDEN_CASE.build()
    n = len(init)
    assert n == g["n"] == 65535 and MG.crc(init) == g["init_crc32"]
    route, cost, st = gpu_two_opt(ctx, xy, None, n, init, mode=1)
    assert MG.crc(route) == g["route_crc32"]
    assert int(np.float32(cost).view(np.uint32)) == g["cost_bits"]
    assert {k: st[k] for k in ("sweeps", "candidates", "moves", "reversed")} == g["stats"]


def test_65536_cities_are_refused(ctx):
    import teeline_amd as TA
    n = 65536
    with pytest.raises(TA.TeelineGpuError) as e:
        gpu_two_opt(ctx, O.synth_xy(n, seed=1), None, n, None, mode=1)
    assert e.value.code == TA._capi.TL_ERR_UNSUPPORTED


HBM_CASES = [cid for cid, c in CASES.items() if c.n in (4098, 4224, 8300) or (c.family == "uniform" and c.n == 4200 and c.seed == 1)]


@pytest.fixture(scope="module")
def hbm_ctx():
    import teeline_amd as TA
    with TA.Context(0, TA.TL_FLAG_2OPT_FORCE_HBM) as c:
        yield c


@pytest.mark.parametrize("cid", HBM_CASES)
def test_forced_hbm_ref_order_matches_the_oracle(hbm_ctx, cid):
    xy, tour = CASES[cid].build()
    n = len(tour)
    want = O.two_opt(xy, None, n, init=tour)
    assert want[3]["moves"] >= 2
    assert_same(gpu_two_opt(hbm_ctx, xy, None, n, tour), want, n)
