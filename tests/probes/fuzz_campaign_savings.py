"""Developer probe: randomized parity campaign of tl_savings (coordinate and matrix form, automatic and explicit hub) against
tests/_savings_oracle.py.
python tests/probes/fuzz_campaign_savings.py [seconds]   (TEELINE_GPU_LIB selects the library, e.g. the race-stress build)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import _oracle as O  # noqa: E402
import _savings_oracle as S  # noqa: E402
import teeline_amd as TA  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
t0 = time.time()
runs = fails = 0
with TA.Context(0) as ctx:
    seed = 0
    while time.time() - t0 < budget:
        seed += 1
        rng = np.random.default_rng(9000 + seed)
        n = int(rng.integers(3, 300)) if seed % 5 else int(rng.integers(300, 1000))
        kind = seed % 4
        if kind == 0:
            xy = rng.random((n, 2)) * 1000
        elif kind == 1:  # a coarse grid: many equal savings, the tie rule decides
            xy = rng.integers(0, int(rng.integers(2, 30)), (n, 2))
        elif kind == 2:
            c = rng.random((int(rng.integers(2, 9)), 2)) * 1000
            xy = c[rng.integers(0, len(c), n)] + rng.normal(0, 1.0, (n, 2))
        else:
            t = np.sort(rng.random(n)) * 1000
            xy = np.stack([t, 0.3 * t], 1)
        xy = np.ascontiguousarray(xy, dtype=np.float32)
        packed = O.dm_build_packed(xy) if seed % 3 == 0 else None
        if packed is not None and seed % 2:  # an integer matrix with inf entries: negative, -inf and NaN savings
            m = len(packed)
            packed = rng.integers(0, 40, m).astype(np.float32)
            packed[rng.permutation(m)[:m // 8]] = np.float32(np.inf)
        hub = int(rng.integers(0, n)) if seed % 7 == 0 else None
        out = np.zeros(n, dtype=np.uint32)
        cost, ghub = C.c_float(), C.c_uint32()
        rc = ctx.lib.tl_savings(ctx.handle, xy.ctypes.data_as(C.c_void_p), None if packed is None else packed.ctypes.data_as(C.c_void_p),
                                n, TA._capi.TL_SAVINGS_HUB_AUTO if hub is None else hub, out.ctypes.data_as(C.c_void_p), C.byref(cost),
                                C.byref(ghub), None)
        route, ocost, ohub = S.savings(xy, packed, n, hub=hub, chunk=4096)
        runs += 1
        if rc != 0 or ghub.value != ohub or out.tolist() != route.tolist() or np.float32(cost.value).tobytes() != np.float32(ocost).tobytes():
            fails += 1
            print(f"SAVINGS MISMATCH seed={seed} n={n} kind={kind} matrix={packed is not None} hub={hub}: rc={rc} hub {ghub.value} / {ohub} "
                  f"gpu {cost.value!r} oracle {float(ocost)!r}", flush=True)
print(f"{runs} runs, {fails} mismatches, {time.time() - t0:.0f} s", flush=True)
