"""Developer probe: randomized parity campaign of tl_christofides (coordinate and matrix form, small n) against
tests/_christofides_oracle.py.
python tests/probes/fuzz_campaign_christofides.py [seconds]   (TEELINE_GPU_LIB selects the library, e.g. the race-stress build)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import _christofides_oracle as X  # noqa: E402
import _oracle as O  # noqa: E402
import teeline_amd as TA  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
t0 = time.time()
runs = fails = 0
with TA.Context(0) as ctx:
    seed = 0
    while time.time() - t0 < budget:
        seed += 1
        rng = np.random.default_rng(7000 + seed)
        n = int(rng.integers(4, 200)) if seed % 5 else int(rng.integers(200, 1300))
        kind = seed % 4
        if kind == 0:
            xy = rng.random((n, 2)) * 1000
        elif kind == 1:  # a coarse grid: equal keys in Prim and equal lengths in the matching, the position rules decide
            xy = rng.integers(0, int(rng.integers(2, 30)), (n, 2))
        elif kind == 2:
            c = rng.random((int(rng.integers(2, 9)), 2)) * 1000
            xy = c[rng.integers(0, len(c), n)] + rng.normal(0, 1.0, (n, 2))
        else:
            t = np.sort(rng.random(n)) * 1000
            xy = np.stack([t, 0.3 * t], 1)
        xy = np.ascontiguousarray(xy, dtype=np.float32)
        packed = O.dm_build_packed(xy) if seed % 3 == 0 else None
        if packed is not None and seed % 2:  # an integer matrix with signed zeros, negative and NaN entries (never a whole row)
            m = len(packed)
            packed = rng.integers(0, 40, m).astype(np.float32)
            idx = rng.permutation(m)
            packed[idx[:m // 16]] = np.float32(np.nan)
            packed[idx[m // 16:m // 8]] = np.float32(-0.0)
            packed[idx[m // 8:m // 6]] = np.float32(-2.0)
        out = np.zeros(n, dtype=np.uint32)
        cost = C.c_float()
        rc = ctx.lib.tl_christofides(ctx.handle, xy.ctypes.data_as(C.c_void_p), None if packed is None else packed.ctypes.data_as(C.c_void_p),
                                     n, out.ctypes.data_as(C.c_void_p), C.byref(cost), None)
        try:
            route, ocost = X.christofides(xy, packed, n)
            bad = rc != 0 or out.tolist() != route.tolist() or np.float32(cost.value).tobytes() != np.float32(ocost).tobytes()
        except X.NotSpanning:
            route, ocost = None, float("nan")
            bad = rc != TA._capi.TL_ERR_UNSUPPORTED
        runs += 1
        if bad:
            fails += 1
            print(f"CHRISTOFIDES MISMATCH seed={seed} n={n} kind={kind} matrix={packed is not None}: rc={rc} "
                  f"gpu {cost.value!r} oracle {float(ocost)!r}", flush=True)
print(f"{runs} runs, {fails} mismatches, {time.time() - t0:.0f} s", flush=True)
