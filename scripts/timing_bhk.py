"""The Bellman-Held-Karp exact solver on the GPU (tl_bellman_karp), DESIGN.md §4.14.

Per n (the first n points of synth_xy(26), EUC_2D), in one run: kernel_ms (init + layers + optimum + walk), the DP layers' share of
it and total_ms of the call — medians of 5 after one warm-up, which also grows the workspace to the table's size — with the
optimum, the route's length and the number of terms; both walks.  With --oracle also the wall time of the numpy restatement
(tests/_bhk_oracle.py, one core) on the same box for n <= 20.  One JSON line per n.
    python scripts/timing_bhk.py [--oracle] [n ...]      (default 14 17 20 22 24 26)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import teeline_amd as TA  # noqa: E402


def med(v):
    return float(np.median(v))


def main():
    args = [a for a in sys.argv[1:] if a != "--oracle"]
    sizes = [int(a) for a in args] or [14, 17, 20, 22, 24, 26]
    oracle = None
    if "--oracle" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _bhk_oracle as oracle
    pts = TA.synth.synth_xy(26)
    with TA.Context(0) as ctx, TA.Context(0, TA.TL_FLAG_BHK_EXACT_WALK) as xctx:
        for n in sizes:
            prob = TA.TspProblem(np.arange(n), pts[:n])
            row = {"n": n, "table_mb": (1 << (n - 1)) * 128 / 1e6}
            for name, c in (("ref", ctx), ("exact", xctx)):
                TA.bellman_karp.solve(prob, ctx=c)  # warm-up: code objects, the table's allocation
                runs = [TA.bellman_karp.solve(prob, ctx=c) for _ in range(5)]
                s = runs[-1]
                row.update({f"{name}_kernel_ms": med([r.stats["kernel_ms"] for r in runs]), f"{name}_layers_ms": med([r.stats["layers_ms"] for r in runs]),
                            f"{name}_total_ms": med([r.stats["total_ms"] for r in runs]), f"{name}_cost": float(s.total),
                            f"{name}_is_tour": int(s.stats["is_tour"])})
            row.update({"optimal": float(s.stats["optimal"]), "layers": int(s.stats["sweeps"]), "terms": int(s.stats["candidates"])})
            row["terms_per_s"] = row["terms"] / (row["ref_layers_ms"] * 1e-3) if row["ref_layers_ms"] > 0 else None
            if oracle is not None and n <= 20:
                t0 = time.perf_counter()
                o = oracle.bellman_karp(pts[:n])
                row["numpy_oracle_s"] = time.perf_counter() - t0
                row["oracle_agrees"] = bool(float(o[2]) == row["optimal"] and float(o[1]) == row["ref_cost"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
