"""Savings construction on the GPU (tl_savings) beside greedy-edge (tl_greedy_edge) and the NN seed, DESIGN.md §4.12.

Per n (synthetic EUC_2D, synth_xy(n)), in one run: each construction's kernel_ms / total_ms (median of 5 after one warm-up), its
bands and edges walked; the NN seed's time; and nn -> 2opt, greedy -> 2opt, savings -> 2opt (each 2-opt stage's time and the final
cost).  One JSON line per n.
    python scripts/timing_savings.py [n ...]      (default 1002 10000 13509)"""
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
    sizes = [int(a) for a in sys.argv[1:]] or [1002, 10000, 13509]
    with TA.Context(0) as ctx:
        for n in sizes:
            xy = TA.synth.synth_xy(n)
            prob = TA.TspProblem(np.arange(n), xy)
            row, seeds = {"n": n}, {}
            for name, mod in (("savings", TA.savings), ("greedy", TA.greedy_edge)):
                mod.solve(prob, ctx=ctx)  # warm-up: code objects, workspace
                runs = [mod.solve(prob, ctx=ctx) for _ in range(5)]
                seeds[name] = s = runs[-1]
                row.update({f"{name}_cost": float(s.total), f"{name}_kernel_ms": med([r.stats["kernel_ms"] for r in runs]),
                            f"{name}_total_ms": med([r.stats["total_ms"] for r in runs]), f"{name}_bands": int(s.stats["sweeps"]),
                            f"{name}_edges_walked": int(s.stats["candidates"])})
            row["hub"] = seeds["savings"].stats["hub"]
            TA.nearest_neighbor.solve(prob, ctx=ctx)
            t0 = time.perf_counter()
            seeds["nn"] = TA.nearest_neighbor.solve(prob, ctx=ctx)
            row["nn_ms"] = (time.perf_counter() - t0) * 1e3
            row["nn_cost"] = float(seeds["nn"].total)
            for name in ("nn", "greedy", "savings"):
                TA.two_opt.solve(prob, None, None, seeds[name].route(), ctx=ctx)
                t0 = time.perf_counter()
                s = TA.two_opt.solve(prob, None, None, seeds[name].route(), ctx=ctx)
                row[f"{name}_2opt_ms"] = (time.perf_counter() - t0) * 1e3
                row[f"{name}_2opt_kernel_ms"] = s.stats["kernel_ms"]
                row[f"{name}_2opt_cost"] = float(s.total)
                row[f"{name}_2opt_moves"] = int(s.stats["moves"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
