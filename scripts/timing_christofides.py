"""Christofides construction on the GPU (tl_christofides) beside the NN and greedy-edge seeds, DESIGN.md §4.13.

Per n (synthetic EUC_2D, synth_xy(n)), in one run: the call split into Prim's tree, the rest of the device stages (odd vertices
and the matching's bands) and the remainder of the call (copies, the host's Euler walk and shortcut, the cost) — medians of 5
after one warm-up — with the bands and pairs walked; the NN and greedy-edge seeds' times; and chr -> 2opt, nn -> 2opt,
greedy -> 2opt (each 2-opt stage's time and the final cost).  One JSON line per n.
    python scripts/timing_christofides.py [n ...]      (default 1002 10000 13509)"""
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
            TA.christofides.solve(prob, ctx=ctx)  # warm-up: code objects, workspace
            runs = [TA.christofides.solve(prob, ctx=ctx) for _ in range(5)]
            seeds["chr"] = s = runs[-1]
            prim = [r.stats["prim_ms"] for r in runs]
            kern = [r.stats["kernel_ms"] for r in runs]
            total = [r.stats["total_ms"] for r in runs]
            row.update({"chr_cost": float(s.total), "chr_prim_ms": med(prim), "chr_matching_ms": med(np.subtract(kern, prim)),
                        "chr_host_ms": med(np.subtract(total, kern)), "chr_kernel_ms": med(kern), "chr_total_ms": med(total),
                        "chr_bands": int(s.stats["sweeps"]), "chr_pairs_walked": int(s.stats["candidates"])})
            for name, mod in (("nn", TA.nearest_neighbor), ("greedy", TA.greedy_edge)):
                mod.solve(prob, ctx=ctx)
                t = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    seeds[name] = mod.solve(prob, ctx=ctx)
                    t.append((time.perf_counter() - t0) * 1e3)
                row[f"{name}_ms"] = med(t)
                row[f"{name}_cost"] = float(seeds[name].total)
            for name in ("chr", "nn", "greedy"):
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
