"""Or-opt over a population (tl_or_opt_population) against the loop over tl_or_opt it replaces.

Per n (synth_xy(n), EUC_2D): `count` seeded random tours (the multi-start generator's restarts 0..count-1 of seed 1) through the
population entry — one workgroup per tour, the descent in LDS — and the same tours one after the other through tl_or_opt, the only
form there was before; the tours, costs and move counts must agree.  Wall and kernel times: the population as the median of
`--repeats` runs after one warm-up (code objects, workspace), the loop once after a warm-up descent (it is the slow side: minutes
at n = 3 000), on `--loop-tours` of the tours (default: all) and scaled to the whole population where fewer ran.  One JSON line
per n.
    python scripts/timing_or_opt_population.py [--count 256] [--repeats 3] [--loop-tours K] [n ...]      (default 200 1002 3000)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import teeline_amd as TA  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-tours", type=int, default=0)
    a = ap.parse_args()
    sizes = a.sizes or [200, 1002, 3000]
    with TA.Context(0) as ctx:
        info = ctx.device_info()
        for n in sizes:
            prob = TA.TspProblem(np.arange(n), TA.synth.synth_xy(n))
            tours = [TA.synth.restart_perm(n, 1, r).tolist() for r in range(a.count)]
            TA.or_opt.solve_population(prob, tours[:2], ctx=ctx)  # warm-up
            wall, kern, sols = [], [], None
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                sols = TA.or_opt.solve_population(prob, tours, ctx=ctx)
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(sols[0].stats["kernel_ms"])
            k = a.loop_tours or a.count
            TA.or_opt.solve(prob, None, None, tours[0], ctx=ctx)  # warm-up
            t0 = time.perf_counter()
            ones = [TA.or_opt.solve(prob, None, None, t, ctx=ctx) for t in tours[:k]]
            loop_wall = (time.perf_counter() - t0) * 1e3 * a.count / k
            loop_kern = sum(s.stats["kernel_ms"] for s in ones) * a.count / k
            same = all(o.route() == s.route() and np.float32(o.total).tobytes() == np.float32(s.total).tobytes() and
                       o.stats["moves"] == s.stats["moves"] for o, s in zip(ones, sols))
            row = {"n": n, "count": a.count, "cus": info["cus"], "moves": int(sum(s.stats["moves"] for s in sols)),
                   "passes": int(sols[0].stats["sweeps"]), "population_wall_ms": float(np.median(wall)), "population_kernel_ms": float(np.median(kern)),
                   "loop_tours_run": k, "loop_wall_ms": loop_wall, "loop_kernel_ms": loop_kern, "same_results": bool(same)}
            row["wall_ratio"] = row["loop_wall_ms"] / row["population_wall_ms"]
            row["kernel_ratio"] = row["loop_kernel_ms"] / row["population_kernel_ms"]
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
