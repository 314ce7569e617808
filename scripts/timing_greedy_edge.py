"""Greedy-edge construction on the GPU (tl_greedy_edge) against the NN seed, DESIGN.md §4.11.

Per n (synthetic EUC_2D, synth_xy(n)): the greedy stage's kernel_ms / total_ms (median of 5 after one warm-up), its bands and
edges walked; for n <= 13 509 also nn -> 2opt and greedy -> 2opt (each stage's time and the final cost) and the CPU oracle's
time for the same greedy tour (tests/_greedy_oracle.py, numpy with the chunked walk: the sorted list of all n(n-1)/2 edges —
the oracle, not the reference).  One JSON line per n.
    python scripts/timing_greedy_edge.py [n ...]      (default 1002 10000 13509 65535)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import teeline_amd as TA  # noqa: E402


def med(v):
    return float(np.median(v))


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1002, 10000, 13509, 65535]
    with TA.Context(0) as ctx:
        for n in sizes:
            xy = TA.synth.synth_xy(n)
            prob = TA.TspProblem(np.arange(n), xy)
            TA.greedy_edge.solve(prob, ctx=ctx)  # warm-up: code objects, workspace
            runs = [TA.greedy_edge.solve(prob, ctx=ctx) for _ in range(5)]
            g = runs[-1]
            row = {"n": n, "greedy_cost": float(g.total), "greedy_kernel_ms": med([r.stats["kernel_ms"] for r in runs]),
                   "greedy_total_ms": med([r.stats["total_ms"] for r in runs]), "bands": int(g.stats["sweeps"]),
                   "edges_walked": int(g.stats["candidates"])}
            if n <= 13509:
                TA.nearest_neighbor.solve(prob, ctx=ctx)
                t0 = time.perf_counter()
                nn = TA.nearest_neighbor.solve(prob, ctx=ctx)
                row["nn_ms"] = (time.perf_counter() - t0) * 1e3
                row["nn_cost"] = float(nn.total)
                for name, seed in (("nn", nn), ("greedy", g)):
                    TA.two_opt.solve(prob, None, None, seed.route(), ctx=ctx)
                    t0 = time.perf_counter()
                    s = TA.two_opt.solve(prob, None, None, seed.route(), ctx=ctx)
                    row[f"{name}_2opt_ms"] = (time.perf_counter() - t0) * 1e3
                    row[f"{name}_2opt_kernel_ms"] = s.stats["kernel_ms"]
                    row[f"{name}_2opt_cost"] = float(s.total)
                    row[f"{name}_2opt_moves"] = int(s.stats["moves"])
                import _greedy_oracle as G
                t0 = time.perf_counter()
                route, cost = G.greedy_edge(xy, chunk=1 << 16)
                row["oracle_cpu_ms"] = (time.perf_counter() - t0) * 1e3
                row["oracle_agrees"] = bool(route.tolist() == [int(v) for v in g.route()] and np.float32(cost) == g.total)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
