"""The branch and bound on the GPU (tl_branch_and_bound), DESIGN.md §4.27.  No threshold: it records.

Per n (uniform integer coordinates in [0, 1000)^2, rng seed 1000 n + SEED[n]; the start tour is the pipeline's nn + 2opt), one JSON
line: the device entry's nodes, leaves, launches, wall and kernel time, nodes per second, the mean and the longest launch at the
plan's slice, and the share of wave-launches that ended with an empty queue (the imbalance); the same instance through
tl_branch_and_bound_host on one core (its figures are kept only where it finishes inside --limit-ms) and, at n <= 26, through
tl_bellman_karp.  A search the time limit ends is recorded with proved = 0: its node rate stands, its wall time is the limit.
A last line runs n = 64 for --limit-ms to give the launch duration at the default slice there.
    python scripts/timing_branch_and_bound.py [--limit-ms MS] [--out FILE] [n ...]      (default 20 26 33 40 48)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import teeline_amd as TA  # noqa: E402

SEED = {20: 1, 26: 2, 33: 27, 40: 0, 48: 0, 64: 0}


def instance(n):
    return np.random.default_rng(1000 * n + SEED.get(n, 0)).integers(0, 1000, size=(n, 2)).astype(np.float32)


def take(argv, flag, default):
    if flag in argv:
        k = argv.index(flag)
        v = argv[k + 1]
        del argv[k:k + 2]
        return v
    return default


def main():
    argv = sys.argv[1:]
    limit = int(take(argv, "--limit-ms", "10000"))
    out = take(argv, "--out", os.path.join(ROOT, "profiles", "branch_and_bound_timing.jsonl"))
    sizes = [int(a) for a in argv] or [20, 26, 33, 40, 48]
    B = TA.branch_and_bound
    rows = []
    with TA.Context(0) as ctx:
        info = ctx.device_info()
        for n in sizes + [64]:
            prob = TA.TspProblem(np.arange(n), instance(n))
            seed = TA.pipeline.run_pipeline_stages(prob, ["nn", "2opt"], ctx=ctx)[-1].solution
            B.solve(prob, None, None, seed.route(), ctx=ctx, max_nodes=1)  # warm-up: the code object, the workspace
            t0 = time.perf_counter()
            s = B.solve(prob, None, None, seed.route(), ctx=ctx, time_limit_ms=limit)
            wall = time.perf_counter() - t0
            st = s.stats
            row = {"n": n, "arch": info["arch"], "cus": info["cus"], "seed_cost": float(seed.total), "cost": float(s.total), "proved": st["proved"],
                   "nodes": st["nodes"], "leaves": st["leaves"], "launches": st["launches"], "wall_s": wall, "kernel_ms": st["kernel_ms"],
                   "nodes_per_s": st["nodes"] / wall, "nodes_per_kernel_s": st["nodes"] / (st["kernel_ms"] * 1e-3) if st["kernel_ms"] else None,
                   "mean_launch_ms": st["kernel_ms"] / st["launches"] if st["launches"] else None, "max_launch_ms": st["max_launch_ms"],
                   "queue_start": st["queue_start"], "queue_end": st["queue_end"],
                   "idle_share": st["idle_wave_launches"] / st["wave_launches"] if st["wave_launches"] else None}
            if n < 64:
                t0 = time.perf_counter()
                h = B.solve_host(prob, None, None, seed.route(), time_limit_ms=limit)
                hw = time.perf_counter() - t0
                row.update({"host_proved": h.stats["proved"], "host_nodes": h.stats["nodes"], "host_nodes_per_s": h.stats["nodes"] / hw})
                if h.stats["proved"]:  # the host run counts only where it finishes
                    row.update({"host_wall_s": hw, "host_agrees": bool(h.route() == s.route() and h.total.tobytes() == s.total.tobytes()) if st["proved"] else None,
                                "speedup": hw / wall if st["proved"] else None})
            if n <= 26:
                TA.bellman_karp.solve(prob, ctx=ctx, exact_walk=True)
                t0 = time.perf_counter()
                b = TA.bellman_karp.solve(prob, ctx=ctx, exact_walk=True)
                row.update({"bhk_wall_s": time.perf_counter() - t0, "bhk_kernel_ms": b.stats["kernel_ms"], "bhk_cost": float(b.total)})
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
