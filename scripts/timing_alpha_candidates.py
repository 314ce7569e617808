"""Alpha-nearness candidate lists.  Two reports, no threshold: what comes out is written down.

(a) tl_alpha_candidates, k = 5, zero penalties, on berlin52 (52), a280 (280), synthetic n = 1 002 and 5 000 and a collinear n = 1 002
    (the tree's depth, n - 2 levels, is the kernel's worst case): the rows' kernel time and the whole call's (1-tree launch, host
    preparation, rows) as medians of `--reps` calls after one warm-up, from the context's HIP events, against
    tests/probes/alpha_cpu_baseline.cpp on one core of the same box.  Inside, the device rows are asserted equal to the probe's (hash).
(b) mean and best cost of 32 seeded LK runs (tl_lk_population, library defaults: 100 epochs, plateau 10, depth 5) on berlin52, a280,
    att532 and synthetic n = 1 002 with the kd-tree's k = 5, alpha k = 5 from zero penalties, and alpha k = 5 from the ascent's best
    pi (1 000 iterations, upper from nearest_neighbor -> two_opt).

    python scripts/timing_alpha_candidates.py [--reps 5] [--json] [--skip-lk]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import teeline_amd as TA  # noqa: E402


def fnv(rows):
    h = 0xCBF29CE484222325
    for b in np.ascontiguousarray(rows, dtype="<u4").tobytes():
        h = ((h ^ b) * 0x100000001B3) & (2 ** 64 - 1)
    return f"{h:016x}"


def instance(name):
    import _oracle as O
    import _one_tree_cases as K
    if name.startswith("synth"):
        return O.synth_xy(int(name[5:]), seed=9)
    if name.startswith("line"):
        return np.array([[3.0 * i, 7.0] for i in range(int(name[4:]))], dtype=np.float32)
    return np.ascontiguousarray(TA.tsplib.read_from_file(os.path.join(K.HERE, "golden", "tsplib", name + ".tsp")).xy, dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--skip-lk", action="store_true")
    a = ap.parse_args()
    ctx = TA.default_context()
    emit = lambda rec: print(json.dumps(rec) if a.json else rec, flush=True)  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "alpha_cpu_baseline")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                               os.path.join(ROOT, "tests", "probes", "alpha_cpu_baseline.cpp"), "-o", exe])
        for name in ("berlin52", "a280", "synth1002", "line1002", "synth5000"):
            xy = instance(name)
            n = len(xy)
            prob = TA.TspProblem(np.arange(n), xy)
            path = os.path.join(tmp, name + ".txt")
            with open(path, "w") as fh:
                fh.write(f"{n}\n" + "\n".join(f"{float(p)!r} {float(q)!r}" for p, q in xy) + "\n")
            runs = [subprocess.run([exe, path, "0", "5"], capture_output=True, text=True, check=True).stdout.split() for _ in range(3)]
            cpu_ms = statistics.median(float(r[2]) for r in runs)
            for threads in (0, 64, 1024):
                rows_ms, call_ms, wall_ms = [], [], []
                for r in range(a.reps + 1):
                    got = TA.alpha_candidates.candidates(prob, 5, ctx=ctx, threads=threads)
                    if r:
                        rows_ms.append(ctx.last_kernel_ms())
                        call_ms.append(got.stats["kernel_ms"])
                        wall_ms.append(got.stats["total_ms"])
                assert fnv(got.rows) == runs[0][0], (name, "the device rows differ from the probe's")
                emit(dict(what="alpha_candidates", instance=name, n=n, k=5, threads=threads or TA.alpha_candidates.plan(n)["threads"], plan=threads == 0,
                          levels=got.stats["sweeps"], rows_kernel_ms=round(statistics.median(rows_ms), 3), tree_plus_rows_kernel_ms=round(statistics.median(call_ms), 3),
                          wall_ms=round(statistics.median(wall_ms), 3), cpu_one_core_ms=round(cpu_ms, 3),
                          ratio_vs_one_core=round(cpu_ms / statistics.median(call_ms), 2), rows_equal_probe=True))
    if a.skip_lk:
        return
    for name in ("berlin52", "a280", "att532", "synth1002"):
        xy = instance(name)
        n = len(xy)
        prob = TA.TspProblem(np.arange(n), xy)
        zero = TA.alpha_candidates.candidates(prob, 5, ctx=ctx)
        asc, b = TA.alpha_candidates.from_ascent(prob, 5, ctx=ctx)
        for kind, rows in (("kdtree_k5", None), ("alpha_k5_zero_pi", zero.rows), ("alpha_k5_ascent_pi", asc.rows)):
            try:
                sols, best = TA.lin_kernighan.solve_population(prob, None, None, seed=1, runs=32, ctx=ctx, candidates=rows)
            except TA.TeelineGpuError as exc:  # (a run whose lk_pass cycles, as the reference's would: reported, not hidden)
                emit(dict(what="lk_32_runs", instance=name, n=n, lists=kind, error=str(exc)))
                continue
            costs = [float(s.total) for s in sols]
            emit(dict(what="lk_32_runs", instance=name, n=n, lists=kind, mean_cost=round(statistics.mean(costs), 3), best_cost=round(min(costs), 3),
                      worst_cost=round(max(costs), 3), kernel_ms=round(sols[0].stats["kernel_ms"], 3), bound=round(b.bound, 3)))


if __name__ == "__main__":
    main()
