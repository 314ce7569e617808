"""TL_MODE_BEST_SWEEP for batches: the per-workgroup form (two_opt_best_lds.hip) against the loop over the chip-wide descent
(a context with tl_two_opt_best_force_scan set: what a caller could do before the batch form existed).

  multistart   256 seeded restarts at n = 200, 1 002, 5 000, tl_two_opt_best_lds_max_n and 10 000 through tl_two_opt_multistart, on a
               default context and on a forced-scan context.  The loop's time is the sum of its descents', so from n = 5 000 on it
               is timed on the first 32 restarts and scaled by 256 / 32 ("scaled": true; sweeps and moves are scaled alike).
  population   256 tours at n = 1 002, each the 2-opt optimum of the NN tour with three random reversals planted, through
               tl_two_opt_best_population: the GA-refinement shape, a few moves per tour.

Kernel time (stats kernel_ms), the median of 3 runs after a warm-up.  us_per_sweep: of one descent — the batch's kernel time over
the mean sweeps per descent for the per-workgroup form (the descents run side by side), over all sweeps for the loop (one after
the other).  Appends one JSON line per measurement to profiles/best_sweep_batch_timing.jsonl as it goes.

  python scripts/timing_best_sweep_batch.py [n | top | population ...]      (no arguments: all of the above; top: the LDS limit)"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import teeline_amd as TA

OUT = os.path.join(ROOT, "profiles", "best_sweep_batch_timing.jsonl")
R, SEED, RUNS = 256, 1, 3
MODE = TA.TL_MODE_BEST_SWEEP


def plan(ctx, n, count, force_scan):
    info = ctx.device_info()
    form, threads = C.c_int(), C.c_int()
    assert ctx.lib.tl_two_opt_best_plan(n, count, info["cus"], info["lds_bytes"], force_scan, C.byref(form), C.byref(threads)) == 0
    return form.value, threads.value


def record(rec):
    with open(OUT, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def timed(call):
    call()  # warm-up: code object, workspace
    stats = [call() for _ in range(RUNS)]
    ms = [s["kernel_ms"] for s in stats]
    return statistics.median(ms), ms, stats[0]


def measure(entry, name, ctx, force_scan, n, count, call):
    form, threads = plan(ctx, n, count, force_scan)
    timed_count = count if form == 0 or n < 5000 else 32
    scale = count / timed_count
    ms, runs, st = timed(lambda: call(ctx, timed_count))
    sweeps, moves = st["sweeps"] * scale, st["moves"] * scale
    per_descent = ms * scale * 1e3 / (sweeps / count if form == 0 else sweeps)
    record({"entry": entry, "context": name, "n": n, "count": count, "timed_count": timed_count, "scaled": scale != 1, "form": form, "threads": threads,
            "kernel_ms": round(ms * scale, 3), "runs_ms": [round(v * scale, 3) for v in runs], "sweeps": sweeps, "moves": moves,
            "us_per_sweep": round(per_descent, 3)})
    return ms * scale


def main():
    with TA.Context(0) as dflt, TA.Context(0) as scan:
        scan.two_opt_best_force_scan()
        top = dflt.two_opt_best_lds_max_n()
        args = sys.argv[1:] or ["200", "1002", "5000", "top", "10000", "population"]
        sizes = [top if v == "top" else int(v) for v in args if v != "population"]
        ctxs = (("default", dflt, 0), ("forced_scan", scan, 1))
        for n in sizes:
            prob = TA.TspProblem(np.arange(n), TA.synth.synth_xy(n))
            ms = [measure("multistart", name, c, force, n, R, lambda cx, cnt: TA.two_opt.multistart(prob, cnt, SEED, 0, ctx=cx, mode=MODE).stats)
                  for name, c, force in ctxs]
            print(f"n = {n}: default {ms[0]:.2f} ms, forced scan {ms[1]:.2f} ms, ratio {ms[1] / ms[0]:.2f}", flush=True)
        if "population" not in args:
            return
        n = 1002
        prob = TA.TspProblem(np.arange(n), TA.synth.synth_xy(n))
        opt = TA.two_opt.solve(prob, None, None, TA.nearest_neighbor.solve(prob, ctx=dflt).route(), ctx=dflt).route()
        rng = np.random.default_rng(SEED)
        tours = []
        for _ in range(R):
            t = list(opt)
            for _ in range(3):
                a, b = sorted(int(v) for v in rng.choice(np.arange(1, n - 1), 2, replace=False))
                t[a:b + 1] = t[a:b + 1][::-1]
            tours.append(t)
        ms = [measure("population", name, c, force, n, R, lambda cx, cnt: pop_stats(prob, tours[:cnt], cx)) for name, c, force in ctxs]
        print(f"population n = {n}: default {ms[0]:.2f} ms, forced scan {ms[1]:.2f} ms, ratio {ms[1] / ms[0]:.2f}", flush=True)


def pop_stats(prob, tours, ctx):
    sols = TA.two_opt.solve_population(prob, tours, ctx=ctx, mode=MODE)
    return dict(sols[0].stats, moves=sum(s.stats["moves"] for s in sols))  # (a Solution's stats are the call's, with its own moves)


if __name__ == "__main__":
    main()
