"""Lin-Kernighan for seeded runs: form 1 of tl_lk_population (one workgroup per run, k_lk_ils_pop) against form 0 (the loop over tl_lk,
whose single search fills the chip with speculative epochs: what a caller could do before the batch form existed).

  instances    berlin52, a280, att532 (tests/golden/tsplib) with the CLI's options (10 000 epochs, plateau 500, k = 3, depth 5) and a
               synthetic n = 1 002 with the library defaults (100 epochs, plateau 10, k = 5, depth 5); seed 1
  counts       1, 2, 4, 8, 16, 64, 256, 512 runs, each on a context with form 1 forced and on one with form 0 forced

Kernel time (stats kernel_ms), the median of 3 calls after a warm-up.  The loop's time is the sum of its runs', so beyond LOOP_RUNS
runs it is timed on the first LOOP_RUNS and scaled by count / LOOP_RUNS ("scaled": true).  A call whose warm-up takes longer than
SLOW_S seconds is not repeated: its one time stands ("calls": 1), and larger counts of that instance and form are left out.  A run
whose lk_pass cycles (TL_ERR_NO_CONVERGE) ends the row: "error" holds the message.
Appends one JSON line per measurement to profiles/lk_population_timing.jsonl as it goes.

  python scripts/timing_lk_population.py [berlin52 | a280 | att532 | 1002 ...]      (no arguments: all four)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import teeline_amd as TA

OUT = os.path.join(ROOT, "profiles", "lk_population_timing.jsonl")
COUNTS, SEED, CALLS, LOOP_RUNS, SLOW_S = (1, 2, 4, 8, 16, 64, 256, 512), 1, 3, 8, 6.0


def record(rec):
    with open(OUT, "a") as fh:
        fh.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def instance(name):
    if name.isdigit():
        n = int(name)
        return TA.TspProblem(np.arange(n), TA.synth.synth_xy(n)), TA.LKOptions()
    prob = TA.tsplib.read_from_file(os.path.join(ROOT, "tests", "golden", "tsplib", f"{name}.tsp")).problem()
    return prob, TA.LKOptions(TA.HeuristicOptions(epochs=10000, platoo_epochs=500, n_nearest=3), 5)


def measure(name, prob, opts, ctx, form, count):
    """the row of one (instance, form, count), or None where the warm-up was slow (the row is written, larger counts are left out)"""
    timed = count if form == 1 else min(count, LOOP_RUNS)
    scale = count / timed

    def call():
        sols, best = TA.lin_kernighan.solve_population(prob, opts, seed=SEED, runs=timed, ctx=ctx)
        return sols[0].stats["kernel_ms"], float(sols[best].total)

    info = ctx.device_info()
    plan = TA.lin_kernighan.population_plan(len(prob), opts, count, cus=info["cus"], lds_bytes=info["lds_bytes"], force_form=form)
    rec = {"instance": name, "n": len(prob), "count": count, "form": plan["form"], "threads": plan["threads"], "per_cu": plan["per_cu"],
           "timed_count": timed, "scaled": scale != 1}
    try:
        t0 = time.time()
        first, best = call()  # warm-up: code object, workspace
        slow = time.time() - t0 > SLOW_S
        ms = [first] if slow else [call()[0] for _ in range(CALLS)]
    except TA.TeelineGpuError as exc:
        record(dict(rec, error=str(exc)))
        return None
    rec.update(kernel_ms=round(statistics.median(ms) * scale, 3), calls_ms=[round(v * scale, 3) for v in ms], calls=len(ms), best_of_timed=best)
    record(rec)
    return None if slow else rec


def main():
    with TA.Context(0) as one_each, TA.Context(0) as loop:
        one_each.lk_population_setting(1, 0)
        loop.lk_population_setting(0, 0)
        for name in sys.argv[1:] or ["berlin52", "a280", "att532", "1002"]:
            prob, opts = instance(name)
            rows = {1: {}, 0: {}}
            for form, ctx in ((1, one_each), (0, loop)):
                for count in COUNTS:
                    rec = measure(name, prob, opts, ctx, form, count)
                    if rec is None:
                        break
                    rows[form][count] = rec["kernel_ms"]
            both = [c for c in COUNTS if c in rows[0] and c in rows[1]]
            faster = [c for c in both if rows[1][c] < rows[0][c]]
            print(f"{name}: " + ", ".join(f"{c}: {rows[1][c]:.1f} / {rows[0][c]:.1f} ms" for c in both) +
                  f"; form 1 faster from count {min(faster) if faster else 'none'}", flush=True)


if __name__ == "__main__":
    main()
