"""3-opt over a population (tl_three_opt_population) against the loop over tl_three_opt it replaces, and the three
constants of the cost model behind tl_three_opt_population_plan.

Sets (synth_xy(n), EUC_2D): `--count` seeded random tours (the multi-start generator's restarts of seed 1) at n = 52, 100, 200, 500,
and at n = 1 002 the same number of near-optimal starts (one tour refined by 2-opt and Or-opt, then `--kicks` random segment
reversals each: a few 3-opt moves per tour, so that a run is minutes and not hours); small counts 1, 8, 64 at n = 100 and 500.
Every set runs through a context that forces the per-workgroup form, through the loop over tl_three_opt (the chip-wide descent, the
only form there was before), and through an unflagged context (what the plan picks).  All three must give the same tours, costs and
move counts.  Wall and kernel ms are medians of `--repeats` runs after a warm-up; `spread` is (max - min) / median of the walls.
Derived per point: R_cu = triples x passes / (rounds x kernel s of the workgroup form) with rounds = ceil(count / CUs), and the
loop's seconds per pass; the last line fits R_chip and T_pass to the loop's seconds per pass over the sizes (least squares on
t = triples / R_chip + T_pass) and gives the largest spread seen, the margin (the larger of 10 % and three times that spread) and
every point at which the unflagged entry lost to the faster form by more than the margin.  auto_loss = auto wall / the faster of the
two forced forms' walls.  One JSON line per point.  Every point is a child process of its own under `timeout -k 10` (--limit
seconds, default 120 below n = 500, 420 from there: the longest point, 256 random tours at n = 500, took about a minute); the script
stops at the first point that fails, disagrees or runs out of time.
    python scripts/timing_three_opt_population.py [--count 256] [--repeats 3] [--loop-tours K] [--sets random,near,small] [--limit S]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import teeline_amd as TA  # noqa: E402


def triples(n):
    return n * (n - 1) * (n - 2) // 6 - (n - 2)


def near_optimal_tours(prob, n, count, kicks, ctx):
    base = TA.pipeline.run_pipeline_stages(prob, ["2opt", "or_opt"], ctx=ctx, init_tour=list(range(n)))[-1].solution.route()
    rng = np.random.default_rng(n)
    tours = []
    for _ in range(count):
        t = list(base)
        for _ in range(kicks):
            i = int(rng.integers(0, n - 12))
            L = int(rng.integers(2, 10))
            t[i:i + L] = t[i:i + L][::-1]
        tours.append(t)
    return tours


def timed(fn, repeats):
    fn()  # warm-up: code objects, workspace
    wall, kern, res = [], [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        res, kms = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(kms)
    return res, float(np.median(wall)), float(np.median(kern)), float((max(wall) - min(wall)) / np.median(wall))


def point(a, kind, n, count):
    """One (set, n, count) point, in this process: prints its JSON line, returns 0 when the three ways agree."""
    with TA.Context(0) as ctx, TA.Context(0, TA.TL_FLAG_3OPT_POP_FORCE_WG) as wg:
        info = ctx.device_info()
        cus = info["cus"]
        prob = TA.TspProblem(np.arange(n), TA.synth.synth_xy(n))
        if kind == "random":
            tours = [TA.synth.restart_perm(n, 1, r).tolist() for r in range(count)]
        else:
            tours = near_optimal_tours(prob, n, count, a.kicks, ctx)

        def pop(c):
            def run():
                sols = TA.three_opt.solve_population(prob, tours, ctx=c)
                return sols, sols[0].stats["kernel_ms"]
            return run

        k = min(a.loop_tours or count, count)

        def loop():
            ones = [TA.three_opt.solve(prob, None, None, t, ctx=ctx) for t in tours[:k]]
            return ones, sum(s.stats["kernel_ms"] for s in ones)

        sols, wg_wall, wg_kern, wg_spread = timed(pop(wg), a.repeats)
        ones, lp_wall, lp_kern, lp_spread = timed(loop, a.repeats)
        auto, au_wall, au_kern, au_spread = timed(pop(ctx), a.repeats)
        scale = count / k
        lp_wall, lp_kern = lp_wall * scale, lp_kern * scale

        def same(x, y):
            return all(o.route() == s.route() and np.float32(o.total).tobytes() == np.float32(s.total).tobytes() and
                       o.stats["moves"] == s.stats["moves"] for o, s in zip(x, y))

        ok = same(ones, sols) and same(sols, auto)
        passes = int(sols[0].stats["sweeps"])
        loop_passes = int(sum(s.stats["sweeps"] for s in ones))
        form, thr, batch = C.c_int(), C.c_int(), C.c_uint32()
        ctx.lib.tl_three_opt_population_plan(n, count, cus, info["lds_bytes"], 8 << 30, 0, C.byref(form), C.byref(thr), C.byref(batch))
        rounds = -(-count // cus)
        # R_cu_mean: the mean tour's triples over the kernel time of one round (the longest tour of a round bounds the kernel)
        row = {"set": kind, "n": n, "count": count, "cus": cus, "moves": int(sum(s.stats["moves"] for s in sols)), "passes": passes,
               "wg_wall_ms": wg_wall, "wg_kernel_ms": wg_kern, "wg_spread": wg_spread,
               "loop_tours_run": k, "loop_wall_ms": lp_wall, "loop_kernel_ms": lp_kern, "loop_spread": lp_spread,
               "auto_form": form.value, "auto_threads": thr.value, "auto_wall_ms": au_wall, "auto_kernel_ms": au_kern, "auto_spread": au_spread,
               "auto_loss": au_wall / min(wg_wall, lp_wall), "faster_form": 1 if wg_wall <= lp_wall else 0,
               "same_results": bool(ok), "wall_ratio_loop_over_wg": lp_wall / wg_wall,
               "R_cu_mean": triples(n) * passes / count / (wg_kern * 1e-3 / rounds) if wg_kern > 0 else None,
               "loop_s_per_pass": lp_wall * 1e-3 / scale / loop_passes}
        print(json.dumps(row), flush=True)
        return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-tours", type=int, default=0, help="run the loop on this many of the tours and scale (0: all)")
    ap.add_argument("--kicks", type=int, default=3)
    ap.add_argument("--sets", default="random,near,small")
    ap.add_argument("--limit", type=int, default=0, help="seconds a point may take (0: 120 below n = 500, 420 from there)")
    ap.add_argument("--point", default="", help="set,n,count: run this one point in this process (what the script starts for every point)")
    a = ap.parse_args()
    if a.point:
        kind, n, count = a.point.split(",")
        return point(a, kind, int(n), int(count))
    sets = a.sets.split(",")
    points = []
    if "random" in sets:
        points += [("random", n, a.count) for n in (52, 100, 200, 500)]
    if "small" in sets:
        points += [("random", n, c) for n in (100, 500) for c in (1, 8, 64)]
    if "near" in sets:
        points += [("near", 1002, a.count)]
    rows = []
    for kind, n, count in points:
        limit = a.limit or (120 if n < 500 else 420)
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--point", f"{kind},{n},{count}",
               "--repeats", str(a.repeats), "--loop-tours", str(a.loop_tours), "--kicks", str(a.kicks)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:  # a mismatch, a failure, or the time limit (124 / 137): nothing more is started on the GPU
            print(json.dumps({"error": "point failed", "set": kind, "n": n, "count": count, "returncode": r.returncode, "limit_s": limit}), flush=True)
            return 1
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    fit = [(triples(r["n"]), r["loop_s_per_pass"]) for r in rows if r["count"] == a.count]
    out = {}
    if len(fit) >= 2:
        slope, icpt = np.polyfit(np.array([f[0] for f in fit], float), np.array([f[1] for f in fit], float), 1)
        out.update({"fit": "loop_s_per_pass = triples / R_chip + T_pass", "R_chip": (1.0 / slope) if slope > 0 else None, "T_pass_s": float(icpt)})
    spread = max(max(r["wg_spread"], r["loop_spread"], r["auto_spread"]) for r in rows)
    margin = max(0.10, 3 * spread)
    out.update({"max_spread": spread, "margin": margin,
                "auto_lost_beyond_margin": [[r["set"], r["n"], r["count"], r["auto_loss"]] for r in rows if r["auto_loss"] > 1 + margin]})
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
