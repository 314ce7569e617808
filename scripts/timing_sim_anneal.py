"""Simulated annealing, default schedule (138 149 epochs): a single chain with speculative windows and with
TL_FLAG_SA_NO_SPECULATION, and populations of 256 / 1 024 chains, against tests/probes/sa_cpu_baseline.cpp on one core of the same
box (times `count` for a population).  Medians of `--reps` runs after one warm-up; kernel time from the context's HIP events.
Also prints the chosen window and the mean epochs advanced per window step (epochs / (accepted + whole windows), from the trace).

    python scripts/timing_sim_anneal.py [--reps 5] [--json]"""
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
from teeline_amd import _capi  # noqa: E402

TSPLIB = os.path.join(ROOT, "tests", "golden", "tsplib")


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: synth\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def single(ctx, xy, reps):
    n = len(xy)
    out, cost, st, o = np.zeros(n, dtype=np.uint32), C.c_float(), _capi.TlStats(), _capi.TlSaOpts(10000, 1e-4, 1e-3, 1000.0)
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_sim_anneal(ctx.handle, vp(xy), n, None, None, C.byref(o), 1, vp(out), C.byref(cost), C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return statistics.median(ks), statistics.median(ws), int(st.moves), int(st.sweeps), float(cost.value)


def steps_per_window(ctx, xy, window):
    """window steps of the default schedule from the accepted epochs: an accepted epoch ends a step, a run of g rejected epochs
    before it (or at the end) takes ceil-free g // window whole steps more"""
    n = len(xy)
    cap = 1 << 16
    out, cost, o = np.zeros(n, dtype=np.uint32), C.c_float(), _capi.TlSaOpts(10000, 1e-4, 1e-3, 1000.0)
    log, ln = np.zeros((cap, 4), dtype=np.uint32), C.c_uint32()
    ctx.check(ctx.lib.tl_sim_anneal_trace(ctx.handle, vp(xy), n, None, None, C.byref(o), 1, vp(out), C.byref(cost), None, vp(log), cap, C.byref(ln)))
    total = TA.simulated_annealing.schedule_epochs()
    ep = log[:min(ln.value, cap), 0].astype(np.int64)
    steps, at = 0, 0
    for e in ep:
        steps += (e - at) // window + 1
        at = e + 1
    steps += -(-(total - at) // window)
    return total / max(steps, 1)


def population(ctx, xy, count, reps):
    n = len(xy)
    out, costs, moves = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32), np.zeros(count, dtype=np.uint32)
    best, st, o = C.c_uint32(), _capi.TlStats(), _capi.TlSaOpts(10000, 1e-4, 1e-3, 1000.0)
    ks = []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_sim_anneal_population(ctx.handle, vp(xy), n, None, None, 0, 0, count, C.byref(o), 1, vp(out), vp(costs), vp(moves), C.byref(best),
                                                   C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
    return statistics.median(ks), float(costs.min()), float(np.median(costs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--skip-population", action="store_true")
    a = ap.parse_args()
    import _sa_cases as K
    tmp = tempfile.mkdtemp(prefix="sa_timing_")
    exe = os.path.join(tmp, "sa_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "probes", "sa_cpu_baseline.cpp"), "-o", exe])
    inst = {}
    for name in ("berlin52", "a280"):
        inst[name] = (os.path.join(TSPLIB, f"{name}.tsp"), K.tsplib(name)["xy"])
    xy = K.synth(1002, 9)
    write_tsp(os.path.join(tmp, "synth1002.tsp"), xy)
    inst["synth1002"] = (os.path.join(tmp, "synth1002.tsp"), xy)
    rows = []
    with TA.Context(0) as spec, TA.Context(0, TA.TL_FLAG_SA_NO_SPECULATION) as nospec:
        info = spec.device_info()
        for name, (path, xy) in inst.items():
            n = len(xy)
            cpu = statistics.median(float(subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.split()[3]) for _ in range(a.reps)) * 1e3
            w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
            spec.lib.tl_sim_anneal_plan(n, 1, info["cus"], info["lds_bytes"], 0, C.byref(w), C.byref(t), C.byref(per))
            k1, w1, moves, epochs, cost = single(spec, xy, a.reps)
            k0, w0, *_ = single(nospec, xy, a.reps)
            row = {"instance": name, "n": n, "epochs": epochs, "accepted": moves, "cost": cost, "window": w.value, "threads": t.value,
                   "epochs_per_window_step": round(steps_per_window(spec, xy, w.value), 2), "cpu_ms": round(cpu, 2),
                   "gpu_kernel_ms": round(k1, 2), "gpu_wall_ms": round(w1, 2), "gpu_no_speculation_kernel_ms": round(k0, 2)}
            if not a.skip_population:
                for count in (256, 1024):
                    spec.lib.tl_sim_anneal_plan(n, count, info["cus"], info["lds_bytes"], 0, C.byref(w), C.byref(t), C.byref(per))
                    kp, cmin, cmed = population(spec, xy, count, max(1, a.reps - 1))
                    row[f"pop{count}"] = {"kernel_ms": round(kp, 2), "cpu_ms_times_count": round(cpu * count, 1), "window": w.value, "per_launch": per.value,
                                          "best_cost": cmin, "median_cost": cmed}
            rows.append(row)
            print(json.dumps(row) if a.json else row, flush=True)


if __name__ == "__main__":
    main()
