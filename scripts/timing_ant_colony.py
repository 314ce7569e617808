"""The ant colony solver: a single run and a batch of 64 runs on berlin52 and a280 (the default 150 epochs) and a synthetic n = 1 002
(10: the default would take the CPU baseline minutes), default options otherwise, no initial tour, against
tests/probes/aco_cpu_baseline.cpp on one core of the same box (times `count` for a batch).  Medians of `--reps` runs after one
warm-up; kernel time from the context's HIP events, wall time of the whole call.  Inside, the GPU's tour and cost bits of run 0 are
asserted equal to the restatement's.

    python scripts/timing_ant_colony.py [--reps 3] [--json] [--instances berlin52:150,a280:150,synth1002:10] [--counts 1,64]"""
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
ALPHA, BETA, RATE, ANTS, SEED = 1.0, 2.0, 0.5, 25, 1  # AcoOptions::default (mod.rs:1091-1112)
WORK = 8 << 30


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: synth\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def run(ctx, xy, count, epochs, reps):
    n = len(xy)
    out, costs = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32)
    best, st = C.c_uint32(), _capi.TlStats()
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_ant_colony_population(ctx.handle, vp(xy), n, None, None, 0, 0, count, epochs, ALPHA, BETA, RATE, ANTS, SEED, vp(out), vp(costs),
                                                   C.byref(best), C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return {"kernel_ms": round(statistics.median(ks), 2), "wall_ms": round(statistics.median(ws), 2), "best_cost": float(costs.min()),
            "us_per_epoch": round(statistics.median(ks) * 1e3 / max(epochs, 1), 2), "run0": (out[0].tolist(), int(costs[:1].view(np.uint32)[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52:150,a280:150,synth1002:10")
    ap.add_argument("--counts", default="1,64")
    a = ap.parse_args()
    import _sa_cases as K
    tmp = tempfile.mkdtemp(prefix="aco_timing_")
    exe = os.path.join(tmp, "aco_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "aco_cpu_baseline.cpp"), "-o", exe])
    counts = [int(v) for v in a.counts.split(",")]
    with TA.Context(0) as ctx:
        info = ctx.device_info()
        for item in a.instances.split(","):
            name, epochs = item.split(":")
            epochs = int(epochs)
            if name.startswith("synth"):
                xy = K.synth(int(name[5:]), 9)
                path = os.path.join(tmp, f"{name}.tsp")
                write_tsp(path, xy)
            else:
                path, xy = os.path.join(TSPLIB, f"{name}.tsp"), K.tsplib(name)["xy"]
            n = len(xy)
            cpu = [subprocess.run([exe, path, "--epochs", str(epochs), "--seed", str(SEED), "--alpha", repr(ALPHA), "--beta", repr(BETA), "--evaporation-rate", repr(RATE), "--num-ants", str(ANTS)],
                                  capture_output=True, text=True, check=True).stdout.splitlines() for _ in range(a.reps if n < 500 else 1)]
            head = cpu[0][0].split()
            cpu_ms = statistics.median(float(c[0].split()[5]) for c in cpu) * 1e3
            row = {"instance": name, "n": n, "epochs": epochs, "ants": ANTS, "improved": int(head[2]), "fallbacks": int(head[3]),
                   "cpu_ms": round(cpu_ms, 2)}
            for count in counts:
                per, t, need = C.c_uint32(), C.c_int(), C.c_uint64()
                ctx.lib.tl_ant_colony_plan(n, ANTS, count, info["cus"], info["lds_bytes"], WORK, C.byref(per), C.byref(t), C.byref(need))
                r = run(ctx, xy, count, epochs, a.reps if count == 1 else max(1, a.reps - 1))
                tour0, bits0 = r.pop("run0")
                assert tour0 == [int(v) for v in cpu[0][1].split()] and bits0 == int(head[4]), "run 0 differs from the CPU restatement"
                r.update(threads=t.value, per_launch=per.value, workspace_mb=round(need.value / 2 ** 20, 1), cpu_ms_times_count=round(cpu_ms * count, 1),
                         speedup=round(cpu_ms * count / r["wall_ms"], 2))
                row[f"runs{count}"] = r
            print(json.dumps(row) if a.json else row, flush=True)


if __name__ == "__main__":
    main()
