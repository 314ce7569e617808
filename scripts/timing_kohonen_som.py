"""The Kohonen map solver: a single run and a batch of 64 runs on berlin52, a280 and a synthetic n = 1 002, each at the default options
(100 000 epochs, learning_rate 0.8, radius_fraction 0.1, neuron_multiplier 8), against tests/probes/som_cpu_baseline.cpp on one core of
the same box (times `count` for a batch): the reference's loop, every neuron of every epoch through the two tests.  Medians of
`--reps` runs after one warm-up; kernel time from the context's HIP events (training and extraction), wall time of the whole call.
Inside, the GPU's tour and cost bits of run 0 are asserted equal to the restatement's.  No threshold: what comes out is written down.
Not measured here: the split between the scan and the update inside an epoch, and the workspace form at size (--form 2 runs it).

    python scripts/timing_kohonen_som.py [--reps 3] [--json] [--instances berlin52,a280,synth1002] [--epochs 100000] [--counts 1,64] [--form 0]"""
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

SEED = 1
WORK = 8 << 30


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(ctx, xy, count, epochs, reps, form):
    n = len(xy)
    out, costs = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32)
    best, st = C.c_uint32(), _capi.TlStats()
    po = _capi.TlSomOpts(epochs, 8, 0.8, 0.1, form, 0, 0)
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_kohonen_som_population(ctx.handle, vp(xy), n, None, 0, count, C.byref(po), SEED, vp(out), vp(costs), C.byref(best), C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return {"kernel_ms": round(statistics.median(ks), 2), "wall_ms": round(statistics.median(ws), 2), "best_cost": float(costs.min()),
            "us_per_epoch": round(statistics.median(ks) * 1e3 / max(epochs, 1), 3), "run0": (out[0].tolist(), int(costs[:1].view(np.uint32)[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52,a280,synth1002")
    ap.add_argument("--epochs", type=int, default=100_000)
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--form", type=int, default=0)
    a = ap.parse_args()
    import _sa_cases as K
    tmp = tempfile.mkdtemp(prefix="som_timing_")
    exe = os.path.join(tmp, "som_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "som_cpu_baseline.cpp"), "-o", exe])
    counts = [int(v) for v in a.counts.split(",")]
    with TA.Context(0) as ctx:
        info = ctx.device_info()
        for name in a.instances.split(","):
            xy = K.synth(int(name[5:]), 9) if name.startswith("synth") else K.tsplib(name)["xy"]
            n = len(xy)
            path = os.path.join(tmp, f"{name}.txt")
            with open(path, "w") as fh:
                fh.write(f"{n}\n" + "".join(f"{float(x)!r} {float(y)!r}\n" for x, y in xy))
            args = [exe, path, "--epochs", str(a.epochs), "--seed", str(SEED)]
            times = [[float(v) for v in subprocess.run(args + ["--time"], capture_output=True, text=True, check=True).stdout.split()] for _ in range(a.reps)]
            cpu_train, cpu_extract = statistics.median(t[0] for t in times), statistics.median(t[1] for t in times)
            cpu_ms = cpu_train + cpu_extract
            ref = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
            row = {"instance": name, "n": n, "neurons": 8 * n, "epochs": a.epochs, "cpu_ms": round(cpu_ms, 2), "cpu_train_ms": round(cpu_train, 2),
                   "cpu_us_per_epoch": round(cpu_train * 1e3 / a.epochs, 3)}
            for count in counts:
                M, t, f, per = C.c_uint32(), C.c_int(), C.c_uint32(), C.c_uint32()
                ctx.lib.tl_kohonen_som_plan(n, 8, a.form, count, info["cus"], info["lds_bytes"], WORK, 0, C.byref(M), C.byref(t), C.byref(f), C.byref(per))
                r = run(ctx, xy, count, a.epochs, a.reps, a.form)
                tour0, bits0 = r.pop("run0")
                assert tour0 == [int(v) for v in ref[1].split()] and bits0 == int(ref[0]), "run 0 differs from the CPU restatement"
                r.update(threads=t.value, form=f.value, cpu_ms_times_count=round(cpu_ms * count, 1), speedup=round(cpu_ms * count / r["wall_ms"], 2),
                         speedup_kernel=round(cpu_ms * count / r["kernel_ms"], 2))
                row[f"runs{count}"] = r
            print(json.dumps(row) if a.json else row, flush=True)


if __name__ == "__main__":
    main()
