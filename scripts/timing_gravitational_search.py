"""The gravitational search solver: a single run and a batch of 64 runs on berlin52 (the default 10 000 epochs), a280 (2 000) and a
synthetic n = 1 002 (200), default options otherwise (25 agents), no initial tour, against tests/probes/gsa_cpu_baseline.cpp on one
core of the same box (times `count` for a batch): swap_sequence with its linear search, the full sequence then `take`, the velocity
applied in order and a full re-sum per move, which is what the reference does.  Medians of `--reps` runs after one warm-up; kernel
time from the context's HIP events, wall time of the whole call.  Inside, the GPU's tour and cost bits of run 0 are asserted equal
to the restatement's.  With --evidence the oracle (tests/_gsa_oracle.py, on the CPU) also gives, per instance over its first
--evidence epochs, the share of live pulls whose j had already moved in the epoch and the mean number of live pulls per move: what
the in-order form of the kernel rests on.

    python scripts/timing_gravitational_search.py [--reps 3] [--json] [--instances berlin52:10000,a280:2000,synth1002:200] [--counts 1,64] [--evidence 20]"""
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
N_NEAREST, SEED = 3, 1  # HeuristicOptions::default (mod.rs:604-611): 25 agents
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
    out, costs, moves = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32), np.zeros(count, dtype=np.uint32)
    best, st = C.c_uint32(), _capi.TlStats()
    po = _capi.TlGsaOpts(epochs, N_NEAREST, 0)
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_gravitational_search_population(ctx.handle, vp(xy), n, None, None, 0, 0, count, C.byref(po), SEED, vp(out), vp(costs), vp(moves),
                                                         C.byref(best), C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return {"kernel_ms": round(statistics.median(ks), 2), "wall_ms": round(statistics.median(ws), 2), "best_cost": float(costs.min()),
            "us_per_epoch": round(statistics.median(ks) * 1e3 / max(epochs, 1), 2), "improved_run0": int(moves[0]),
            "run0": (out[0].tolist(), int(costs[:1].view(np.uint32)[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52:10000,a280:2000,synth1002:200")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--evidence", type=int, default=0)
    a = ap.parse_args()
    import _sa_cases as K
    tmp = tempfile.mkdtemp(prefix="gsa_timing_")
    exe = os.path.join(tmp, "gsa_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "gsa_cpu_baseline.cpp"), "-o", exe])
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
            args = [exe, path, "--epochs", str(epochs), "--seed", str(SEED), "--n-nearest", str(N_NEAREST)]
            cpu = [subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines() for _ in range(a.reps if n < 200 else 1)]
            head = cpu[0][0].split()
            cpu_ms = statistics.median(float(c[0].split()[4]) for c in cpu) * 1e3
            row = {"instance": name, "n": n, "epochs": epochs, "agents": 25, "improved": int(head[2]), "cpu_ms": round(cpu_ms, 2)}
            for count in counts:
                P, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
                ctx.lib.tl_gravitational_search_plan(n, N_NEAREST, count, info["cus"], info["lds_bytes"], WORK, 0, C.byref(P), C.byref(t), C.byref(per))
                r = run(ctx, xy, count, epochs, a.reps)
                tour0, bits0 = r.pop("run0")
                assert tour0 == [int(v) for v in cpu[0][1].split()] and bits0 == int(head[3]), "run 0 differs from the CPU restatement"
                r.update(threads=t.value, per_launch=per.value, cpu_ms_times_count=round(cpu_ms * count, 1), speedup=round(cpu_ms * count / r["wall_ms"], 2),
                         speedup_kernel=round(cpu_ms * count / r["kernel_ms"], 2))
                row[f"runs{count}"] = r
            if a.evidence:
                import _gsa_oracle as GO
                res = GO.solve(xy, None, n, None, epochs=min(a.evidence, epochs), n_nearest=N_NEAREST, seed=SEED, seq=GO.swap_sequence_inverse)
                row["oracle_evidence"] = dict(GO.evidence(res), epochs=min(a.evidence, epochs))
            print(json.dumps(row) if a.json else row, flush=True)


if __name__ == "__main__":
    main()
