"""Tabu search, default 10 000 epochs: a single chain and populations of 256 / 1 024 chains, in the default form and with
TL_FLAG_TABU_FULL_COMPARE, from a nearest-neighbour start and from a 2-opt local optimum, against tests/probes/tabu_cpu_baseline.cpp on
one core of the same box (times `count` for a population).  Medians of `--reps` runs after one warm-up; kernel time from the
context's HIP events, wall time of the whole call.  Also prints the mean attempts per epoch (candidates / epochs), the forced epochs
and the list's hits (from the CPU restatement, whose chain is the same).

    python scripts/timing_tabu_search.py [--reps 3] [--json] [--instances berlin52,a280,synth1002] [--counts 1,256,1024] [--skip-full]"""
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
EPOCHS = 10000
WORK = 8 << 30


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def write_tsp(path, xy):
    with open(path, "w") as fh:
        fh.write(f"NAME: synth\nTYPE: TSP\nDIMENSION: {len(xy)}\nEDGE_WEIGHT_TYPE: EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(xy):
            fh.write(f"{k + 1} {float(x)!r} {float(y)!r}\n")
        fh.write("EOF\n")


def run(ctx, xy, start, count, reps):
    n = len(xy)
    out, costs, moves = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32), np.zeros(count, dtype=np.uint32)
    best, st = C.c_uint32(), _capi.TlStats()
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_tabu_search_population(ctx.handle, vp(xy), n, None, vp(start), 1, 0, count, EPOCHS, 1, vp(out), vp(costs), vp(moves), C.byref(best),
                                                    C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return {"kernel_ms": round(statistics.median(ks), 2), "wall_ms": round(statistics.median(ws), 2), "best_cost": float(costs.min()),
            "attempts_per_epoch": round(st.candidates / st.sweeps, 2), "chain0": (out[0].tolist(), float(costs[0]), int(moves[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52,a280,synth1002")
    ap.add_argument("--counts", default="1,256,1024")
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()
    import _sa_cases as K
    tmp = tempfile.mkdtemp(prefix="tabu_timing_")
    exe = os.path.join(tmp, "tabu_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "tabu_cpu_baseline.cpp"), "-o", exe])
    inst = {}
    for name in a.instances.split(","):
        if name.startswith("synth"):
            xy = K.synth(int(name[5:]), 9)
            write_tsp(os.path.join(tmp, f"{name}.tsp"), xy)
            inst[name] = (os.path.join(tmp, f"{name}.tsp"), xy)
        else:
            inst[name] = (os.path.join(TSPLIB, f"{name}.tsp"), K.tsplib(name)["xy"])
    counts = [int(v) for v in a.counts.split(",")]
    with TA.Context(0) as plain, TA.Context(0, TA.TL_FLAG_TABU_FULL_COMPARE) as full:
        info = plain.device_info()
        for name, (path, xy) in inst.items():
            n = len(xy)
            prob = TA.TspProblem(np.arange(n), xy)
            nn = TA.nearest_neighbor.solve(prob, None, None, None, ctx=plain)
            opt = TA.two_opt.solve(prob, None, None, nn.route(), ctx=plain)
            for start_name, sol in (("nn", nn), ("2opt", opt)):
                start = np.ascontiguousarray(prob.positions_of(sol.route()), dtype=np.uint32)
                ini = os.path.join(tmp, f"{name}_{start_name}.init")
                open(ini, "w").write(" ".join(str(int(v)) for v in start) + "\n")
                cpu = [subprocess.run([exe, path, "--epochs", str(EPOCHS), "--seed", "1", "--init", ini], capture_output=True, text=True, check=True).stdout.splitlines()
                       for _ in range(a.reps if n < 500 else 1)]
                head = cpu[0][0].split()
                cpu_ms = statistics.median(float(c[0].split()[6]) for c in cpu) * 1e3
                row = {"instance": name, "n": n, "start": start_name, "start_cost": float(sol.total), "epochs": int(head[0]), "hits": int(head[1]), "forced": int(head[2]),
                       "new_bests": int(head[3]), "attempts_per_epoch": round(int(head[4]) / int(head[0]), 2), "cpu_ms": round(cpu_ms, 2)}
                for count in counts:
                    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
                    plain.lib.tl_tabu_search_plan(n, count, info["cus"], info["lds_bytes"], WORK, 0, C.byref(w), C.byref(t), C.byref(per))
                    reps = a.reps if count == 1 else max(1, a.reps - 1)
                    r = run(plain, xy, start, count, reps)
                    tour0, cost0, bests0 = r.pop("chain0")
                    if count == 1:  # the same chain as the CPU restatement's
                        assert tour0 == [int(v) for v in cpu[0][1].split()] and np.float32(cost0).view(np.uint32) == int(head[5]) and bests0 == int(head[3])
                    r.update(window=w.value, threads=t.value, per_launch=per.value, cpu_ms_times_count=round(cpu_ms * count, 1))
                    if not a.skip_full:
                        rf = run(full, xy, start, count, reps)
                        assert rf.pop("chain0") == (tour0, cost0, bests0)
                        r["full_compare_kernel_ms"] = rf["kernel_ms"]
                    row[f"chains{count}"] = r
                print(json.dumps(row) if a.json else row, flush=True)


if __name__ == "__main__":
    main()
