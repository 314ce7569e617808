"""The stochastic hill climb at the defaults (10 000 epochs, plateau 500) from a shuffle: a single chain at the plan's window and at
window = 1, and populations of 256 / 1 024 chains, against tests/probes/hill_cpu_baseline.cpp on one core of the same box (times
`count` for a population).  Medians of `--reps` runs after one warm-up; kernel time from the context's HIP events, wall time of the
whole call.  The single chain is asserted equal to the CPU restatement (tour, cost bits, acceptances).  Also prints the mean epochs a
window step advances, counted by the numpy statement of the window rule (tests/_hill_oracle.py) on the same chain.

    python scripts/timing_hill_climb.py [--reps 3] [--json] [--instances berlin52,a280,synth1002] [--counts 1,256,1024]"""
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
EPOCHS, PLATOO = 10000, 500


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(ctx, xy, start, count, window, reps):
    n = len(xy)
    out, costs, moves = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32), np.zeros(count, dtype=np.uint32)
    best, st = C.c_uint32(), _capi.TlStats()
    o = _capi.TlHillOpts(EPOCHS, PLATOO, window, 0)
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_hill_climb_population(ctx.handle, vp(xy), n, None, vp(start), 1, 0, count, C.byref(o), 1, vp(out), vp(costs), vp(moves), C.byref(best),
                                                   C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return {"kernel_ms": round(statistics.median(ks), 3), "wall_ms": round(statistics.median(ws), 3), "best_cost": float(costs.min()),
            "chain0": (out[0].tolist(), int(costs[:1].view(np.uint32)[0]), int(moves[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52,a280,synth1002")
    ap.add_argument("--counts", default="1,256,1024")
    a = ap.parse_args()
    import _hill_oracle as HO
    import _sa_cases as K
    tmp = tempfile.mkdtemp(prefix="hill_timing_")
    exe = os.path.join(tmp, "hill_cpu_baseline")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                           os.path.join(ROOT, "tests", "probes", "hill_cpu_baseline.cpp"), "-o", exe])
    counts = [int(v) for v in a.counts.split(",")]
    with TA.Context(0) as ctx:
        info = ctx.device_info()
        for name in a.instances.split(","):
            xy = K.synth(int(name[5:]), 9) if name.startswith("synth") else K.tsplib(name)["xy"]
            n = len(xy)
            path = os.path.join(tmp, f"{name}.txt")
            with open(path, "w") as fh:
                fh.write(f"{n} xy\n" + "".join(f"{float(x)!r} {float(y)!r}\n" for x, y in xy))
            prob = TA.TspProblem(np.arange(n), xy)
            sh = TA.pipeline.random_shuffle(prob, 1, ctx=ctx)
            start = np.ascontiguousarray(prob.positions_of(sh.route()), dtype=np.uint32)
            ini = os.path.join(tmp, f"{name}.init")
            open(ini, "w").write(" ".join(str(int(v)) for v in start) + "\n")
            cpu = [subprocess.run([exe, path, "--epochs", str(EPOCHS), "--platoo", str(PLATOO), "--seed", "1", "--init", ini], capture_output=True, text=True,
                                  check=True).stdout.splitlines() for _ in range(a.reps)]
            head = cpu[0][0].split()
            cpu_ms = statistics.median(float(c[0].split()[5]) for c in cpu) * 1e3
            row = {"instance": name, "n": n, "start_cost": float(sh.total), "epochs": int(head[0]), "accepts": int(head[1]), "restarts": int(head[2]),
                   "cpu_ms": round(cpu_ms, 3)}
            for W in (64, 256):  # the window rule in numpy on the same chain: how far a window step gets
                _res, rec = HO.windows(xy, None, n, start, W=W, seed=1, epochs=EPOCHS, platoo_epochs=PLATOO)
                row[f"epochs_per_window_step_W{W}"] = round((EPOCHS + 1) / len(rec), 2)
                row[f"windows_without_event_W{W}"] = round(sum(1 for r in rec if r[4] == "none") / len(rec), 3)
            for count in counts:
                w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
                ctx.lib.tl_hill_climb_plan(n, count, info["cus"], info["lds_bytes"], 0, C.byref(w), C.byref(t), C.byref(per))
                reps = a.reps if count == 1 else max(1, a.reps - 1)
                r = run(ctx, xy, start, count, 0, reps)
                chain0 = r.pop("chain0")
                if count == 1:  # the same chain as the CPU restatement's
                    assert chain0 == ([int(v) for v in cpu[0][1].split()], int(head[4]), int(head[1])), name
                    r1 = run(ctx, xy, start, 1, 1, reps)
                    assert r1.pop("chain0") == chain0, name
                    r["window1_kernel_ms"] = r1["kernel_ms"]
                r.update(window=w.value, threads=t.value, per_launch=per.value, cpu_ms_times_count=round(cpu_ms * count, 1),
                         speedup_kernel=round(cpu_ms * count / r["kernel_ms"], 2))
                row[f"chains{count}"] = r
            print(json.dumps(row) if a.json else row, flush=True)


if __name__ == "__main__":
    main()
