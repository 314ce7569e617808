"""The Fourier-curve solver: one job and batches of 64 and 256 jobs (a lambda x lr grid) on berlin52, a280 and a synthetic n = 1 002,
each at the default options (k_max 4, m 200, epochs 400: 1 600 gradient steps), against tests/probes/fourier_cpu_baseline.cpp on one
core of the same box in its tree-per-step form (what fourier.rs does per step: a fresh kd-tree of the samples, a query per city; the
kd-tree is this project's own text) — times the job count for a batch — and, beside it, its brute-force search form, which is NOT
what the reference does.  Medians of `--reps` runs after one warm-up; kernel time from the context's HIP events (steps and decode),
wall time of the whole call.  Inside, job 0's tour and cost bits are asserted equal to the restatement's specification form.  No
threshold: what comes out is written down.  Not measured here: the split of a step into gamma, search, sums and update.

    python scripts/timing_fourier_curve.py [--reps 3] [--json] [--instances berlin52,a280,synth1002] [--counts 1,64,256]"""
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


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def grid(count):
    """job 0 is the default option set; the others vary lambda (outer) and lr (inner) around it"""
    side = int(round(count ** 0.5))
    las = [0.05 * (1.0 + 0.25 * i) for i in range(max(count // side, 1))]
    lrs = [0.05 * (1.0 + 0.1 * i) for i in range(side)]
    return [(la, lr) for la in las for lr in lrs][:count]


def run(ctx, xy, count, reps):
    n = len(xy)
    jobs = grid(count)
    arr = (_capi.TlFourierOpts * count)(*[_capi.TlFourierOpts(4, 200, 400, 0, la, 0.5, lr, 0, 0) for la, lr in jobs])
    out, costs = np.zeros((count, n), dtype=np.uint32), np.zeros(count, dtype=np.float32)
    best, st = C.c_uint32(), _capi.TlStats()
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_fourier_curve_batch(ctx.handle, vp(xy), n, None, arr, count, vp(out), vp(costs), None, 0, C.byref(best), C.byref(st), None, 0, None))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return statistics.median(ks), statistics.median(ws), out[0].tolist(), int(costs[0].view(np.uint32)), int(best.value)


def cpu(exe, path, form):
    args = [exe, path] + (["--time", form] if form else [])
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("cost_bits")][0]
    ms = [float(v) for ln in lines if ln.startswith("ms ") for v in ln.split()[1:]]
    return sum(ms), int(lines[at].split()[1], 16), [int(v) for v in lines[at + 1].split()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52,a280,synth1002")
    ap.add_argument("--counts", default="1,64,256")
    a = ap.parse_args()
    import _sa_cases as K
    ctx = TA.default_context()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fourier_cpu_baseline")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                               os.path.join(ROOT, "tests", "probes", "fourier_cpu_baseline.cpp"), "-o", exe])
        for name in a.instances.split(","):
            xy = K.synth(1002, 11) if name == "synth1002" else K.tsplib(name)["xy"]
            xy = np.ascontiguousarray(xy, dtype=np.float32)
            n = len(xy)
            path = os.path.join(tmp, name + ".txt")
            with open(path, "w") as fh:
                fh.write(f"{n}\n" + "\n".join(f"{float(p)!r} {float(q)!r}" for p, q in xy) + "\n")
            _ms, spec_bits, spec_tour = cpu(exe, path, None)
            tree_ms = statistics.median(cpu(exe, path, "tree")[0] for _ in range(a.reps))
            brute_ms = statistics.median(cpu(exe, path, "brute")[0] for _ in range(a.reps))
            for count in (int(v) for v in a.counts.split(",")):
                k_ms, w_ms, tour0, bits0, best = run(ctx, xy, count, a.reps)
                assert tour0 == spec_tour and bits0 == spec_bits, (name, count)
                rec = dict(solver="fourier_curve", instance=name, n=n, jobs=count, steps=1600, kernel_ms=round(k_ms, 3), wall_ms=round(w_ms, 3),
                           us_per_step=round(k_ms * 1e3 / 1600, 3), cpu_tree_ms_one_job=round(tree_ms, 3), cpu_brute_ms_one_job_not_the_references=round(brute_ms, 3),
                           ratio_vs_tree=round(tree_ms * count / k_ms, 2), ratio_vs_brute=round(brute_ms * count / k_ms, 2), best_job=best,
                           job0_equals_restatement=True)
                print(json.dumps(rec) if a.json else rec, flush=True)


if __name__ == "__main__":
    main()
