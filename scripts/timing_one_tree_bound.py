"""The Held-Karp lower bound: one job and batches of 64 and 256 jobs (roots x lambda0 around the defaults) on
berlin52, a280 and a synthetic n = 1 002, 100 iterations each, against tests/probes/one_tree_cpu_baseline.cpp on one core of the
same box (job 0's options; times the iterations all jobs ran for a batch).  Medians of `--reps` runs after one warm-up; kernel time
from the context's HIP events.  Inside, job 0's bound is asserted equal to the probe's bit for bit.  Also: the duration of ONE launch
of the plan's span, and the bound at the default options (1 000 iterations, upper from nearest_neighbor -> two_opt) with its ratio to
the known optimum where tests/golden/tsplib holds the optimal tour (berlin52).  No threshold: what comes out is written down.
The matrix form is timed on the instances of n <= 300 (a packed triangle built from the same distances: the same bits).
Not measured here: the split of an iteration into root edges, Prim rounds and the pi update; whether matrix rows stay in L2 (no
counters are read; the matrix rows' time against the coordinate form's is what there is).

    python scripts/timing_one_tree_bound.py [--reps 3] [--json] [--instances berlin52,a280,synth1002] [--counts 1,64,256]"""
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

ITERS = 100


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def option_sets(count, n, upper, iterations=ITERS, span=0):
    """job 0 is the default option set; the others move the root and lambda0"""
    return [_capi.TlOneTreeOpts((7 * j) % n, iterations, 10, span, 2.0 * (1.0 + 0.125 * (j % 8)) if j else 2.0, upper, 0) for j in range(count)]


def run(ctx, xy, sets, reps, packed=None):
    n, count = len(xy), len(sets)
    arr = (_capi.TlOneTreeOpts * count)(*sets)
    res = (_capi.TlOneTreeResult * count)()
    best, st = C.c_uint32(), _capi.TlStats()
    ks, ws = [], []
    for r in range(reps + 1):
        ctx.check(ctx.lib.tl_one_tree_bound_batch(ctx.handle, vp(xy), vp(packed), n, arr, count, res, None, None, None, None, 0, C.byref(best), C.byref(st)))
        if r:
            ks.append(st.kernel_ms)
            ws.append(st.total_ms)
    return statistics.median(ks), statistics.median(ws), res, int(st.sweeps)


def cpu(exe, path, upper, o):
    out = subprocess.run([exe, path, repr(float(upper)), str(o.root), str(o.iterations), repr(float(o.lambda0)), str(o.patience)], capture_output=True,
                         text=True, check=True).stdout.split()
    return float.fromhex(out[0]), int(out[2]), float(out[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--instances", default="berlin52,a280,synth1002")
    ap.add_argument("--counts", default="1,64,256")
    a = ap.parse_args()
    import _one_tree_cases as K
    import _one_tree_oracle as H
    ctx = TA.default_context()
    lds = ctx.device_info()["lds_bytes"]
    emit = lambda rec: print(json.dumps(rec) if a.json else rec, flush=True)  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "one_tree_cpu_baseline")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "teeline_amd", "csrc"),
                               os.path.join(ROOT, "tests", "probes", "one_tree_cpu_baseline.cpp"), "-o", exe])
        for name in a.instances.split(","):
            xy = K.random_xy(1002, 11) if name == "synth1002" else K.tsp(name)[0]
            xy = np.ascontiguousarray(xy, dtype=np.float32)
            n = len(xy)
            prob = TA.TspProblem(np.arange(n), xy)
            upper, _ = TA.one_tree_bound.upper_from_solvers(prob, ctx)
            path = os.path.join(tmp, name + ".txt")
            with open(path, "w") as fh:
                fh.write(f"{n}\n" + "\n".join(f"{float(p)!r} {float(q)!r}" for p, q in xy) + "\n")
            job0 = option_sets(1, n, upper)[0]
            runs = [cpu(exe, path, upper, job0) for _ in range(a.reps)]
            cpu_bound, cpu_iters, cpu_ms = runs[0][0], runs[0][1], statistics.median(r[2] for r in runs)
            for count in (int(v) for v in a.counts.split(",")):
                k_ms, w_ms, res, iters = run(ctx, xy, option_sets(count, n, upper), a.reps)
                assert res[0].bound.hex() == cpu_bound.hex() and res[0].iterations_run == cpu_iters, (name, count)
                longest = max(r.iterations_run for r in res)
                emit(dict(what="one_tree_bound", instance=name, n=n, jobs=count, iterations_all_jobs=iters, kernel_ms=round(k_ms, 3), wall_ms=round(w_ms, 3),
                          us_per_round=round(k_ms * 1e3 / (longest * (n - 1)), 3), cpu_ms_one_job=round(cpu_ms, 3),
                          ratio_vs_one_core=round(cpu_ms / cpu_iters * iters / k_ms, 2), job0_equals_probe=True))
            # the matrix form of the same instance (rows read from the expanded square matrix): the same bits, its own time
            if n <= 300:
                row = H.rows_of(xy, None, n)
                packed = np.ascontiguousarray([row(i)[j] for i in range(1, n) for j in range(i)], dtype=np.float32)
                for count in (int(v) for v in a.counts.split(",")):
                    k_ms, w_ms, res, iters = run(ctx, xy, option_sets(count, n, upper), a.reps, packed)
                    assert res[0].bound.hex() == cpu_bound.hex(), (name, count, "matrix form")
                    longest = max(r.iterations_run for r in res)
                    emit(dict(what="one_tree_bound_matrix_form", instance=name, n=n, jobs=count, iterations_all_jobs=iters, kernel_ms=round(k_ms, 3),
                              wall_ms=round(w_ms, 3), us_per_round=round(k_ms * 1e3 / (longest * (n - 1)), 3),
                              ratio_vs_one_core=round(cpu_ms / cpu_iters * iters / k_ms, 2), matrix_bytes=4 * n * n, job0_equals_probe=True))
            # one launch of the plan's span
            span = C.c_uint32()
            assert ctx.lib.tl_one_tree_bound_plan(n, lds, None, C.byref(span)) == 0
            k_ms, _, res, _ = run(ctx, xy, option_sets(1, n, upper, iterations=span.value), a.reps)
            emit(dict(what="one_launch", instance=name, n=n, span=span.value, iterations_run=res[0].iterations_run, kernel_ms=round(k_ms, 3)))
            # the defaults
            b = TA.one_tree_bound.bound(prob, None, ctx=ctx)
            rec = dict(what="defaults", instance=name, n=n, upper=b.upper, bound=b.bound, gap_pct_of_upper=round(b.gap_pct(b.upper), 4), stop=b.stats["stop_name"],
                       iterations_run=b.stats["iterations_run"], kernel_ms=round(b.stats["kernel_ms"], 3))
            if os.path.exists(os.path.join(ROOT, "tests", "golden", "tsplib", name + ".opt.tour")):
                opt = H.tour_length_f64(H.rows_of(xy, None, n), K.opt_tour_positions(name))
                rec.update(optimal_tour_f64=opt, bound_over_optimum=round(b.bound / opt, 6))
            emit(rec)


if __name__ == "__main__":
    main()
