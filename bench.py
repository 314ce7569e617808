#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X 2-opt engine (BASELINE.json metric).

metric : 2-opt candidate swaps evaluated/sec (+ final tour cost), EUC_2D n = 10 000
workload: BASELINE configs 3/4 — synthetic EUC_2D n=10000 (xorshift64 generator),
          multi-start REF_ORDER 2-opt: R seeded random restarts per GPU, every restart a full
          first-improvement descent to its local optimum (the reference's algorithm, two_opt.rs:26-61),
          one descent per CU, all concurrently.  One "step" = one such batch.
          Weak scaling (default): rank k runs restarts [k*R, (k+1)*R); after every step the ranks min-all-reduce
          (RCCL) the packed key (f32 cost bits << 32 | restart id) of their best tour.
          --restarts-total T: strong scaling as BASELINE configs[3] words it — T restarts in all, sharded in
          contiguous blocks over the ranks (reported as "scaling": "strong").
          Inputs (coordinates) are resident in HBM before the timed region; restart permutations are
          generated on the device inside the timed region (they are part of the job).
candidates are counted as the reference's loop visits them: sweeps x (n-3)(n-2)/2 per descent.

Usage: python bench.py --gpus N --steps K --warmup W
  N > 1 under torch.distributed.run (RANK / WORLD_SIZE set): this process is one rank of N.
  N > 1 bare (no WORLD_SIZE): bench.py starts the N ranks itself — a child `python -m torch.distributed.run --nnodes=1
        --nproc-per-node N --master-addr 127.0.0.1 ...` of this same file, started before anything here touches the GPU —
        relays rank 0's JSON line and exits with the child's code; a line whose `ranks_seen` is not N is an error.
  --single-process: no RCCL, ONE process drives N devices through tl_two_opt_multistart_devices (the path a Rust caller
        has); cross-check of the RCCL number.
  --dry-launch: rehearsal of the launch + collective plumbing on CPU (gloo, a stub step, no GPU, no oracle): NOT a measurement.
  --full: everything beside the headline — the untimed work-count launch and the roofline, the strong-scaling loop where it is
        a loop of its own, the extras (other kernels, sizes and flags), the CPU baselines and the bit-for-bit parity check of
        the timed restarts against the oracle.  Without it a run sets up, warms up, times the K steps and prints the line.
  --dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step handed back as DIR/<name>.npy (dump_outputs).
With --full, rank 0 prints the long material first (`EXTRAS {...}` lines, also written whole to ./bench_extras.json); the LAST
stdout line is always ONE compact JSON object of at most 4096 bytes (asserted) — the line the driver parses.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
ALG_BYTES_PER_CANDIDATE = 8.0   # one new tour-ordered (x,y) per j-step, on-the-fly form
SIMDS_PER_CU = 4                # MI355X_MICROARCH.md: 4 SIMD-32 per CU
VALU_CYCLES_PER_WAVE_INST = 2.0  # MI355X_MICROARCH.md: a wave64 VALU instruction issues over 2 cycles on a SIMD-32
REFCLK_HZ = 100e6               # s_memrealtime ticks (constant 100 MHz)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--restarts", type=int, default=256, help="restarts per GPU per step (one per CU); weak scaling")
    ap.add_argument("--restarts-total", type=int, default=0,
                    help="strong scaling: this many restarts in all, sharded over the ranks (BASELINE configs[3]: 256)")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the single-descent / no-prune / matrix-build extras")
    ap.add_argument("--no-end-to-end", action="store_true",
                    help="skip extras.drop_in_end_to_end (it starts the CLI as child processes: not under a profiler)")
    ap.add_argument("--no-work-count", action="store_true",
                    help="skip the one untimed launch of the counting kernel variant (PMC passes: only the timed kernel runs)")
    ap.add_argument("--single-process", action="store_true",
                    help="N > 1 without RCCL: one process, one tl_ctx per device, tl_two_opt_multistart_devices")
    ap.add_argument("--rccl-in-library", action="store_true",
                    help="with --single-process: the library's own RCCL collective (TL_FLAG_MULTISTART_RCCL: min-all-reduce of the keys + "
                         "broadcast of the winner's tour over ncclCommInitAll communicators) instead of the host minimum")
    ap.add_argument("--force-launcher", action="store_true",
                    help="take the self-launch path even for --gpus 1 (one rank under torch.distributed.run, RCCL initialised): "
                         "the rehearsal of that path on a one-GPU box")
    ap.add_argument("--dry-launch", action="store_true",
                    help="CPU rehearsal of the N-rank launch and the collectives (gloo, stub step): prints a line with value null")
    ap.add_argument("--full", action="store_true",
                    help="also the work count + roofline, the strong-scaling loop, the extras, the CPU baselines and the oracle parity check")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's outputs (tours, costs, descent counters, the winner) as DIR/<name>.npy")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_outputs and (a.single_process or a.dry_launch):
        ap.error("--dump-outputs writes the outputs of the device-resident batch path: not with --single-process or --dry-launch")
    return a


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(a):
    """`bench.py --gpus N` (N > 1) started bare: run the N ranks as children of a torch.distributed.run child.  Nothing in
    this process has touched the GPU (argparse + imports only), and the ranks are fresh processes, never a re-exec.
    Relays rank 0's JSON line; non-zero exit if the child failed, printed no line, or the line saw another rank count."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if a.gpus == 1:
        env["TL_BENCH_FORCE_DIST"] = "1"   # --force-launcher: one rank, but through the process group and RCCL all the same
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{"metric"')]
    for ln in proc.stdout.splitlines():
        if ln.startswith("EXTRAS "):
            print(ln)                       # the long material stays on stdout, ahead of the result line
        elif not ln.startswith('{"metric"'):
            print(ln, file=sys.stderr)
    if proc.returncode != 0:
        for ln in lines:
            print(ln)
        raise SystemExit(proc.returncode)
    if len(lines) != 1:
        raise SystemExit(f"bench.py: the {a.gpus}-rank child printed {len(lines)} result lines instead of one")
    seen = json.loads(lines[0]).get("ranks_seen")
    print(lines[0])
    if seen != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the job saw {seen} ranks")
    return 0


def cpu_baseline(n, seed, xy):
    """Oracle ("port" of two_opt.rs:26-61) timed on this host's cores: one full restart descent per core,
    all cores concurrently (ctypes releases the GIL).  Bounded: ~5e8 candidates per core (~5-10 s)."""
    import threading
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle as O
    O.lib()
    cores = max(1, min(os.cpu_count() or 1, 32))
    res = [None] * cores

    def work(k):
        init = O.restart_perm(n, seed, k)
        rc, p, c, st = O.two_opt(xy, None, n, init=init, flavor=0)
        res[k] = (st["candidates"], np.float32(c), st["sweeps"], st["moves"])

    t0 = time.perf_counter()
    th = [threading.Thread(target=work, args=(k,)) for k in range(cores)]
    [t.start() for t in th]
    [t.join() for t in th]
    wall = time.perf_counter() - t0
    total = sum(r[0] for r in res)
    # the reference's own cost model (packed matrix + 2 SipHash id lookups per distance), 1 core, 1 sweep
    t1 = time.perf_counter()
    rc, p, c, st = O.two_opt(xy, None, n, init=O.restart_perm(n, seed, 0), flavor=1, max_candidates=1)
    wall_f = time.perf_counter() - t1
    return res, {
        "value": total / wall, "unit": "candidates/s", "cores": cores, "kind": "port",
        "sample": f"{cores} full restart descents (restarts 0..{cores - 1}, n={n}, ~{total / cores:.2e} candidates each), "
                  f"one per core, on-the-fly f32 distances (best-effort flavour); wall {wall:.1f} s",
        "per_core": total / wall / cores,
        "ref_faithful_1core": {"value": st["candidates"] / wall_f, "unit": "candidates/s",
                               "sample": f"1 sweep ({st['candidates']} candidates) of restart 0 with the packed matrix + "
                                         f"two SipHash-1-3 id lookups per distance (distance_matrix.rs:197-212), "
                                         f"incl. 200 MB matrix build; wall {wall_f:.1f} s"},
    }


def instance_xy(name, n, TA):
    """The real TSPLIB instance where somebody has supplied it — <name>.tsp under $TEELINE_TSPLIB_DIR, data/ or tests/golden/tsplib/ (the
    reference fetches pr1002 / usa13509 with download_data.sh; they are not in its tree and there is no network here) — else the
    labelled synthetic stand-in of equal n.  Returns (xy in file order, label)."""
    for d in (os.environ.get("TEELINE_TSPLIB_DIR"), os.path.join(ROOT, "data"), os.path.join(ROOT, "tests", "golden", "tsplib")):
        if d and os.path.exists(os.path.join(d, name + ".tsp")):
            t = TA.tsplib.read_from_file(os.path.join(d, name + ".tsp"))
            if len(t.xy) == n:
                return np.ascontiguousarray(t.xy, dtype=np.float32), f"{name}.tsp ({os.path.join(d, name + '.tsp')})"
    return TA.synth.synth_xy(n), f"synthetic EUC_2D n={n} stand-in for {name}.tsp (the file is not in the reference tree)"


def latest_profile(pattern):
    import glob
    f = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return f[-1] if f else None


def scan_valu_roofline(kernel, n, ms, info, clock_hz, also=()):
    """VALU-issue roofline of a whole-chip scan kernel (3-opt / Or-opt find_best_move; a BEST_SWEEP sweep; an LK round): wave64 VALU
    instructions of ONE launch from the committed rocprofv3 PMC pass (profiles/rNN_scans_pmc.json, scripts/pmc_scans.sh: same instance,
    same tour, so the count is a property of the launch) over the time measured live here; peak = SIMDs x live clock / 2.
    `also`: further kernels of the same unit of work (the step kernel of a round), their instructions added.  None if no profile matches."""
    prof = latest_profile("r*_scans_pmc.json")
    if not prof or clock_hz <= 0:
        return None
    try:
        allp = json.load(open(prof))
        pj = allp.get(kernel)
        if not pj or pj.get("n") != n:
            return None
        simds = info["cus"] * SIMDS_PER_CU
        peak = simds * clock_hz / VALU_CYCLES_PER_WAVE_INST / 1e9
        insts = float(pj["SQ_INSTS_VALU"]) + sum(float(allp[k]["SQ_INSTS_VALU"]) for k in also if k in allp)
        ach = insts / (ms * 1e-3) / 1e9
        r = {"bound": "valu_issue", "achieved": ach, "peak": peak, "unit": "G wave64-VALU-instructions/s", "frac": ach / peak, "traffic": None,
             "kernel": " + ".join((kernel,) + tuple(also)), "kernel_ms": ms, "valu_insts_per_launch": insts, "source": os.path.relpath(prof, ROOT),
             "formula": "frac = SQ_INSTS_VALU / (simds * kernel_s * clock_hz / 2); clock = the headline kernel's live in-kernel clock of this run"}
        for k in ("SQ_INSTS_SALU", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_BUSY_CU_CYCLES", "kernel_ms_profiled", "kernel_ms_profiled_mean", "launches"):
            if k in pj:
                r.setdefault("pmc", {})[k] = pj[k]
        return r
    except Exception as exc:
        return {"source_error": repr(exc)}


def valu_roofline(n, R, seed, first, info, k_ms, clock_hz, work, cand_per_launch, launches):
    """What bounds k_two_opt_ref_lds is VALU issue, not HBM (the tour never leaves LDS: DESIGN.md §4.2).
    achieved = wave64 VALU instructions per launch / kernel time; peak = SIMDs x clock / 2 (a wave64 VALU instruction
    occupies a SIMD-32 for 2 cycles).  The instruction count is SQ_INSTS_VALU of a rocprofv3 --pmc pass over this same
    launch (profiles/rNN_valu_roofline.json): the launch is deterministic (seeded restarts), and the in-kernel work
    counters measured live here must equal the ones recorded with the PMC pass for the count to be used.  Kernel time
    and the shader clock are measured live."""
    simds = info["cus"] * SIMDS_PER_CU
    r = {"bound": "valu_issue", "achieved": None, "peak": None, "unit": "G wave64-VALU-instructions/s", "frac": None,
         "traffic": None, "kernel": "k_two_opt_ref_lds", "kernel_ms_avg": k_ms, "launches": launches,
         "simds": simds, "clock_mhz_live": clock_hz / 1e6,
         "formula": "frac = SQ_INSTS_VALU / (simds * kernel_s * clock_hz / 2)",
         "algorithmic_hbm_view": {"bytes_per_candidate": ALG_BYTES_PER_CANDIDATE,
                                  "GBps": cand_per_launch * ALG_BYTES_PER_CANDIDATE / (k_ms * 1e-3) / 1e9,
                                  "note": "SURVEY.md §8(d)'s 8 B per candidate against 8 TB/s would read above 1: the kernel "
                                          "does not move those bytes (tour in LDS, exact tile bounds), so HBM is not the bound"}}
    if clock_hz > 0:
        r["peak"] = simds * clock_hz / VALU_CYCLES_PER_WAVE_INST / 1e9
    prof = latest_profile("r*_valu_roofline.json")
    if prof and first == 0 and work["l1_candidates"]:
        try:
            pj = json.load(open(prof))
            r["source"] = os.path.relpath(prof, ROOT)
            # same batch, same work: the speculative tiles a wave decides past the row's first hit depend on wave timing, so
            # the counters (and SQ_INSTS_VALU) of two launches of the same batch differ by a few 0.1 %: 2 % tolerance
            pw = pj.get("work", {})
            same = (pj.get("n") == n and pj.get("restarts") == R and pj.get("seed") == seed and
                    all(abs(int(pw.get(k, -1)) - work[k]) <= 0.02 * max(work[k], 1) for k in ("l0_tile_bounds", "l1_candidates", "l2_candidates")))
            r["work_matches_profile"] = bool(same)
            if same and r["peak"]:
                insts = float(pj["SQ_INSTS_VALU"])
                r["valu_insts_per_launch"] = insts
                r["achieved"] = insts / (k_ms * 1e-3) / 1e9
                r["frac"] = r["achieved"] / r["peak"]
                r["traffic"] = pj.get("hbm_traffic_bytes_per_launch")
                for k in ("SQ_INSTS_VALU_TRANS_F32", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY",
                          "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CU_CYCLES"):
                    if k in pj:
                        r.setdefault("pmc", {})[k] = pj[k]
                if "SQ_INSTS_SALU" in pj and clock_hz > 0:
                    # the scalar pipe beside the vector one: a SIMD issues one scalar instruction per 4 cycles at best (16.3 cycles per
                    # instruction with four waves per SIMD each running a dependent scalar chain: tests/probes/step_sync_probe.hip,
                    # profiles/r03_step_sync_probe.jsonl), i.e. one per cycle per CU
                    salu = float(pj["SQ_INSTS_SALU"]) / (k_ms * 1e-3)
                    salu_peak = info["cus"] * clock_hz
                    r["salu_issue"] = {"achieved": salu / 1e9, "peak": salu_peak / 1e9, "unit": "G SALU-instructions/s", "frac": salu / salu_peak,
                                       "formula": "SQ_INSTS_SALU / (cus * kernel_s * clock_hz): one scalar issue per cycle per CU"}
                    # SIMD issue slots taken by both pipes together if they did not overlap (VALU 2 cycles, SALU 4 cycles of a SIMD)
                    r["simd_issue_frac_valu_plus_salu"] = (insts * 2.0 + float(pj["SQ_INSTS_SALU"]) * 4.0) / (simds * k_ms * 1e-3 * clock_hz)
                    r["binding_pipe"] = "salu_issue" if r["salu_issue"]["frac"] > r["frac"] else "valu_issue"
        except Exception as exc:  # a malformed profile file must not break the bench line
            r["source_error"] = repr(exc)
    return r


def write_tsplib(path, name, xy):
    """EUC_2D TSPLIB file whose coordinates read back (strtof, tsplib.rs:356-377) as exactly these f32 values."""
    with open(path, "w") as fh:
        fh.write(f"NAME : {name}\nTYPE : TSP\nDIMENSION : {len(xy)}\nEDGE_WEIGHT_TYPE : EUC_2D\nNODE_COORD_SECTION\n")
        for k, (x, y) in enumerate(np.asarray(xy, dtype=np.float32), 1):
            fh.write(f"{k} {float(x):.9g} {float(y):.9g}\n")
        fh.write("EOF\n")


def drop_in_end_to_end(TA, with_cpu):
    """What a user of the drop-in sees (BASELINE configs[0] is "berlin52 via teeline-cli", which the reference does
    in 0.01 s, docs/benchmarks.md:28): `teeline-gpu pipeline --steps=nn,2opt -i FILE` as a FRESH process, its wall split into process
    start + exit, reading the file, tl_create, the first (cold) run of the stage list, a steady run and the kernels' own time
    (teeline_gpu_cli.cpp --timing --repeat 3) — beside the oracle doing the same nn -> 2opt on one host core.  Same tour cost asserted."""
    import subprocess
    import tempfile
    from teeline_amd import build as B
    cli = B.CLI if os.path.exists(B.CLI) else B.build_cli()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    O = None
    if with_cpu:
        import _oracle as O
    # what starting ANY process costs from here (this interpreter is a large parent: fork + exec + pipes), measured with /bin/true
    spawn = []
    for _ in range(5):
        t0 = time.perf_counter()
        subprocess.run(["/bin/true"], capture_output=True)
        spawn.append((time.perf_counter() - t0) * 1e3)
    spawn_ms = float(np.median(spawn))
    rows = {}
    sizes = [("berlin52", None), ("synthetic_n200", 200), ("synthetic_n500", 500), ("synthetic_n1002", 1002), ("synthetic_n2000", 2000),
             ("synthetic_n5000", 5000), ("synthetic_n10000", 10000)]
    with tempfile.TemporaryDirectory(prefix="teeline_e2e_") as tmp:
        for name, n in sizes:
            if n is None:
                f = os.path.join(ROOT, "tests", "golden", "tsplib", "berlin52.tsp")
                xy = np.ascontiguousarray(TA.tsplib.read_from_file(f).xy, dtype=np.float32)
            else:
                xy = TA.synth.synth_xy(n)
                f = os.path.join(tmp, name + ".tsp")
                write_tsplib(f, name, xy)
            cmd = [cli, "pipeline", "--steps=nn,2opt", "-i", f, "--timing", "--repeat", "3"]
            best = None
            for _ in range(2):  # the second process start finds the library and the file in the page cache
                t0 = time.perf_counter()
                pr = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                wall = (time.perf_counter() - t0) * 1e3
                if pr.returncode != 0:
                    raise RuntimeError(f"{' '.join(cmd)}: rc {pr.returncode}: {pr.stderr[-300:]}")
                tj = json.loads([ln for ln in pr.stderr.splitlines() if ln.startswith('{"timing_ms"')][-1])["timing_ms"]
                if best is None or wall < best[0]:
                    best = (wall, tj, pr.stdout)
            wall, tj, stdout = best
            runs = tj["runs"]
            steady = min(runs[1:], key=lambda r: r["wall_ms"])
            extra = sum(r["wall_ms"] for r in runs[1:])
            row = {"n": int(len(xy)), "fresh_process_wall_ms": wall - extra - spawn_ms,
                   "process_start_ms": tj.get("before_main"), "process_exit_ms": wall - spawn_ms - tj["main_total"] - max(tj.get("before_main", 0.0), 0.0),
                   "read_input_ms": tj["read_input"], "tl_create_ms": tj["tl_create"],
                   "first_call_ms": runs[0]["wall_ms"], "steady_call_ms": steady["wall_ms"],
                   "steady_kernel_ms": sum(st["kernel_ms"] for st in steady["stages"]), "output_ms": tj["output"],
                   "first_call_stages_ms": {st["solver"]: st["wall_ms"] for st in runs[0]["stages"]},
                   "steady_call_stages_ms": {st["solver"]: st["wall_ms"] for st in steady["stages"]},
                   "cost": stdout.split()[0]}
            if O is not None:
                t0 = time.perf_counter()
                _rc, nn_route, _c = O.nearest_neighbor(xy, None, len(xy), 3)
                _rc, _route, cost, _st = O.two_opt(xy, None, len(xy), init=nn_route)
                row["oracle_one_core_ms"] = (time.perf_counter() - t0) * 1e3
                assert f"{float(cost):.5f}" == row["cost"], f"{name}: CLI cost {row['cost']} != oracle {float(cost):.5f}"
                row["fresh_process_vs_one_core"] = row["oracle_one_core_ms"] / row["fresh_process_wall_ms"]
                row["steady_call_vs_one_core"] = row["oracle_one_core_ms"] / row["steady_call_ms"]
            if n == 1002:  # what leaving through exit() (the HIP runtime's static teardown) would add: the CLI leaves through _exit
                t0 = time.perf_counter()
                subprocess.run(cmd + ["--full-exit"], capture_output=True, text=True, timeout=300)
                row["wall_ms_with_full_exit"] = (time.perf_counter() - t0) * 1e3 - extra - spawn_ms
            rows[name] = row
    out = {"command": "teeline_amd/teeline-gpu pipeline --steps=nn,2opt -i FILE --timing --repeat 3 (fresh process; best of two starts)", "instances": rows,
           "spawn_overhead_ms": spawn_ms,
           "note": "fresh_process_wall_ms = the process's wall with ONE run of the stage list (the two extra --repeat runs and spawn_overhead_ms — what "
                   "starting /bin/true costs from this interpreter — subtracted); process_start_ms = "
                   "exec to main() (dynamic loading of libamdhip64 and libteeline_gpu, 10 ms resolution), process_exit_ms = the rest outside main(); "
                   "first_call = cold run (code-object load of the kernels used, workspace allocation, LDS attribute), steady_call = a later run "
                   "in the same process (what a long-lived caller such as teeline-api pays per request)"}
    if O is not None:
        order = sorted(rows.values(), key=lambda r: r["n"])
        cf = [r["n"] for r in order if r["fresh_process_vs_one_core"] > 1.0]
        cs = [r["n"] for r in order if r["steady_call_vs_one_core"] > 1.0]
        out["crossover_n_fresh_process"] = cf[0] if cf else None
        out["crossover_n_steady_call"] = cs[0] if cs else None
        out["cpu_baseline"] = {"kind": "port", "cores": 1, "unit": "ms per nn -> 2opt pipeline", "sample": "the oracle's nearest_neighbor + two_opt on the same "
                               "instance, one core, in-process (no process start, no file parse): oracle_one_core_ms per instance; same final cost asserted"}
    return out


METRIC = "2-opt candidate swaps evaluated/sec + final tour cost, TSPLIB EUC_2D n=10000"
STRONG_TOTAL = 256  # BASELINE.json configs[3]: "256 random restarts sharded 1/2/4/8 GPUs"
XCU_ROUND_US = (1.4, 2.1)  # profiles/r02_xcu_sync_probe.json: one cross-CU agreement round (flag in L2 / device-scope atomic), measured
SCALING_NOTE = ("value / weak_per_gpu = R restarts PER GPU (one descent per CU; weak scaling, the headline); strong_256_total = 256 restarts IN ALL "
                "dealt over the ranks (configs[3] as worded).  The strong reading is flat by design: a descent is sequential and holds one CU, a batch "
                "lasts as long as its slowest descent whether a GPU runs 256 or 32, so efficiency ~1/N.  Spreading ONE descent over CUs does not pay: "
                "a cross-CU round costs 1.4-2.1 us among <= 32 workgroups (profiles/r02_xcu_sync_probe.json) — about one whole 2.2 us step — and ~10 us among 256 (NOTEBOOK r5.6)")

LINE_LIMIT = 4096  # the driver stopped parsing the line when it grew to 22 KB; the LAST stdout line stays below this
SIDECAR = "bench_extras.json"


def _round_floats(o, sig=7):
    """floats to `sig` significant digits (the line is a report, not a checkpoint); containers walked."""
    if isinstance(o, float):
        return float(f"{o:.{sig}g}") if o == o and abs(o) != float("inf") else None
    if isinstance(o, dict):
        return {k: _round_floats(v, sig) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_round_floats(v, sig) for v in o]
    return o


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(full):
    """The ONE line the driver parses: the contract's keys, `roofline` and `cpu_baseline` in short form, the like-for-like rates and
    the parity record.  Everything else (extras, per-level counters, notes) lives in the sidecar / the EXTRAS lines.  Asserted
    <= LINE_LIMIT bytes by emit()."""
    out = _pick(full, ("metric", "value", "unit", "n_gpus", "ranks_seen", "devices_driven", "steps", "warmup", "ms_per_step", "ms_per_step_per_rank", "launcher",
                       "higher_is_better", "dry_launch", "scaling", "vs_baseline", "dtype", "data"))
    cfg = full.get("config") or {}
    out["config"] = _pick(cfg, ("workload", "n", "restarts_per_gpu", "restarts_total", "mode", "restart_seed", "launcher"))
    if len(out["config"].get("workload", "")) > 260:
        out["config"]["workload"] = out["config"]["workload"][:257] + "..."
    out.update(_pick(full, ("final_tour_cost", "best_restart", "stub_units_all_ranks")))
    r = full.get("roofline")
    if isinstance(r, dict):
        rr = _pick(r, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms_avg", "launches", "simds", "clock_mhz_live",
                       "source", "work_matches_profile", "binding_pipe", "simd_issue_frac_valu_plus_salu"))
        if isinstance(r.get("salu_issue"), dict):
            rr["salu_issue"] = _pick(r["salu_issue"], ("frac",))
        pmc = r.get("pmc") or {}
        if pmc.get("SQ_WAVE_CYCLES") and pmc.get("SQ_WAIT_ANY") is not None:
            rr["wait_any_frac"] = float(pmc["SQ_WAIT_ANY"]) / float(pmc["SQ_WAVE_CYCLES"])
        if isinstance(r.get("algorithmic_hbm_view"), dict):
            rr["algorithmic_hbm_GBps_at_8B_per_candidate"] = r["algorithmic_hbm_view"].get("GBps")
        out["roofline"] = rr
    else:
        out["roofline"] = r
    c = full.get("cpu_baseline")
    if isinstance(c, dict):
        cc = _pick(c, ("value", "unit", "cores", "kind", "sample", "per_core"))
        if len(cc.get("sample", "")) > 240:
            cc["sample"] = cc["sample"][:237] + "..."
        if isinstance(c.get("ref_faithful_1core"), dict):
            cc["ref_faithful_1core"] = _pick(c["ref_faithful_1core"], ("value",))
        out["cpu_baseline"] = cc
    else:
        out["cpu_baseline"] = c
    for k in ("value_l1_evaluated", "value_every_candidate_exact", "value_with_two_descents_per_cu"):
        if isinstance(full.get(k), dict):
            out[k] = _pick(full[k], ("value", "restarts_per_gpu"))
    for k, v in full.items():
        if k == "weak_per_gpu" or (k.startswith("strong_") and k.endswith("_total")):
            out[k] = _pick(v, ("ms_per_step", "value", "restarts_per_rank", "final_tour_cost", "best_restart", "stub_units_all_ranks", "cross_cu_round_us")) if isinstance(v, dict) else v
    out.update(_pick(full, ("scaling_note", "candidates_per_step_per_gpu", "descents_not_converged", "device", "parity_checked_restarts", "parity_mismatches")))
    if isinstance(out.get("parity_mismatches"), list) and len(out["parity_mismatches"]) > 2:
        out["parity_mismatches"] = out["parity_mismatches"][:2] + [f"... {len(full['parity_mismatches'])} in all: see {SIDECAR}"]
    ex = full.get("extras")
    if isinstance(ex, dict):
        out["extras_file"] = SIDECAR
        out["extras_keys"] = sorted(ex.keys())
        if "error" in ex:
            out["extras_error"] = str(ex["error"])[:200]
    return _round_floats(out)


def emit(full, stream=None):
    """Print the result: first the long material — one `EXTRAS {...}` line per extra (and one for the headline's long objects), also
    written whole to ./bench_extras.json (and gpurun_out/ where that exists) — then, LAST, the compact line, asserted <= LINE_LIMIT."""
    stream = stream or sys.stdout
    line = json.dumps(compact_line(full), separators=(",", ":"))
    if len(line.encode()) > LINE_LIMIT:
        raise SystemExit(f"bench.py: the result line is {len(line.encode())} bytes (> {LINE_LIMIT}): move material to the sidecar")
    side = _round_floats(full, 9)
    for d in (os.getcwd(), os.path.join(ROOT, "gpurun_out")):
        try:
            if "extras" in side and os.path.isdir(d) and os.access(d, os.W_OK):
                with open(os.path.join(d, SIDECAR), "w") as fh:
                    json.dump(side, fh, indent=1)
        except OSError:
            pass
    ex = side.get("extras") if isinstance(side.get("extras"), dict) else {}
    for k, v in ex.items():
        print("EXTRAS " + json.dumps({k: v}, separators=(",", ":")), file=stream)
    head = {k: side[k] for k in ("roofline", "cpu_baseline", "candidates_touched", "config") if k in side}
    if head:
        print("EXTRAS " + json.dumps({"headline_detail": head}, separators=(",", ":")), file=stream)
    print(line, file=stream)
    stream.flush()
    return line


DUMP_LIMIT = 64 << 20  # bytes of .npy data --dump-outputs may write in all


def dump_outputs(d, seed, d_pos, d_cost, d_stats, best_tour, best_cost, best_restart):
    """--dump-outputs DIR: what tl_two_opt_batch_dev and the collective handed back in the last timed step, on rank 0:
    tours.npy (restarts x n city ids, f32: exact below 2^24), costs.npy (f32), descent_stats.npy (sweeps, moves, reversed, status
    per descent, f64: the deterministic words; the rest are clocks and speculative-work counters), best_tour.npy (the winner's
    tour every rank receives, f32) and best.npy (its cost and restart id, f64).  Past DUMP_LIMIT the tours are a fixed sample of
    rows drawn with the restart seed, listed in tour_rows.npy."""
    os.makedirs(d, exist_ok=True)
    R, n = d_pos.shape
    assert n < (1 << 24)
    rows = np.arange(R)
    keep = (DUMP_LIMIT - (1 << 20)) // (4 * n)  # 1 MB left for the small arrays
    if R > keep:
        rows = np.sort(np.random.default_rng(seed).choice(R, keep, replace=False))
        np.save(os.path.join(d, "tour_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(d, "tours.npy"), d_pos[torch.from_numpy(rows).to(d_pos.device)].cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "costs.npy"), d_cost.cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "descent_stats.npy"), d_stats[:, :4].cpu().numpy().astype(np.float64))
    np.save(os.path.join(d, "best_tour.npy"), best_tour.cpu().numpy().astype(np.float32))
    np.save(os.path.join(d, "best.npy"), np.array([best_cost, best_restart], dtype=np.float64))


def gather_rank_ms(ms_local, device, dist):
    """every rank's own ms_per_step, in rank order (the headline ms_per_step is their maximum)."""
    t = torch.tensor([float(ms_local)], dtype=torch.float64, device=device)
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return [float(t.item())]
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [float(o.item()) for o in out]


def dry_launch(a, rank, world):
    """The N-rank plumbing without a GPU: gloo process group, the same sharding, key packing, min-all-reduce, tour hand-round
    and whole-job aggregation as a real run, around a STUB step (deterministic fake costs; no kernel, no oracle).  What it
    proves is the launch path and the rank count — the printed line carries value null and "dry_launch": true."""
    import torch.distributed as dist
    from teeline_amd.host import multistart as ms
    dev = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = dist.get_world_size() if world > 1 else 1
    if seen != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the process group has {seen} ranks")
    n = 64

    def stub_loop(first, R):
        """the collectives of a..steps steps around the stub costs of restarts [first, first + R)"""
        ids = torch.arange(first, first + R, dtype=torch.int64)
        costs = (((ids * 3 + 1) % 8) + ids // 8).to(torch.float32) + 1.0       # stub: a fixed cost per restart id (restart 5 wins)
        tours = torch.stack([torch.roll(torch.arange(n, dtype=torch.int32), int(r)) for r in ids.tolist()]) if R else torch.zeros((0, n), dtype=torch.int32)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            keys = ms.pack_keys(costs, first)
            best = ms.allreduce_best(keys, dist if world > 1 else None)
            tour = ms.share_best_tour(keys, tours, best, dist if world > 1 else None)
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        total, dt_max = ms.aggregate_throughput(R * a.steps, dt, dev, dist if world > 1 else None)
        return best, tour, dt, total, dt_max, R

    strong_total = a.restarts_total if a.restarts_total > 0 else STRONG_TOTAL
    first, R = ms.shard_total(rank, world, a.restarts_total) if a.restarts_total > 0 else ms.shard(rank, 4)
    best, tour, dt, total, dt_max, R = stub_loop(first, R)
    per_rank = gather_rank_ms(dt / max(a.steps, 1) * 1e3, dev, dist if world > 1 else None)
    # the second reading of the same line: configs[3] as worded — a fixed total dealt over the ranks
    sf, sR = ms.shard_total(rank, world, strong_total)
    _b2, _t2, _dt2, s_total, s_dt_max, _ = stub_loop(sf, sR)
    cost, restart = ms.unpack_key(best.item())
    ok = tour.tolist() == torch.roll(torch.arange(n, dtype=torch.int32), int(restart)).tolist()
    if world > 1:
        dist.destroy_process_group()
    if not ok:
        raise SystemExit("bench.py --dry-launch: the shared tour is not the winner's")
    if rank == 0:
        emit({"metric": METRIC, "value": None, "unit": "candidates/s", "n_gpus": world, "ranks_seen": seen,
                          "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt_max / max(a.steps, 1) * 1e3,
                          "ms_per_step_per_rank": per_rank, "higher_is_better": True, "dry_launch": True,
                          "scaling": "strong" if a.restarts_total > 0 else "weak", "vs_baseline": None, "dtype": "f32",
                          "data": "stub", "config": {"workload": "dry launch: gloo ranks, stub step (no GPU, no kernel, no oracle) — not a measurement"},
                          "stub_units_all_ranks": total, "best_restart": restart, "launcher": "torch.distributed.run" if world > 1 else "none",
                          "weak_per_gpu": {"ms_per_step": dt_max / max(a.steps, 1) * 1e3, "value": None, "restarts_per_rank": R},
                          f"strong_{strong_total}_total": {"ms_per_step": s_dt_max / max(a.steps, 1) * 1e3, "value": None, "restarts_per_rank": sR,
                                                           "stub_units_all_ranks": s_total, "cross_cu_round_us": list(XCU_ROUND_US)},
                          "scaling_note": SCALING_NOTE})


def single_process(a):
    """--single-process: ONE process, one tl_ctx per device, the restarts dealt over them by tl_two_opt_multistart_devices
    (no RCCL: the minimum of N packed keys is taken on the host inside the library).  The cross-check of the RCCL number and
    the fallback where no launcher is available.  The entry takes host buffers (80 KB of coordinates up, costs / counters and the
    winner's tour down per call), so this rate includes that PCIe traffic."""
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: libteeline_gpu has no CPU fallback")
    if torch.cuda.device_count() < a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but {torch.cuda.device_count()} device(s) visible")
    import teeline_amd as TA
    n = a.n
    xy = TA.synth.synth_xy(n)
    prob = TA.TspProblem(np.arange(n), xy)
    ctxs = [TA.Context(d, TA.TL_FLAG_MULTISTART_RCCL if (a.rccl_in_library and d == 0) else 0) for d in range(a.gpus)]
    strong = a.restarts_total > 0
    count = a.restarts_total if strong else a.restarts * a.gpus
    per_sweep = (n - 3) * (n - 2) // 2
    for _ in range(max(a.warmup, 0)):
        TA.two_opt.multistart_devices(prob, count, ctxs, seed=a.seed)
    cands, kms = 0, []
    t0 = time.perf_counter()
    for _ in range(a.steps):
        sol = TA.two_opt.multistart_devices(prob, count, ctxs, seed=a.seed)
        cands += sol.stats["sweeps"] * per_sweep
        kms.append(sol.stats["kernel_ms"])
    dt = time.perf_counter() - t0
    info = ctxs[0].device_info()
    emit({
        "metric": METRIC, "value": cands / dt, "unit": "candidates/s", "n_gpus": a.gpus, "ranks_seen": 1, "devices_driven": a.gpus,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True,
        "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"configs[3]: synthetic EUC_2D n={n}, multi-start REF_ORDER 2-opt, {count} seeded random restarts dealt over "
                               f"{a.gpus} device(s) by ONE process (tl_two_opt_multistart_devices; " +
                               ("the library's RCCL collective: key min-all-reduce + broadcast of the winner's tour)" if a.rccl_in_library
                                else f"no collective: host min of {a.gpus} keys)"),
                   "n": n, "restarts_total": count, "mode": "REF_ORDER", "restart_seed": a.seed,
                   "launcher": "single-process" + (" + RCCL inside the library" if a.rccl_in_library else "")},
        "final_tour_cost": float(sol.total), "best_restart": sol.stats["best_restart"],
        "slowest_shard_kernel_ms": float(np.mean(kms)), "device": info,
        "note": "host-buffer entry: the rate includes the per-call PCIe traffic (coordinates up; costs, counters and the winner's tour down)",
        "roofline": None, "cpu_baseline": None})
    for c in ctxs:
        c.close()


def main():
    a = parse()
    launched = "WORLD_SIZE" in os.environ
    if (a.gpus > 1 or a.force_launcher) and not launched and not a.single_process:
        # started bare: be the launcher (before any torch.cuda / teeline_amd call in this process)
        raise SystemExit(self_launch(a))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.single_process:
        if world > 1:
            raise SystemExit("--single-process under a multi-rank launcher")
        return single_process(a)
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: refusing to report a {world}-rank run as {a.gpus} GPUs")
    if a.dry_launch:
        return dry_launch(a, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: libteeline_gpu has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or os.environ.get("TL_BENCH_FORCE_DIST"):  # the env override exercises the RCCL path with one rank
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    import teeline_amd as TA
    from teeline_amd import _capi
    n = a.n
    strong = a.restarts_total > 0
    if strong:
        first, R = TA.multistart.shard_total(rank, world, a.restarts_total)
    else:
        first, R = TA.multistart.shard(rank, a.restarts)
    if R == 0:
        raise SystemExit(f"--restarts-total {a.restarts_total} leaves rank {rank} without a restart")
    xy = TA.synth.synth_xy(n)
    ctx = TA.Context(local)
    info = ctx.device_info()
    lib, h = ctx.lib, ctx.handle

    d_xy = torch.from_numpy(xy).to(dev)
    per_sweep = (n - 3) * (n - 2) // 2
    # Everything of a step is enqueued on ONE explicit stream: the descent kernel (through the C ABI), the key packing
    # and the collective.  (A NULL stream would mean the context's own non-blocking stream, unordered with torch's.)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    if dist is not None:  # RCCL communicator set-up (lazy on the first collective) is not part of any timed step
        with torch.cuda.stream(stream):
            dist.all_reduce(torch.zeros(1, dtype=torch.int64, device=dev), op=dist.ReduceOp.MIN)

    def timed_loop(first, R, steps, warmup):
        """warmup untimed + exactly `steps` timed steps of restarts [first, first + R) on this rank, bracketed by barrier +
        synchronize on both sides.  A rank without restarts (strong reading, more ranks than restarts) still takes part in
        every collective."""
        d_pos = torch.empty((max(R, 1), n), dtype=torch.int32, device=dev)
        d_cost = torch.full((max(R, 1),), float("inf"), dtype=torch.float32, device=dev)
        d_stats = torch.zeros((max(R, 1), _capi.TL_DEV_STATS_STRIDE), dtype=torch.int64, device=dev)
        sweeps_dev = torch.zeros((), dtype=torch.int64, device=dev)
        best_tour = [None]

        def step(events=None):
            with torch.cuda.stream(stream):
                if events is not None:
                    events[0].record(stream)
                if R:
                    ctx.check(lib.tl_two_opt_batch_dev(h, d_xy.data_ptr(), n, None, a.seed, first, R, _capi.TL_MODE_REF_ORDER,
                                                       d_pos.data_ptr(), d_cost.data_ptr(), d_stats.data_ptr(),
                                                       C.c_void_p(stream.cuda_stream)))
                if events is not None:
                    events[1].record(stream)
                sweeps_dev.add_(d_stats[:, 0].sum())
                # RCCL over xGMI: one 8-byte min-all-reduce per round, then the winner's tour (n x 4 B) to every rank
                keys = TA.multistart.pack_keys(d_cost, first)
                best = TA.multistart.allreduce_best(keys, dist)
                best_tour[0] = TA.multistart.share_best_tour(keys, d_pos, best, dist)
                return best

        for _ in range(max(warmup, 0)):
            step()
        sync()
        sweeps_dev.zero_()
        sync()
        # HIP events around every launch, on the stream the kernel is launched on
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        t0 = time.perf_counter()
        for k in range(steps):
            key = step(events=evs[k])
        sync()
        dt = time.perf_counter() - t0
        return {"dt": dt, "kernel_ms": [e0.elapsed_time(e1) for e0, e1 in evs], "cands": int(sweeps_dev.item()) * per_sweep, "key": key,
                "d_pos": d_pos, "d_cost": d_cost, "d_stats": d_stats, "best_tour": best_tour[0], "R": R, "first": first}

    L = timed_loop(first, R, a.steps, a.warmup)
    dt, kernel_ms, cands, key = L["dt"], L["kernel_ms"], L["cands"], L["key"]
    d_pos, d_cost, d_stats, best_tour = L["d_pos"], L["d_cost"], L["d_stats"], [L["best_tour"]]
    st_host = d_stats.cpu().numpy().astype(np.uint64)       # the last launch (every launch does the same work)
    cost_host = d_cost.cpu().numpy()
    # The clock the CUs held: st[9] shader clocks over st[10] ticks of the constant 100 MHz reference, per descent.
    # The work the cascade really did: one more launch of the same batch, UNTIMED, with the counting instantiation of the
    # kernel (TL_FLAG_COUNT_WORK; the counters cost ~8 %, so the timed kernel does not carry them): st[5..8].
    work = {"l0_tile_bounds": 0, "l1_candidates": 0, "l2_candidates": 0, "l3_candidates": 0}
    if a.full and not a.no_work_count:
        with TA.Context(local, TA.TL_FLAG_COUNT_WORK) as cc:
            d_pos2, d_cost2, d_stats2 = torch.empty_like(d_pos), torch.empty_like(d_cost), torch.zeros_like(d_stats)
            with torch.cuda.stream(stream):
                cc.check(lib.tl_two_opt_batch_dev(cc.handle, d_xy.data_ptr(), n, None, a.seed, first, R, _capi.TL_MODE_REF_ORDER,
                                                  d_pos2.data_ptr(), d_cost2.data_ptr(), d_stats2.data_ptr(),
                                                  C.c_void_p(stream.cuda_stream)))
            torch.cuda.synchronize()
            assert torch.equal(d_pos2, d_pos) and torch.equal(d_cost2, d_cost), "the counting kernel variant gave other tours"
            w = d_stats2.cpu().numpy().astype(np.uint64)
            work = {"l0_tile_bounds": int(w[:, 5].sum()), "l1_candidates": int(w[:, 6].sum()),
                    "l2_candidates": int(w[:, 7].sum()), "l3_candidates": int(w[:, 8].sum()),
                    "pruned_rows": int(w[:, 11].sum()), "pruned_row_tile_passes": int(w[:, 12].sum())}
    ticks = st_host[:, 10].astype(np.float64)
    clock_hz = float(np.mean(st_host[:, 9].astype(np.float64) / np.maximum(ticks, 1.0))) * REFCLK_HZ if ticks.min() > 0 else 0.0

    total, dt_max = TA.multistart.aggregate_throughput(cands, dt, dev, dist)
    ranks_seen = dist.get_world_size() if dist is not None else 1
    if ranks_seen != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the process group has {ranks_seen} ranks")
    per_rank_ms = gather_rank_ms(dt / a.steps * 1e3, dev, dist)
    best_cost, best_restart = TA.multistart.unpack_key(key.item())
    # The other reading of configs[3], in the same line: a FIXED total of restarts dealt over the ranks (strong scaling).  At one
    # GPU with the default 256 per GPU it is the timed loop above, word for word; otherwise (--full) a second timed loop of the same K steps.
    weak_obj = strong_obj = None
    if not strong:
        weak_obj = {"ms_per_step": dt_max / a.steps * 1e3, "value": total / dt_max, "restarts_per_rank": R}
        if world == 1 and R == STRONG_TOTAL:
            strong_obj = dict(weak_obj, note="one GPU: the same batch as the headline loop (not run twice)")
        elif a.full:
            sf, sR = TA.multistart.shard_total(rank, world, STRONG_TOTAL)
            S = timed_loop(sf, sR, a.steps, min(a.warmup, 1))
            s_total, s_dt_max = TA.multistart.aggregate_throughput(S["cands"], S["dt"], dev, dist)
            skey_cost, skey_restart = TA.multistart.unpack_key(S["key"].item())
            strong_obj = {"ms_per_step": s_dt_max / a.steps * 1e3, "value": s_total / s_dt_max, "restarts_per_rank": sR,
                          "final_tour_cost": skey_cost, "best_restart": skey_restart}
    else:
        strong_obj = {"ms_per_step": dt_max / a.steps * 1e3, "value": total / dt_max, "restarts_per_rank": R}

    if strong_obj is not None:
        strong_obj["cross_cu_round_us"] = list(XCU_ROUND_US)
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    if a.dump_outputs:
        dump_outputs(a.dump_outputs, a.seed, d_pos, d_cost, d_stats, best_tour[0], best_cost, best_restart)
    bt = best_tour[0].cpu().numpy()
    assert sorted(bt.tolist()) == list(range(n)), "the shared best tour is not a permutation"
    status_bad = int((d_stats[:, 3] != 0).sum().item())
    k_ms = float(np.mean(kernel_ms))
    cand_per_launch = cands / a.steps
    out = {
        "metric": METRIC,
        "value": total / dt_max,
        "unit": "candidates/s",
        "n_gpus": world, "ranks_seen": ranks_seen, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": dt_max / a.steps * 1e3, "ms_per_step_per_rank": per_rank_ms,
        "launcher": "torch.distributed.run" if "WORLD_SIZE" in os.environ else "none",
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"configs[2]/[3]: synthetic EUC_2D n={n} (xorshift64 seed 88172645463325252), multi-start "
                               f"REF_ORDER 2-opt to local optimum, {R} seeded random restarts per GPU (one descent per CU), "
                               f"on-the-fly f32 distances, tour resident in LDS",
                   "n": n, "restarts_per_gpu": R, "restarts_total": a.restarts_total if strong else R * world, "mode": "REF_ORDER",
                   "restart_seed": a.seed, "collective": "RCCL min-all-reduce of (cost_bits<<32|restart) per step + SUM-all-reduce of the winner's tour (n x 4 B)" if world > 1 else "none (1 GPU)"},
        "final_tour_cost": best_cost, "best_restart": best_restart,
        "weak_per_gpu": weak_obj,
        f"strong_{a.restarts_total if strong else STRONG_TOTAL}_total": strong_obj,
        "scaling_note": SCALING_NOTE,
        "candidates_per_step_per_gpu": cand_per_launch,
        "descents_not_converged": status_bad,
        "device": info,
        "roofline": None,
    }
    if a.full:
        out["candidates_touched"] = {
            **work,
            "l1_candidates_per_s": work["l1_candidates"] / (k_ms * 1e-3),
            "fraction_of_algorithmic": work["l1_candidates"] / max(cand_per_launch, 1.0),
            "note": "per launch, counted by the kernel's counting instantiation in one untimed launch of the same batch (same tours, "
                    "asserted): tile bounds evaluated by L0 (64 tiles per wave pass), candidates whose "
                    "squared-distance test L1 ran, candidates that went on to the v_sqrt_f32 test L2, and to the exact L3; "
                    "`value` counts candidates as the reference's loop visits them (SURVEY.md §8(d)), L0 decides most of "
                    "them a tile at a time",
        }
        out["value_l1_evaluated"] = {"value": out["candidates_touched"]["l1_candidates_per_s"], "unit": "candidates/s",
                                     "note": "candidates whose own squared-distance test (L1) ran, per second of kernel time — what is left after the tile bound L0"}
        out["roofline"] = valu_roofline(n, R, a.seed, first, info, k_ms, clock_hz, work, cand_per_launch, a.steps)
    if world == 1 and a.full and not a.no_extras:
        extras = {}
        try:  # the extras must never cost the run its headline line
            # Two descents per CU: with more restarts than CUs the library keeps the tours as grid coordinates (7 B per city instead
            # of 10; exact decode, checked per instance) so that two tours of n = 10^4 share a CU's LDS.  Same tours: the first R
            # restarts of the double batch must be the timed batch's.
            R2 = 2 * R
            d_pos2 = torch.empty((R2, n), dtype=torch.int32, device=dev)
            d_cost2 = torch.empty(R2, dtype=torch.float32, device=dev)
            d_stats2 = torch.zeros((R2, _capi.TL_DEV_STATS_STRIDE), dtype=torch.int64, device=dev)
            ms2 = []
            for _ in range(2):
                with torch.cuda.stream(stream):
                    ctx.check(lib.tl_two_opt_batch_dev(h, d_xy.data_ptr(), n, None, a.seed, first, R2, _capi.TL_MODE_REF_ORDER,
                                                       d_pos2.data_ptr(), d_cost2.data_ptr(), d_stats2.data_ptr(), C.c_void_p(stream.cuda_stream)))
                torch.cuda.synchronize()
                ms2.append(ctx.last_kernel_ms())
            assert torch.equal(d_pos2[:R], d_pos) and torch.equal(d_cost2[:R], d_cost), "the two-descents-per-CU batch gave other tours"
            cands2 = int(d_stats2[:, 0].sum().item()) * per_sweep
            extras["multistart_two_descents_per_cu"] = {"restarts": R2, "kernel_ms": min(ms2), "candidates_per_s": cands2 / (min(ms2) * 1e-3),
                                                        "vs_one_per_cu": (cands2 / (min(ms2) * 1e-3)) / (cand_per_launch / (k_ms * 1e-3)),
                                                        "note": "tl_two_opt_batch_dev with 2 x the CU count of restarts; first half bit-identical to the timed batch (asserted)"}
            # The late phase (from the sixth sweep on a row reads per-city neighbour lists instead of walking tiles, the rest of a sweep is
            # one step: teeline_amd/csrc/two_opt_nl.hip) against the same kernel without it, same batch, same tours.
            with TA.Context(local, TA.TL_FLAG_2OPT_NO_NL) as cn:
                ms3 = []
                for _ in range(2):
                    with torch.cuda.stream(stream):
                        cn.check(lib.tl_two_opt_batch_dev(cn.handle, d_xy.data_ptr(), n, None, a.seed, first, R, _capi.TL_MODE_REF_ORDER,
                                                          d_pos2.data_ptr(), d_cost2.data_ptr(), d_stats2.data_ptr(), C.c_void_p(stream.cuda_stream)))
                    torch.cuda.synchronize()
                    ms3.append(cn.last_kernel_ms())
                assert torch.equal(d_pos2[:R], d_pos) and torch.equal(d_cost2[:R], d_cost), "the tile-only kernel gave other tours"
            late_clk = (d_stats[:, 13] >> 24).double()
            extras["late_phase_neighbour_lists"] = {
                "kernel_ms_without": min(ms3), "kernel_ms_with": k_ms, "speedup": min(ms3) / k_ms,
                "late_phase_share_of_descent_cycles": {"mean": float((late_clk / d_stats[:, 9].double()).mean().item()),
                                                       "max": float((late_clk / d_stats[:, 9].double()).max().item())},
                "late_steps_per_descent_mean": float((d_stats[:, 14] >> 32).double().mean().item()),
                "note": "TL_FLAG_2OPT_NO_NL: every pruned row walks its tiles in every sweep (the round-3 kernel); default: the main loop's pruned rows stop at a posted "
                        "hit before every live tile and a reversal inside one tile folds its new edges into the tile's bound instead of a rebuild; the sweeps after one with fewer than n / 40 moves (here: from the sixth on) "
                        "decide a row from one 128-byte record pair (16 nearest of a, reverse 24-nearest of b) + the few cities with a long tour edge; "
                        "lists built once per instance (k_nl_knn, inside kernel_ms of the first call), validated on the device per call; same tours (asserted)"}
            prob = TA.TspProblem(np.arange(n), xy)
            init = TA.synth.restart_perm(n, a.seed, 0)
            sol = TA.two_opt.solve(prob, None, None, [int(v) for v in init], ctx=ctx)
            extras["single_descent_random_start"] = {"candidates_per_s": sol.stats["candidates"] / (sol.stats["kernel_ms"] * 1e-3),
                                                     "kernel_ms": sol.stats["kernel_ms"], "cost": float(sol.total),
                                                     "moves": sol.stats["moves"], "sweeps": sol.stats["sweeps"]}
            rc_nn = TA.nearest_neighbor.solve(prob, ctx=ctx)
            sol_g = TA.two_opt.solve(prob, None, None, rc_nn.route(), ctx=ctx)
            extras["single_descent_nn_start"] = {"candidates_per_s": sol_g.stats["candidates"] / (sol_g.stats["kernel_ms"] * 1e-3),
                                                 "kernel_ms": sol_g.stats["kernel_ms"], "cost": float(sol_g.total), "nn_cost": float(rc_nn.total),
                                                 "moves": sol_g.stats["moves"], "sweeps": sol_g.stats["sweeps"],
                                                 "note": "BASELINE configs[2]: one REF_ORDER descent from the NN seed on ONE CU; expected cost 77647.55469"}
            sol_b = TA.two_opt.solve(prob, None, None, rc_nn.route(), ctx=ctx, mode=TA.TL_MODE_BEST_SWEEP)
            bs_us = sol_b.stats["kernel_ms"] * 1e3 / max(sol_b.stats["sweeps"], 1)
            extras["best_sweep_nn_start"] = {"candidates_per_s": sol_b.stats["candidates"] / (sol_b.stats["kernel_ms"] * 1e-3),
                                             "kernel_ms": sol_b.stats["kernel_ms"], "cost": float(sol_b.total), "sweeps": sol_b.stats["sweeps"],
                                             "us_per_sweep": bs_us,
                                             "note": "TL_MODE_BEST_SWEEP (own mode, whole chip per sweep), single descent; a sweep = k_bs_scan + k_bs_apply",
                                             # measured: the VALU instructions of one sweep's two kernels (PMC pass, per-launch means) over the live time per sweep
                                             "roofline": scan_valu_roofline("k_bs_scan", n, bs_us * 1e-3, info, clock_hz, also=("k_bs_apply",)),
                                             # modelled, NOT a counter: what a sweep cannot go below as two dependent launches
                                             "latency_model": {"floor_us_per_sweep": 2 * 1.45, "frac": 2 * 1.45 / bs_us,
                                                               "source": "MI355X_MICROARCH.md price list, row `boundary`: 1.45 us between two dependent trivial kernels; "
                                                                         "a sweep is k_bs_scan -> k_bs_apply -> next k_bs_scan"}}
            if not a.no_cpu_baseline:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import _oracle as O
                nn_pos = np.asarray([int(v) for v in rc_nn.route()], dtype=np.uint32)
                cap_moves = 40  # bounded sample: ~50 M candidates per sweep on one core
                t0c = time.perf_counter()
                _rc, _p, _c, st_b = O.two_opt(xy, None, n, init=nn_pos, best=True, max_moves=cap_moves)
                wc = time.perf_counter() - t0c
                extras["best_sweep_nn_start"]["cpu_baseline"] = {
                    "value": st_b["candidates"] / wc, "unit": "candidates/s", "cores": 1, "kind": "port",
                    "sample": f"the first {st_b['sweeps']} sweeps ({st_b['moves']} moves) of the same BEST_SWEEP descent (NN start, n = {n}) by the "
                              f"oracle's tlo_two_opt_best on one core; wall {wc:.1f} s"}
            with TA.Context(local, TA.TL_FLAG_NO_PRUNE) as c2:
                s2 = TA.two_opt.multistart(prob, R, seed=a.seed, first=0, ctx=c2)
                s2 = TA.two_opt.multistart(prob, R, seed=a.seed, first=0, ctx=c2)
                extras["no_prune_multistart"] = {"candidates_per_s": s2.stats["candidates"] / (s2.stats["kernel_ms"] * 1e-3),
                                                 "kernel_ms": s2.stats["kernel_ms"], "best_cost": float(s2.total),
                                                 "note": "TL_FLAG_NO_PRUNE: every candidate decided with two fresh correctly rounded sqrt — the like-for-like "
                                                         "rate against a CPU loop that evaluates every candidate (the top-level cpu_baseline does)",
                                                 "roofline": scan_valu_roofline("k_two_opt_ref_lds_no_prune", n, s2.stats["kernel_ms"], info, clock_hz)}
                assert np.float32(s2.total).tobytes() == np.float32(best_cost).tobytes() or first != 0, "NO_PRUNE gave another best tour"
            for _ in range(3):  # warm-up: workspace allocation and first touch of its 200 MB, and the clock after the batches above
                dm, ms = TA.distance_matrix.build(np.arange(n), xy, ctx=ctx, return_ms=True)
            dm_ms = []
            for _ in range(10):
                dm, ms = TA.distance_matrix.build(np.arange(n), xy, ctx=ctx, return_ms=True)
                dm_ms.append(ms)
            ms = float(np.mean(dm_ms))
            gb = n * (n - 1) / 2 * 4 / 1e9
            extras["dm_build_packed"] = {"kernel_ms": ms, "kernel_ms_min": float(min(dm_ms)), "launches": len(dm_ms), "GBps": gb / (ms * 1e-3), "frac_of_hbm_peak": gb / (ms * 1e-3) / HBM_PEAK_GBPS,
                                         "bytes": n * (n - 1) // 2 * 4}
            # the HBM-bound kernel of the path (DistanceMatrix::build): a roofline object of its own, traffic from its PMC passes
            rdm = {"bound": "hbm", "achieved": gb / (ms * 1e-3), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": gb / (ms * 1e-3) / HBM_PEAK_GBPS,
                   "traffic": None, "kernel": "k_dm_build_packed_blocked", "kernel_ms_avg": ms,
                   "note": "4 B written per distance; a plain fill of the same 200 MB reaches 6.65 TB/s on this part (scripts/hbm_fill_probe.py), "
                           "row-blocked build: column coordinates loaded once per 4 rows (DESIGN.md §4.1)"}
            dpath = latest_profile("r*_dm_build_hbm_traffic.json")
            if dpath and n == 10000:
                try:
                    dj = json.load(open(dpath))
                    rdm["traffic"] = dj.get("traffic_bytes_per_launch")
                    rdm["traffic_source"] = dj.get("source")
                except Exception:
                    pass
            extras["dm_build_packed"]["roofline"] = rdm
            # BASELINE configs[1]: pr1002-sized instance (the file is not in the reference tree -> synthetic n = 1002, labelled),
            # full REF_ORDER sweep to the local optimum with every distance gathered from the fp32 matrix in HBM
            n2 = 1002
            xy2, label2 = instance_xy("pr1002", n2, TA)
            dm2 = TA.distance_matrix.build(np.arange(n2), xy2, ctx=ctx)
            pm2 = TA.TspProblem(np.arange(n2), xy2, TA.distance_matrix.DistanceMatrix(n2, dm2.items, np.arange(n2), "explicit"))
            nn2 = [int(v) for v in TA.nearest_neighbor.solve(TA.TspProblem(np.arange(n2), xy2), ctx=ctx).route()]
            cfg1 = {}
            for name, init in (("nn_start", nn2), ("identity_start", None)):
                for _ in range(2):
                    sm = TA.two_opt.solve(pm2, None, None, init, ctx=ctx)
                cps = sm.stats["candidates"] / (sm.stats["kernel_ms"] * 1e-3)
                cfg1[name] = {"kernel_ms": sm.stats["kernel_ms"], "candidates_per_s": cps, "cost": float(sm.total),
                              "sweeps": sm.stats["sweeps"], "moves": sm.stats["moves"],
                              "algorithmic_GBps_at_16B_per_candidate": cps * 16.0 / 1e9}
            # what the drop-in does with this instance: pr1002 is EUC_2D, so the shim's tl_dm_is_euc2d check on problem.distances
            # (integration/teeline-gpu/gpu.rs Boundary::matrix) sends it down the coordinate kernel — same tours, same costs (asserted)
            pc2 = TA.TspProblem(np.arange(n2), xy2)
            via = {}
            for name, init in (("nn_start", nn2), ("identity_start", None)):
                for _ in range(2):
                    sc = TA.two_opt.solve(pc2, None, None, init, ctx=ctx)
                sm = TA.two_opt.solve(pm2, None, None, init, ctx=ctx)
                assert list(sc.route()) == list(sm.route()) and np.float32(sc.total).tobytes() == np.float32(sm.total).tobytes(), "matrix form != coordinate form"
                via[name] = {"kernel_ms": sc.stats["kernel_ms"], "candidates_per_s": sc.stats["candidates"] / (sc.stats["kernel_ms"] * 1e-3)}
            cfg1["drop_in_route_for_euc2d_problems"] = dict(via, note="the matrix of an EUC_2D problem equals the on-the-fly f32 distances bit for bit; "
                                                                      "the shim checks that once per call (tl_dm_is_euc2d) and runs the coordinate kernel")
            # what a move costs here against what it can cost with one step per move.  The floor is MEASURED: the
            # coordinate kernel walks the very same descent (same tours, asserted above) with every operand in LDS — its time per
            # move is what the step around a move costs on this design with no matrix at all; 10^9 candidates/s from the identity
            # start would need 3.5e6 candidates / 1e9 = 3.5 ms over 5 003 moves = 0.70 us per move, below that floor.
            mv_id = max(cfg1["identity_start"]["moves"], 1)
            cfg1["us_per_move_identity_start"] = cfg1["identity_start"]["kernel_ms"] * 1e3 / mv_id
            cfg1["floor_us_per_move"] = via["identity_start"]["kernel_ms"] * 1e3 / mv_id
            cfg1["us_per_move_needed_for_1e9_per_s"] = cfg1["identity_start"]["sweeps"] * ((n2 - 3) * (n2 - 2) // 2) / 1e9 * 1e6 / mv_id
            cfg1["floor_note"] = ("floor_us_per_move = the coordinate kernel's time per move on the same descent (all operands in LDS, measured in this "
                                  "run); the matrix form adds one dependent L2 gather of the new b's row per move.  The 1e9 candidates/s target from the "
                                  "identity start needs us_per_move_needed_for_1e9_per_s, which is below the floor: unreachable with one step per move "
                                  "(round 4 built the coordinate kernel's deferred-row structure for this kernel — commit b6c7f95 — parity green, 7.82 ms "
                                  "against 7.74: not kept, NOTEBOOK.md)")
            cfg1["instance"] = label2
            cfg1["note"] = ("one descent = one workgroup on ONE CU; latency-bound (a step per move), the 4 MB full matrix stays in L2/MALL; "
                            "kernel_ms includes the packed -> full expansion")
            # the same kernel with the chip full: a population of 256 tours (the seeded restart permutations 0..255), one descent
            # per CU, every distance gathered from the one 4 MB matrix in L2 — the throughput form of configs[1]
            pop = [[int(v) for v in TA.synth.restart_perm(n2, a.seed, r)] for r in range(256)]
            for _ in range(2):
                sols = TA.two_opt.solve_population(pm2, pop, ctx=ctx)
            pst = sols[0].stats
            pcps = pst["candidates"] / (pst["kernel_ms"] * 1e-3)
            L2_GATHER_PEAK_GBPS = 17000.0  # MI355X_MICROARCH.md "Indexed rows": rows served from the XCDs' L2, 16.8-18.8 TB/s chip-wide
            cfg1["population_256_random_tours"] = {
                "kernel_ms": pst["kernel_ms"], "candidates_per_s": pcps, "moves": pst["moves"], "sweeps": pst["sweeps"],
                "best_cost": float(min(float(s_.total) for s_ in sols)),
                "roofline": {"bound": "l2_gather", "achieved": pcps * 16.0 / 1e9, "peak": L2_GATHER_PEAK_GBPS, "unit": "GB/s",
                             "frac": pcps * 16.0 / 1e9 / L2_GATHER_PEAK_GBPS, "traffic": None, "kernel": "k_two_opt_ref_dm",
                             "note": "16 algorithmic bytes per candidate (perm[j+1], D[a][c], D[b][e], D[c][e]; SURVEY.md §8(d)) against the "
                                     "L2-served gather rate of the guide; the descent is bound by the chain of dependent latencies of a "
                                     "step, not by that bandwidth"}}
            # round 5: the late sweeps on lists cut from the matrix rows (two_opt_dm.hip) — which sweeps took them, and the same runs with
            # the lists off (TL_FLAG_2OPT_NO_NL: the round-4 kernel's block shapes throughout); a larger matrix shows the n^2 / n gap
            for name, init in (("nn_start", nn2), ("identity_start", None)):
                TA.two_opt.solve(pm2, None, None, init, ctx=ctx)
                cnt = ctx.two_opt_last_counters()
                cfg1[name].update(steps=cnt[4], steps_on_lists=cnt[5], sweeps_on_lists=cnt[6], rows_walking_matrix_rows_wave0=cnt[7], rows_from_cached_records_wave0=cnt[8])
            with TA.Context(local, TA.TL_FLAG_2OPT_NO_NL) as c3:
                off = {}
                for name, init in (("nn_start", nn2), ("identity_start", None)):
                    for _ in range(2):
                        so = TA.two_opt.solve(pm2, None, None, init, ctx=c3)
                    assert list(so.route()) == list(TA.two_opt.solve(pm2, None, None, init, ctx=ctx).route()), "lists on / off: another tour"
                    off[name + "_kernel_ms"] = so.stats["kernel_ms"]
                for _ in range(2):
                    so = TA.two_opt.solve_population(pm2, pop, ctx=c3)
                off["population_256_kernel_ms"] = so[0].stats["kernel_ms"]
                cfg1["without_lists"] = off
                nb = 3000
                xyb = TA.synth.synth_xy(nb)
                dmb = TA.distance_matrix.build(np.arange(nb), xyb, ctx=ctx)
                pmb = TA.TspProblem(np.arange(nb), xyb, TA.distance_matrix.DistanceMatrix(nb, dmb.items, np.arange(nb), "explicit"))
                popb = [[int(v) for v in TA.synth.restart_perm(nb, a.seed, r)] for r in range(256)]
                big = {}
                for label, cx in (("with_lists", ctx), ("without_lists", c3)):
                    for _ in range(2):
                        sb = TA.two_opt.solve_population(pmb, popb, ctx=cx)
                    big[label] = {"kernel_ms": sb[0].stats["kernel_ms"], "candidates_per_s": sb[0].stats["candidates"] / (sb[0].stats["kernel_ms"] * 1e-3),
                                  "best_cost": float(min(float(s_.total) for s_ in sb))}
                assert big["with_lists"]["best_cost"] == big["without_lists"]["best_cost"]
                cfg1["population_256_n3000"] = big
            cfg1["lists_note"] = ("sweeps that follow one with at most n^2 / 4000 moves, while at most 1024 cities have a tour edge beyond their 16th-nearest distance, "
                                  "decide a row from a's 16 nearest, b's reverse list and the long cities (DESIGN.md §4.4); same tours, asserted")
            extras["two_opt_matrix_in_hbm_n1002"] = cfg1
            n3 = 1002
            p3 = TA.TspProblem(np.arange(n3), TA.synth.synth_xy(n3))
            nn3 = [int(v) for v in TA.nearest_neighbor.solve(p3, ctx=ctx).route()]
            TA.three_opt.find_best_move(p3, nn3, ctx=ctx)
            TA.three_opt.find_best_move(p3, nn3, ctx=ctx)
            ms3 = ctx.last_kernel_ms()
            tri = n3 * (n3 - 1) * (n3 - 2) // 6 - (n3 - 2)
            extras["three_opt_scan_n1002"] = {"triples_per_s": tri / (ms3 * 1e-3), "kernel_ms": ms3, "triples": tri,
                                              "roofline": scan_valu_roofline("k_three_opt_scan", n3, ms3, info, clock_hz)}
            if not a.no_cpu_baseline:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import _oracle as O
                t0c = time.perf_counter()
                omv = O.three_opt_find_best_move(p3.xy, None, np.asarray(nn3, dtype=np.uint32))
                wc = time.perf_counter() - t0c
                gmv = TA.three_opt.find_best_move(p3, nn3, ctx=ctx)
                assert gmv[:4] == omv[:4] and np.float32(gmv[4]).tobytes() == np.float32(omv[4]).tobytes(), "3-opt scan differs from the oracle"
                extras["three_opt_scan_n1002"]["cpu_baseline"] = {"value": tri / wc, "unit": "triples/s", "cores": 1, "kind": "port",
                                                                  "sample": f"the same scan (one find_best_move over all {tri} triples of the NN tour, n = {n3}) by the oracle on one core; wall {wc:.2f} s; same move and savings bits as the GPU's (asserted)"}
            n5 = 5000
            p5 = TA.TspProblem(np.arange(n5), TA.synth.synth_xy(n5))
            nn5 = [int(v) for v in TA.nearest_neighbor.solve(p5, ctx=ctx).route()]
            TA.or_opt.find_best_move(p5, nn5, ctx=ctx)
            TA.or_opt.find_best_move(p5, nn5, ctx=ctx)
            ms5 = ctx.last_kernel_ms()
            extras["or_opt_scan_n5000"] = {"placements_per_s": 6.0 * n5 * n5 / (ms5 * 1e-3), "kernel_ms": ms5,
                                           "placements": 6 * n5 * n5, "note": "3 segment lengths x n starts x n insertion points x {fwd, rev} (or_opt.rs:80-164)",
                                           "roofline": scan_valu_roofline("k_or_scan", n5, ms5, info, clock_hz)}
            if not a.no_cpu_baseline:
                t0c = time.perf_counter()
                omv5 = O.or_opt_find_best_move(p5.xy, None, np.asarray(nn5, dtype=np.uint32))
                wc = time.perf_counter() - t0c
                gmv5 = TA.or_opt.find_best_move(p5, nn5, ctx=ctx)
                assert (gmv5 is None) == (omv5 is None) and (gmv5 is None or tuple(gmv5[:4]) == tuple(omv5[:4])), "Or-opt scan differs from the oracle"
                extras["or_opt_scan_n5000"]["cpu_baseline"] = {"value": 6.0 * n5 * n5 / wc, "unit": "placements/s", "cores": 1, "kind": "port",
                                                               "sample": f"the same scan (one find_best_move, n = {n5}, NN tour) by the oracle on one core; wall {wc:.2f} s; same move as the GPU's (asserted)"}
            # BASELINE configs[4] size: Lin-Kernighan ILS at n = 13 509 (synthetic points), candidate lists through the kd-tree
            n13 = 13509
            xy13, label13 = instance_xy("usa13509", n13, TA)
            p13 = TA.TspProblem(np.arange(n13), xy13)
            lk_opts = TA.LKOptions(TA.HeuristicOptions(epochs=20, platoo_epochs=10, n_nearest=5), 5)
            TA.lin_kernighan.solve(p13, lk_opts, ctx=ctx, seed=1)
            slk = TA.lin_kernighan.solve(p13, lk_opts, ctx=ctx, seed=1)
            lk_ms, lk_rounds, lk_moves = slk.stats["kernel_ms"], slk.stats["sweeps"], slk.stats["moves"]
            # What bounds a round: it is a chain of dependent latencies, not bytes or flops — two dependent kernel boundaries (scan ->
            # step -> scan; 1.45 us each between trivial kernels: MI355X_MICROARCH.md price list, row "boundary") and, inside the
            # scan, the longest walk's dependent L2 look-ups (max_depth 5 levels x 3 look-ups x ~200 cycles at the live clock).
            lk_floor_us = 2 * 1.45 + 15 * 200.0 / max(clock_hz, 1.0) * 1e6
            extras["lin_kernighan_n13509_20_epochs"] = {"kernel_ms": lk_ms, "total_ms": slk.stats["total_ms"], "cost": float(slk.total),
                                                        "instance": label13, "scans": lk_rounds, "moves": lk_moves, "moves_per_s": lk_moves / (lk_ms * 1e-3),
                                                        "us_per_round": lk_ms * 1e3 / max(lk_rounds, 1),
                                                        # measured: VALU instructions of a round's kernels (PMC pass, per-launch means over the same run) over the live time per round
                                                        "roofline": scan_valu_roofline("k_lk_scan_sub", n13, lk_ms / max(lk_rounds, 1), info, clock_hz, also=("k_lk_control",)),
                                                        # modelled, NOT a counter: the chain of dependent latencies a round cannot go below
                                                        "latency_model": {"bound": "dependent_latency", "floor_us_per_round": lk_floor_us, "frac": lk_floor_us / (lk_ms * 1e3 / max(lk_rounds, 1)),
                                                                          "formula": "floor = 2 x 1.45 us kernel boundary + 15 dependent L2 look-ups x 200 cycles / live clock",
                                                                          "source": "constants from MI355X_MICROARCH.md (price list row `boundary`; L2 hit latency), not from a counter of this run"},
                                                        "note": "tl_lk incl. NN seed and k-NN lists; the same run is a golden-checked -m gpu test (tests/test_gpu_full_size.py)"}
            if not a.no_cpu_baseline:
                # CPU side of the same workload, bounded: ONE ILS epoch — a double-bridge kick of the GPU run's final tour, then the
                # oracle's lk_pass (lin_kernighan.rs:454-481) to the next local optimum — on one core; unit: applied moves per second
                final = np.asarray([int(v) for v in slk.route()], dtype=np.uint32)
                cand13 = TA.lin_kernighan.build_candidates(p13, 5, ctx=ctx) if hasattr(TA.lin_kernighan, "build_candidates") else O.build_candidates_kdtree(p13.xy, 5)[0]
                q13 = n13 // 4
                kicked = O.double_bridge(final, q13 // 3, q13 // 2, q13 - 7)
                t0c = time.perf_counter()
                _, _, st_lk = O.lk_pass(p13.xy, kicked, np.asarray(cand13, dtype=np.uint32), 5)
                wc = time.perf_counter() - t0c
                extras["lin_kernighan_n13509_20_epochs"]["cpu_baseline"] = {"value": st_lk["moves"] / wc, "unit": "moves/s", "cores": 1, "kind": "port",
                    "sample": f"one ILS epoch at n = {n13}: double-bridge kick of the GPU run's final tour, then the oracle's lk_pass to the next local optimum ({st_lk['moves']} moves, {st_lk['sweeps']} find_lk_move scans) on one core; wall {wc:.1f} s"}
            # LK on the instances the reference publishes wall times for (bench/baseline-solvers.tsv:17-31, docs/benchmarks.md:47), with the CLI's
            # defaults (mod.rs:596-613,1321-1325: epochs 10 000, platoo 500, n_nearest 3, depth 5): the LDS form with speculative epochs
            # (default at these sizes) beside the chip-wide scans, the oracle on one core and the reference's own published range
            pub = {}
            published_s = {"berlin52": [0.10, 0.22], "a280": [1.1, 3.1], "att532": [14.0, 37.0]}
            for nm in ("berlin52", "a280", "att532"):
                f = os.path.join(ROOT, "tests", "golden", "tsplib", nm + ".tsp")
                xyp = np.ascontiguousarray(TA.tsplib.read_from_file(f).xy, dtype=np.float32)
                pp = TA.TspProblem(np.arange(len(xyp)), xyp)
                lo = TA.LKOptions(TA.HeuristicOptions(epochs=10000, platoo_epochs=500, n_nearest=3), 5)
                row = {"n": int(len(xyp)), "reference_published_wall_s": published_s[nm]}
                for label, flags in (("lds_speculative_epochs", 0), ("chip_wide_scans", TA.TL_FLAG_LK_CHIP_WIDE)):
                    with TA.Context(local, flags) as cl:
                        best = None
                        for _ in range(2):
                            t0l = time.perf_counter()
                            sl = TA.lin_kernighan.solve(pp, lo, ctx=cl, seed=1)
                            wl = (time.perf_counter() - t0l) * 1e3
                            if best is None or sl.stats["kernel_ms"] < best[0]:
                                best = (sl.stats["kernel_ms"], wl, sl)
                    k_ms_l, w_ms_l, sl = best
                    row[label] = {"kernel_ms": k_ms_l, "wall_ms": w_ms_l, "rounds": sl.stats["sweeps"], "moves": sl.stats["moves"],
                                  "us_per_round": k_ms_l * 1e3 / max(sl.stats["sweeps"], 1), "cost": float(sl.total)}
                    row.setdefault("_route", list(sl.route()))
                    assert list(sl.route()) == row["_route"], f"LK {nm}: the two forms differ"
                if not a.no_cpu_baseline:
                    import _oracle as O
                    t0c = time.perf_counter()
                    _rc, orr, oc, ost, _sn = O.lin_kernighan_trace(xyp, epochs=10000, platoo_epochs=500, n_nearest=3, max_depth=5, seed=1, cap=2048)
                    wo = (time.perf_counter() - t0c) * 1e3
                    assert orr.tolist() == row["_route"] and ost["sweeps"] == row["lds_speculative_epochs"]["rounds"], f"LK {nm}: GPU != oracle"
                    row["cpu_baseline"] = {"value": wo, "unit": "ms", "cores": 1, "kind": "port",
                                           "sample": "the whole run (same options, same seeded kicks) by the oracle on one core: same tour and round count (asserted)"}
                    row["speedup_vs_one_core"] = wo / row["lds_speculative_epochs"]["wall_ms"]
                del row["_route"]
                pub[nm] = row
            extras["lk_published_instances"] = dict(pub, note="tl_lk with the CLI's defaults incl. NN seed and candidate lists; kernel_ms = device time, wall_ms = the call; "
                                                              "lds_speculative_epochs: k_lk_ils, one workgroup per epoch, a batch of consecutive epochs at once, taken in order up to the "
                                                              "first accepted one (same tours, counters and messages as the sequential loop); reference_published_wall_s: the reference's "
                                                              "own CLI on its laptop (bench/baseline-solvers.tsv:17-31)")
        except Exception as exc:
            extras["error"] = repr(exc)
        if not a.no_end_to_end:
            try:
                extras["drop_in_end_to_end"] = drop_in_end_to_end(TA, not a.no_cpu_baseline)
            except Exception as exc:
                extras["drop_in_end_to_end"] = {"error": repr(exc)}
        out["extras"] = extras
        if "no_prune_multistart" in extras and "candidates_per_s" in extras["no_prune_multistart"]:
            # `value` counts candidates DECIDED (82 % of them a tile at a time by the exact L0 bound); the two like-for-like rates beside it:
            out["value_every_candidate_exact"] = {"value": extras["no_prune_multistart"]["candidates_per_s"], "unit": "candidates/s",
                                                  "note": "TL_FLAG_NO_PRUNE: every candidate evaluated with the reference's own arithmetic (4 correctly rounded sqrt), same tours"}
        if "multistart_two_descents_per_cu" in extras:  # the same kernel with a batch of 2 x CUs restarts (two descents per CU), for the record
            out["value_with_two_descents_per_cu"] = {"value": extras["multistart_two_descents_per_cu"]["candidates_per_s"], "unit": "candidates/s",
                                                     "restarts_per_gpu": extras["multistart_two_descents_per_cu"]["restarts"]}
    if world == 1 and a.full and not a.no_cpu_baseline:
        res, out["cpu_baseline"] = cpu_baseline(n, a.seed, xy)
        # the oracle's descents of restarts 0..cores-1 are the same units the GPU just ran: cost bits and sweep / move
        # counters must agree, or the headline number counts something else than the reference's loop
        bad = []
        for k, (cnd, c, sw, mv) in enumerate(res):
            if first <= k < first + R:
                j = k - first
                if np.float32(cost_host[j]).tobytes() != np.float32(c).tobytes() or int(st_host[j, 0]) != sw or int(st_host[j, 1]) != mv:
                    bad.append((k, float(cost_host[j]), float(c), int(st_host[j, 0]), sw, int(st_host[j, 1]), mv))
        if "extras" in out and isinstance(out["extras"].get("no_prune_multistart"), dict):
            out["extras"]["no_prune_multistart"]["cpu_baseline"] = dict(out["cpu_baseline"], note="the top-level cpu_baseline: the oracle evaluates every candidate exactly, like this kernel form")
        out["parity_checked_restarts"] = sum(1 for k in range(len(res)) if first <= k < first + R)
        out["parity_mismatches"] = bad
        if bad:
            emit(out)
            raise SystemExit(f"bench.py: GPU restarts differ from the oracle: {bad[:4]}")
    emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
