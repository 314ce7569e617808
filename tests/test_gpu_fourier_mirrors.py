"""The Fourier-curve solver's mirrors on the GPU: the Python mirror and its batch, the pipeline step, the C++ mirror and the CLI
command `fourier_curve` with its comma lists, and the raw C call on berlin52, against the oracle (tests/_fourier_oracle.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _fourier_oracle as FO
import _sa_cases as K

pytestmark = pytest.mark.gpu

bits = FO.bits
O = dict(k_max=3, m=60, lam=0.05, lambda_decay=0.5, lr=0.05, epochs=30)
GRID = [(la, lr) for la in (0.05, 0.2) for lr in (0.05, 0.1, 0.02)]


def _best(results):
    return int(np.argmin([(bits(r["cost"]) << 32) | k for k, r in enumerate(results)]))


def test_python_mirror_batch_and_pipeline(ctx):
    import teeline_amd as TA
    FCu = TA.fourier_curve
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    res = FO.solve(prob.xy, None, 52, **O)
    msgs = []
    sol = FCu.solve(prob, FCu.FourierOptions(**O), lambda k, p: msgs.append(k), [int(v) for v in prob.ids[::-1]], ctx=ctx)  # (start tour and channel ignored)
    assert msgs == [] and sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    assert FO.f64_words(sol.stats["coeffs"].view(np.float64)).tolist() == FO.f64_words(res["coeffs"]).tolist()
    singles = [FO.solve(prob.xy, None, 52, **dict(O, lam=la, lr=lr)) for la, lr in GRID]
    jobs = [FCu.FourierOptions(**dict(O, lam=la, lr=lr)) for la, lr in GRID]
    best = FCu.solve_many(prob, jobs, ctx=ctx)
    b = _best(singles)
    assert best.stats["job"] == b and best.route() == prob.ids[singles[b]["tour"]].tolist() and bits(best.total) == bits(singles[b]["cost"])
    every = FCu.solve_many(prob, jobs, ctx=ctx, return_all=True)
    assert [s.route() for s in every] == [prob.ids[r["tour"]].tolist() for r in singles]
    assert TA.pipeline.steps_for_solve("fourier_curve") == ["fourier_curve"]
    outs = TA.pipeline.run_pipeline_stages(prob, ["nn", "fourier_curve", "2opt"], {"fourier_curve": FCu.FourierOptions(**O)}, ctx=ctx)
    assert [x.name for x in outs] == ["nn", "fourier_curve", "2opt"] and outs[1].solution.route() == sol.route()  # the seed tour is ignored
    assert TA.validate_tour(outs[-1].solution.route(), prob) and outs[-1].solution.total <= outs[1].solution.total
    outs = TA.pipeline.run_pipeline_stages(prob, ["fourier_curve"], ctx=ctx, fourier_jobs=jobs)
    assert outs[0].solution.route() == best.route()
    with pytest.raises(ValueError, match="the Fourier-curve solver of this build is `fourier_curve`"):
        TA.pipeline.steps_for_solve("fourier")
    with pytest.raises(ValueError, match="unknown solver `branch_bound`"):
        TA.pipeline.steps_for_solve("branch_bound")
    # ids are not positions; n < 2 is trivial; a problem without coordinates is refused
    ids = [5, 10, 15, 20, 25]
    i = np.arange(5, dtype=np.float64)
    circ = np.stack([np.cos(2.0 * np.pi * i / 5), np.sin(2.0 * np.pi * i / 5)], axis=1).astype(np.float32)
    small = TA.TspProblem(ids, circ)
    fast = dict(O, k_max=2, m=50, epochs=20)
    want = FO.solve(circ, None, 5, **fast)
    assert FCu.solve(small, FCu.FourierOptions(**fast), ctx=ctx).route() == [ids[p] for p in want["tour"]]
    assert FCu.solve(TA.TspProblem([7], [[1.0, 2.0]]), ctx=ctx).route() == [7]


def test_cli_equals_the_oracle(ctx):
    """fails without the feature: the parent's CLI does not know `fourier_curve`"""
    import teeline_amd as TA
    from teeline_amd import _capi, build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--k-max", "3", "--m", "60", "--lambda-decay", "0.5", "--epochs", "30"]
    fmt = lambda res: TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()  # noqa: E731
    res = FO.solve(prob.xy, None, 52, **O)
    for extra in ([], ["--no-seed"]):  # the solver runs alone either way: no seed stage
        r = subprocess.run([cli, "solve", "fourier_curve", "-i", tsp, "--lambda", "0.05", "--lr", "0.05"] + extra + args0, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines()[-2:] == fmt(res)
    # the raw C entry gives what the CLI printed
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = _capi.TlFourierOpts(3, 60, 30, 0, 0.05, 0.5, 0.05, 0, 0)
    assert ctx.lib.tl_fourier_curve(ctx.handle, prob.xy.ctypes.data_as(C.c_void_p), 52, None, C.byref(po), out.ctypes.data_as(C.c_void_p), C.byref(cost), None, None) == 0
    assert out.tolist() == res["tour"].tolist() and bits(np.float32(cost.value)) == bits(res["cost"])
    # the comma lists: their product is the batch, the best kept
    singles = [FO.solve(prob.xy, None, 52, **dict(O, lam=la, lr=lr)) for la, lr in GRID]
    r = subprocess.run([cli, "solve", "fourier_curve", "-i", tsp, "--lambda", "0.05,0.2", "--lr", "0.05,0.1,0.02"] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(singles[_best(singles)]), r.stderr
    # defaults
    r = subprocess.run([cli, "solve", "fourier_curve", "-i", tsp], capture_output=True, text=True, timeout=120)
    dflt = FO.solve(prob.xy, None, 52, log_cap=0, **FO.DEFAULTS)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(dflt)
    r = subprocess.run([cli, "solve", "fourier", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the Fourier-curve solver of this build is `fourier_curve`" in r.stderr
    r = subprocess.run([cli, "solve", "branch_bound", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "fourier_curve" not in r.stderr
    r = subprocess.run([cli, "pipeline", "--steps=fourier_curve,2opt", "-i", tsp, "--lambda", "0.05", "--lr", "0.05"] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = TA.pipeline.run_pipeline_stages(prob, ["fourier_curve", "2opt"], {"fourier_curve": TA.fourier_curve.FourierOptions(**O)}, ctx=ctx)[-1].solution
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(want).splitlines()
