"""The Kohonen map solver's mirrors on the GPU: the Python mirror's message sequence and best run, the pipeline step, the C++ mirror
and the CLI command `kohonen_som` and the raw C call on berlin52, against the oracle (tests/_som_oracle.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _sa_cases as K
import _som_oracle as SO

pytestmark = pytest.mark.gpu

bits = SO.bits
O = dict(epochs=25, learning_rate=0.7, radius_fraction=0.2, neuron_multiplier=4)


def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    KS = TA.kohonen_som
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    opts = KS.SOMOptions(**O)
    res = SO.solve(prob.xy, None, 52, seed=1, **O)
    msgs = []
    sol = KS.solve(prob, opts, lambda k, p: msgs.append((k, p)), [int(v) for v in prob.ids[::-1]], ctx=ctx, seed=1)  # (the start tour is ignored)
    want = SO.messages(res, prob.ids)
    assert [k for k, _ in msgs] == [k for k, _ in want] == ["EpochUpdate", "PathUpdate"] * 12 + ["PathUpdate", "Done"]
    for (k, p), (_k, w) in zip(msgs, want):
        if k == "PathUpdate":
            assert p[0] == w[0] and bits(p[1]) == bits(w[1])
        else:
            assert p == w
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    plain = KS.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and KS.solve(prob, opts, None, None, ctx=ctx, seed=1, form=2).route() == sol.route()
    msgs2 = []
    bestsol = KS.solve(prob, opts, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [SO.solve(prob.xy, None, 52, seed=1, run=r, **O) for r in range(4)]
    r = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r]["tour"]].tolist() and bits(bestsol.total) == bits(singles[r]["cost"])
    assert [(k, p) if k != "PathUpdate" else (k, p[0]) for k, p in msgs2] == [(k, p) if k != "PathUpdate" else (k, p[0]) for k, p in SO.messages(singles[r], prob.ids)]
    assert TA.pipeline.steps_for_solve("kohonen_som") == ["kohonen_som"]
    outs = TA.pipeline.run_pipeline_stages(prob, ["kohonen_som", "2opt"], {"kohonen_som": opts}, ctx=ctx, lk_seed=3, som_runs=2)
    two = [SO.solve(prob.xy, None, 52, seed=3, run=k, **O) for k in range(2)]
    b = two[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(two)]))]
    assert [x.name for x in outs] == ["kohonen_som", "2opt"] and outs[0].solution.route() == prob.ids[b["tour"]].tolist()
    assert TA.validate_tour(outs[-1].solution.route(), prob) and outs[-1].solution.total <= outs[0].solution.total
    with pytest.raises(ValueError, match="the seeded Kohonen map of this build is `kohonen_som`"):
        TA.pipeline.steps_for_solve("som")
    # n < 2: the trivial route and no message at all
    one = TA.TspProblem([7], [[1.0, 2.0]])
    quiet = []
    assert KS.solve(one, opts, lambda k, p: quiet.append(k), None, ctx=ctx).route() == [7] and quiet == []


def test_cli_equals_the_oracle(ctx):
    """fails without the feature: the parent's CLI refuses `kohonen_som` as a CPU-only name"""
    import teeline_amd as TA
    from teeline_amd import _capi, build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "25", "--seed", "3", "--learning_rate", "0.7", "--radius_fraction", "0.2", "--neuron_multiplier", "4"]
    fmt = lambda res: TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()  # noqa: E731
    res = SO.solve(prob.xy, None, 52, seed=3, **O)
    for extra in ([], ["--no-seed"]):  # the map runs alone either way: no seed stage
        r = subprocess.run([cli, "solve", "kohonen_som", "-i", tsp] + extra + args0, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.splitlines()[-2:] == fmt(res)
    # the raw C entry gives what the CLI printed
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = _capi.TlSomOpts(25, 4, 0.7, 0.2, 0, 0, 0)
    assert ctx.lib.tl_kohonen_som(ctx.handle, prob.xy.ctypes.data_as(C.c_void_p), 52, None, C.byref(po), 3, out.ctypes.data_as(C.c_void_p), C.byref(cost), None) == 0
    assert out.tolist() == res["tour"].tolist() and bits(np.float32(cost.value)) == bits(res["cost"])
    for alias in ("som", "kohonen"):
        r = subprocess.run([cli, "solve", alias, "-i", tsp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the seeded Kohonen map of this build is `kohonen_som`" in r.stderr
    # the C++ mirror's messages: EpochUpdate + PathUpdate per checkpoint, the final PathUpdate (25 % 2 != 0), Done
    r = subprocess.run([cli, "solve", "kohonen_som", "--progress-digest", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=[0-9a-f]{16} epoch_updates=(\d+)", r.stderr)
    assert r.returncode == 0 and m, r.stderr
    assert [int(v) for v in m.groups()] == [13, 0, 1, 12]
    r = subprocess.run([cli, "solve", "kohonen_som", "--runs", "3", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    three = [SO.solve(prob.xy, None, 52, seed=3, run=k, **O) for k in range(3)]
    best = three[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(three)]))]
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(best)
    r = subprocess.run([cli, "pipeline", "--steps=kohonen_som,2opt", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = TA.pipeline.run_pipeline_stages(prob, ["kohonen_som", "2opt"], {"kohonen_som": TA.kohonen_som.SOMOptions(**O)}, ctx=ctx, lk_seed=3)[-1].solution
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(want).splitlines()
