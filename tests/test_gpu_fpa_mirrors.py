"""The flower pollination solver's mirrors on the GPU: the Python mirror's and the C++ mirror's message sequences, the pipeline step
and the CLI command `flower_pollination` on berlin52, against the oracle (tests/_fpa_oracle.py)."""
import os
import subprocess

import numpy as np
import pytest

import _fpa_cases as FC
import _fpa_oracle as FO
import _sa_cases as K

pytestmark = pytest.mark.gpu

GOLDEN = FC.golden_cases()
bits = FO.bits


def okey(key, n, init, o):
    return (key, n, None if init is None else tuple(int(v) for v in init), tuple(sorted(o.items())))


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    FP = TA.flower_pollination
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    xy, _pk, n, init, o = GOLDEN["berlin52"]
    opts = FP.FPAOptions(epochs=o["epochs"])
    res = FO.solve_cached(okey("berlin52", n, init, o), prob.xy, None, 52, None, **o)
    msgs = []
    sol = FP.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    want = FO.messages(res, prob.ids)
    assert [k for k, _ in msgs] == [k for k, _ in want] and sum(k == "EpochUpdate" for k, _ in msgs) == o["epochs"]
    for (k, p), (_k, w) in zip(msgs, want):
        if k == "PathUpdate":
            assert p[0] == w[0] and bits(p[1]) == bits(w[1])
        else:
            assert p == w
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    plain = FP.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == res["counters"]["improved"]
    short = FP.FPAOptions(epochs=5, n_nearest=31, mutation_probability=0.25)
    so = dict(epochs=5, n_nearest=31, mutation_probability=0.25, seed=1)
    msgs2 = []
    bestsol = FP.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [FO.solve_cached(okey("mirror", 52, None, dict(so, run=r)), prob.xy, None, 52, None, **dict(so, run=r)) for r in range(4)]
    r = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r]["tour"]].tolist() and bits(bestsol.total) == bits(singles[r]["cost"])
    assert [k for k, _ in msgs2] == [k for k, _ in FO.messages(singles[r])]
    steps = TA.pipeline.steps_for_solve("flower_pollination")
    assert steps == ["shuffle", "flower_pollination"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"flower_pollination": short}, ctx=ctx, lk_seed=3)
    assert [x.name for x in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = FO.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), **dict(so, seed=3))
    assert outs[-1].solution.route() == prob.ids[seeded["tour"]].tolist() and bits(outs[-1].solution.total) == bits(seeded["cost"])
    with pytest.raises(ValueError, match="the seeded flower pollination of this build is `flower_pollination`"):
        TA.pipeline.steps_for_solve("fpa")
    with pytest.raises(ValueError, match="mutation_probability"):
        FP.solve(prob, FP.FPAOptions(mutation_probability=2.0), None, None, ctx=ctx)


def test_cli_equals_the_oracle(ctx):
    import re
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "6", "--seed", "3", "--n-nearest", "31", "--mutation-probability", "0.25"]
    o = dict(epochs=6, n_nearest=31, mutation_probability=0.25, seed=3)
    fmt = lambda res: TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()  # noqa: E731
    r = subprocess.run([cli, "solve", "flower_pollination", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    shuffled = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=3)[0].solution
    res = FO.solve(prob.xy, None, 52, prob.positions_of(shuffled.route()), **o)
    assert r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "flower_pollination", "--no-seed", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    res = FO.solve(prob.xy, None, 52, None, **o)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "fpa", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the seeded flower pollination of this build is `flower_pollination`" in r.stderr
    # the C++ mirror's messages: PathUpdate(start) and one per improvement, EpochUpdate per epoch, Done
    r = subprocess.run([cli, "solve", "flower_pollination", "--no-seed", "--progress-digest", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=[0-9a-f]{16} epoch_updates=(\d+)", r.stderr)
    assert r.returncode == 0 and m, r.stderr
    assert [int(v) for v in m.groups()] == [len(res["improvements"]), 0, 1, o["epochs"]]
    r = subprocess.run([cli, "solve", "flower_pollination", "--no-seed", "--runs", "3", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    three = [FO.solve(prob.xy, None, 52, None, **dict(o, run=k)) for k in range(3)]
    best = three[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(three)]))]
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(best)
    r = subprocess.run([cli, "pipeline", "--steps=shuffle,flower_pollination,2opt", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = TA.pipeline.run_pipeline_stages(prob, ["shuffle", "flower_pollination", "2opt"],
                                           {"flower_pollination": TA.flower_pollination.FPAOptions(epochs=6, n_nearest=31, mutation_probability=0.25)}, ctx=ctx, lk_seed=3)[-1].solution
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(want).splitlines()
