"""The gravitational search solver's mirrors on the GPU: the Python mirror's and the C++ mirror's message sequences, the pipeline step
and the CLI command `gravitational_search` on berlin52, against the oracle (tests/_gsa_oracle.py)."""
import os
import subprocess

import numpy as np
import pytest

import _gsa_cases as GC
import _gsa_oracle as GO
import _sa_cases as K

pytestmark = pytest.mark.gpu

GOLDEN = GC.golden_cases()
bits = GO.bits


def okey(key, n, init, o):
    return (key, n, None if init is None else tuple(int(v) for v in init), tuple(sorted(o.items())))


def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    GS = TA.gravitational_search
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    xy, _pk, n, init, o = GOLDEN["berlin52"]
    opts = TA.HeuristicOptions(epochs=o["epochs"])
    res = GO.solve_cached(okey("berlin52", n, init, o), prob.xy, None, 52, None, **o)
    assert len(res["improvements"]) >= 2
    msgs = []
    sol = GS.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    want = GO.messages(res, prob.ids)
    assert [k for k, _ in msgs] == [k for k, _ in want] and sum(k == "EpochUpdate" for k, _ in msgs) == o["epochs"]
    for (k, p), (_k, w) in zip(msgs, want):
        if k == "PathUpdate":
            assert p[0] == w[0] and bits(p[1]) == bits(w[1])
        else:
            assert p == w
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    plain = GS.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == res["counters"]["improved"]
    short = TA.HeuristicOptions(epochs=5, n_nearest=31)
    so = dict(epochs=5, n_nearest=31, seed=1)
    msgs2 = []
    bestsol = GS.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [GO.solve_cached(okey("mirror", 52, None, dict(so, run=r)), prob.xy, None, 52, None, **dict(so, run=r)) for r in range(4)]
    r = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r]["tour"]].tolist() and bits(bestsol.total) == bits(singles[r]["cost"])
    assert [k for k, _ in msgs2] == [k for k, _ in GO.messages(singles[r])]
    steps = TA.pipeline.steps_for_solve("gravitational_search")
    assert steps == ["shuffle", "gravitational_search"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"gravitational_search": short}, ctx=ctx, lk_seed=3)
    assert [x.name for x in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = GO.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), **dict(so, seed=3))
    assert outs[-1].solution.route() == prob.ids[seeded["tour"]].tolist() and bits(outs[-1].solution.total) == bits(seeded["cost"])
    with pytest.raises(ValueError, match="the seeded gravitational search of this build is `gravitational_search`"):
        TA.pipeline.steps_for_solve("gsa")


def test_cli_equals_the_oracle(ctx):
    """fails without the feature: the parent's CLI refuses `gravitational_search` as a CPU-only name"""
    import re
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "6", "--seed", "3", "--n-nearest", "31"]
    o = dict(epochs=6, n_nearest=31, seed=3)
    fmt = lambda res: TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()  # noqa: E731
    r = subprocess.run([cli, "solve", "gravitational_search", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    shuffled = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=3)[0].solution
    res = GO.solve(prob.xy, None, 52, prob.positions_of(shuffled.route()), **o)
    assert r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "gravitational_search", "--no-seed", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    res = GO.solve(prob.xy, None, 52, None, **o)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(res)
    # the C entry gives what the CLI printed
    from teeline_amd import _capi
    import ctypes as C
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = _capi.TlGsaOpts(6, 31, 0)
    assert ctx.lib.tl_gravitational_search(ctx.handle, prob.xy.ctypes.data_as(C.c_void_p), 52, None, None, C.byref(po), 3, out.ctypes.data_as(C.c_void_p), C.byref(cost), None) == 0
    assert out.tolist() == res["tour"].tolist() and bits(np.float32(cost.value)) == bits(res["cost"])
    r = subprocess.run([cli, "solve", "gsa", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the seeded gravitational search of this build is `gravitational_search`" in r.stderr
    # the C++ mirror's messages: PathUpdate(start) and one per improvement, EpochUpdate per epoch, Done
    r = subprocess.run([cli, "solve", "gravitational_search", "--no-seed", "--progress-digest", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=[0-9a-f]{16} epoch_updates=(\d+)", r.stderr)
    assert r.returncode == 0 and m, r.stderr
    assert [int(v) for v in m.groups()] == [len(res["improvements"]), 0, 1, o["epochs"]]
    r = subprocess.run([cli, "solve", "gravitational_search", "--no-seed", "--runs", "3", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    three = [GO.solve(prob.xy, None, 52, None, **dict(o, run=k)) for k in range(3)]
    best = three[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(three)]))]
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(best)
    r = subprocess.run([cli, "pipeline", "--steps=shuffle,gravitational_search,2opt", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = TA.pipeline.run_pipeline_stages(prob, ["shuffle", "gravitational_search", "2opt"],
                                           {"gravitational_search": TA.HeuristicOptions(epochs=6, n_nearest=31)}, ctx=ctx, lk_seed=3)[-1].solution
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(want).splitlines()
