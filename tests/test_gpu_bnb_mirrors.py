"""The branch and bound's mirrors on the GPU (-m gpu): branch_and_bound.solve, the pipeline stage, the C++ mirror and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import _bnb_cases as K
import _bnb_oracle as B

pytestmark = pytest.mark.gpu

TSPLIB = os.path.join(K.HERE, "golden", "tsplib")


def test_solve_the_pipeline_stage_and_the_three_stage_pipeline_agree(ctx):
    import teeline_amd as TA
    xy = K.random_xy(14, 6)
    ids = np.arange(1, 15)[::-1].copy()  # the smallest id is the last position
    prob = TA.TspProblem(ids, xy)
    D = B.dist_matrix(xy)
    want = K.call(None, xy, None, 14, start=13)
    msgs = []
    sol = TA.branch_and_bound.solve(prob, None, lambda kind, payload: msgs.append(kind), ctx=ctx)
    assert sol.route() == [int(ids[p]) for p in want[1]] and sol.total.tobytes() == want[2].tobytes()
    assert sol.stats["proved"] == 1 and sol.stats["improved"] == 1 and sol.stats["nodes"] > 0 and sol.stats["leaves"] > 0 and sol.stats["launches"] >= 1
    assert msgs == ["PathUpdate", "PathUpdate", "Done"]
    # the result is the instance's: the stage started from NN's tour, or from NN + 2-opt's, returns the same tour unless the seed is
    # already of the optimum's length — then the seed itself
    for steps in (["nn", "branch_and_bound"], ["nn", "2opt", "branch_and_bound"]):
        out = TA.pipeline.run_pipeline_stages(prob, steps, ctx=ctx)
        last, seed = out[-1].solution, out[-2].solution
        assert out[-1].name == "branch_and_bound" and last.stats["proved"] == 1
        if last.stats["improved"]:
            assert last.route() == sol.route() and last.total.tobytes() == sol.total.tobytes()
        else:
            assert last.route() == seed.route() and last.total.tobytes() == sol.total.tobytes()
        pos = prob.positions_of(last.route())
        assert last.total.tobytes() == B.tour_length(D, [int(p) for p in pos]).tobytes()
    assert TA.pipeline.steps_for_solve("branch_and_bound") == ["nn", "branch_and_bound"]
    with pytest.raises(ValueError, match="unknown solver `branch_bound`"):
        TA.pipeline.steps_for_solve("branch_bound")
    # n_nearest through HeuristicOptions, as the reference reads it
    sol3 = TA.branch_and_bound.solve(prob, TA.HeuristicOptions(n_nearest=3), ctx=ctx)
    want3 = K.call(None, xy, None, 14, start=13, K=3)
    assert sol3.route() == [int(ids[p]) for p in want3[1]] and sol3.total.tobytes() == want3[2].tobytes()


def test_cli_and_cpp_mirror(ctx):
    """fails without the feature: the parent's CLI does not know `branch_and_bound`"""
    from teeline_amd import build
    cli = build.build_cli()
    r = subprocess.run([cli, "solve", "branch_and_bound", "-i", os.path.join(TSPLIB, "berlin52.tsp"), "--max-nodes", "1000"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    head, route = r.stdout.splitlines()[:2]
    assert sorted(int(v) for v in route.split()) == list(range(1, 53)) and float(head.split()[0]) > 7000.0
    assert "proved=0" in r.stderr
    r = subprocess.run([cli, "solve", "branch_and_bound", "-i", os.path.join(TSPLIB, "gr17.tsp")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("2085.00000 0\n") and "proved=0" not in r.stderr, r.stdout + r.stderr
    r = subprocess.run([cli, "pipeline", "--steps=nn,2opt,branch_and_bound", "-i", os.path.join(TSPLIB, "gr17.tsp")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("2085.00000 0\n"), r.stdout + r.stderr
    r = subprocess.run([cli, "solve", "branch_bound", "-i", os.path.join(TSPLIB, "gr17.tsp")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr
