"""The mirrors of the Held-Karp bound (-m gpu): teeline_amd.one_tree_bound and the C++ mirror (through the CLI
command `bound`, which is a few lines over it) agree with the C ABI and the oracle; `solve --lower-bound` adds its lines and nothing else."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _one_tree_cases as K
import _one_tree_oracle as H

pytestmark = pytest.mark.gpu


def berlin():
    import teeline_amd as TA
    xy, pk, n = K.tsp("berlin52")
    return TA.TspProblem(np.arange(1, n + 1), xy), xy, n


def test_bound_takes_its_upper_from_nn_and_two_opt(ctx):
    import teeline_amd as TA
    prob, xy, n = berlin()
    b = TA.one_tree_bound.bound(prob, ctx=ctx, log_cap=1000)
    seed = TA.nearest_neighbor.solve(prob, ctx=ctx)
    two = TA.two_opt.solve(prob, None, None, seed.route(), ctx=ctx)
    assert b.upper == float(two.total) and b.upper_route == two.route()
    w = H.ascent(xy, None, n, upper=b.upper)
    rc, got = K.call(ctx, xy, None, n, upper=b.upper)
    assert rc == 0
    K.assert_same(got, w, "the C ABI")
    assert K.bits(b.bound) == K.bits(w["bound"]) and b.pi.tobytes() == w["pi"].tobytes() and np.array_equal(b.parent, w["parent"])
    assert b.is_tour and b.route == [int(prob.ids[p]) for p in w["tour"]] and TA.validate_tour(b.route, prob)
    assert [np.asarray(r).tobytes() for r in b.log] == [np.asarray(r).tobytes() for r in w["log"]]
    assert b.stats["stop_name"] == "tour" and b.stats["iterations_run"] == w["iterations_run"] and b.stats["kernel_ms"] > 0
    assert b.gap_pct(b.bound) == 0.0 and abs(b.gap_pct(b.upper) - 100.0 * (b.upper - w["bound"]) / w["bound"]) < 1e-12


def test_bound_batch_and_host_agree(ctx):
    import teeline_amd as TA
    prob, xy, n = berlin()
    upper = K.nn_upper(xy, None, n)
    sets = [dict(root=0, iterations=30), dict(root=51, iterations=30, lambda0=1.0), dict(root=7, iterations=12, patience=2)]
    every = TA.one_tree_bound.bound_batch(prob, upper, sets, ctx=ctx, return_all=True, log_cap=30)
    for j, s in enumerate(sets):
        w = H.ascent(xy, None, n, upper=upper, **s)
        h = TA.one_tree_bound.bound_host(prob, upper, log_cap=30, **s)
        for b in (every[j], h):
            assert K.bits(b.bound) == K.bits(w["bound"]) and b.pi.tobytes() == w["pi"].tobytes() and len(b.log) == w["iterations_run"]
            assert b.stats["best_iter"] == w["best_iter"] and b.stats["stop"] == w["stop"]
    best = TA.one_tree_bound.bound_batch(prob, upper, sets, ctx=ctx)
    bounds = [b.bound for b in every]
    assert best.stats["job"] == bounds.index(max(bounds)) and best.stats["bounds"] == bounds


def test_a_matrix_problem(ctx):
    import teeline_amd as TA
    ts = TA.tsplib.read_from_file(str(__import__("pathlib").Path(K.HERE) / "golden" / "tsplib" / "gr17.tsp"))
    prob = ts.problem(ctx=ctx)
    xy, pk, n = K.tsp("gr17")
    b = TA.one_tree_bound.bound(prob, 2187.0, iterations=60, ctx=ctx)
    w = H.ascent(None, pk, n, upper=2187.0, iterations=60)
    assert K.bits(b.bound) == K.bits(w["bound"]) and b.pi.tobytes() == w["pi"].tobytes()


@pytest.fixture(scope="module")
def cli():
    from teeline_amd import build
    return build.build_cli()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "goldens_one_tree.json")))


def sh(cli, *args):
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_bound_prints_the_golden_bound(cli, tsplib_dir, golden):
    g = golden["berlin52"]
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    r = sh(cli, "bound", "-i", f, "--upper", repr(g["upper"]))
    m = re.fullmatch(r"bound=(\S+) job=0 of 1 \(lambda=2 patience=10\) upper=(\S+) \(--upper\) gap_pct=(\S+)( proved=1)?\n", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)).hex() == g["bound"] and float(m.group(2)) == g["upper"] and bool(m.group(4)) == bool(g["is_tour"])
    assert abs(float(m.group(3)) - 100.0 * (g["upper"] - float.fromhex(g["bound"])) / float.fromhex(g["bound"])) < 1e-4
    j = json.loads(sh(cli, "bound", "-i", f, "--upper", repr(g["upper"]), "--output-format", "json").stdout)
    assert float(j["bound"]).hex() == g["bound"] and j["proved"] == bool(g["is_tour"]) and j["iterations_run"] == g["iterations_run"]
    assert j["upper"] == g["upper"] and j["job"] == 0 and j["jobs"] == 1 and list(j) == sorted(j)


def test_cli_bound_grid_root_and_tour(ctx, cli, tsplib_dir):
    xy, pk, n = K.tsp("berlin52")
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    upper = 7900.0
    las, pats = (2.0, 0.5, 1.0), (10, 2)
    j = json.loads(sh(cli, "bound", "-i", f, "--upper", "7900", "--root", "5", "--iterations", "40", "--lambda", "2,0.5,1", "--patience=10,2",
                      "--output-format", "json").stdout)
    sets = [dict(upper=upper, root=5, iterations=40, lambda0=la, patience=pa) for la in las for pa in pats]  # lambda the outer index
    rc, got, best = K.call_batch(ctx, xy, pk, n, sets)
    assert rc == 0 and j["jobs"] == 6 and j["job"] == best and float(j["bound"]).hex() == got[best]["bound"].hex()
    assert (j["lambda"], j["patience"]) == (sets[best]["lambda0"], sets[best]["patience"]) and j["proved"] == bool(got[best]["is_tour"])
    # --tour: the file's tour priced by tl_tour_length is the upper bound
    t = sh(cli, "bound", "-i", f, "--tour", os.path.join(tsplib_dir, "berlin52.opt.tour"), "--iterations", "40", "--output-format", "json")
    jt = json.loads(t.stdout)
    assert jt["upper_from"] == "--tour" and np.float32(jt["upper"]) == np.float32(7544.36572)
    rc, one = K.call(ctx, xy, pk, n, upper=jt["upper"], iterations=40)
    assert rc == 0 and float(jt["bound"]).hex() == one["bound"].hex()
    # neither: nn -> 2opt
    jn = json.loads(sh(cli, "bound", "-i", f, "--iterations", "40", "--output-format", "json").stdout)
    assert jn["upper_from"] == "nn,2opt" and np.float32(jn["upper"]) == np.float32(8384.18848)


def test_solve_lower_bound_adds_its_lines_and_nothing_else(ctx, cli, tsplib_dir, golden_dir):
    g = json.load(open(os.path.join(golden_dir, "goldens.json")))["berlin52"]["nn_two_opt"]
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    expected = "8384.18848 0\n" + "".join(f"{v} " for v in g["route_ids"]) + "\n"
    plain = sh(cli, "solve", "2opt", "-i", f)
    assert plain.stdout == expected and "bound" not in plain.stderr and "gap_pct" not in plain.stderr  # byte for byte what it was
    with_lb = sh(cli, "solve", "2opt", "-i", f, "--lower-bound")
    assert with_lb.stdout == expected
    xy, pk, n = K.tsp("berlin52")
    rc, want = K.call(ctx, xy, pk, n, upper=float(np.float32(8384.18848)))
    assert rc == 0
    lines = with_lb.stderr.strip().split("\n")[-3:] if want["is_tour"] else with_lb.stderr.strip().split("\n")[-2:]
    assert float(lines[0].split("=")[1]).hex() == want["bound"].hex() and lines[0].startswith("bound=")
    gap = 100.0 * (float(np.float32(8384.18848)) - want["bound"]) / want["bound"]
    assert lines[1] == f"gap_pct={gap:.4f}" and (lines[2:] == ["proved=1"]) == bool(want["is_tour"])
    assert with_lb.stderr.replace("\n".join(lines) + "\n", "") == plain.stderr
    # JSON mode: the two keys join the object, the rest is what it was
    jp = json.loads(sh(cli, "solve", "2opt", "-i", f, "--output-format", "json").stdout)
    jl = json.loads(sh(cli, "solve", "2opt", "-i", f, "--output-format", "json", "--lower-bound").stdout)
    assert "bound" not in jp and "gap_pct" not in jp
    assert float(jl.pop("bound")).hex() == want["bound"].hex() and abs(jl.pop("gap_pct") - gap) < 1e-9 and jl == jp
    # pipeline takes the flag too
    p = sh(cli, "pipeline", "--steps=nn,2opt", "-i", f, "--lower-bound")
    assert p.stdout == expected and p.stderr.strip().split("\n")[-len(lines):] == lines
