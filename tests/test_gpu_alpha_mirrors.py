"""The mirrors of the alpha-nearness lists (-m gpu) on berlin52: the Python module against the numpy oracle, the C++
mirror through the CLI (`candidates --alpha`, `solve lk --candidates alpha[:K]` with --runs and in a pipeline) against the Python one."""
import os
import subprocess

import numpy as np
import pytest

import _alpha_oracle as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def berlin(tsplib_dir):
    import teeline_amd as TA
    path = os.path.join(tsplib_dir, "berlin52.tsp")
    return path, TA.tsplib.read_from_file(path).problem()


@pytest.fixture(scope="module")
def cli():
    from teeline_amd import build
    return build.build_cli()


def same(got, want):
    assert np.array_equal(got.rows, want["cand"]) and got.rows.dtype == np.uint32
    assert np.ascontiguousarray(got.alpha).tobytes() == np.ascontiguousarray(want["alpha"]).tobytes()
    assert np.array_equal(got.parent, want["parent"]) and tuple(got.root_nb) == tuple(want["root_nb"])


@pytest.mark.parametrize("k,root", [(5, 0), (1, 51), (60, 7)])  # 60: clipped to n - 1 = 51 columns
def test_python_candidates_against_the_oracle(ctx, berlin, k, root):
    import teeline_amd as TA
    _, p = berlin
    want = A.candidates(p.xy, None, len(p), None, root, k)
    dev = TA.alpha_candidates.candidates(p, k, root=root, ctx=ctx)
    host = TA.alpha_candidates.candidates_host(p, k, root=root)
    assert dev.rows.shape == (52, min(k, 51))
    same(dev, want)
    same(host, want)
    assert dev.stats["kernel_ms"] > 0 and dev.stats["candidates"] == 52 * 51
    pi = np.linspace(-3.0, 4.0, 52)
    same(TA.alpha_candidates.candidates(p, k, pi, root=root, ctx=ctx, threads=128), A.candidates(p.xy, None, 52, pi, root, k))
    same(TA.alpha_candidates.candidates_host(p, k, pi, root=root), A.candidates(p.xy, None, 52, pi, root, k))


def test_python_from_ascent_plan_and_errors(ctx, berlin):
    import teeline_amd as TA
    _, p = berlin
    got, b = TA.alpha_candidates.from_ascent(p, 5, iterations=60, ctx=ctx)
    assert b.stats["iterations_run"] == 60 and np.array_equal(got.pi, b.pi) and np.array_equal(got.parent, b.parent)
    same(got, A.candidates(p.xy, None, 52, b.pi, 0, 5))
    assert TA.alpha_candidates.plan(52) == {"threads": 64, "lds_bytes": 16 * 52} and TA.alpha_candidates.plan(1002, 64)["threads"] == 256
    for bad in (lambda: TA.alpha_candidates.plan(100, 65), lambda: TA.alpha_candidates.candidates(p, 65, ctx=ctx),
                lambda: TA.alpha_candidates.candidates_host(p, 0), lambda: TA.alpha_candidates.candidates(p, 5, root=52, ctx=ctx)):
        with pytest.raises(TA.TeelineGpuError):
            bad()
    with pytest.raises(ValueError):
        TA.alpha_candidates.candidates(p, 5, np.zeros(51), ctx=ctx)


def test_a_calls_candidates_leave_the_contexts_own_lists(berlin):
    """solve(candidates=rows) on a context that has lists set through Context.lk_candidates: afterwards the context has those again."""
    import teeline_amd as TA
    _, p = berlin
    h = TA.HeuristicOptions(epochs=30, platoo_epochs=10, n_nearest=5)
    key = lambda s: (tuple(int(v) for v in s.route()), np.float32(s.total).tobytes())  # noqa: E731
    with TA.Context(0) as c:
        own = TA.alpha_candidates.candidates(p, 5, ctx=c).rows
        other = TA.lin_kernighan.build_candidates(p, 8, ctx=c)[:, 3:]
        assert c.lk_candidates_set() is None
        plain = key(TA.lin_kernighan.solve(p, TA.LKOptions(h, 5), ctx=c, seed=2))
        c.lk_candidates(own)
        with_own = key(TA.lin_kernighan.solve(p, TA.LKOptions(h, 5), ctx=c, seed=2))
        with_other = key(TA.lin_kernighan.solve(p, TA.LKOptions(h, 5), ctx=c, seed=2, candidates=other))
        assert np.array_equal(c.lk_candidates_set(), own)
        assert key(TA.lin_kernighan.solve(p, TA.LKOptions(h, 5), ctx=c, seed=2)) == with_own
        sols, _ = TA.lin_kernighan.solve_population(p, TA.LKOptions(h, 5), seed=2, runs=2, ctx=c, candidates=other)
        assert key(sols[0]) == with_other and np.array_equal(c.lk_candidates_set(), own)
        c.lk_candidates(None)
        assert c.lk_candidates_set() is None and key(TA.lin_kernighan.solve(p, TA.LKOptions(h, 5), ctx=c, seed=2)) == plain
        assert len({plain, with_own, with_other}) == 3


def cli_rows(out, p):
    ids, rows = [], []
    for line in out.splitlines():
        head, _, rest = line.partition(":")
        ids.append(int(head))
        rows.append([int(v) for v in rest.split()])
    assert ids == [int(v) for v in p.ids]
    return rows


@pytest.mark.parametrize("k", [5, 60])
def test_the_candidates_command(ctx, cli, berlin, k):
    import teeline_amd as TA
    path, p = berlin
    r = subprocess.run([cli, "candidates", "--alpha", "-k", str(k), "-i", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got, _ = TA.alpha_candidates.from_ascent(p, k, ctx=ctx)  # the ascent at its defaults, upper from nn -> 2opt: what the command runs
    assert cli_rows(r.stdout, p) == p.ids[got.rows].tolist()
    r = subprocess.run([cli, "candidates", "--alpha", "-k", str(k), "--ascent-iterations", "0", "--root", "7", "-i", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert cli_rows(r.stdout, p) == p.ids[A.candidates(p.xy, None, 52, None, 7, k)["cand"]].tolist()
    r = subprocess.run([cli, "candidates", "--alpha", "-k", "65", "-i", path], capture_output=True, text=True)
    assert r.returncode == 1 and "64" in r.stderr and r.stdout == ""
    assert subprocess.run([cli, "candidates", "-k", "5", "-i", path], capture_output=True, text=True).returncode == 2


def test_solve_lk_on_alpha_lists_through_the_cli(ctx, cli, berlin):
    import teeline_amd as TA
    path, p = berlin
    nn = TA.nearest_neighbor.solve(p, ctx=ctx).route()
    opts = TA.LKOptions(TA.HeuristicOptions(epochs=300, platoo_epochs=30, n_nearest=3), 5)  # (n_nearest 3, depth 5: the CLI's defaults)
    short = ["--epochs", "300", "--platoo_epochs", "30"]
    for k, iters in ((5, 1000), (8, 0)):
        rows = TA.alpha_candidates.from_ascent(p, k, iterations=iters, ctx=ctx)[0].rows if iters else TA.alpha_candidates.candidates(p, k, ctx=ctx).rows
        flag = ["--candidates", f"alpha:{k}"] if k != 5 else ["--candidates", "alpha"]
        more = [] if iters == 1000 else ["--ascent-iterations", str(iters)]
        want = TA.lin_kernighan.solve(p, opts, None, nn, ctx=ctx, seed=1, candidates=rows)
        r = subprocess.run([cli, "solve", "lk", "--seed", "1", "--stats", "-i", path] + short + flag + more, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        head, route = r.stdout.splitlines()[:2]
        assert head == f"{float(want.total):.5f} 0" and [int(v) for v in route.split()] == [int(v) for v in want.route()]
        assert f"lists=alpha:{k}" in r.stderr
        if iters == 0:
            continue
        # --runs, and the same as a pipeline
        sols, best = TA.lin_kernighan.solve_population(p, opts, [nn], seed=1, runs=3, ctx=ctx, candidates=rows)
        for cmd in (["solve", "lk"], ["pipeline", "--steps=nn,lk"]):
            r = subprocess.run([cli] + cmd + ["--runs", "3", "--seed", "1", "--stats", "-i", path] + short + flag + more, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            head, route = r.stdout.splitlines()[:2]
            assert head == f"{float(sols[best].total):.5f} 0" and [int(v) for v in route.split()] == [int(v) for v in sols[best].route()]
            assert f"best_run={best}" in r.stderr and f"lists=alpha:{k}" in r.stderr
    plain = subprocess.run([cli, "solve", "lk", "--seed", "1", "--stats", "-i", path] + short, capture_output=True, text=True)
    want = TA.lin_kernighan.solve(p, opts, None, nn, ctx=ctx, seed=1)
    assert plain.returncode == 0 and "lists=kdtree:3" in plain.stderr and plain.stdout.splitlines()[0] == f"{float(want.total):.5f} 0"
    r = subprocess.run([cli, "solve", "2opt", "--candidates", "alpha", "-i", path], capture_output=True, text=True)
    assert r.returncode == 0 and "no lk step" in r.stderr
