"""Lin-Kernighan for seeded runs (-m gpu): tl_lk_population in both forms — form 1, one workgroup per run with the whole ILS of that run
in its CU's LDS (k_lk_ils_pop), and form 0, the loop over tl_lk — against the oracle run by run (tests/_lk_population_cases.py: tour,
cost bits, scans / searches / moves / exchanged edges), with seed run_seed(S, r) for run r.  Three contexts: form 1 forced, form 0
forced, and form 1 whose slices are a few scans long (the state's round trip through LkState and the global arrays)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import _lk_population_cases as P
import _oracle as O
import _tsplib as T
from _raw_context import _vp, jitter_context

pytestmark = pytest.mark.gpu

FORMS = ["form1", "form0", "sliced"]
vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
ENTRIES = {"tl_lk_population": [vp, vp, u32, vp, vp, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp], "tl_lk_population_setting": [vp, C.c_int, u32]}
CLI_KW = dict(epochs=10000, platoo_epochs=500, n_nearest=3, max_depth=5)


@pytest.fixture(scope="module")
def forms():
    import teeline_amd as TA
    TA._capi.load()
    c = {k: TA.Context(0) for k in FORMS}
    c["form1"].lk_population_setting(1, 0)
    c["form0"].lk_population_setting(0, 0)
    c["sliced"].lk_population_setting(1, 3)
    yield c
    for v in c.values():
        v.close()


def prob(xy, packed=None):
    import teeline_amd as TA
    n = len(xy)
    dm = None if packed is None else TA.distance_matrix.DistanceMatrix(n, packed, np.arange(n), "geo")
    return TA.TspProblem(np.arange(n), xy, dm)


def population(ctx, xy, kw, seed, runs, first_run=0, inits=None, packed=None):
    """[(route, total, stats)] per run, and the best index"""
    import teeline_amd as TA
    h = TA.HeuristicOptions(epochs=kw["epochs"], platoo_epochs=kw["platoo_epochs"], n_nearest=kw["n_nearest"])
    tours = None if inits is None else [[int(v) for v in t] for t in inits]
    sols, best = TA.lin_kernighan.solve_population(prob(xy, packed), TA.LKOptions(h, kw["max_depth"]), tours, seed=seed, runs=runs, first_run=first_run, ctx=ctx)
    return [(np.asarray(s.route(), dtype=np.uint32), s.total, s.stats) for s in sols], best


def best_of(got):
    return min(range(len(got)), key=lambda i: (np.float32(got[i][1]), i))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(P.CASES))
def test_every_run_is_the_oracles(forms, form, name):
    xy, kw, seed, runs, inits = P.case_inputs(name)
    got, best = population(forms[form], xy, kw, seed, runs, inits=inits)
    P.check_population(got, name, xy, kw, seed, runs, inits=inits)
    assert best == best_of(got)


@pytest.mark.parametrize("form", FORMS)
def test_berlin52_with_the_cli_options(forms, form, tsplib_dir):
    xy = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))["xy"]
    got, best = population(forms[form], xy, CLI_KW, 1, 8)
    P.check_population(got, "berlin52", xy, CLI_KW, 1, 8, cap=4096)
    assert f"{float(got[0][1]):.5f}" == "7544.36572"
    assert got[best][1] <= got[0][1] and best == best_of(got)


@pytest.mark.parametrize("form", ["form1", "form0"])
@pytest.mark.parametrize("count", [1, 2, 257, 513])
def test_more_runs_than_the_chip_holds_at_once(forms, form, count):
    # 256 CUs: 257 runs are more than one per CU, 513 more than two
    xy, kw = O.synth_xy(12, seed=12), P._kw(12, 4, 3)
    got, best = population(forms[form], xy, kw, 9, count)
    P.check_population(got, "n12", xy, kw, 9, count)
    assert best == best_of(got)


@pytest.mark.parametrize("form", FORMS)
def test_a_run_does_not_depend_on_the_call_it_is_in(forms, form, ctx):
    import teeline_amd as TA
    xy, kw = O.synth_xy(40, seed=40), P._kw(15, 5, 5)
    whole, _ = population(forms[form], xy, kw, 6, 10)
    P.check_population(whole, "n40", xy, kw, 6, 10)
    part, _ = population(forms[form], xy, kw, 6, 3, first_run=5)
    for (r1, c1, s1), (r2, c2, s2) in zip(part, whole[5:8]):
        assert r1.tolist() == r2.tolist() and np.float32(c1).tobytes() == np.float32(c2).tobytes()
        assert [s1[k] for k in ("sweeps", "candidates", "moves", "reversed")] == [s2[k] for k in ("sweeps", "candidates", "moves", "reversed")]
    # run 0 is tl_lk with the plain seed, bit for bit, counters included
    h = TA.HeuristicOptions(epochs=kw["epochs"], platoo_epochs=kw["platoo_epochs"], n_nearest=kw["n_nearest"])
    sol = TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, kw["max_depth"]), ctx=ctx, seed=6)
    assert list(sol.route()) == whole[0][0].tolist() and np.float32(sol.total).tobytes() == np.float32(whole[0][1]).tobytes()
    assert [sol.stats[k] for k in ("sweeps", "candidates", "moves", "reversed")] == [whole[0][2][k] for k in ("sweeps", "candidates", "moves", "reversed")]


@pytest.mark.parametrize("form", FORMS)
def test_start_tours_none_one_and_one_per_run(forms, form):
    n, kw = 40, P._kw(15, 5, 5)
    xy = O.synth_xy(n, seed=40)
    each = [O.restart_perm(n, 31, r) for r in range(4)]  # random starts: the first passes differ in length, the runs finish in different slices
    for key, inits in (("n40", None), ("n40_one", each[:1]), ("n40_each", each)):
        got, _ = population(forms[form], xy, kw, 6, 4, inits=inits)
        P.check_population(got, key, xy, kw, 6, 4, inits=inits)


def raw_population(ctx, xy, init, init_count, first, count, opts, seed, out, costs=None, cnt=None, best=None):
    import teeline_amd as TA
    o = None if opts is None else C.byref(TA._capi.TlLkOpts(*opts))
    return ctx.lib.tl_lk_population(ctx.handle, _vp(xy), len(xy), None, _vp(init), init_count, first, count, o, seed, _vp(out), _vp(costs), _vp(cnt),
                                    None if best is None else C.byref(best), None)


@pytest.mark.parametrize("form", ["form1", "form0"])
def test_errors_leave_the_outputs_alone(forms, form):
    import teeline_amd as TA
    ctx, n = forms[form], 20
    xy = O.synth_xy(n, seed=3)
    out, costs = np.full(3 * n, 77, np.uint32), np.full(3, -1.0, np.float32)
    init = np.stack([O.restart_perm(n, 1, r) for r in range(3)])
    init[2, 4] = init[2, 5]  # row 2 is no permutation
    assert raw_population(ctx, xy, init, 3, 0, 3, (5, 5, 5, 5), 1, out, costs) == TA._capi.TL_ERR_BADARG
    assert b"tour 2" in ctx.lib.tl_last_error(ctx.handle)
    good = np.ascontiguousarray(init[:2])
    for opts, code in (((5, 5, 0, 5), TA._capi.TL_ERR_BADARG), ((5, 5, 5, 17), TA._capi.TL_ERR_UNSUPPORTED)):  # tl_lk's own checks and codes
        assert raw_population(ctx, xy, None, 0, 0, 3, opts, 1, out, costs) == code
    assert raw_population(ctx, xy, good, 2, 0, 3, (5, 5, 5, 5), 1, out, costs) == TA._capi.TL_ERR_BADARG  # init_count: none of 0, 1, count
    assert raw_population(ctx, xy, None, 1, 0, 3, (5, 5, 5, 5), 1, out, costs) == TA._capi.TL_ERR_BADARG
    assert raw_population(ctx, xy, None, 0, 0, 0, (5, 5, 5, 5), 1, out, costs) == 0                       # count == 0: nothing written
    assert out.tolist() == [77] * (3 * n) and costs.tolist() == [-1.0] * 3
    got, _ = population(ctx, xy, P._kw(5, 5, 5), 1, 2)  # the context is usable
    P.check_population(got, "n20", xy, P._kw(5, 5, 5), 1, 2)


@pytest.mark.parametrize("form", ["form1", "form0"])
def test_equal_costs_go_to_the_lowest_run(forms, form):
    # no epochs and one start for all: every run is the same first pass, a guaranteed tie
    n = 30
    xy = O.synth_xy(n, seed=8)
    start = np.ascontiguousarray(O.restart_perm(n, 2, 0))
    out, costs, best = np.empty(4 * n, np.uint32), np.empty(4, np.float32), C.c_uint32(9)
    assert raw_population(forms[form], xy, start, 1, 0, 4, (0, 10, 5, 5), 1, out, costs, None, best) == 0
    assert len(set(costs.view(np.uint32).tolist())) == 1 and best.value == 0
    assert all(out[r * n:(r + 1) * n].tolist() == out[:n].tolist() for r in range(4))


def test_slice_lengths_do_not_change_a_result(forms):
    # slices of 1, 7 and 64 scans against the default's 8192: runs end in different launches, a pass spans several
    ctx = forms["sliced"]
    xy, kw, seed, runs, inits = P.case_inputs("n201")
    want, _ = population(forms["form1"], xy, kw, seed, runs, inits=inits)
    try:
        for scans in (1, 7, 64):
            ctx.lk_population_setting(1, scans)
            got, _ = population(ctx, xy, kw, seed, runs, inits=inits)
            P.check_population(got, "n201", xy, kw, seed, runs, inits=inits)
            assert [g[0].tolist() for g in got] == [w[0].tolist() for w in want]
    finally:
        ctx.lk_population_setting(1, 3)


@pytest.mark.parametrize("form", FORMS)
def test_geo_problem_seed_and_totals_go_through_the_matrix(forms, form, tsplib_dir):
    e = T.parse_tsplib(os.path.join(tsplib_dir, "burma14.tsp"))
    xy, packed = e["xy"], O.dm_build_packed(e["xy"], geo=True)
    kw = P._kw(20, 10, 5)
    got, _ = population(forms[form], xy, kw, 3, 4, packed=packed)
    P.check_population(got, "burma14", xy, kw, 3, 4, packed=packed)
    for route, cost, _st in got:
        assert np.float32(cost) == O.tour_length(None, packed, route)  # problem.distances' total, not Euclid's


def test_a_busy_context_refuses_a_second_thread(forms, tsplib_dir):
    import time

    import teeline_amd as TA
    ctx = forms["form1"]
    xy = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))["xy"]
    res, codes = {}, []

    def long_call():  # (64 runs of 10 000 epochs: tens of milliseconds inside the entry)
        while "got" not in res:
            try:
                res["got"] = population(ctx, xy, CLI_KW, 1, 64)[0]
            except TA.TeelineGpuError as exc:  # the other thread was inside: again
                assert exc.code == TA._capi.TL_ERR_BUSY
                res["refused"] = res.get("refused", 0) + 1

    t = threading.Thread(target=long_call)
    small, kw = O.synth_xy(12, seed=12), P._kw(12, 4, 3)
    t.start()
    t0 = time.time()
    while t.is_alive() and time.time() - t0 < 30:
        try:
            population(ctx, small, kw, 9, 2)
            codes.append(0)
        except TA.TeelineGpuError as exc:
            codes.append(exc.code)
    t.join()
    assert TA._capi.TL_ERR_BUSY in codes and set(codes) <= {0, TA._capi.TL_ERR_BUSY}, codes[:20]
    P.check_population(res["got"][:8], "berlin52", xy, CLI_KW, 1, 8, cap=4096)  # the long call was not disturbed


def test_one_context_lk_then_population_then_two_opt(ctx):
    import teeline_amd as TA
    xy, kw = O.synth_xy(40, seed=40), P._kw(15, 5, 5)
    h = TA.HeuristicOptions(epochs=kw["epochs"], platoo_epochs=kw["platoo_epochs"], n_nearest=kw["n_nearest"])
    sol = TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, kw["max_depth"]), ctx=ctx, seed=6)
    got, _ = population(ctx, xy, kw, 6, 4)  # the default context: the plan's own choice of form
    P.check_population(got, "n40", xy, kw, 6, 4)
    assert list(sol.route()) == got[0][0].tolist()
    s2 = TA.two_opt.solve(prob(xy), ctx=ctx)
    rc, route, cost, _st = O.two_opt(xy, None, 40)
    assert rc == 0 and list(s2.route()) == route.tolist() and np.float32(s2.total).tobytes() == np.float32(cost).tobytes()


def test_jitter_build():
    """n = 64, 8 runs on the race-stress build (-DTL_JITTER: waves leave every barrier far apart), form 1."""
    jctx = jitter_context(ENTRIES)
    try:
        assert jctx.lib.tl_lk_population_setting(jctx.handle, 1, 0) == 0
        xy, kw, seed, runs = O.synth_xy(64, seed=2), P._kw(), 5, 8
        n = len(xy)
        opts = (C.c_uint32 * 4)(kw["epochs"], kw["platoo_epochs"], kw["n_nearest"], kw["max_depth"])
        out, costs, cnt = np.empty(runs * n, np.uint32), np.empty(runs, np.float32), np.empty(runs * 4, np.uint64)
        rc = jctx.lib.tl_lk_population(jctx.handle, _vp(xy), n, None, None, 0, 0, runs, opts, seed, _vp(out), _vp(costs), _vp(cnt), None, None)
        assert rc == 0, jctx.lib.tl_last_error(jctx.handle)
        got = [(out[r * n:(r + 1) * n], costs[r], dict(zip(("sweeps", "candidates", "moves", "reversed"), (int(v) for v in cnt[4 * r:4 * r + 4])))) for r in range(runs)]
        P.check_population(got, "n64_k5", xy, kw, seed, runs)
    finally:
        jctx.close()


def test_cli_runs(ctx, tsplib_dir):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    path = os.path.join(tsplib_dir, "berlin52.tsp")
    p = TA.tsplib.read_from_file(path).problem()
    h = TA.HeuristicOptions(epochs=10000, platoo_epochs=500, n_nearest=3)
    sols, best = TA.lin_kernighan.solve_population(p, TA.LKOptions(h, 5), seed=1, runs=4, ctx=ctx)
    r = subprocess.run([cli, "solve", "lk", "--runs", "4", "--seed", "1", "--stats", "-i", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head, route = r.stdout.splitlines()[:2]
    assert head == f"{float(sols[best].total):.5f} 0" and [int(v) for v in route.split()] == [int(v) for v in sols[best].route()]
    assert f"best_run={best}" in r.stderr
    plain = subprocess.run([cli, "solve", "lk", "--seed", "1", "--stats", "-i", path], capture_output=True, text=True)
    one = subprocess.run([cli, "solve", "lk", "--runs", "1", "--seed", "1", "--stats", "-i", path], capture_output=True, text=True)
    assert plain.returncode == 0 and one.returncode == 0 and one.stdout == plain.stdout
    assert "best_run" not in plain.stderr and "best_run" not in one.stderr
    assert plain.stdout.splitlines()[0] == f"{float(sols[0].total):.5f} 0"
