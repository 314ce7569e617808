"""TL_MODE_BEST_SWEEP for batches (-m gpu): tl_two_opt_multistart, tl_two_opt_multistart_devices, tl_two_opt_batch_dev in mode 1 and
tl_two_opt_best_population — one LDS-resident descent per workgroup (two_opt_best_lds.hip) — against tlo_two_opt_best, descent by
descent: tours element for element, costs bit for bit, sweeps, moves and reversed.  Random starts stay at n <= 300 (the oracle is
O(moves * n^2)); larger n uses the planted starts of tests/_best_sweep_cases.py, a handful of moves from a fixed point."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _best_sweep_cases as B
import _oracle as O
from _raw_context import _vp, jitter_context

pytestmark = pytest.mark.gpu

MODE = 1  # TL_MODE_BEST_SWEEP
vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
ENTRIES = {
    "tl_two_opt_multistart": [vp, vp, u32, u64, u32, u32, i32, vp, vp, vp, vp, vp],
    "tl_two_opt_best_population": [vp, vp, u32, vp, u32, vp, vp, vp, vp],
}

_oracle_cache = {}


def oracle(key, xy, tour):
    """tlo_two_opt_best of one start, computed once per process (the jitter test runs the same cases again)."""
    if key not in _oracle_cache:
        rc, route, cost, st = O.two_opt(xy, None, len(tour), init=np.asarray(tour, dtype=np.uint32), best=True)
        assert rc == 0
        route.setflags(write=False)
        _oracle_cache[key] = (route, int(np.float32(cost).view(np.uint32)), st)
    return _oracle_cache[key]


def oracle_restart(n, seed, r):
    return oracle(("restart", n, seed, r), O.synth_xy(n, seed=seed), O.restart_perm(n, seed, r))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(c, rc):
    if hasattr(c, "check"):
        c.check(rc)
    else:
        assert rc == 0, c.lib.tl_last_error(c.handle)


def device(c):
    cus, lds = C.c_int(), C.c_int()
    assert c.lib.tl_device_info(c.handle, C.byref(cus), C.byref(lds), None, 0) == 0
    return cus.value, lds.value


def plan(ctx, n, count, force_scan=0):
    cus, lds = device(ctx)
    form, threads = C.c_int(-1), C.c_int(-1)
    assert ctx.lib.tl_two_opt_best_plan(n, count, cus, lds, force_scan, C.byref(form), C.byref(threads)) == 0
    return form.value, threads.value


def multistart(c, xy, n, seed, first, count, mode=MODE):
    from teeline_amd import _capi
    xy = np.ascontiguousarray(xy, dtype=np.float32)
    pos, costs = np.full(n, 0xFFFFFFFF, np.uint32), np.zeros(count, np.float32)
    cost, best, st = C.c_float(), C.c_uint32(), _capi.TlStats()
    check(c, c.lib.tl_two_opt_multistart(c.handle, _vp(xy), n, seed, first, count, mode, _vp(pos), C.byref(cost), C.byref(best), _vp(costs), C.byref(st)))
    return pos, cost.value, best.value, costs, st.as_dict()


def population(c, xy, tours):
    from teeline_amd import _capi
    xy = np.ascontiguousarray(xy, dtype=np.float32)
    init = np.ascontiguousarray(np.stack(tours), dtype=np.uint32)
    count, n = init.shape
    out, costs, moves = np.full((count, n), 0xFFFFFFFF, np.uint32), np.zeros(count, np.float32), np.full(count, 0xFFFFFFFF, np.uint32)
    st = _capi.TlStats()
    check(c, c.lib.tl_two_opt_best_population(c.handle, _vp(xy), n, _vp(init), count, _vp(out), _vp(costs), _vp(moves), C.byref(st)))
    return out, costs, moves, st.as_dict()


def check_multistart(c, n, seed, first, count):
    """Every restart's cost, the winner (lowest cost, then lowest restart) with its tour, and the summed counters."""
    want = [oracle_restart(n, seed, first + r) for r in range(count)]
    pos, cost, best, costs, st = multistart(c, O.synth_xy(n, seed=seed), n, seed, first, count)
    assert bits(costs).tolist() == [w[1] for w in want]
    k = min(range(count), key=lambda r: (want[r][1], r))  # costs are >= 0: their bits order like the floats
    assert best == first + k and int(bits([cost])[0]) == want[k][1]
    assert pos.tolist() == want[k][0].tolist(), "the winner's tour differs from the oracle"
    for key in ("sweeps", "moves", "reversed", "candidates"):
        assert st[key] == sum(w[2][key] for w in want), key
    return costs


def check_population(c, key, xy, tours):
    """Every tour of one call against its own oracle run: the isolation check is that they all hold at once."""
    want = [oracle((key, k), xy, t) for k, t in enumerate(tours)]
    out, costs, moves, st = population(c, xy, tours)
    for k, w in enumerate(want):
        assert out[k].tolist() == w[0].tolist(), f"tour {k} differs from the oracle"
        assert int(bits(costs)[k]) == w[1], f"cost of tour {k}"
        assert int(moves[k]) == w[2]["moves"], f"moves of tour {k}"
    for name in ("sweeps", "moves", "reversed", "candidates"):
        assert st[name] == sum(w[2][name] for w in want), name
    return want


# ---------------------------------------------------------------- 1. multistart equals the oracle per restart
SIZES = [3, 4, 5, 6, 19, 20, 63, 64, 65, 66, 67, 127, 128, 129, 130, 200, 300]


@pytest.mark.parametrize("n", SIZES)
def test_multistart_equals_the_oracle_per_restart(ctx, n):
    """n = 3: no rows; 19: one row per wave of 16; n = 0, 1, 63 mod 64: the tile edges.  (TL_ERR_UNSUPPORTED before this form existed.)"""
    assert plan(ctx, n, 8)[0] == 0
    check_multistart(ctx, n, seed=n, first=5, count=8)


# ---------------------------------------------------------------- 2. independence of the split
def test_result_does_not_depend_on_the_split(ctx):
    import teeline_amd as TA
    n, R, f, seed = 130, 24, 7, 11
    assert plan(ctx, n, R)[0] == 0
    whole = check_multistart(ctx, n, seed, f, R)
    parts = [multistart(ctx, O.synth_xy(n, seed=seed), n, seed, f + a, b - a)[3] for a, b in ((0, 5), (5, 6), (6, 24))]
    assert bits(np.concatenate(parts)).tolist() == bits(whole).tolist()
    prob = TA.TspProblem(np.arange(n), O.synth_xy(n, seed=seed))
    one, costs1 = TA.two_opt.multistart(prob, R, seed, f, ctx=ctx, mode=MODE, return_costs=True)
    with TA.Context(0) as c2:
        two, costs2 = TA.two_opt.multistart_devices(prob, R, [ctx, c2], seed, f, mode=MODE, return_costs=True)
    assert bits(costs2).tolist() == bits(costs1).tolist() == bits(whole).tolist()
    assert two.route() == one.route() and two.stats["best_restart"] == one.stats["best_restart"]
    for k in ("sweeps", "moves", "reversed", "candidates"):
        assert two.stats[k] == one.stats[k]


# ---------------------------------------------------------------- 3. population equals single-tour
CASES = {c.id + f"#{k}": c for k, c in enumerate(B.CASES)}


def case_population(case):
    """The planted tour, the unplanted fixed point, each single plant alone, the plants in reverse order."""
    base = B.snake if case.family == "snake" else (lambda n, plants=(): B.uniform(n, case.seed, plants))
    xy, planted = case.build()
    tours = [planted, base(case.n)[1]] + [base(case.n, [p])[1] for p in case.plants] + [base(case.n, case.plants[::-1])[1]]
    return xy, tours


@pytest.mark.parametrize("cid", list(CASES))
def test_population_equals_single_tour(ctx, cid):
    case = CASES[cid]
    assert case.n <= ctx.two_opt_best_lds_max_n()
    xy, tours = case_population(case)
    assert plan(ctx, case.n, len(tours))[0] == 0
    want = check_population(ctx, cid, xy, tours)
    assert want[0][2]["moves"] >= 2 and want[1][2]["moves"] == 0 and want[1][2]["sweeps"] == 1  # many moves and none in one call


# ---------------------------------------------------------------- 4. more tours than CUs
def test_more_tours_than_cus(ctx):
    n, seed = 64, 21
    count = 2 * device(ctx)[0] + 3
    assert plan(ctx, n, count)[0] == 0
    xy = O.synth_xy(n, seed=seed)
    check_population(ctx, "cus", xy, [O.restart_perm(n, seed, r) for r in range(count)])


# ---------------------------------------------------------------- 5. rows beyond one pass of the workgroup
@pytest.mark.parametrize("n", [1027, 1028])
def test_rows_beyond_one_pass_of_the_workgroup(ctx, n):
    """n - 3 = 1024 and 1025 rows on 16 waves of 64 rows a pass"""
    assert plan(ctx, n, 1)[0] == 0
    xy, tour = B.uniform(n, 9, [(100, 400), (333, 900), (1000, n - 2)])
    check_population(ctx, f"rows{n}", xy, [tour])


# ---------------------------------------------------------------- 6. at and beyond the LDS limit
def test_at_and_beyond_the_lds_limit(ctx):
    top = ctx.two_opt_best_lds_max_n()
    assert 4096 < top < 65535
    for n, form in ((top, 0), (top + 1, 1)):
        assert plan(ctx, n, 1)[0] == form
        xy, tour = B.uniform(n, 7, [(50, 2100), (4090, 4200), (6000, n - 2), (n - 40, n - 3)])
        check_population(ctx, f"limit{n}", xy, [tour])


def test_golden_65535_runs_the_loop(ctx, golden_dir):
    import sys
    sys.path.insert(0, golden_dir)
    import make_goldens_best_sweep as MG
    with open(os.path.join(golden_dir, "goldens_best_sweep.json")) as fh:
        g = json.load(fh)["snake65535_best_sweep"]
    xy, init = B.GOLDEN_CASE.build()
    assert plan(ctx, len(init), 2)[0] == 1
    out, costs, moves, st = population(ctx, xy, [init, init])
    for k in range(2):
        assert MG.crc(out[k]) == g["route_crc32"] and int(bits(costs)[k]) == g["cost_bits"] and int(moves[k]) == g["stats"]["moves"]
    assert {k: st[k] for k in ("sweeps", "candidates", "moves", "reversed")} == {k: 2 * v for k, v in g["stats"].items()}


# ---------------------------------------------------------------- 7. forced scan is identical
@pytest.fixture(scope="module")
def scan_ctx():
    import teeline_amd as TA
    with TA.Context(0) as c:
        c.two_opt_best_force_scan()  # (a setting, not a create flag: bit 31, the last one, stays the bit no flag has)
        yield c


@pytest.mark.parametrize("n", [65, 129, 300])
def test_forced_scan_gives_the_same_bytes(ctx, scan_ctx, n):
    assert plan(ctx, n, 6)[0] == 0 and plan(ctx, n, 6, 1)[0] == 1
    xy = O.synth_xy(n, seed=n)
    a, b = multistart(ctx, xy, n, n, 2, 6), multistart(scan_ctx, xy, n, n, 2, 6)
    assert a[0].tobytes() == b[0].tobytes() and bits([a[1]]).tobytes() == bits([b[1]]).tobytes() and a[2] == b[2] and a[3].tobytes() == b[3].tobytes()
    assert {k: a[4][k] for k in ("sweeps", "moves", "reversed", "candidates")} == {k: b[4][k] for k in ("sweeps", "moves", "reversed", "candidates")}
    tours = [O.restart_perm(n, n, r) for r in range(4)]
    pa, pb = population(ctx, xy, tours), population(scan_ctx, xy, tours)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pa[:3], pb[:3]))


# ---------------------------------------------------------------- 8. tl_two_opt_batch_dev with mode 1
def batch_dev(ctx, xy, n, inits, seed, first, count):
    import torch
    from teeline_amd import _capi
    dev = torch.device("cuda", 0)
    d_xy = torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float32)).to(dev)
    d_init = None if inits is None else torch.from_numpy(np.ascontiguousarray(inits).astype(np.int64).astype(np.int32)).to(dev)
    d_pos = torch.zeros((count, n), dtype=torch.int32, device=dev)
    d_cost = torch.zeros(count, dtype=torch.float32, device=dev)
    d_stats = torch.full((count, _capi.TL_DEV_STATS_STRIDE), -1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream()
    rc = ctx.lib.tl_two_opt_batch_dev(ctx.handle, d_xy.data_ptr(), n, None if d_init is None else d_init.data_ptr(), seed, first, count, MODE,
                                      d_pos.data_ptr(), d_cost.data_ptr(), d_stats.data_ptr(), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    return rc, d_pos.cpu().numpy().astype(np.uint32), d_cost.cpu().numpy(), d_stats.cpu().numpy()


def test_batch_dev_in_best_sweep_mode(ctx):
    from teeline_amd import _capi
    n, R, seed, first = 130, 12, 11, 7
    xy = O.synth_xy(n, seed=seed)
    want = [oracle_restart(n, seed, first + r) for r in range(R)]

    def same(r, pos, cost, st):
        w = want[r]
        assert pos.tolist() == w[0].tolist() and int(bits(cost)[0]) == w[1]
        assert st[:4].tolist() == [w[2]["sweeps"], w[2]["moves"], w[2]["reversed"], 0] and not st[4:].any()

    rc, pos, cost, st = batch_dev(ctx, xy, n, None, seed, first, R)  # seeded starts
    assert rc == 0
    for r in range(R):
        same(r, pos[r], cost[r], st[r])
    inits = np.stack([O.restart_perm(n, seed, first + r) for r in range(R)]).astype(np.uint32)
    inits[4, 17] = n + 5  # a position >= n: that descent is refused, its neighbours are untouched
    rc, pos, cost, st = batch_dev(ctx, xy, n, inits, 0, 0, R)
    assert rc == 0
    for r in range(R):
        if r == 4:
            assert st[r].tolist() == [0, 0, 0, 2] + [0] * 12 and np.isnan(cost[r]) and not pos[r].any()
        else:
            same(r, pos[r], cost[r], st[r])
    with pytest.raises(Exception) as e:  # no counters of this mode
        ctx.two_opt_last_counters()
    assert e.value.code == _capi.TL_ERR_BADARG
    top = ctx.two_opt_best_lds_max_n()
    rc, _, _, _ = batch_dev(ctx, O.synth_xy(top + 1, seed=1), top + 1, None, 1, 0, 1)
    assert rc == _capi.TL_ERR_UNSUPPORTED


# ---------------------------------------------------------------- 9. contract edges
def test_contract_edges(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    n, seed = 66, 5
    xy = O.synth_xy(n, seed=seed)
    tours = np.stack([O.restart_perm(n, seed, r) for r in range(3)]).astype(np.uint32)
    lib, h = ctx.lib, ctx.handle
    out, costs, moves = np.full((3, n), 77, np.uint32), np.full(3, 7.0, np.float32), np.full(3, 77, np.uint32)
    # count == 0: TL_OK, nothing written
    assert lib.tl_two_opt_best_population(h, _vp(xy), n, _vp(tours), 0, _vp(out), _vp(costs), _vp(moves), None) == 0
    assert (out == 77).all() and (costs == 7.0).all() and (moves == 77).all()
    # a row that is no permutation: named, nothing written
    bad = tours.copy()
    bad[2, 3] = bad[2, 4]
    assert lib.tl_two_opt_best_population(h, _vp(xy), n, _vp(bad), 3, _vp(out), _vp(costs), _vp(moves), None) == _capi.TL_ERR_BADARG
    assert b"tour 2" in lib.tl_last_error(h)
    assert (out == 77).all() and (costs == 7.0).all() and (moves == 77).all()
    # a matrix problem is refused; n = 2 is the reference's panic
    dmp = TA.TspProblem(np.arange(n), xy, TA.distance_matrix.DistanceMatrix(n, O.dm_build_packed(xy), np.arange(n), "explicit"))
    with pytest.raises(TA.TeelineGpuError) as e:
        TA.two_opt.solve_population(dmp, [list(range(n))], ctx=ctx, mode=MODE)
    assert e.value.code == _capi.TL_ERR_UNSUPPORTED
    two = np.arange(2, dtype=np.uint32)
    assert lib.tl_two_opt_best_population(h, _vp(xy), 2, _vp(two), 1, _vp(out), _vp(costs), None, None) == _capi.TL_ERR_REF_PANICS
    pos, cost, best = np.zeros(2, np.uint32), C.c_float(), C.c_uint32()
    assert lib.tl_two_opt_multistart(h, _vp(xy), 2, 1, 0, 4, MODE, _vp(pos), C.byref(cost), C.byref(best), None, None) == _capi.TL_ERR_REF_PANICS
    # the context between REF_ORDER batches: the later results are unchanged
    prob = TA.TspProblem(np.arange(n), xy)
    lists = [[int(v) for v in t] for t in tours]
    ref0 = TA.two_opt.solve_population(prob, lists, ctx=ctx)
    best0 = check_population(ctx, "edges", xy, list(tours))
    ref1 = TA.two_opt.solve_population(prob, lists, ctx=ctx)
    best1 = TA.two_opt.solve_population(prob, lists, ctx=ctx, mode=MODE)
    for k in range(3):
        assert ref1[k].route() == ref0[k].route() and bits([ref1[k].total]).tolist() == bits([ref0[k].total]).tolist()
        assert best1[k].route() == best0[k][0].tolist() and int(bits([best1[k].total])[0]) == best0[k][1]
        assert best1[k].stats["moves"] == best0[k][2]["moves"]


# ---------------------------------------------------------------- 10. jitter build
def test_jitter_build():
    """Items 1 (a subset), 3 (two CASES) and 4 on the race-stress build (-DTL_JITTER: waves leave every barrier far apart)."""
    jctx = jitter_context(ENTRIES)
    try:
        for n in (3, 19, 64, 65, 130, 200):
            check_multistart(jctx, n, seed=n, first=5, count=8)
        for cid in list(CASES)[6:8]:  # the two n = 300 snakes: nested plants, and the 33-column tie
            xy, tours = case_population(CASES[cid])
            check_population(jctx, cid, xy, tours)
        n, seed = 64, 21
        xy = O.synth_xy(n, seed=seed)
        check_population(jctx, "cus", xy, [O.restart_perm(n, seed, r) for r in range(2 * jctx.cus + 3)])
    finally:
        jctx.close()


# ---------------------------------------------------------------- 11. CLI
def test_cli_runs(ctx, tsplib_dir):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    path = os.path.join(tsplib_dir, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(path).problem()
    sol = TA.two_opt.multistart(prob, 8, 1, 0, ctx=ctx, mode=MODE)
    r = subprocess.run([cli, "solve", "2opt", "--best-sweep", "--runs", "8", "--seed", "1", "--stats", "-i", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head, route = r.stdout.splitlines()[:2]
    assert head == f"{float(sol.total):.5f} 0" and [int(v) for v in route.split()] == [int(v) for v in sol.route()]
    assert f"best_restart={sol.stats['best_restart']}" in r.stderr
    plain = subprocess.run([cli, "solve", "2opt", "--best-sweep", "-i", path], capture_output=True, text=True)
    one = subprocess.run([cli, "solve", "2opt", "--best-sweep", "--runs", "1", "-i", path], capture_output=True, text=True)
    assert plain.returncode == 0 and one.returncode == 0 and one.stdout == plain.stdout and plain.stdout != r.stdout
    assert "best_restart" not in plain.stderr
