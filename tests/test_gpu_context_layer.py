"""The batch and context layer of the C ABI (-m gpu): what hands work to the kernels in batches and keeps state between calls.

1. The beyond-the-LDS branch of tl_two_opt_multistart / _devices / tl_two_opt_population, reached through TL_FLAG_2OPT_FORCE_HBM at sizes
   the oracle affords: every cost, the winner by packed (cost, restart) key, the summed counters, the deal over 1 ... R + 2 contexts
   (empty shards, first != 0), a tie between restarts, the LDS path on the same job, and the real limit tl_two_opt_lds_max_n + 1.
2. tl_two_opt_last_counters answers with 2-opt counters or with TL_ERR_BADARG, never with another solver's data.
3. (tests/test_gpu_lk.py: re-entry from the live callback of every LK form.)
4. The matrix form's list of long cities: a late sweep that passes its capacity leaves the lists (hub instance, n = 3000).
5. One grow-only context, a dozen jobs in several orders, behind large jobs of each kind: no result depends on what ran before.
   (The solvers added since — the constructions, the exact solvers, the population scans, the seeded chains and populations, the
   Kohonen map, the Fourier curve — have their order tests, the pair sequence over their host paths and their share of section 2 in
   tests/test_gpu_context_solvers.py, which runs behind this file's fillers too.)

Measured on the MI355X: the 22 tests of this file take 16 s together (6 s of them test_multistart_one_past_the_lds_limit_over_two_contexts, 3 s
the split of n = 2000 over 1 ... 9 contexts); the three added cases of the re-entry test in tests/test_gpu_lk.py 0.2 s.
"""
import ctypes as C

import numpy as np
import pytest

import _greedy_oracle as G
import _oracle as O

pytestmark = pytest.mark.gpu

COUNTERS = ("sweeps", "candidates", "moves", "reversed")
R = 7


def f32bits(v):
    return int(np.float32(v).view(np.uint32))


def key(cost, restart):
    """tl_pack_cost_key: (f32 bits << 32) | restart"""
    return (f32bits(cost) << 32) | int(restart)


def prob(xy, packed=None):
    import teeline_amd as TA
    n = len(xy)
    dm = None if packed is None else TA.distance_matrix.DistanceMatrix(n, packed, np.arange(n), "explicit")
    return TA.TspProblem(np.arange(n), xy, dm)


@pytest.fixture(scope="module")
def hbm():
    """a context whose batch entries go through the HBM form at every n"""
    import teeline_amd as TA
    c = TA.Context(0, TA.TL_FLAG_2OPT_FORCE_HBM)
    yield c
    c.close()


_oracle_cache = {}


def oracle_restart(xy_seed, n, seed, r):
    """(route, cost, stats) of the oracle's descent from restart r's permutation; instances are O.synth_xy(n, xy_seed)"""
    k = (xy_seed, n, seed, r)
    if k not in _oracle_cache:
        rc, route, cost, st = O.two_opt(O.synth_xy(n, seed=xy_seed), None, n, init=O.restart_perm(n, seed, r))
        assert rc == 0
        _oracle_cache[k] = (route, cost, st)
    return _oracle_cache[k]


def outputs(sol, costs):
    """everything a multi-start call returns but the two times, in comparable form"""
    return (list(sol.route()), f32bits(sol.total), sol.stats["best_restart"], costs.tobytes(), tuple(sol.stats[k] for k in COUNTERS))


def oracle_outputs(per_restart, first):
    """the same tuple from the oracle's per-restart results: the winner is the minimum packed (cost, restart) key"""
    keys = [key(c, first + i) for i, (_, c, _) in enumerate(per_restart)]
    b = int(np.argmin(keys))
    costs = np.asarray([c for _, c, _ in per_restart], dtype=np.float32)
    return (per_restart[b][0].tolist(), f32bits(per_restart[b][1]), first + b, costs.tobytes(),
            tuple(sum(st[k] for _, _, st in per_restart) for k in COUNTERS))


def assert_times(stats):
    assert 0.0 < stats["kernel_ms"] <= stats["total_ms"], (stats["kernel_ms"], stats["total_ms"])


def ran_the_hbm_form(ctx):
    """The HBM form keeps no kernel-side counters: after it tl_two_opt_last_counters has nothing to return; after the LDS batch it has."""
    import teeline_amd as TA
    try:
        ctx.two_opt_last_counters()
    except TA.TeelineGpuError as e:
        assert e.code == TA._capi.TL_ERR_BADARG
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the HBM-form batch path
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 5])
@pytest.mark.parametrize("n", [257, 1002, 2000])
def test_forced_hbm_multistart_equals_the_oracle_and_the_lds_path(ctx, hbm, n, first):
    import teeline_amd as TA
    seed, xy_seed = 99, 40 + n
    xy = O.synth_xy(n, seed=xy_seed)
    want = oracle_outputs([oracle_restart(xy_seed, n, seed, r) for r in range(first, first + R)], first)
    sol, costs = TA.two_opt.multistart(prob(xy), R, seed=seed, first=first, ctx=hbm, return_costs=True)
    assert ran_the_hbm_form(hbm)
    got = outputs(sol, costs)
    for name, g, w in zip(("winning tour", "best cost bits", "best_restart", "costs", "counters"), got, want):
        assert g == w, f"n={n} first={first}: {name} differs from the oracle"
    assert_times(sol.stats)
    # the same restarts through a flag-less context: the LDS batch kernel
    sol2, costs2 = TA.two_opt.multistart(prob(xy), R, seed=seed, first=first, ctx=ctx, return_costs=True)
    assert not ran_the_hbm_form(ctx)
    assert outputs(sol2, costs2) == got
    assert_times(sol2.stats)


@pytest.mark.parametrize("n", [257, 1002, 2000])
def test_forced_hbm_multistart_is_independent_of_the_split(hbm, n):
    """1, 2, 3, 5 and R + 2 contexts on device 0 (R + 2: two empty shards at the end; first = 5).  Only ctxs[0] carries the flag — it
    decides for the call, as the header says."""
    import teeline_amd as TA
    seed, first, xy_seed = 99, 5, 40 + n
    xy = O.synth_xy(n, seed=xy_seed)
    want = oracle_outputs([oracle_restart(xy_seed, n, seed, r) for r in range(first, first + R)], first)
    for k in (1, 2, 3, 5, R + 2):
        cs = [hbm] + [TA.Context(0) for _ in range(k - 1)]
        try:
            sol, costs = TA.two_opt.multistart_devices(prob(xy), R, cs, seed=seed, first=first, return_costs=True)
            assert all(ran_the_hbm_form(c) for c in cs[:min(k, R)])
        finally:
            [c.close() for c in cs[1:]]
        assert outputs(sol, costs) == want, f"n={n}: {k} contexts"
        assert_times(sol.stats)


def test_kernel_ms_with_an_empty_shard(hbm):
    """kernel_ms of the HBM-form multi-start is the largest of the shards' summed device times.  One restart over two contexts leaves the
    second shard empty: like the one-context call the value is one shard's sum — positive and within the call's wall time.  (Several
    contexts on ONE device cannot show a speed-up: no ratio is asserted.)"""
    import teeline_amd as TA
    n = 1002
    xy = O.synth_xy(n, seed=40 + n)
    one = TA.two_opt.multistart(prob(xy), 1, seed=99, first=6, ctx=hbm)
    with TA.Context(0) as c2:
        two = TA.two_opt.multistart_devices(prob(xy), 1, [hbm, c2], seed=99, first=6)
        with pytest.raises(TA.TeelineGpuError):  # (the empty shard's context was never used)
            c2.two_opt_last_counters()
    assert_times(one.stats)
    assert_times(two.stats)
    assert list(one.route()) == list(two.route()) == oracle_restart(40 + n, n, 99, 6)[0].tolist()


@pytest.mark.parametrize("m,seed,first,tied", [(8, 2, 5, (6, 11)), (12, 5, 5, (8, 10))])
def test_equal_costs_go_to_the_lower_restart(ctx, hbm, m, seed, first, tied):
    """Two restarts that end at the same f32 cost with different tours: a 2 x m unit lattice (every length exact), instances found with the
    oracle — m = 8, seed 2: restarts 6 and 11 both reach 16.0, the minimum of restarts 5..11; m = 12, seed 5: restarts 8 and 10 reach
    25.414213.  Over two contexts restarts 5..8 and 9..11 are dealt apart, so the tie is decided across shards as well as inside one."""
    import teeline_amd as TA
    n = 2 * m
    xy = np.array([[x, y] for y in range(2) for x in range(m)], np.float32)
    per = []
    for r in range(first, first + R):
        rc, route, cost, st = O.two_opt(xy, None, n, init=O.restart_perm(n, seed, r))
        per.append((route, cost, st))
    lo, hi = tied
    bits = [f32bits(c) for _, c, _ in per]
    assert bits[lo - first] == bits[hi - first] == min(bits) and per[lo - first][0].tolist() != per[hi - first][0].tolist()  # the instance is what it says
    want = oracle_outputs(per, first)
    assert want[2] == lo
    got = TA.two_opt.multistart(prob(xy), R, seed=seed, first=first, ctx=hbm, return_costs=True)
    assert outputs(*got) == want
    got = TA.two_opt.multistart(prob(xy), R, seed=seed, first=first, ctx=ctx, return_costs=True)
    assert outputs(*got) == want
    for k in (2, 3, R):
        cs = [hbm] + [TA.Context(0) for _ in range(k - 1)]
        try:
            assert outputs(*TA.two_opt.multistart_devices(prob(xy), R, cs, seed=seed, first=first, return_costs=True)) == want, f"{k} contexts"
        finally:
            [c.close() for c in cs[1:]]


def test_forced_hbm_population_equals_single_descents_and_the_oracle(hbm):
    import teeline_amd as TA
    n = 1002
    xy = O.synth_xy(n, seed=61)
    optimum = O.two_opt(xy, None, n, init=O.restart_perm(n, 4, 2))[1]
    tours = [np.arange(n, dtype=np.uint32), O.nearest_neighbor(xy, None, n, 3)[1], O.restart_perm(n, 4, 0), O.restart_perm(n, 4, 1), optimum]
    sols = TA.two_opt.solve_population(prob(xy), [[int(v) for v in t] for t in tours], ctx=hbm)
    assert ran_the_hbm_form(hbm)
    assert_times(sols[0].stats)
    total = dict.fromkeys(COUNTERS, 0)
    for k, (t, s) in enumerate(zip(tours, sols)):
        rc, route, cost, st = O.two_opt(xy, None, n, init=t)
        one = TA.two_opt.solve(prob(xy), None, None, [int(v) for v in t], ctx=hbm)
        assert list(s.route()) == route.tolist() == list(one.route()), f"tour {k}"
        assert f32bits(s.total) == f32bits(cost) == f32bits(one.total), f"tour {k}"
        assert all(one.stats[c] == st[c] for c in COUNTERS)
        for c in COUNTERS:
            total[c] += st[c]
    assert all(sols[0].stats[c] == total[c] for c in COUNTERS)  # (the call's counters are the sum over its tours)
    assert O.two_opt(xy, None, n, init=optimum)[3]["moves"] == 0


def test_multistart_one_past_the_lds_limit_over_two_contexts(ctx):
    """n = tl_two_opt_lds_max_n + 1 without the flag: two seeded restarts dealt over two contexts (one per context) against two tl_two_opt
    calls from the oracle's start permutations.  A random start of 16 K cities is seconds of descent in the HBM form; the oracle would
    need minutes, so the single descents stand in for it (they are the oracle's elsewhere: test_large_n_path_matches_oracle).
    Measured on the MI355X: 6.1 s for the four descents (two in the multi-start call, two single), well under a tenth of the suite's limit, so
    both restarts stay — one per context, which is all R = 2 over two contexts can be."""
    import teeline_amd as TA
    n = ctx.two_opt_lds_max_n() + 1
    xy = O.synth_xy(n, seed=11)
    seed, first = 7, 2
    with TA.Context(0) as c2:
        sol, costs = TA.two_opt.multistart_devices(prob(xy), 2, [ctx, c2], seed=seed, first=first, return_costs=True)
        assert ran_the_hbm_form(ctx) and ran_the_hbm_form(c2)
        singles = [TA.two_opt.solve(prob(xy), None, None, [int(v) for v in O.restart_perm(n, seed, first + r)], ctx=c) for r, c in enumerate((c2, ctx))]
    b = int(np.argmin([key(s.total, first + r) for r, s in enumerate(singles)]))
    assert [f32bits(c) for c in costs] == [f32bits(s.total) for s in singles]
    assert list(sol.route()) == list(singles[b].route()) and f32bits(sol.total) == f32bits(singles[b].total) and sol.stats["best_restart"] == first + b
    for c in COUNTERS:
        assert sol.stats[c] == singles[0].stats[c] + singles[1].stats[c]
    assert_times(sol.stats)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. tl_two_opt_last_counters
# ---------------------------------------------------------------------------------------------------------------------------------
def _lk_args(c, xy, n, out, cost, st, o):
    return (c.handle, xy.ctypes.data_as(C.c_void_p), n, None, None, C.byref(o), 9, out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(st))


def _other_user(kind, c, xy, n):
    """one call of another user of the context's out_stats buffer (or, for tl_lk, of the context)"""
    import torch
    from teeline_amd import _capi
    out = np.empty(n, dtype=np.uint32)
    cost, st, o = C.c_float(), _capi.TlStats(), _capi.TlLkOpts(30, 10, 5, 5)
    if kind in ("lk", "lk_ils_lds"):
        c.check(c.lib.tl_lk(*_lk_args(c, xy, n, out, cost, st, o)))
    elif kind == "lk_trace":
        cap = 64  # (64 f32 distances: more than the 128 bytes of one descent's counters)
        snaps, dists, ln = np.empty((cap, n), dtype=np.uint32), np.empty(cap, dtype=np.float32), C.c_uint32()
        c.check(c.lib.tl_lk_trace(*_lk_args(c, xy, n, out, cost, st, o), snaps.ctypes.data_as(C.c_void_p), dists.ctypes.data_as(C.c_void_p), cap, C.byref(ln)))
        assert ln.value >= 1
    elif kind == "lk_live":
        seen = []
        cb = _capi.LK_PROGRESS_FN(lambda user, pos, nn, d: seen.append(d))
        c.check(c.lib.tl_lk_live(*_lk_args(c, xy, n, out, cost, st, o), cb, None))
        assert seen
    elif kind == "batch_dev":
        dev = torch.device("cuda:0")
        d_xy = torch.from_numpy(xy).to(dev)
        d_pos = torch.empty((2, n), dtype=torch.int32, device=dev)
        d_cost = torch.empty(2, dtype=torch.float32, device=dev)
        d_stats = torch.zeros(2 * _capi.TL_DEV_STATS_STRIDE, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()  # (the context's own stream is not ordered with torch's)
        c.check(c.lib.tl_two_opt_batch_dev(c.handle, d_xy.data_ptr(), n, None, 3, 0, 2, _capi.TL_MODE_REF_ORDER, d_pos.data_ptr(), d_cost.data_ptr(),
                                           d_stats.data_ptr(), None))
        c.last_kernel_ms()  # (waits for the batch)
        assert int(d_stats[0].item()) >= 1
    else:
        raise ValueError(kind)


def _refused(c):
    import teeline_amd as TA
    with pytest.raises(TA.TeelineGpuError) as e:
        c.two_opt_last_counters()
    assert e.value.code == TA._capi.TL_ERR_BADARG and "tl_two_opt_last_counters" in str(e.value)


def _descent_counters(c, xy, n, init):
    import teeline_amd as TA
    sol = TA.two_opt.solve(prob(xy), None, None, [int(v) for v in init], ctx=c)
    rc, route, cost, st = O.two_opt(xy, None, n, init=init)
    cnt = c.two_opt_last_counters()
    assert (cnt[0], cnt[1], cnt[2], cnt[3]) == (st["sweeps"], st["moves"], st["reversed"], 0), "not this descent's counters"
    assert list(sol.route()) == route.tolist()
    return cnt


@pytest.mark.parametrize("kind", ["lk", "lk_ils_lds", "lk_trace", "lk_live", "batch_dev"])
def test_last_counters_are_two_opt_counters_or_an_error(kind):
    import teeline_amd as TA
    n = 700 if kind == "lk_ils_lds" else 400
    xy = O.synth_xy(n, seed=12)
    flags = TA.TL_FLAG_LK_ILS_LDS if kind == "lk_ils_lds" else TA.TL_FLAG_NONE
    # on a fresh context: nothing but the other call has happened
    with TA.Context(0, flags) as c:
        _other_user(kind, c, xy, n)
        _refused(c)
        _descent_counters(c, xy, n, O.restart_perm(n, 1, 0))  # ... and a following descent's counters are its own again
    # behind a descent whose counters the context holds
    with TA.Context(0, flags) as c:
        before = _descent_counters(c, xy, n, O.restart_perm(n, 1, 1))
        _other_user(kind, c, xy, n)
        if kind in ("lk", "lk_ils_lds"):  # tl_lk without snapshots does not touch the buffer: still the last 2-opt call's counters, word for word
            assert c.two_opt_last_counters() == before
        else:
            _refused(c)
        _descent_counters(c, xy, n, O.restart_perm(n, 1, 2))


def test_last_counters_after_forms_without_kernel_side_counters(hbm):
    """The HBM form and BEST_SWEEP keep their counters elsewhere: after them the call must not hand out an earlier descent's."""
    import teeline_amd as TA
    n = 300
    xy = O.synth_xy(n, seed=2)
    with TA.Context(0) as c:
        _descent_counters(c, xy, n, O.restart_perm(n, 1, 0))
        TA.two_opt.solve(prob(xy), None, None, None, ctx=c, mode=TA.TL_MODE_BEST_SWEEP)
        _refused(c)
    TA.two_opt.solve(prob(xy), None, None, None, ctx=hbm)
    _refused(hbm)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the list of long cities
# ---------------------------------------------------------------------------------------------------------------------------------
LONG_CAP = 1024  # kDmLongCap (teeline_amd/csrc/tl_kernels.h)


def hub_instance(n=3000, cluster=400, moved=275, seed=5):
    """n - cluster cities in the unit square, `cluster` cities in a 0.05 square far away (their 16 nearest are all in the cluster); the
    tour is the NN tour with `moved` cluster cities put between spread cities: each of them and both its tour neighbours are long."""
    rng = np.random.default_rng(seed)
    spread = rng.random((n - cluster, 2), dtype=np.float32)
    far = np.float32(40.0) + rng.random((cluster, 2), dtype=np.float32) * np.float32(0.05)
    xy = np.concatenate([spread, far]).astype(np.float32)
    nn = O.nearest_neighbor(xy, None, n, 3)[1]
    is_far = nn >= n - cluster
    farc, rest = nn[is_far], nn[~is_far]
    out, step, k = [], len(rest) // (moved + 1), 0
    for i, c in enumerate(rest):
        out.append(c)
        if (i + 1) % step == 0 and k < moved and i > 3:
            out.append(farc[k])
            k += 1
    out.extend(farc[k:])
    return xy, np.asarray(out, np.uint32)


def long_city_counts(packed, n, init, trace):
    """What the kernel's list of long cities holds, from the oracle's move list: per sweep (long cities at its start, whether it may run on
    the lists, the move of the sweep at which the list passes LONG_CAP or None).  A city is long while one of its tour edges inside
    the open path exceeds its 16th smallest distance; within a sweep cities only enter the list (a move's four end points)."""
    rc, route, cost, st, ij, dist, sw = trace
    full = O.dm_expand_full(packed, n)
    f = full.copy()
    np.fill_diagonal(f, np.inf)
    dk = np.partition(f, 15, axis=1)[:, 15]
    perm = np.asarray(init, np.int64).copy()

    def is_long(k):
        u = perm[k]
        return (k >= 1 and not full[perm[k - 1], u] <= dk[u]) or (k + 1 < n and not full[u, perm[k + 1]] <= dk[u])

    rows, m = [], 0
    for s in range(1, st["sweeps"] + 1):
        listed = {int(perm[k]) for k in range(n) if is_long(k)}
        nl0, passed, mv = len(listed), None, 0
        while m < len(ij) and sw[m] == s:
            i, j = int(ij[m][0]), int(ij[m][1])
            perm[i + 1:j + 1] = perm[i + 1:j + 1][::-1].copy()
            listed.update(int(perm[k]) for k in (i, i + 1, j, j + 1) if k < n and is_long(k))
            m += 1
            mv += 1
            if passed is None and len(listed) > LONG_CAP:
                passed = mv
        rows.append((nl0, nl0 <= LONG_CAP, passed))
    assert perm.tolist() == route.tolist()
    return rows


def test_a_late_sweep_that_outgrows_the_long_list_leaves_the_lists():
    """n = 3000, one far cluster: the first sweep starts with 994 long cities (<= 1024: it runs on the lists under TL_FLAG_2OPT_NL_ALWAYS), its
    moves make more, and at its 570th move the list is full — the rest of the sweep has to run in the other block shapes.  The counts are
    derived here from the oracle's move list; tour, cost bits and counters must be the oracle's in all three forms."""
    import teeline_amd as TA
    xy, init = hub_instance()
    n = len(xy)
    packed = O.dm_build_packed(xy)
    trace = O.two_opt_trace(None, packed, n, init=init)
    rows = long_city_counts(packed, n, init, trace)
    assert rows[0][1] and rows[0][2] is not None and rows[0][2] > 16, rows[:3]  # sweep 1: on the lists, then past their capacity
    assert all(late and passed is None for _, late, passed in rows[1:])
    rc, oroute, ocost, ost = trace[:4]
    for name, flags in (("always", TA.TL_FLAG_2OPT_NL_ALWAYS), ("default", TA.TL_FLAG_NONE), ("off", TA.TL_FLAG_2OPT_NO_NL)):
        with TA.Context(0, flags) as c:
            sol = TA.two_opt.solve(prob(xy, packed), None, None, [int(v) for v in init], ctx=c)
            cnt = c.two_opt_last_counters()
        assert list(sol.route()) == oroute.tolist(), name
        assert f32bits(sol.total) == f32bits(ocost), name
        assert all(sol.stats[k] == ost[k] for k in COUNTERS), name
        if name == "always":
            assert cnt[6] == ost["sweeps"], "every sweep begins on the lists here"
        if name == "off":
            assert cnt[5:8] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. call order on one grow-only context
# ---------------------------------------------------------------------------------------------------------------------------------
def _lk(c, xy, n, epochs, seed):
    import teeline_amd as TA
    h = TA.HeuristicOptions(epochs=epochs, platoo_epochs=10, n_nearest=5)
    sol = TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, 5), None, None, ctx=c, seed=seed)
    return ("lk", list(sol.route()), f32bits(sol.total), tuple(sol.stats[k] for k in COUNTERS))


def _sol(s):
    return (list(s.route()), f32bits(s.total), tuple(s.stats[k] for k in COUNTERS))


def _rc(s):
    return (list(s.route()), f32bits(s.total))


def _sm(s):
    """route, cost bits, sweeps and moves (what the 3-opt / Or-opt parity tests compare)"""
    return _rc(s) + (s.stats["sweeps"], s.stats["moves"])


def _osm(o):
    rc, route, cost, st = o
    assert rc == 0
    return (route.tolist(), f32bits(cost), st["sweeps"], st["moves"])


def _osol(o):
    rc, route, cost, st = o
    assert rc == 0
    return (route.tolist(), f32bits(cost), tuple(st[k] for k in COUNTERS))


def _dm_full(c, xy, n):
    from teeline_amd import _capi
    out = np.empty((n, n), dtype=np.float32)
    ms = C.c_double()
    c.check(c.lib.tl_dm_build(c.handle, xy.ctypes.data_as(C.c_void_p), n, _capi.TL_DIST_EUC2D, _capi.TL_DM_FULL, out.ctypes.data_as(C.c_void_p), C.byref(ms)))
    return out.tobytes()


def _trace(c, xy, n, init):
    from teeline_amd import _capi
    out, log = np.empty(n, dtype=np.uint32), np.empty(16 * n, dtype=np.uint32)
    cost, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
    c.check(c.lib.tl_two_opt_trace(c.handle, xy.ctypes.data_as(C.c_void_p), n, None, init.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                   C.byref(cost), C.byref(st), log.ctypes.data_as(C.c_void_p), len(log), C.byref(ln)))
    assert ln.value <= len(log)
    return (out.tolist(), f32bits(cost.value), tuple(getattr(st, k) for k in COUNTERS), log[:ln.value].tolist())


def _otrace(xy, n, init):
    rc, route, cost, st, ij, dist, sw = O.two_opt_trace(xy, None, n, init=init)
    words, cur = O.trace_words(ij, sw)
    words += [0xFFFFFFFF] * (st["sweeps"] - cur)
    return (route.tolist(), f32bits(cost), tuple(st[k] for k in COUNTERS), words)


def _jobs():
    """(name, size for the orders, run(ctx) -> outputs, oracle() -> the same outputs).  Every instance its own seed."""
    import teeline_amd as TA
    jobs = []

    def add(name, n, run, want):
        jobs.append((name, n, run, want))

    xy_a = O.synth_xy(700, seed=101)
    add("dm_build packed", 700, lambda c: TA.distance_matrix.build(np.arange(700), xy_a, ctx=c).items.tobytes(), lambda: O.dm_build_packed(xy_a).tobytes())
    xy_b = O.synth_xy(333, seed=102)
    add("dm_build full", 333, lambda c: _dm_full(c, xy_b, 333), lambda: O.dm_expand_full(O.dm_build_packed(xy_b), 333).tobytes())
    xy_c, init_c = O.synth_xy(3000, seed=103), O.restart_perm(3000, 2, 0)
    add("2-opt coordinates", 3000, lambda c: _sol(TA.two_opt.solve(prob(xy_c), None, None, [int(v) for v in init_c], ctx=c)),
        lambda: _osol(O.two_opt(xy_c, None, 3000, init=init_c)))
    xy_d, init_d = O.synth_xy(1002, seed=104), O.nearest_neighbor(O.synth_xy(1002, seed=104), None, 1002, 3)[1]
    pk_d = O.dm_build_packed(xy_d)
    add("2-opt matrix", 1002, lambda c: _sol(TA.two_opt.solve(prob(xy_d, pk_d), None, None, [int(v) for v in init_d], ctx=c)),
        lambda: _osol(O.two_opt(None, pk_d, 1002, init=init_d)))
    xy_e, init_e = O.synth_xy(150, seed=105), O.restart_perm(150, 2, 1)
    add("2-opt trace", 150, lambda c: _trace(c, xy_e, 150, init_e), lambda: _otrace(xy_e, 150, init_e))
    xy_f = O.synth_xy(500, seed=106)
    add("multi-start", 500, lambda c: outputs(*TA.two_opt.multistart(prob(xy_f), 5, seed=3, first=2, ctx=c, return_costs=True)),
        lambda: oracle_outputs([O.two_opt(xy_f, None, 500, init=O.restart_perm(500, 3, r))[1:] for r in range(2, 7)], 2))
    xy_g = O.synth_xy(260, seed=107)
    pop_g = [O.restart_perm(260, 5, r) for r in range(3)]
    add("population", 260, lambda c: [_rc(s) for s in TA.two_opt.solve_population(prob(xy_g), [[int(v) for v in t] for t in pop_g], ctx=c)],
        lambda: [_osol(O.two_opt(xy_g, None, 260, init=t))[:2] for t in pop_g])
    xy_h, init_h = O.synth_xy(52, seed=108), O.restart_perm(52, 6, 0)
    add("3-opt", 52, lambda c: _sm(TA.three_opt.solve(prob(xy_h), None, None, [int(v) for v in init_h], ctx=c)),
        lambda: _osm(O.three_opt(xy_h, None, 52, init=init_h)))
    xy_i, init_i = O.synth_xy(200, seed=109), O.restart_perm(200, 6, 1)
    add("Or-opt", 200, lambda c: _sm(TA.or_opt.solve(prob(xy_i), None, None, [int(v) for v in init_i], ctx=c)),
        lambda: _osm(O.or_opt(xy_i, None, 200, init=init_i)))
    xy_j = O.synth_xy(1200, seed=110)
    add("candidates k=3", 1200, lambda c: TA.lin_kernighan.build_candidates(prob(xy_j), 3, ctx=c).tolist(), lambda: _cand(xy_j, 3))
    xy_k = O.synth_xy(90, seed=111)
    add("candidates k=40", 90, lambda c: TA.lin_kernighan.build_candidates(prob(xy_k), 40, ctx=c).tolist(), lambda: _cand(xy_k, 40))
    xy_l = O.synth_xy(2000, seed=112)
    add("NN seed", 2000, lambda c: _rc(TA.nearest_neighbor.solve(prob(xy_l), ctx=c)), lambda: (lambda r: (r[1].tolist(), f32bits(r[2])))(O.nearest_neighbor(xy_l, None, 2000, 3)))
    xy_m = O.synth_xy(400, seed=113)
    add("LK, LDS form", 400, lambda c: _lk(c, xy_m, 400, 30, 4), lambda: ("lk",) + _osol(O.lin_kernighan_trace(xy_m, epochs=30, platoo_epochs=10, seed=4)[:4]))
    xy_n = O.synth_xy(1000, seed=114)
    add("LK, chip-wide form", 1000, lambda c: _lk(c, xy_n, 1000, 12, 5), lambda: ("lk",) + _osol(O.lin_kernighan_trace(xy_n, epochs=12, platoo_epochs=10, seed=5)[:4]))
    xy_o = O.synth_xy(600, seed=115)
    add("greedy edge", 600, lambda c: _rc(TA.greedy_edge.solve(prob(xy_o), ctx=c)), lambda: (lambda r: (r[0].tolist(), f32bits(r[1])))(G.greedy_edge(xy_o)))
    return jobs


def _cand(xy, k):
    lists, tie_free = O.build_candidates_kdtree(xy, k)
    assert tie_free  # (with ties the reference's order is the tree's visiting order, which the brute-force kernel does not promise)
    return lists.tolist()


def _fill_with_stale_data(c):
    """a large job of each kind, so that the small jobs behind it run inside buffers full of another solver's data"""
    import teeline_amd as TA
    n = 4000
    xy = O.synth_xy(n, seed=201)
    nn = [int(v) for v in O.nearest_neighbor(xy, None, n, 3)[1]]
    packed = TA.distance_matrix.build(np.arange(n), xy, ctx=c).items          # dm
    TA.two_opt.solve(prob(xy, packed), None, None, nn, ctx=c)                  # dmfull, dmx, out_*
    TA.two_opt.solve(prob(xy), None, None, nn, ctx=c)                          # xy, init, nl
    TA.two_opt.solve_population(prob(xy), [nn] * 8, ctx=c)                     # init, out_pos, out_cost, out_stats for 8 tours
    TA.two_opt.solve(prob(xy), None, None, nn, ctx=c, mode=TA.TL_MODE_BEST_SWEEP)  # work
    TA.lin_kernighan.build_candidates(prob(xy), 40, ctx=c)                     # kd, misc
    TA.nearest_neighbor.solve(prob(xy), ctx=c)
    h = TA.HeuristicOptions(epochs=2, platoo_epochs=2, n_nearest=8)
    TA.lin_kernighan.solve(prob(xy), TA.LKOptions(h, 5), lambda k, p: None, None, ctx=c)  # work; out_pos / out_stats as the snapshot ring
    TA.greedy_edge.solve(prob(xy[:1500]), ctx=c)
    TA.or_opt.find_best_move(prob(xy), np.asarray(nn, np.uint32), ctx=c)
    TA.three_opt.find_best_move(prob(xy[:1000]), np.arange(1000, dtype=np.uint32), ctx=c)


def test_call_order_on_one_context_does_not_show_in_any_result():
    import teeline_amd as TA
    jobs = _jobs()
    want = [w() for _, _, _, w in jobs]
    by_size = sorted(range(len(jobs)), key=lambda k: (-jobs[k][1], k))
    orders = {"largest first": by_size, "smallest first": by_size[::-1], "seeded shuffle": [int(v) for v in np.random.default_rng(8).permutation(len(jobs))]}
    with TA.Context(0) as c:
        _fill_with_stale_data(c)
        for oname, order in orders.items():
            for k in order:
                got = jobs[k][2](c)
                assert got == want[k], f"order '{oname}', job {k} ({jobs[k][0]}, n={jobs[k][1]}) differs from the oracle"
    for k, (name, n, run, _) in enumerate(jobs):  # ... and each on a context of its own
        with TA.Context(0) as c:
            assert run(c) == want[k], f"fresh context, job {k} ({name}, n={n}) differs from the oracle"
