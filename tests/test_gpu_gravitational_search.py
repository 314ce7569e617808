"""The gravitational search solver on the GPU (tl_gravitational_search*, csrc/gravitational_search.hip) against the statement of its
specification (tests/_gsa_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every
record of the improvement log with its route, every word of the per-epoch record (every agent's cost bits, velocity length and
live pulls, and g's bits — which pin the draws, the masses and the stable ranking, the pulls from the positions as they stand, the
cut to v_max and the sequential sums) and the stats against the oracle's counters — in both input forms, for the runs of a batch and
for every span of epochs a launch; and the device's pull alone (tl_gsa_selftest_pull) on planted pairs."""
import ctypes as C
import functools

import numpy as np
import pytest

import _gsa_cases as GC
import _gsa_oracle as GO
import _sa_cases as K
import _swarm_harness as H
from _raw_context import _vp

pytestmark = pytest.mark.gpu

WORK = H.WORK
bits = GO.bits
FAST = GO.swap_sequence_inverse  # (tests/test_gsa_oracle.py: equal to the literal search)
GOLDEN = GC.golden_cases()


GSA = H.GSA
_opts = GSA.opts
gpu_trace, gpu_population, plan, check_run = (functools.partial(f, GSA) for f in (H.gpu_trace, H.gpu_population, H.plan, H.check_run))
okey = H.okey


# ---------------------------------------------------------------- the device's pull alone
def device_pull(ctx, src, dst, prefix, n):
    count = len(src)
    a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (src, dst)]
    p = np.ascontiguousarray(prefix, dtype=np.uint32)
    pairs = np.full((count, 20), 0xDEADBEEF, dtype=np.uint32)
    ln = np.full(count, 0xFFFFFFFF, dtype=np.uint32)
    rc = ctx.lib.tl_gsa_selftest_pull(ctx.handle, _vp(a[0]), _vp(a[1]), _vp(p), n, count, _vp(pairs), _vp(ln))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    return pairs, ln


def check_pulls(ctx, n, cases):
    names = sorted(cases)
    pairs, ln = device_pull(ctx, [cases[k][0] for k in names], [cases[k][1] for k in names], [cases[k][2] for k in names], n)
    for r, name in enumerate(names):
        src, dst, m = cases[name]
        want = GO.pairs_words(GO.pull([int(v) for v in src], [int(v) for v in dst], m, seq=FAST))
        assert ln[r] == len(want) and pairs[r, :len(want)].tolist() == want and (pairs[r, len(want):] == 0xFFFFFFFF).all(), (n, name)
    return {name: int(ln[r]) for r, name in enumerate(names)}


def test_selftest_pull_on_planted_pairs(ctx):
    """identical permutations; agreement on the first 60 / 64 / 70 / 255 / 256 positions and a difference after — the prefix starts in
    a later chunk of 64 positions and crosses a chunk boundary (the condition prefix_past_64_positions, which no small seeded run
    reaches); one n-cycle in both directions; three pairs spread over five chunks; m = 0, 1, 20 and above the sequence's length"""
    lens = check_pulls(ctx, 600, GC.planted_pairs(600))
    assert lens["identical"] == 0 and lens["prefix_above_the_length"] == 1 and lens["prefix_1"] == 1 and lens["prefix_20"] == 20 and lens["prefix_0"] == 0
    assert lens["agree_255"] == 20 and lens["one_n_cycle_down"] == 20 and lens["sparse_pairs"] == 3


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130, 300])
def test_selftest_pull_sizes(ctx, n):
    rng = np.random.default_rng(n)
    perm = lambda: rng.permutation(n).astype(np.uint32)  # noqa: E731
    base = perm()
    cases = {"same": (base, base.copy(), 20), "up": (base, np.roll(base, -1), 20), "down": (base, np.roll(base, 1), 20)}
    for k in range(6):
        cases[f"random_{k}"] = (perm(), perm(), (0, 1, 2, 7, 19, 20)[k])
    check_pulls(ctx, n, cases)


def test_selftest_pull_at_the_limit(ctx):
    n = ctx.lib.tl_gravitational_search_max_n(ctx.handle)
    assert n >= 19000
    rng = np.random.default_rng(5)
    base = rng.permutation(n).astype(np.uint32)
    late = base.copy()
    late[n - 40:] = np.roll(base[n - 40:], 1)  # the first pair at n - 40: the wave walks every chunk
    check_pulls(ctx, n, {"random": (base, rng.permutation(n).astype(np.uint32), 20), "late": (base, late, 20), "down": (base, np.roll(base, 1), 20)})


def test_selftest_pull_refusals(ctx):
    from teeline_amd import _capi
    a = np.arange(8, dtype=np.uint32)
    p = np.array([21], dtype=np.uint32)
    out, ln = np.zeros(20, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert ctx.lib.tl_gsa_selftest_pull(ctx.handle, _vp(a), _vp(a), _vp(p), 8, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG  # a prefix above 20
    bad = a.copy()
    bad[0] = 1
    p[0] = 3
    assert ctx.lib.tl_gsa_selftest_pull(ctx.handle, _vp(a), _vp(bad), _vp(p), 8, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_gsa_selftest_pull(ctx.handle, _vp(a), _vp(a), _vp(p), 0, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_gsa_selftest_pull(ctx.handle, None, _vp(a), _vp(p), 8, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG


# ---------------------------------------------------------------- whole runs
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    """berlin52 in the coordinate form and gr17 in the matrix form, each with and without an initial tour; N = 65 agents"""
    xy, packed, n, init, o = GOLDEN[name]
    res = check_run(ctx, name, xy, packed, n, init, o)
    GC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(GC.SEEDED))
def test_seeded_cases(ctx, name):
    """n = 3, 5, 6, 8, 52, 130, 600: each shows on the oracle's record the conditions it is there for"""
    xy, _packed, n, init, o, want = GC.seeded_case(name)
    res = check_run(ctx, ("seeded", name), xy, None, n, init, o, seq=FAST if n >= 600 else GO.swap_sequence_literal)
    assert want and set(want) <= GC.conditions(res)


@pytest.mark.parametrize("n", [2, 65])
def test_further_sizes(ctx, n):
    xy = K.synth(n, 900 + n)
    check_run(ctx, "size", xy, None, n, GC.start_tour(n, n) if n == 65 else None, dict(epochs=4, n_nearest=3, seed=n, run=1))


def test_at_the_lds_limit(ctx):
    """n = tl_gravitational_search_max_n, one epoch, N = 25"""
    n = ctx.lib.tl_gravitational_search_max_n(ctx.handle)
    info = ctx.device_info()
    assert n == max(m for m in range(info["lds_bytes"] // 9, info["lds_bytes"] // 8 + 1) if 1536 + ((4 * m + 15) & ~15) + 2 * ((2 * m + 15) & ~15) <= info["lds_bytes"])
    xy = K.synth(n, 77)
    res = check_run(ctx, "limit", xy, None, n, None, dict(epochs=1, n_nearest=3, seed=9, run=0), seq=FAST)
    assert any(m["pulls"] for m in res["epochs"][0]["moves"])


def test_small_n_runs_on_the_host(ctx):
    for n in (0, 1):
        o = dict(epochs=3, n_nearest=3, seed=1, run=0)
        res = GO.solve(K.small(3)[:n], None, n, None, **o)
        rc, out, cost, log, ln, st, routes, elog = gpu_trace(ctx, K.small(3), None, n, None, o)
        assert rc == 0 and out.tolist() == list(range(n)) and cost == 0 and ln == 1 and log.tolist() == GO.log_words(res).tolist()
        assert elog.tolist() == GO.epoch_words(res).tolist() and (st["sweeps"], st["candidates"], st["moves"]) == (3, 75, 0)


# ---------------------------------------------------------------- population, spans
def test_population_equals_single_runs_and_offsets(ctx):
    xy, _packed, n, _init, o = GOLDEN["berlin52"]
    o = dict(o, epochs=8)
    singles = [GO.solve_cached(okey("pop", n, None, dict(o, run=r)), xy, None, n, None, **dict(o, run=r)) for r in range(5)]
    rc, out, costs, moves, best, st = gpu_population(ctx, xy, None, n, None, 0, 0, 3, o)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    for r in range(3):
        assert out[r].tolist() == singles[r]["tour"].tolist() and bits(costs[r]) == bits(singles[r]["cost"]) and moves[r] == singles[r]["counters"]["improved"]
        rc1, o1, c1, _l, _n, _s, _r, _e = gpu_trace(ctx, xy, None, n, None, dict(o, run=r))
        assert rc1 == 0 and o1.tolist() == out[r].tolist() and bits(c1) == bits(costs[r])
    assert best == int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles[:3])]))
    assert (st["sweeps"], st["candidates"], st["moves"]) == (24, 3 * 8 * 25, sum(s["counters"]["improved"] for s in singles[:3]))
    rc, out, costs, moves, _b, _s = gpu_population(ctx, xy, None, n, None, 0, 3, 2, o)  # first_run = 3: runs 3 and 4
    assert rc == 0 and [out[k].tolist() for k in range(2)] == [singles[3 + k]["tour"].tolist() for k in range(2)]
    inits = np.stack([GC.start_tour(n, 40 + k) for k in range(2)])
    rc, out, costs, _m, _b, _s = gpu_population(ctx, xy, None, n, inits, 2, 1, 2, o)  # a start tour per run
    for k in range(2):
        want = GO.solve(xy, None, n, inits[k], **dict(o, run=1 + k))
        assert rc == 0 and out[k].tolist() == want["tour"].tolist() and bits(costs[k]) == bits(want["cost"])


@pytest.mark.parametrize("span", [1, 3, 7])
def test_the_result_does_not_depend_on_the_span(ctx, span):
    """one epoch per launch, three, seven (a last span of two) against the default, the whole schedule in one launch: identical traces"""
    for name in ("berlin52", "gr17_matrix_init"):
        xy, packed, n, init, o = GOLDEN[name]
        o = dict(o, epochs=9)
        whole = gpu_trace(ctx, xy, packed, n, init, o)
        parts = gpu_trace(ctx, xy, packed, n, init, o, span=span)
        assert whole[0] == parts[0] == 0
        for a, b in zip(whole[1:], parts[1:]):
            assert (a.tolist() == b.tolist()) if isinstance(a, np.ndarray) else (a == b or isinstance(a, dict))
        assert {k: whole[5][k] for k in ("sweeps", "candidates", "moves")} == {k: parts[5][k] for k in ("sweeps", "candidates", "moves")}
        check_run(ctx, ("span", name), xy, packed, n, init, o, span=span)


def test_log_capacities(ctx):
    xy, _packed, n, init, o = GOLDEN["small8_init"]
    res = GO.solve_cached(okey("small8_init", n, init, o), xy, None, n, init, **o)
    assert len(res["improvements"]) >= 3
    rc, out, cost, log, ln, _st, routes, elog = gpu_trace(ctx, xy, None, n, init, o, cap=2, route_cap=1, epoch_cap=3)
    assert rc == 0 and ln == len(res["improvements"]) and log.tolist() == GO.log_words(res, route_cap=1)[:2].tolist()
    assert routes.tolist() == GO.route_words(res, n)[:1].tolist() and elog.tolist() == GO.epoch_words(res)[:3].tolist()
    assert out.tolist() == res["tour"].tolist() and bits(cost) == bits(res["cost"])


# ---------------------------------------------------------------- refusals
def test_refusals_and_error_paths(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    xy = K.tsplib("berlin52")["xy"]
    o = dict(epochs=2, n_nearest=4097, seed=1)
    assert gpu_trace(ctx, xy, None, 52, None, o, route_cap=1, epoch_cap=0)[0] == _capi.TL_ERR_UNSUPPORTED  # N > 4096
    top = ctx.lib.tl_gravitational_search_max_n(ctx.handle)
    out, cost = np.zeros(4, dtype=np.uint32), C.c_float()
    po = _opts(dict(epochs=1, n_nearest=3))
    # n > max_n: refused before anything of size n is read (xy holds 52 cities only)
    assert ctx.lib.tl_gravitational_search(ctx.handle, _vp(xy), top + 1, None, None, C.byref(po), 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_UNSUPPORTED
    assert plan(ctx, top)[1:3] == (25, 256) and plan(ctx, top + 1)[1:] == (0, 0, 0) and plan(ctx, 52, 4097)[1:] == (0, 0, 0)
    assert plan(ctx, 52, 3, 1, WORK, 1 << 31)[0] == _capi.TL_ERR_UNSUPPORTED
    with TA.Context(0, 1 << 31) as odd:  # a bit no flag has
        assert gpu_trace(odd, xy, None, 52, None, dict(epochs=1, n_nearest=3, seed=1))[0] == _capi.TL_ERR_UNSUPPORTED
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 4
    assert gpu_trace(ctx, xy, None, 52, bad, dict(epochs=1, n_nearest=3, seed=1))[0] == _capi.TL_ERR_BADARG
    assert gpu_trace(ctx, xy, None, 52, None, dict(epochs=0xFFFFFFFF, n_nearest=3, seed=1), epoch_cap=0, route_cap=1)[0] == _capi.TL_ERR_UNSUPPORTED
    # where the reference panics: an inf entry on the start tour makes that cost inf, worst - c NaN and with it every mass
    g = K.tsplib("gr17")
    packed = np.array(g["packed"], dtype=np.float32)
    init = np.arange(17, dtype=np.uint32)
    packed[1 * (1 - 1) // 2 + 0] = np.inf  # d(1, 0): an edge of the start tour 0, 1, 2, ..
    with pytest.raises(GO.RefPanics):
        GO.solve(g["xy"], packed, 17, init, epochs=2, seed=1)
    rc = gpu_trace(ctx, g["xy"], packed, 17, init, dict(epochs=2, n_nearest=3, seed=1))[0]
    assert rc == _capi.TL_ERR_REF_PANICS and "partial_cmp" in ctx.lib.tl_last_error(ctx.handle).decode()
    rc, _out, cost0, *_rest = gpu_trace(ctx, g["xy"], packed, 17, init, dict(epochs=0, n_nearest=3, seed=1))  # no epoch: no ranking, no panic
    assert rc == 0 and bits(cost0) == bits(GO.solve(g["xy"], packed, 17, init, epochs=0, seed=1)["cost"])
    packed[:] = np.nan  # a NaN start cost: the first-minimum search panics, whatever the epochs
    assert gpu_trace(ctx, g["xy"], packed, 17, init, dict(epochs=0, n_nearest=3, seed=1))[0] == _capi.TL_ERR_REF_PANICS
    good = gpu_trace(ctx, g["xy"], np.array(g["packed"], dtype=np.float32), 17, init, dict(epochs=2, n_nearest=3, seed=1))  # the context is usable afterwards
    assert good[0] == 0 and sorted(good[1].tolist()) == list(range(17))


def test_new_symbols_resolve(ctx):
    """what fails without the feature"""
    for sym in ("tl_gravitational_search", "tl_gravitational_search_trace", "tl_gravitational_search_population", "tl_gsa_selftest_pull"):
        assert getattr(ctx.lib, sym)


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """a handful of the cases above on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the live list and its
    wave counts, the slots handed from the pulling waves to the applying lane, the header words, the position written back before the
    next agent reads it"""
    vp, u32 = C.c_void_p, C.c_uint32
    jctx = H.jitter(GSA, {"tl_gsa_selftest_pull": [vp, vp, vp, vp, u32, u32, vp, vp]})
    try:
        for name in ("small8", "small5_truncated", "synth130_26_agents", "berlin52_default"):
            xy, packed, n, init, o, _want = GC.seeded_case(name)
            check_run(jctx, ("seeded", name), xy, packed, n, init, o)
        xy, packed, n, init, o = GOLDEN["synth65"]
        check_run(jctx, "synth65", xy, packed, n, init, dict(o, epochs=2))
        check_pulls(jctx, 600, GC.planted_pairs(600))
    finally:
        jctx.close()
