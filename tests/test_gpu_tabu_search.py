"""Tabu search on the GPU (tl_tabu_search*, csrc/tabu_search.hip) against the numpy statement of its specification
(tests/_tabu_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every entry of the
per-epoch log (taken attempt, from, to, cost) and the stats against the oracle's counters — in both input forms, both membership
forms and for the chains of a population."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from _raw_context import _vp, jitter_context
import _sa_cases as K
from _swarm_oracle import bits
import _tabu_cases as TC
import _tabu_oracle as TO

pytestmark = pytest.mark.gpu

WORK = 8 << 30  # the workspace the entries plan with (include/teeline_gpu.h)


def gpu_trace(ctx, xy, packed, n, init, epochs, seed, chain=0, cap=None):
    from teeline_amd import _capi
    cap = cap if cap is not None else epochs + 1
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    log = np.zeros((max(cap, 1), 4), dtype=np.uint32)
    cost, ln, st = C.c_float(-1.0), C.c_uint32(), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_tabu_search_trace_chain(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), epochs, seed, chain, _vp(out), C.byref(cost), C.byref(st),
                                            _vp(log), cap, C.byref(ln))
    return rc, out[:n], np.float32(cost.value), log[:min(ln.value, cap)], ln.value, st.as_dict()


def gpu_population(ctx, xy, packed, n, init, init_count, first, count, epochs, seed):
    from teeline_amd import _capi
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    costs = np.full(count, -1.0, dtype=np.float32)
    moves = np.full(count, 0xFFFFFFFF, dtype=np.uint32)
    best, st = C.c_uint32(0xFFFFFFFF), _capi.TlStats()
    ini = None if init is None else np.ascontiguousarray(init, dtype=np.uint32)
    rc = ctx.lib.tl_tabu_search_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(ini), init_count, first, count, epochs, seed, _vp(out), _vp(costs),
                                           _vp(moves), C.byref(best), C.byref(st))
    return rc, out, costs, moves, best.value, st.as_dict()


def want_log(log):
    return [(a, f, t, bits(c)) for a, f, t, c in log]


def check_chain(ctx, key, xy, packed, n, init, epochs, seed, chain=0):
    """one chain against the oracle: tour, cost, every log entry, stats"""
    tour, cost, log, cnt = TO.solve_cached((key, seed, chain), xy, packed, n, init, epochs=epochs, seed=seed, chain=chain)
    rc, out, gcost, glog, ln, st = gpu_trace(ctx, xy, packed, n, init, epochs, seed, chain)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert ln == epochs + 1 == len(log), (key, ln)
    got = [tuple(int(v) for v in r) for r in glog]
    first_diff = next((i for i, (g, w) in enumerate(zip(got, want_log(log))) if g != w), None)
    assert first_diff is None, (key, first_diff, got[first_diff], want_log(log)[first_diff])
    assert out.tolist() == tour.tolist(), key
    assert bits(gcost) == bits(cost), (key, gcost, cost)
    assert st["sweeps"] == epochs + 1 and st["candidates"] == cnt["candidates"] and st["moves"] == cnt["bests"] and st["reversed"] == cnt["reversed"], (key, st, cnt)
    return log, cnt


def plan(ctx, n, count=1):
    info = ctx.device_info()
    w, t, per = C.c_uint32(), C.c_int(), C.c_uint32()
    assert ctx.lib.tl_tabu_search_plan(n, count, info["cus"], info["lds_bytes"], WORK, ctx.flags, C.byref(w), C.byref(t), C.byref(per)) == 0
    return w.value, t.value, per.value, info["cus"]


@pytest.fixture(scope="module")
def full():
    import teeline_amd as TA
    c = TA.Context(0, TA.TL_FLAG_TABU_FULL_COMPARE)
    yield c
    c.close()


opt_start = TC.opt_start


GOLDEN = TC.golden_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    xy, packed, n, init, epochs, seed, chain = GOLDEN[name]
    log, cnt = check_chain(ctx, name, xy, packed, n, init, epochs, seed, chain)
    TC.check_conditions(name, n, epochs, log, cnt)


@pytest.mark.parametrize("name", TC.HIT_CASES)
def test_full_compare_gives_the_same_chain(full, name):
    import teeline_amd as TA
    assert full.flags == TA.TL_FLAG_TABU_FULL_COMPARE == 1 << 30
    xy, packed, n, init, epochs, seed, chain = GOLDEN[name]
    _log, cnt = check_chain(full, name, xy, packed, n, init, epochs, seed, chain)
    assert cnt["hits"] >= 1


@pytest.mark.parametrize("n", [62, 63, 64, 65])
def test_size_edges(ctx, n):
    """n + 1 = 63, 64, 65, 66 attempts: one wave's lanes, and one more"""
    xy = K.synth(n, 300 + n)
    _log, cnt = check_chain(ctx, f"synth{n}", xy, None, n, None, 150, 40 + n)
    assert cnt["bests"] >= 1 and cnt["deepest"] >= 1


PLAN_EDGE_SEEDS = {-1: 1, 0: 1, 1: 5}  # picked on the CPU with the oracle (the conditions are asserted below)


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_plan_edges_single_chain(ctx, off):
    """n = W - 1, W, W + 1 for the plan's W, from a 2-opt local optimum.  With n = W - 1 an epoch has W attempts, 0 .. W - 1: the deepest
    possible one, attempt n, is the last lane of the only round; from n = W on attempt W opens a second round."""
    W = plan(ctx, 100)[0]
    n = W + off
    assert plan(ctx, n)[0] == W
    xy = K.synth(n, n)
    log, cnt = check_chain(ctx, f"opt{n}", xy, None, n, opt_start(xy), 59, PLAN_EDGE_SEEDS[off])
    assert cnt["forced"] >= 1 and max(a for a, *_x in log) >= min(W, n)
    if off == 1:
        assert any(W <= a < n for a, *_x in log), "a checked attempt taken in the second round"


POP_EDGE_SEEDS = {-1: 1, 0: 1, 1: 8}


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_plan_edges_population_width(ctx, off):
    """the same at the width a chain has once there are more chains than CUs: chain 0 of such a population"""
    cus = ctx.device_info()["cus"]
    W = plan(ctx, 100, cus + 1)[0]
    n = W + off
    xy = K.synth(n, n)
    start = opt_start(xy)
    seed = POP_EDGE_SEEDS[off]
    tour, cost, log, cnt = TO.solve_cached((f"opt{n}", seed, 0), xy, None, n, start, epochs=59, seed=seed, chain=0)
    assert cnt["forced"] >= 1 and max(a for a, *_x in log) >= min(W, n)
    if off == 1:
        assert any(W <= a < n for a, *_x in log)
    rc, out, costs, moves, _best, _st = gpu_population(ctx, xy, None, n, start, 1, 0, cus + 1, 59, seed)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert out[0].tolist() == tour.tolist() and bits(costs[0]) == bits(cost) and moves[0] == cnt["bests"]
    last = TO.solve_cached((f"opt{n}", seed, cus), xy, None, n, start, epochs=59, seed=seed, chain=cus)
    assert out[cus].tolist() == last[0].tolist() and bits(costs[cus]) == bits(last[1]) and moves[cus] == last[3]["bests"]


def test_hit_beyond_one_wave(ctx, full):
    """n = 65 from a 2-opt local optimum, seed 7 (picked on the CPU with the oracle): the list refuses an improving candidate"""
    xy = K.synth(65, 65)
    start = opt_start(xy)
    for c in (ctx, full):
        _log, cnt = check_chain(c, "opt65_hit", xy, None, 65, start, 59, 7)
        assert cnt["hits"] == 1 and cnt["forced"] >= 1


def test_matrix_form_equals_coordinate_form(ctx):
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    pk = np.empty(52 * 51 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(b["xy"]), 52, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    tour, cost, log, _cnt = TO.solve_cached(("berlin52", 1, 0), b["xy"], None, 52, None, epochs=600, seed=1, chain=0)
    rc, out, gcost, glog, ln, _st = gpu_trace(ctx, None, pk, 52, None, 600, 1)
    assert rc == 0 and out.tolist() == tour.tolist() and bits(gcost) == bits(cost) and ln == 601
    assert [tuple(int(v) for v in r) for r in glog] == want_log(log)


def test_plain_entry_and_truncated_trace(ctx):
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    tour, cost, log, cnt = TO.solve_cached(("berlin52", 1, 0), b["xy"], None, 52, None, epochs=600, seed=1, chain=0)
    out, gcost, st = np.zeros(52, dtype=np.uint32), C.c_float(), _capi.TlStats()
    assert ctx.lib.tl_tabu_search(ctx.handle, _vp(b["xy"]), 52, None, None, 600, 1, _vp(out), C.byref(gcost), C.byref(st)) == 0
    assert out.tolist() == tour.tolist() and bits(gcost.value) == bits(cost)
    assert (st.sweeps, st.candidates, st.moves, st.reversed) == (601, cnt["candidates"], cnt["bests"], cnt["reversed"])
    rc, out2, _c, glog, ln, _ = gpu_trace(ctx, b["xy"], None, 52, None, 600, 1, cap=5)  # truncation is reported
    assert rc == 0 and ln == 601 and len(glog) == 5 and out2.tolist() == tour.tolist()
    assert [tuple(int(v) for v in r) for r in glog] == want_log(log)[:5]
    log1, ln1 = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()  # tl_tabu_search_trace is chain 0
    assert ctx.lib.tl_tabu_search_trace(ctx.handle, _vp(b["xy"]), 52, None, None, 600, 1, _vp(out), C.byref(gcost), None, _vp(log1), 4, C.byref(ln1)) == 0
    assert ln1.value == 601 and log1.tolist() == glog[:4].tolist()


# ---------------------------------------------------------------- population
POP_EPOCHS = 40


def check_population(ctx, xy, n, init, init_count, first, count, sample):
    rc, out, costs, moves, best, st = gpu_population(ctx, xy, None, n, init, init_count, first, count, POP_EPOCHS, 31)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        start = None if init_count == 0 else init if init_count == 1 else init[r]
        key = ("pop", n, None if start is None else tuple(int(v) for v in start))
        tour, cost, _log, cnt = TO.solve_cached((key, 31, first + r), xy, None, n, start, epochs=POP_EPOCHS, seed=31, chain=first + r)
        assert out[r].tolist() == tour.tolist() and bits(costs[r]) == bits(cost) and moves[r] == cnt["bests"], (count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == (POP_EPOCHS + 1) * count and st["moves"] == int(moves.sum())
    return out, costs, moves


def test_population_counts(ctx):
    n = 5
    xy = K.small(n)
    _w, _t, per, cus = plan(ctx, n, 10 ** 6)
    assert per >= cus
    check_population(ctx, xy, n, None, 0, 0, 1, [0])
    check_population(ctx, xy, n, None, 0, 0, 2, [0, 1])
    check_population(ctx, xy, n, None, 0, 0, cus + 1, range(cus + 1))
    count = per + 1  # one more than a launch holds: a second launch
    edge = sorted({0, 1, cus, per - 1, per})
    out, costs, moves = check_population(ctx, xy, n, None, 0, 0, count, edge)
    for c in (per - 1, per):  # first_chain = c, count = 1 equals chain c of the larger population
        rc, o1, c1, m1, b1, _ = gpu_population(ctx, xy, None, n, None, 0, c, 1, POP_EPOCHS, 31)
        assert rc == 0 and b1 == 0 and o1[0].tolist() == out[c].tolist() and bits(c1[0]) == bits(costs[c]) and m1[0] == moves[c]
    assert gpu_population(ctx, xy, None, n, None, 0, 0, 0, POP_EPOCHS, 31)[0] == 0  # count == 0: TL_OK, nothing written


def test_population_start_tours_and_chain_ids(ctx):
    b = K.tsplib("berlin52")
    rng = np.random.default_rng(5)
    count = 6
    one = rng.permutation(52).astype(np.uint32)
    own = np.stack([rng.permutation(52) for _ in range(count)]).astype(np.uint32)
    check_population(ctx, b["xy"], 52, None, 0, 3, count, range(count))
    check_population(ctx, b["xy"], 52, one, 1, 0, count, range(count))
    check_population(ctx, b["xy"], 52, own, count, 100, count, range(count))
    rc, *_ = gpu_population(ctx, b["xy"], None, 52, own, 2, 0, count, POP_EPOCHS, 31)
    assert rc == -1 and ctx.lib.tl_last_error(ctx.handle).decode() == "tl_tabu_search_population: init_count is 2: 0 (city order), 1 (one start tour) or count (6)"
    assert gpu_population(ctx, b["xy"], None, 52, None, 1, 0, count, POP_EPOCHS, 31)[0] == -1  # init_count 1 without a tour
    assert ctx.lib.tl_last_error(ctx.handle).decode() == "tl_tabu_search_population: NULL argument"
    assert gpu_population(ctx, b["xy"], None, 52, None, 0, 2 ** 32 - 3, count, POP_EPOCHS, 31)[0] == -1
    assert ctx.lib.tl_last_error(ctx.handle).decode() == "tl_tabu_search_population: chain ids beyond 2^32 - 1"
    bad = own.copy()
    bad[4, 0] = bad[4, 1]
    rc, *_ = gpu_population(ctx, b["xy"], None, 52, bad, count, 0, count, POP_EPOCHS, 31)
    assert rc == -1 and "start tour 4" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_best_index_and_its_tie_rule(ctx):
    """Ten cities at (0, 0) and ten at (1, 0): a tour costs its number of crossings, exactly, and two is the least a cycle can have.  A
    chain that starts sorted can never find a shorter candidate and returns its start tour at cost 2; equal costs go to the lower chain.
    (The minimum among unequal costs is asserted for every population of this file by check_population.)"""
    xy = np.ascontiguousarray(np.array([[0, 0]] * 10 + [[1, 0]] * 10, dtype=np.float32))
    srt = np.arange(20, dtype=np.uint32)
    alt = np.ascontiguousarray(np.arange(20, dtype=np.uint32).reshape(2, 10).T.reshape(-1))  # 0 10 1 11 ...: twenty crossings
    rc, out, costs, moves, best, _ = gpu_population(ctx, xy, None, 20, srt, 1, 0, 3, 30, 7)
    assert rc == 0 and best == 0 and [bits(c) for c in costs] == [bits(2.0)] * 3 and (out == srt).all() and (moves == 0).all()
    init = np.stack([alt, srt, srt, alt])
    rc, out, costs, moves, best, _ = gpu_population(ctx, xy, None, 20, init, 4, 0, 4, 1, 7)  # two epochs: a reversal removes four crossings at the most
    assert rc == 0 and best == 1 and (out[1] == srt).all() and (out[2] == srt).all() and bits(costs[1]) == bits(costs[2]) == bits(2.0)
    assert min(costs[0], costs[3]) >= 12.0
    for r in (0, 3):
        tour, cost, _log, cnt = TO.solve_cached(("two_points", 7, r), xy, None, 20, alt, epochs=1, seed=7, chain=r)
        assert out[r].tolist() == tour.tolist() and bits(costs[r]) == bits(cost) and moves[r] == cnt["bests"]


# ---------------------------------------------------------------- lists longer than one look-up round
def check_population_chains(ctx, key, xy, packed, n, init, init_count, count, epochs, seed, sample, oracle_xy=None):
    """chains `sample` of a population against the oracle: best tour, cost, new bests.  key: the name the oracle's chains are cached under
    (check_chain's); oracle_xy: the coordinates behind a matrix"""
    rc, out, costs, moves, best, st = gpu_population(ctx, xy, packed, n, init, init_count, 0, count, epochs, seed)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert (np.sort(out, axis=1) == np.arange(n)).all()
    for r in sample:
        tour, cost, _log, cnt = TO.solve_cached((key, seed, r), xy if oracle_xy is None else oracle_xy, None, n, init, epochs=epochs, seed=seed, chain=r)
        assert out[r].tolist() == tour.tolist() and bits(costs[r]) == bits(cost) and moves[r] == cnt["bests"], (key, count, r)
    keys = [(bits(c) << 32) | r for r, c in enumerate(costs)]
    assert best == int(np.argmin(keys)) and st["sweeps"] == (epochs + 1) * count and st["moves"] == int(moves.sum())
    return st


@pytest.mark.parametrize("n", sorted(TC.WRAP_SEEDS))
def test_wrapped_ring_beyond_one_round_population_width(ctx, full, n):
    """One wave per chain looks 64 listed routes up per round.  n = 66 .. 70 from a 2-opt local optimum for 161 epochs: the list grows past
    64 routes and wraps, and (TC.check_wrapped_ring on the oracle's record) refuses a candidate because of a route at a ring index >= 64,
    refuses one after the wrap and lets improving candidates through after it.  Chain 0 of cus + 1 chains, the last chain, and chain 0
    again where every listed route is compared."""
    key, xy, packed, _n, start, epochs, seed = TC.wrap_chain(n)
    cus = ctx.device_info()["cus"]
    W = plan(ctx, n, cus + 1)[0]
    assert W == plan(ctx, n, cus + 1)[1] == 64
    _tour, _cost, log, _cnt = TO.solve_cached((key, seed, 0), xy, None, n, start, epochs=epochs, seed=seed, chain=0)
    TC.check_wrapped_ring(n, W, log, TO.record_of((key, seed, 0)))
    for c in (ctx, full):
        check_population_chains(c, key, xy, None, n, start, 1, cus + 1, epochs, seed, (0, cus))
    for c in (ctx, full):  # the same chain alone (four waves: one round), with its log
        check_chain(c, key, xy, None, n, start, epochs, seed)


def test_long_list_beyond_one_round_single_chain(ctx, full):
    """A chain alone looks 256 listed routes up per round.  n = 300 from city order for 331 epochs: improving candidates are looked up in
    a list of more than 256 routes, before and after the ring wraps at epoch 300 (TC.check_long_list).  No seed of 1 .. 13 000 gives this
    chain a true refusal, at any index (scanned with the oracle), so none at an index >= 256 is asserted.  What this case can show is a
    false hit in rows >= 256, with the hashes or with every listed route compared: that changes the chain.  Rows >= 256 that are never
    looked at change nothing here, the list refusing nothing; the one-wave case above is the one that sees a look-up cut short."""
    key, xy, packed, n, init, epochs, seed = TC.long_chain()
    W = plan(ctx, n)[0]
    assert W == 256
    for c in (ctx, full):
        log, _cnt = check_chain(c, key, xy, packed, n, init, epochs, seed)
        TC.check_long_list(n, W, log, TO.record_of((key, seed, 0)))


TOP_EPOCHS = 12


def test_at_the_lds_limit(ctx):
    """n = tl_tabu_search_lds_max_n from a seeded permutation: the ring is n x n 16-bit entries.  One chain with its log, and two chains."""
    top = ctx.lib.tl_tabu_search_lds_max_n(ctx.handle)
    assert 0 < top <= 65535 and plan(ctx, top)[0] > 0 and plan(ctx, top + 1)[:3] == (0, 0, 0)
    xy = K.synth(top, 78)
    start = np.random.default_rng(top).permutation(top).astype(np.uint32)
    _log, cnt = check_chain(ctx, "top", xy, None, top, start, TOP_EPOCHS, 9)
    assert cnt["bests"] >= 1
    assert plan(ctx, top, 2)[2] >= 2
    check_population_chains(ctx, "top", xy, None, top, start, 1, 2, TOP_EPOCHS, 9, (0, 1))


def test_matrix_form_past_one_trip(ctx):
    """n = 257 as a packed EUC_2D matrix: the chain of the coordinate form, alone and as chain 0 of cus + 1 one-wave chains"""
    from teeline_amd import _capi
    n, epochs, seed = 257, 150, 257
    xy = K.synth(n, n)
    pk = np.empty(n * (n - 1) // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), n, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    tour, cost, log, cnt = TO.solve_cached(("synth257", seed, 0), xy, None, n, None, epochs=epochs, seed=seed, chain=0)
    rc, out, gcost, glog, ln, st = gpu_trace(ctx, None, pk, n, None, epochs, seed)
    assert rc == 0 and out.tolist() == tour.tolist() and bits(gcost) == bits(cost) and ln == epochs + 1
    assert [tuple(int(v) for v in r) for r in glog] == want_log(log)
    assert (st["candidates"], st["moves"], st["reversed"]) == (cnt["candidates"], cnt["bests"], cnt["reversed"])
    cus = ctx.device_info()["cus"]
    assert plan(ctx, n, cus + 1)[1] == 64
    check_population_chains(ctx, "synth257", None, pk, n, None, 0, cus + 1, epochs, seed, (0, cus), oracle_xy=xy)


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller(ctx):
    """a stale ring must not leak: the larger instance leaves its routes and hashes where the smaller ones' lists begin"""
    import teeline_amd as TA
    with TA.Context(0) as c, TA.Context(0, TA.TL_FLAG_TABU_FULL_COMPARE) as f:
        for cc in (c, f):
            for name in ("berlin52", "small4", "gr17_matrix", "grid4x4", "small3", "small2"):
                xy, packed, n, init, epochs, seed, chain = GOLDEN[name]
                check_chain(cc, name, xy, packed, n, init, epochs, seed, chain)


def test_errors(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    b = K.tsplib("berlin52")
    err = lambda: ctx.lib.tl_last_error(ctx.handle).decode()  # noqa: E731
    bad = np.arange(52, dtype=np.uint32)
    bad[3] = 52
    assert gpu_trace(ctx, b["xy"], None, 52, bad, 10, 1)[0] == _capi.TL_ERR_BADARG and "permutation" in err()
    assert gpu_trace(ctx, b["xy"], None, 52, None, 0, 1, cap=4)[0] == _capi.TL_ERR_UNSUPPORTED and "never ends" in err()
    assert gpu_trace(ctx, b["xy"], None, 52, None, 2 ** 32 - 1, 1, cap=4)[0] == _capi.TL_ERR_UNSUPPORTED
    assert gpu_trace(ctx, b["xy"], None, 1, None, 3, 1)[0] == _capi.TL_ERR_REF_PANICS
    assert gpu_trace(ctx, b["xy"], None, 0, None, 3, 1)[0] == _capi.TL_ERR_REF_PANICS
    # just above the LDS-resident limit: refused before anything of size n is read (the arrays passed hold 52 cities)
    top = ctx.lib.tl_tabu_search_lds_max_n(ctx.handle)
    assert 0 < top <= 65535 and plan(ctx, top)[0] > 0 and plan(ctx, top + 1)[:3] == (0, 0, 0)
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    rc = ctx.lib.tl_tabu_search(ctx.handle, _vp(b["xy"]), top + 1, None, None, 5, 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "LDS-resident limit" in err()
    assert ctx.lib.tl_tabu_search(ctx.handle, None, 52, None, None, 5, 1, _vp(out), C.byref(cost), None) == _capi.TL_ERR_BADARG
    assert err() == "tl_tabu_search: NULL argument"
    log, ln = np.zeros((4, 4), dtype=np.uint32), C.c_uint32()
    assert ctx.lib.tl_tabu_search_trace(ctx.handle, _vp(b["xy"]), 52, None, None, 5, 1, _vp(out), C.byref(cost), None, None, 4, C.byref(ln)) == _capi.TL_ERR_BADARG
    with TA.Context(0, 1 << 31) as odd:  # a bit no flag has
        assert gpu_trace(odd, b["xy"], None, 52, None, 5, 1)[0] == _capi.TL_ERR_UNSUPPORTED


def test_busy(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    xy, small = K.synth(1000, 9), K.small(5)
    tour, cost, _log, _cnt = TO.solve_cached(("small5", 5, 0), small, None, 5, None, epochs=200, seed=5, chain=0)
    with TA.Context(0) as c:
        res = {}

        def long_call():
            out, gcost = np.zeros(1000, dtype=np.uint32), C.c_float()
            res["rc"] = c.lib.tl_tabu_search(c.handle, _vp(xy), 1000, None, None, 10000, 1, _vp(out), C.byref(gcost), None)
            res["out"] = out

        t = threading.Thread(target=long_call)
        t.start()
        busy = 0
        while t.is_alive():
            rc, out, gcost, *_ = gpu_trace(c, small, None, 5, None, 200, 5)
            assert rc in (0, _capi.TL_ERR_BUSY)
            if rc == 0:
                assert out.tolist() == tour.tolist() and bits(gcost) == bits(cost)
            busy += rc == _capi.TL_ERR_BUSY
        t.join()
        assert res["rc"] in (0, _capi.TL_ERR_BUSY)
        busy += res["rc"] == _capi.TL_ERR_BUSY
        assert busy >= 1, "the two threads never met inside the context"
        if res["rc"] == 0:
            assert sorted(res["out"].tolist()) == list(range(1000))
        rc, out, gcost, *_ = gpu_trace(c, small, None, 5, None, 200, 5)  # the context works afterwards
        assert rc == 0 and out.tolist() == tour.tolist()


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_and_chains(ctx):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    opts = TA.HeuristicOptions(epochs=600)
    tour, cost, log, cnt = TO.solve_cached(("berlin52", 1, 0), prob.xy, None, 52, None, epochs=600, seed=1, chain=0)
    msgs = []
    sol = TA.tabu_search.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    assert [k for k, _ in msgs] == ["PathUpdate"] * (cnt["bests"] + 1) + ["Done"]
    assert msgs[0][1] == (prob.ids.tolist(), 0.0)
    best, want = TO.tour_length(TO.dist_fn(prob.xy, None, 52), np.arange(52)), []
    for _a, _f, _t, c in log:
        if c < best:
            best = c
            want.append(bits(c))
    assert [bits(m[1][1]) for m in msgs[1:-1]] == want
    assert msgs[-2][1][0] == sol.route() == prob.ids[tour].tolist() and bits(sol.total) == bits(cost)
    plain = TA.tabu_search.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == cnt["bests"] and plain.stats["candidates"] == cnt["candidates"]
    # chains > 1: the best chain, and its own replay
    short = TA.HeuristicOptions(epochs=150)
    msgs2 = []
    bestsol = TA.tabu_search.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, chains=5)
    singles = [TO.solve_cached(("berlin52_150", 1, c), prob.xy, None, 52, None, epochs=150, seed=1, chain=c) for c in range(5)]
    c = int(np.argmin([(bits(s[1]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["chain"] == c and bestsol.route() == prob.ids[singles[c][0]].tolist() and bits(bestsol.total) == bits(singles[c][1])
    assert len(msgs2) == singles[c][3]["bests"] + 2 and msgs2[-2][1][0] == bestsol.route()
    # the pipeline: `solve tabu_search` is nn -> tabu_search, the stage draws from the pipeline's one seed
    steps = TA.pipeline.steps_for_solve("tabu_search")
    assert steps == ["nn", "tabu_search"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"tabu_search": short}, ctx=ctx, lk_seed=3)
    assert [o.name for o in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = TO.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), epochs=150, seed=3)
    assert outs[-1].solution.route() == prob.ids[seeded[0]].tolist() and bits(outs[-1].solution.total) == bits(seeded[1])
    outs2 = TA.pipeline.run_pipeline_stages(prob, steps, {"tabu_search": short}, ctx=ctx, lk_seed=3, tabu_chains=3)
    assert outs2[-1].solution.total <= outs[-1].solution.total


def test_cli_equals_python_mirror(ctx):
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    opts = TA.HeuristicOptions(epochs=150)
    args0 = ["--epochs", "150", "--seed", "1"]
    for args, steps in ((["solve", "tabu_search"], ["nn", "tabu_search"]), (["pipeline", "--steps=nn,2opt,tabu_search"], ["nn", "2opt", "tabu_search"]),
                        (["solve", "tabu_search", "--no-seed"], ["tabu_search"])):
        r = subprocess.run([cli] + args + ["-i", tsp] + args0, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs = TA.pipeline.run_pipeline_stages(prob, steps, {"tabu_search": opts, "2opt": opts, "nn": opts}, ctx=ctx, lk_seed=1)
        assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(outs[-1].solution).splitlines(), args
    r = subprocess.run([cli, "solve", "tabu_search", "-i", tsp, "--tabu-chains", "4"] + args0, capture_output=True, text=True, timeout=120)
    nn = TA.pipeline.run_pipeline_stages(prob, ["nn"], {"nn": opts}, ctx=ctx)[0].solution
    best = TA.tabu_search.solve(prob, opts, None, nn.route(), ctx=ctx, seed=1, chains=4)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(best).splitlines()
    r = subprocess.run([cli, "solve", "tabu", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "tabu_search" in r.stderr


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """The cases with hits on the race-stress build (-DTL_JITTER: waves leave every barrier far apart)."""
    from teeline_amd import _capi
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    jctx = jitter_context({"tl_tabu_search_trace_chain": [vp, vp, u32, vp, vp, u32, u64, u32, vp, C.POINTER(C.c_float), C.POINTER(_capi.TlStats), vp, u32, C.POINTER(u32)],
                           "tl_tabu_search_population": [vp, vp, u32, vp, vp, u32, u32, u32, u32, u64, vp, vp, vp, C.POINTER(u32), C.POINTER(_capi.TlStats)]})
    try:
        for name in TC.HIT_CASES:
            xy, packed, n, init, epochs, seed, chain = GOLDEN[name]
            check_chain(jctx, name, xy, packed, n, init, epochs, seed, chain)
        key, xy, packed, n, start, epochs, seed = TC.wrap_chain(66)  # the wrapped ring with a refusal in the look-up's second round
        check_population_chains(jctx, key, xy, None, n, start, 1, jctx.cus + 1, epochs, seed, (0, jctx.cus))
        log = TO.solve_cached((key, seed, 0), xy, None, n, start, epochs=epochs, seed=seed, chain=0)[2]
        TC.check_wrapped_ring(n, 64, log, TO.record_of((key, seed, 0)))
    finally:
        jctx.close()
