"""The flower pollination solver on the GPU (tl_flower_pollination*, csrc/flower_pollination.hip) against the statement of its
specification (tests/_fpa_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every
record of the improvement log with its route, every word of the per-epoch record (every flower's cost bits, move kind with j and
k, sequence and prefix lengths, accepted and built-again bits — which pin the draws, the Lévy step, the orbit form of the swap
sequence, the sequential sums, the commit's order and its second builds) and the stats against the oracle's counters — in both
input forms and for the runs of a batch; and the device's move alone (tl_fpa_selftest_pollinate)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _fpa_cases as FC
import _fpa_oracle as FO
import _sa_cases as K
import _swarm_harness as H
from _raw_context import _vp

pytestmark = pytest.mark.gpu

NT = FC.THREADS
bits = FO.bits
FAST = FO.swap_sequence_inverse  # (tests/test_fpa_oracle.py: equal to the literal search)


FPA = H.FPA
_opts = FPA.opts
gpu_trace, plan, check_run = (functools.partial(f, FPA) for f in (H.gpu_trace, H.plan, H.check_run))


# ---------------------------------------------------------------- the device's move alone
def device_pollinate(ctx, fl, src, tgt, prefix, n):
    count = len(fl)
    a = [np.ascontiguousarray(x, dtype=np.uint32) for x in (fl, src, tgt)]
    p = np.ascontiguousarray(prefix, dtype=np.uint32)
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    ln = np.full(count, 0xFFFFFFFF, dtype=np.uint32)
    rc = ctx.lib.tl_fpa_selftest_pollinate(ctx.handle, _vp(a[0]), _vp(a[1]), _vp(a[2]), _vp(p), n, count, _vp(out), _vp(ln))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    return out, ln


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, NT - 1, NT, NT + 1, 600, 1002])
def test_selftest_pollinate(ctx, n):
    """source = target (an empty sequence), source = flower (a global move), three different tours (a local one), one long cycle
    (an orbit of n - 1 steps) and its reverse (every orbit one step); prefixes 0, 1, half, whole and beyond: the literal loops"""
    rng = np.random.default_rng(n)
    perm = lambda: rng.permutation(n).astype(np.uint32)  # noqa: E731
    ident = np.arange(n, dtype=np.uint32)
    rows = []
    for _ in range(3):
        a, b, c = perm(), perm(), perm()
        rows += [(a, b, b), (a, a, b), (a, b, c)]
    rows += [(perm(), ident, np.roll(ident, 1)), (perm(), ident, np.roll(ident, -1)), (ident, np.roll(ident, 1), ident)]
    tuples, prefix = [], []
    for f, s, t in rows:
        ln = len(FO.swap_sequence_literal(s, t))
        for p in sorted({0, 1, ln // 2, ln, ln + 7}):
            tuples.append((f, s, t))
            prefix.append(p)
    out, lens = device_pollinate(ctx, [t[0] for t in tuples], [t[1] for t in tuples], [t[2] for t in tuples], prefix, n)
    for (f, s, t), p, o, ln in zip(tuples, prefix, out, lens):
        wl, wt = FO.pollinate(f, s, t, p)
        assert ln == wl and o.tolist() == wt, (n, p, wl)
    if n >= 600:
        assert max(lens) > NT and max(min(p, ln) for p, ln in zip(prefix, lens)) > NT


def test_selftest_errors(ctx):
    from teeline_amd import _capi
    t = np.arange(4, dtype=np.uint32).reshape(1, 4)
    bad = np.array([[0, 1, 2, 2]], dtype=np.uint32)
    out, ln, p = np.zeros((1, 4), dtype=np.uint32), np.zeros(1, dtype=np.uint32), np.ones(1, dtype=np.uint32)
    f = ctx.lib.tl_fpa_selftest_pollinate
    for a in ((bad, t, t), (t, bad, t), (t, t, bad)):
        assert f(ctx.handle, _vp(a[0]), _vp(a[1]), _vp(a[2]), _vp(p), 4, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert f(ctx.handle, _vp(t), None, _vp(t), _vp(p), 4, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert f(ctx.handle, _vp(t), _vp(t), _vp(t), _vp(p), 0, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert f(ctx.handle, _vp(t), _vp(t), _vp(t), _vp(p), 4, 0, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG


def test_host_queries_equal_the_oracle(ctx):
    lib = ctx.lib
    key = FO.chain_key(9, 2)
    for N in (25, 26, 64):
        for i in range(N):
            j, k = C.c_uint32(), C.c_uint32()
            assert lib.tl_fpa_partners(9, 2, 3, i, N, C.byref(j), C.byref(k)) == 0
            assert (j.value, k.value) == FO.partners(key, FO.event(3, N, i), i, N)
    assert lib.tl_fpa_draw(9, 2, 77, 15) == FO.draw_key(key, 77, 15)
    for p in (0.0, 0.001, 0.01, 0.5, 1.0):
        assert lib.tl_fpa_switch_prob(p) == FO.switch_prob(p)
    for x, ln in ((0.0, 7), (1.0, 8), (1.0000001, 8), (9.0, 7), (float("nan"), 7), (float("inf"), 7), (0.3, 0)):
        assert lib.tl_fpa_global_swaps(x, ln) == FO.global_swaps(x, ln) and lib.tl_fpa_local_swaps(x, ln) == FO.local_swaps(x, ln)


# ---------------------------------------------------------------- whole runs
GOLDEN = FC.golden_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    """berlin52 with and without an initial tour, gr17 in matrix form, N = 31 and 65"""
    xy, packed, n, init, o = GOLDEN[name]
    res = check_run(ctx, name, xy, packed, n, init, o)
    FC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(FC.SEEDED))
def test_seeded_conditions(ctx, name):
    """a global flower built again after gbest improved, with another outcome than its staged one; a local flower built again
    because j, because k was accepted earlier; one whose j and k, both above it, are accepted later and which is not built again; a
    chain; gbest improved by flower 0 and by flower N - 1; two improvements in an epoch; the gbest flower's empty global sequence;
    an empty local sequence; a prefix of 1, of the whole sequence with |levy| >= 2, of more than 256: each asserted from the
    oracle's record, the run equal word for word"""
    xy, packed, n, init, o, want = FC.seeded_case(name)
    res = check_run(ctx, name, xy, packed, n, init, o, seq=FAST if n >= 600 else FO.swap_sequence_literal)
    assert set(want) <= FC.conditions(res), (name, set(want) - FC.conditions(res))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_smallest_sizes(ctx, n):
    """n = 1: nothing moves; n = 2 and 3: empty local sequences (flowers j and k equal) beside real ones"""
    xy = FC.instance(max(n, 3))[:n] if n < 3 else FC.instance(n)
    res = check_run(ctx, "size", xy, None, n, None, dict(epochs=40, n_nearest=3, mutation_probability=0.5, seed=11 + n, run=0))
    check_run(ctx, "size_init", xy, None, n, FC.start_tour(n, n), dict(epochs=6, n_nearest=3, mutation_probability=0.001, seed=11 + n, run=1))
    moves = [m for ep in res["epochs"] for m in ep["moves"]]
    if n == 1:
        assert len(res["improvements"]) == 1 and not any(m["accepted"] or m["len"] for m in moves)
    if n in (2, 3):
        assert any(not m["glob"] and m["len"] == 0 for m in moves) and any(not m["glob"] and m["len"] > 0 for m in moves)


def test_n_0(ctx):
    o = dict(epochs=2, n_nearest=3, mutation_probability=0.5, seed=1, run=0)
    res = FO.solve(None, None, 0, None, **o)
    rc, out, gcost, glog, ln, st, _routes, elog = gpu_trace(ctx, K.small(3), None, 0, None, o)
    assert rc == 0 and len(out) == 0 and bits(gcost) == 0 and ln == 1 and glog.tolist() == FO.log_words(res).tolist() and st["moves"] == 0
    assert elog.tolist() == FO.epoch_words(res).tolist()


@pytest.mark.parametrize("n,epochs", [(52, 60), (65, 40), (130, 12), (NT + 1, 6), (300, 4)])
def test_sizes(ctx, n, epochs):
    """just past one wave, two waves and a bit, just past one workgroup pass, well past it"""
    res = check_run(ctx, "sizes", FC.instance(n), None, n, None, dict(epochs=epochs, n_nearest=3, mutation_probability=0.001, seed=n, run=0))
    assert any(m["again"] for ep in res["epochs"] for m in ep["moves"])


def test_matrix_forms(ctx):
    xy = FC.instance(257)
    from teeline_amd import _capi
    pk = np.empty(257 * 256 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), 257, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    check_run(ctx, "m257", None, pk, 257, None, dict(epochs=3, n_nearest=3, mutation_probability=0.25, seed=257, run=0))


@pytest.mark.parametrize("n_nearest", [25, 26, 64, 65])
def test_flower_counts(ctx, n_nearest):
    res = check_run(ctx, "flowers", FC.instance(40), None, 40, FC.start_tour(40, 4), dict(epochs=6, n_nearest=n_nearest, mutation_probability=0.1, seed=40, run=0))
    assert res["flowers"] == n_nearest


@pytest.mark.parametrize("p", [0.001, 0.01, 1.0])
def test_mutation_probabilities(ctx, p):
    """0.001 gives 0.8; 0.01 is taken as it is (nearly every move local); 1.0: every move global"""
    res = check_run(ctx, "sp", FC.instance(30), None, 30, None, dict(epochs=8, n_nearest=3, mutation_probability=p, seed=30, run=0))
    share = np.mean([m["glob"] for ep in res["epochs"] for m in ep["moves"]])
    assert share == 1.0 if p == 1.0 else (0.7 < share < 0.9) if p == 0.001 else share < 0.1


@pytest.mark.parametrize("epochs", [0, 1, 2])
def test_epochs(ctx, epochs):
    xy = K.small(8)
    check_run(ctx, "epochs", xy, None, 8, None, dict(epochs=epochs, n_nearest=3, mutation_probability=0.001, seed=5, run=0))
    res = check_run(ctx, "epochs_init", xy, None, 8, FC.start_tour(8, 2), dict(epochs=epochs, n_nearest=3, mutation_probability=0.001, seed=5, run=0))
    if epochs == 0:  # the start gbest: the first minimum over the initial tour and 24 shuffles
        assert len(res["improvements"]) == 1


def test_n_1002(ctx):
    res = check_run(ctx, "n1002", FC.instance(1002), None, 1002, None, dict(epochs=3, n_nearest=3, mutation_probability=0.001, seed=1002, run=0), seq=FAST)
    assert max(m["prefix"] for ep in res["epochs"] for m in ep["moves"]) > 2 * NT


def test_largest_n(ctx):
    """tl_flower_pollination_max_n with two epochs; one city more is refused before anything of size n is read (the arrays passed
    hold 52 cities)"""
    from teeline_amd import _capi
    top = ctx.lib.tl_flower_pollination_max_n(ctx.handle)
    lds = ctx.device_info()["lds_bytes"]
    up = lambda v: (v + 15) & ~15  # noqa: E731
    need = lambda n: 768 + up(4 * n) + 3 * up(2 * n)  # noqa: E731
    assert 4096 < top <= 65535 and need(top) <= lds < need(top + 1) and plan(ctx, top)[3] >= 1 and plan(ctx, top + 1) == (0, 0, 0, 0)
    check_run(ctx, "top", K.synth(top, 5), None, top, None, dict(epochs=2, n_nearest=3, mutation_probability=0.5, seed=7, run=0), seq=FAST)
    b = K.tsplib("berlin52")
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = _opts(dict(epochs=1, n_nearest=3))
    rc = ctx.lib.tl_flower_pollination(ctx.handle, _vp(b["xy"]), top + 1, None, None, C.byref(po), 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "exceeds the limit" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_plain_entry_defaults_and_truncated_trace(ctx):
    H.plain_entry_defaults_and_truncated_trace(FPA, ctx, GOLDEN)


# ---------------------------------------------------------------- batches
POP = dict(epochs=4, n_nearest=3, mutation_probability=0.25, seed=31)


def test_batches(ctx):
    H.batches(FPA, ctx, FC, POP)


def test_more_runs_than_one_launch_sequence(ctx):
    """the run is the grid's y: a sequence holds at most 65535 runs; at n = 3 a 65536th run goes in a second one"""
    H.more_runs_than_one_launch_sequence(FPA, ctx, dict(epochs=2, n_nearest=3, mutation_probability=0.5, seed=3), 2 * (4 * 25 * 60 + 120 + 12 * 25) + 9 * 256)


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller():
    """stale flowers, staged tours and logs must not leak: the larger instance leaves its tables where the smaller one's begin"""
    H.context_reuse(FPA, [("sizes", FC.instance(130), None, 130, None, dict(epochs=12, n_nearest=3, mutation_probability=0.001, seed=130, run=0)),
                          ("epochs", K.small(8), None, 8, None, dict(epochs=2, n_nearest=3, mutation_probability=0.001, seed=5, run=0)),
                          ("gr17_matrix",) + GOLDEN["gr17_matrix"]])


def test_errors(ctx):
    from teeline_amd import _capi
    H.common_errors(FPA, ctx, "flowers")
    b = K.tsplib("berlin52")
    for p in (float("nan"), float("inf"), -0.5, 1.5):
        rc = gpu_trace(ctx, b["xy"], None, 52, None, dict(epochs=2, n_nearest=3, seed=1, mutation_probability=p))[0]
        assert rc == _capi.TL_ERR_BADARG and "mutation_probability" in ctx.lib.tl_last_error(ctx.handle).decode()
    j = C.c_uint32()
    assert ctx.lib.tl_fpa_partners(1, 0, 0, 25, 25, C.byref(j), C.byref(j)) == _capi.TL_ERR_BADARG


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """a handful of the cases above on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the pairs' block
    reused for the edge lengths, the compaction's wave counts, the commit's second builds, its "accepted" bits and its cost rows"""
    jctx = H.jitter(FPA)
    try:
        for name in ("small8_every_condition", "synth130_26_flowers", "berlin52_default"):
            xy, packed, n, init, o, _want = FC.seeded_case(name)
            check_run(jctx, name, xy, packed, n, init, o)
    finally:
        jctx.close()
