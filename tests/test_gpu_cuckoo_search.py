"""The cuckoo search solver on the GPU (tl_cuckoo_search*, csrc/cuckoo_search.hip) against the statement of its specification
(tests/_cs_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every record of the
improvement log with its route, every word of the per-epoch record (every nest's cost bits, every cuckoo's k, target, accepted and
flown-again bits, every abandonment — which pin the Lévy step, the gather, the sequential sums, the commit's order and its second
flights) and the stats against the oracle's counters — in both input forms and for the runs of a batch; and the device's Lévy step
and gather alone (tl_cs_selftest_levy, tl_cs_selftest_reversals)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _cs_cases as CC
import _cs_oracle as CO
import _sa_cases as K
import _swarm_harness as H
from _raw_context import _vp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = CC.THREADS
bits = CO.bits


CS = H.CS
_opts = CS.opts
gpu_trace, plan, check_run = (functools.partial(f, CS) for f in (H.gpu_trace, H.plan, H.check_run))
okey = H.okey


# ---------------------------------------------------------------- the device's Lévy step and gather
def test_selftest_levy_equals_the_host(ctx):
    """a few thousand word tuples plus the edge words: the device's step bit for bit — which decides whether f64 sqrt, / and the
    fixed sequences give the same bits on the device as on the host — its resamples and its k"""
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "goldens_cs.json")))
    rng = np.random.default_rng(5)
    edge = np.asarray([[int(x) for x in w] for w, _v, _t, _k in gold["levy"]], dtype=np.uint64)
    words = np.ascontiguousarray(np.concatenate([edge, rng.integers(0, 2 ** 64, size=(4000, CO.WORDS), dtype=np.uint64)]))
    count = len(words)
    want, tries = CO.levy_spec(words)
    for n in (52, 1002):
        vb, k, t = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
        rc = ctx.lib.tl_cs_selftest_levy(ctx.handle, _vp(words), count, n, _vp(vb), _vp(k), _vp(t))
        assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
        bad = np.nonzero(vb != want.view(np.uint64))[0]
        assert len(bad) == 0, (len(bad), [(int(i), hex(int(vb[i])), hex(int(want.view(np.uint64)[i]))) for i in bad[:4]])
        assert t.tolist() == tries.tolist() and k.tolist() == CO.flight_length_np(np.abs(want), n).tolist()
        lib = ctx.lib
        for i in range(0, count, 97):
            r = C.c_uint32()
            hv = lib.tl_levy_from_words(words[i].ctypes.data_as(C.c_void_p), C.byref(r))
            assert CO.f64_bits(hv) == int(vb[i]) and r.value == t[i] and lib.tl_cs_flight_length(abs(hv), n) == k[i]
    assert max(tries) == 4 and (tries > 0).sum() >= 4  # the resample path ran on the device


def device_reversals(ctx, tours, pair_lists, n):
    count = len(tours)
    kcap = max(1, max(len(p) for p in pair_lists))
    pairs = np.zeros((count, kcap, 2), dtype=np.uint32)
    lens = np.asarray([len(p) for p in pair_lists], dtype=np.uint32)
    for c, pl in enumerate(pair_lists):
        if pl:
            pairs[c, :len(pl)] = np.asarray(pl, dtype=np.uint32)
    tours = np.ascontiguousarray(tours, dtype=np.uint32)
    out = np.full((count, n), 0xFFFFFFFF, dtype=np.uint32)
    rc = ctx.lib.tl_cs_selftest_reversals(ctx.handle, _vp(tours), _vp(pairs), _vp(lens), n, kcap, count, _vp(out))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    return out


@pytest.mark.parametrize("n", [2, 3, 5, 63, 64, 65, NT - 1, NT, NT + 1, 600, 1002])
def test_selftest_reversals(ctx, n):
    """no reversal, one, the whole tour, j = i + 1, n / 2 random ones (more pairs than a workgroup pass at n = 600, 1002): the
    literal loop's result"""
    rng = np.random.default_rng(n)
    K2 = n // 2
    lists = [[], [(0, n - 1)], [(n - 2, n - 1)], [(0, n - 1)] * K2, [(0, 1)] * K2]
    for k in (1, max(K2 // 2, 1), K2, K2, K2):
        pl = []
        for _ in range(k):
            i = int(rng.integers(0, n - 1))
            pl.append((i, int(rng.integers(i + 1, n))))
        lists.append(pl)
    tours = np.stack([rng.permutation(n) for _ in lists])
    got = device_reversals(ctx, tours, lists, n)
    for row, pl, g in zip(tours, lists, got):
        assert g.tolist() == CO.reverse_literal(row.tolist(), pl), (n, len(pl))
    if n >= 600:
        assert len(lists[-1]) > NT


def test_selftest_errors(ctx):
    from teeline_amd import _capi
    t = np.arange(4, dtype=np.uint32).reshape(1, 4)
    out = np.zeros((1, 4), dtype=np.uint32)
    ln = np.array([1], dtype=np.uint32)
    for bad in ([[1, 1]], [[2, 1]], [[0, 4]]):
        p = np.asarray(bad, dtype=np.uint32).reshape(1, 1, 2)
        assert ctx.lib.tl_cs_selftest_reversals(ctx.handle, _vp(t), _vp(p), _vp(ln), 4, 1, 1, _vp(out)) == _capi.TL_ERR_BADARG
    p = np.asarray([[0, 1]], dtype=np.uint32).reshape(1, 1, 2)
    assert ctx.lib.tl_cs_selftest_reversals(ctx.handle, _vp(t), _vp(p), _vp(ln), 4, 3, 1, _vp(out)) == _capi.TL_ERR_BADARG  # kcap > n / 2
    assert ctx.lib.tl_cs_selftest_reversals(ctx.handle, _vp(t), None, _vp(ln), 4, 1, 1, _vp(out)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_cs_selftest_levy(ctx.handle, None, 1, 52, _vp(out), _vp(out), _vp(out)) == _capi.TL_ERR_BADARG


# ---------------------------------------------------------------- whole runs
GOLDEN = CC.golden_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    """berlin52 with and without an initial tour, gr17 in matrix form, N = 31 and 65"""
    xy, packed, n, init, o = GOLDEN[name]
    res = check_run(ctx, name, xy, packed, n, init, o)
    CC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(CC.SEEDED))
def test_seeded_conditions(ctx, name):
    """a cuckoo flying again from an overwritten nest and accepted, two in an epoch, a chain, c = t, accepted flights that leave
    and that improve best, best improved by an abandonment, best's nest abandoned while best stands, a nest replaced and then
    abandoned, k = 1, n / 2 and above 256, a whole-tour and an adjacent reversal: each asserted from the oracle's record, the run
    equal word for word"""
    xy, packed, n, init, o, want = CC.seeded_case(name)
    res = check_run(ctx, name, xy, packed, n, init, o)
    assert set(want) <= CC.conditions(res, n), (name, set(want) - CC.conditions(res, n))
    if n == 600:
        assert max(max(ep["ks"]) for ep in res["epochs"]) > 256


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_smallest_sizes(ctx, n):
    """n / 2 is 1 or 2; at n = 2 every cost ties and best stays the start's nest 0"""
    xy = CC.instance(n)
    res = check_run(ctx, "size", xy, None, n, None, dict(epochs=300, n_nearest=3, mutation_probability=0.5, seed=11 + n, run=0))
    check_run(ctx, "size_init", xy, None, n, CC.start_tour(n, n), dict(epochs=6, n_nearest=3, mutation_probability=0.001, seed=11 + n, run=1))
    if n == 2:
        assert len(res["improvements"]) == 1 and res["improvements"][0][1] == 0


@pytest.mark.parametrize("n,epochs", [(52, 300), (65, 300), (130, 20), (NT + 1, 8)])
def test_sizes(ctx, n, epochs):
    """just past one wave, two waves and a bit, just past one workgroup pass; many epochs at the small sizes: late epochs accept little"""
    res = check_run(ctx, "sizes", CC.instance(n), None, n, None, dict(epochs=epochs, n_nearest=3, mutation_probability=0.001, seed=n, run=0))
    assert any(any(ep["again"]) for ep in res["epochs"])


def test_matrix_forms(ctx):
    xy = CC.instance(257)
    from teeline_amd import _capi
    pk = np.empty(257 * 256 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), 257, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    check_run(ctx, "m257", None, pk, 257, None, dict(epochs=3, n_nearest=3, mutation_probability=0.25, seed=257, run=0))


@pytest.mark.parametrize("n_nearest", [25, 26, 64, 65])
def test_nest_counts(ctx, n_nearest):
    res = check_run(ctx, "nests", CC.instance(40), None, 40, CC.start_tour(40, 4), dict(epochs=6, n_nearest=n_nearest, mutation_probability=0.1, seed=40, run=0))
    assert res["nests"] == n_nearest


@pytest.mark.parametrize("p", [0.0, 0.001, 0.5, 1.0])
def test_mutation_probabilities(ctx, p):
    res = check_run(ctx, "pa", CC.instance(30), None, 30, None, dict(epochs=8, n_nearest=3, mutation_probability=p, seed=30, run=0))
    share = np.mean([a for ep in res["epochs"] for a in ep["abandoned"]])
    assert (share > 0.9) if p == 1.0 else (0.3 < share < 0.7) if p == 0.5 else share < 0.1


@pytest.mark.parametrize("epochs", [0, 1, 2])
def test_epochs(ctx, epochs):
    xy = K.small(8)
    check_run(ctx, "epochs", xy, None, 8, None, dict(epochs=epochs, n_nearest=3, mutation_probability=0.001, seed=5, run=0))
    res = check_run(ctx, "epochs_init", xy, None, 8, CC.start_tour(8, 2), dict(epochs=epochs, n_nearest=3, mutation_probability=0.001, seed=5, run=0))
    if epochs == 0:  # the start best: the first minimum over the initial tour and 24 shuffles
        assert len(res["improvements"]) == 1


def test_n_1002(ctx):
    res = check_run(ctx, "n1002", CC.instance(1002), None, 1002, None, dict(epochs=3, n_nearest=3, mutation_probability=0.001, seed=1002, run=0))
    assert max(max(ep["ks"]) for ep in res["epochs"]) == 501


def test_largest_n(ctx):
    """tl_cuckoo_search_max_n; one city more is refused before anything of size n is read (the arrays passed hold 52 cities)"""
    from teeline_amd import _capi
    top = ctx.lib.tl_cuckoo_search_max_n(ctx.handle)
    lds = ctx.device_info()["lds_bytes"]
    up = lambda v: (v + 15) & ~15  # noqa: E731
    need = lambda n: 576 + up(4 * (n // 2)) + up(4 * n) + 2 * up(2 * n)  # noqa: E731
    assert 4096 < top <= 65535 and need(top) <= lds < need(top + 1) and plan(ctx, top)[3] >= 1 and plan(ctx, top + 1) == (0, 0, 0, 0)
    b = K.tsplib("berlin52")
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = _opts(dict(epochs=1, n_nearest=3))
    rc = ctx.lib.tl_cuckoo_search(ctx.handle, _vp(b["xy"]), top + 1, None, None, C.byref(po), 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "exceeds the limit" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_small_n(ctx):
    from teeline_amd import _capi
    for n in (0, 1):
        xy = K.small(3)
        o = dict(epochs=0, n_nearest=3, seed=1, run=0)
        res = CO.solve(xy[:n], None, n, None, **o)
        rc, out, gcost, glog, ln, st, routes, _elog = gpu_trace(ctx, xy, None, n, None, o)
        assert rc == 0 and out.tolist() == list(range(n)) and bits(gcost) == 0 and ln == 1 and glog.tolist() == CO.log_words(res).tolist() and st["moves"] == 0
        assert gpu_trace(ctx, xy, None, n, None, dict(o, epochs=1))[0] == _capi.TL_ERR_REF_PANICS and "panics" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_plain_entry_defaults_and_truncated_trace(ctx):
    H.plain_entry_defaults_and_truncated_trace(CS, ctx, GOLDEN)


# ---------------------------------------------------------------- batches
POP = dict(epochs=4, n_nearest=3, mutation_probability=0.25, seed=31)


def test_batches(ctx):
    H.batches(CS, ctx, CC, POP)


def test_more_runs_than_one_launch_sequence(ctx):
    """the run is the grid's y: a sequence holds at most 65535 runs; at n = 3 a 65536th run goes in a second one"""
    H.more_runs_than_one_launch_sequence(CS, ctx, dict(epochs=1, n_nearest=3, mutation_probability=0.5, seed=3), 2 * (6 * 25 * 60 + 120 + 16 * 25) + 11 * 256)


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller():
    """stale nests, staged tours and logs must not leak: the larger instance leaves its tables where the smaller one's begin"""
    H.context_reuse(CS, [("sizes", CC.instance(130), None, 130, None, dict(epochs=20, n_nearest=3, mutation_probability=0.001, seed=130, run=0)),
                         ("epochs", K.small(8), None, 8, None, dict(epochs=2, n_nearest=3, mutation_probability=0.001, seed=5, run=0)),
                         ("gr17_matrix",) + GOLDEN["gr17_matrix"]])


def test_errors(ctx):
    from teeline_amd import _capi
    H.common_errors(CS, ctx, "nests")
    b = K.tsplib("berlin52")
    for p in (float("nan"), float("inf"), -0.5, 1.5):
        rc = gpu_trace(ctx, b["xy"], None, 52, None, dict(epochs=2, n_nearest=3, seed=1, mutation_probability=p))[0]
        assert rc == _capi.TL_ERR_BADARG and "mutation_probability" in ctx.lib.tl_last_error(ctx.handle).decode()


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    CS = TA.cuckoo_search
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    xy, _pk, n, init, o = GOLDEN["berlin52"]
    opts = CS.CSOptions(epochs=o["epochs"])
    res = CO.solve_cached(okey("berlin52", n, init, o), prob.xy, None, 52, None, **o)
    msgs = []
    sol = CS.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    want = CO.messages(res, prob.ids)
    assert [k for k, _ in msgs] == [k for k, _ in want] and sum(k == "EpochUpdate" for k, _ in msgs) == o["epochs"]
    for (k, p), (_k, w) in zip(msgs, want):
        if k == "PathUpdate":
            assert p[0] == w[0] and bits(p[1]) == bits(w[1])
        else:
            assert p == w
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    plain = CS.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == res["counters"]["improved"]
    short = CS.CSOptions(epochs=5, n_nearest=31, mutation_probability=0.25)
    so = dict(epochs=5, n_nearest=31, mutation_probability=0.25, seed=1)
    msgs2 = []
    bestsol = CS.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [CO.solve_cached(okey("mirror", 52, None, dict(so, run=r)), prob.xy, None, 52, None, **dict(so, run=r)) for r in range(4)]
    r = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r]["tour"]].tolist() and bits(bestsol.total) == bits(singles[r]["cost"])
    assert [k for k, _ in msgs2] == [k for k, _ in CO.messages(singles[r])]
    steps = TA.pipeline.steps_for_solve("cuckoo_search")
    assert steps == ["shuffle", "cuckoo_search"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"cuckoo_search": short}, ctx=ctx, lk_seed=3)
    assert [x.name for x in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = CO.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), **dict(so, seed=3))
    assert outs[-1].solution.route() == prob.ids[seeded["tour"]].tolist() and bits(outs[-1].solution.total) == bits(seeded["cost"])
    with pytest.raises(ValueError, match="the seeded cuckoo search of this build is `cuckoo_search`"):
        TA.pipeline.steps_for_solve("cs")
    with pytest.raises(ValueError, match="mutation_probability"):
        CS.solve(prob, CS.CSOptions(mutation_probability=2.0), None, None, ctx=ctx)


def test_cli_equals_the_oracle(ctx):
    import re
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "6", "--seed", "3", "--n-nearest", "31", "--mutation-probability", "0.25"]
    o = dict(epochs=6, n_nearest=31, mutation_probability=0.25, seed=3)
    fmt = lambda res: TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()  # noqa: E731
    r = subprocess.run([cli, "solve", "cuckoo_search", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    shuffled = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=3)[0].solution
    res = CO.solve(prob.xy, None, 52, prob.positions_of(shuffled.route()), **o)
    assert r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "cuckoo_search", "--no-seed", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    res = CO.solve(prob.xy, None, 52, None, **o)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "cs", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the seeded cuckoo search of this build is `cuckoo_search`" in r.stderr
    # the C++ mirror's messages: PathUpdate(start) and one per improvement, EpochUpdate per epoch, Done
    r = subprocess.run([cli, "solve", "cuckoo_search", "--no-seed", "--progress-digest", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=[0-9a-f]{16} epoch_updates=(\d+)", r.stderr)
    assert r.returncode == 0 and m, r.stderr
    assert [int(v) for v in m.groups()] == [len(res["improvements"]), 0, 1, o["epochs"]]
    r = subprocess.run([cli, "solve", "cuckoo_search", "--no-seed", "--runs", "3", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    three = [CO.solve(prob.xy, None, 52, None, **dict(o, run=k)) for k in range(3)]
    best = three[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(three)]))]
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(best)
    r = subprocess.run([cli, "pipeline", "--steps=shuffle,cuckoo_search,2opt", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = TA.pipeline.run_pipeline_stages(prob, ["shuffle", "cuckoo_search", "2opt"],
                                           {"cuckoo_search": TA.cuckoo_search.CSOptions(epochs=6, n_nearest=31, mutation_probability=0.25)}, ctx=ctx, lk_seed=3)[-1].solution
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(want).splitlines()


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """a handful of the cases above on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the LDS blocks
    reused within a flight, the commit's second flights, its "overwritten" bits and its cost rows"""
    jctx = H.jitter(CS)
    try:
        for name in ("small8_every_condition", "synth130_26_nests", "berlin52_default_pa"):
            xy, packed, n, init, o, _want = CC.seeded_case(name)
            check_run(jctx, name, xy, packed, n, init, o)
    finally:
        jctx.close()
