"""The particle swarm solver on the GPU (tl_particle_swarm*, csrc/particle_swarm.hip) against the statement of its specification
(tests/_pso_oracle.py), by exact equality throughout: the best tour element for element, its cost bit for bit, every record of the
improvement log with its route, every word of the per-epoch record (every particle's cost bits and velocity length — which pin the
keeps, the truncation, the swap sequences and the sequential sums of every step, and through the later particles of an improving
epoch the second pass of the commit) and the stats against the oracle's counters — in both input forms and for the runs of a
batch; and the device's swap sequence alone on given permutation pairs (tl_pso_selftest_swap_sequence)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import _pso_cases as PC
import _pso_oracle as PO
import _sa_cases as K
import _swarm_harness as H
from _raw_context import _vp

pytestmark = pytest.mark.gpu

NT = PC.THREADS
bits = PO.bits


PSO = H.PSO
_opts = PSO.opts
gpu_trace, plan, check_run = (functools.partial(f, PSO) for f in (H.gpu_trace, H.plan, H.check_run))
okey = H.okey


# ---------------------------------------------------------------- the device's swap sequence
def device_sequences(ctx, src, dst):
    src, dst = np.ascontiguousarray(src, dtype=np.uint32), np.ascontiguousarray(dst, dtype=np.uint32)
    count, n = src.shape
    pairs = np.zeros((count, n, 2), dtype=np.uint32)
    lens = np.zeros(count, dtype=np.uint32)
    rc = ctx.lib.tl_pso_selftest_swap_sequence(ctx.handle, _vp(src), _vp(dst), n, count, _vp(pairs), _vp(lens))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert all((pairs[c, lens[c]:] == 0xFFFFFFFF).all() for c in range(count))
    return [[(int(i), int(j)) for i, j in pairs[c, :lens[c]]] for c in range(count)]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, NT - 1, NT, NT + 1, 2 * NT + 44, 1002])
def test_selftest_swap_sequence(ctx, n):
    """identity, one transposition, one n-cycle (an orbit across every pass of the strided loop), its inverse, random pairs: the
    literal loop's pairs"""
    rng = np.random.default_rng(n)
    ident = np.arange(n)
    rows = [(ident, ident)]
    if n >= 2:
        t = ident.copy()
        t[[0, n - 1]] = t[[n - 1, 0]]
        rows += [(ident, t), (ident, np.roll(ident, 1)), (ident, np.roll(ident, -1)), (np.roll(ident, 3), ident[::-1].copy())]
    rows += [(rng.permutation(n), rng.permutation(n)) for _ in range(5)]
    got = device_sequences(ctx, np.stack([a for a, _ in rows]), np.stack([b for _, b in rows]))
    for (a, b), seq in zip(rows, got):
        assert seq == PO.swap_sequence_literal(a, b), (n, a[:8], b[:8])
        assert PO.apply_swaps(a, seq) == [int(v) for v in b]
    assert got[0] == []
    if n >= 2:
        assert got[1] == [(0, n - 1)] and len(got[2]) == n - 1 == len(got[3])
        if n > NT:
            assert max(PO.orbits(*rows[2])[1]) == n  # one orbit longer than a pass


def test_selftest_reference_vectors_and_errors(ctx):
    from teeline_amd import _capi
    assert device_sequences(ctx, [[0, 1, 2, 3]], [[0, 2, 1, 3]]) == [[(1, 2)]]  # route.rs: [1,2,3,4] -> [1,3,2,4]
    assert device_sequences(ctx, [[0, 1, 2, 3]], [[0, 1, 2, 3]]) == [[]]
    bad = np.array([[0, 1, 1, 3]], dtype=np.uint32)
    good = np.arange(4, dtype=np.uint32).reshape(1, 4)
    out, ln = np.zeros((1, 4, 2), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert ctx.lib.tl_pso_selftest_swap_sequence(ctx.handle, _vp(bad), _vp(good), 4, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_pso_selftest_swap_sequence(ctx.handle, _vp(good), None, 4, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG
    assert ctx.lib.tl_pso_selftest_swap_sequence(ctx.handle, _vp(good), _vp(good), 0, 1, _vp(out), _vp(ln)) == _capi.TL_ERR_BADARG


# ---------------------------------------------------------------- whole runs
GOLDEN = PC.golden_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases(ctx, name):
    xy, packed, n, init, o = GOLDEN[name]
    res = check_run(ctx, name, xy, packed, n, init, o)
    PC.check_conditions(name, n, res, o)


@pytest.mark.parametrize("name", sorted(PC.SEEDED))
def test_seeded_conditions(ctx, name):
    """the redo path (two improvements in one epoch, a later particle seeing the new gbest), improvements by the first and the
    last particle, truncation inside the cognitive and the social part and none, a keep of 0 and one above its length: each
    asserted from the oracle's record, the run equal word for word"""
    xy, packed, n, init, o, want = PC.seeded_case(name)
    res = check_run(ctx, name, xy, packed, n, init, o)
    assert set(want) <= PC.conditions(res), (name, set(want) - PC.conditions(res))


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_smallest_sizes(ctx, n):
    """v_max is 1 or 2, the sequences are empty or nearly so"""
    xy = PC.instance(n)
    check_run(ctx, "size", xy, None, n, None, dict(epochs=6, n_nearest=3, seed=11 + n, run=0))
    check_run(ctx, "size_init", xy, None, n, PC.start_tour(n, n), dict(epochs=6, n_nearest=3, seed=11 + n, run=1))


@pytest.mark.parametrize("n,epochs", [(65, 5), (130, 4), (NT + 1, 3), (300, 3), (2 * NT + 88, 3)])
def test_second_trips_of_the_strided_loops(ctx, n, epochs):
    """just past one wave, two waves and a bit, just past one workgroup pass, n = 600: orbits longer than a pass"""
    res = check_run(ctx, "trips", PC.instance(n), None, n, None, dict(epochs=epochs, n_nearest=3, seed=n, run=0))
    if n > 2 * NT:  # the social sequences of epoch 0 walk orbits longer than one pass (a random permutation's longest cycle is ~0.62 n)
        start = res["improvements"][0][3]
        assert max(max(PO.orbits(PO.shuffled(PO.chain_key(n, 0), n, i), start)[1]) for i in range(30)) > NT


def test_matrix_forms(ctx):
    xy = PC.instance(257)
    from teeline_amd import _capi
    pk = np.empty(257 * 256 // 2, dtype=np.float32)
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _vp(xy), 257, _capi.TL_DIST_EUC2D, _capi.TL_DM_PACKED_LOWER, _vp(pk), None))
    check_run(ctx, "m257", None, pk, 257, None, dict(epochs=3, n_nearest=3, seed=257, run=0))


@pytest.mark.parametrize("n_nearest", [30, 31, 64, 65])
def test_particle_counts(ctx, n_nearest):
    res = check_run(ctx, "particles", PC.instance(40), None, 40, PC.start_tour(40, 4), dict(epochs=6, n_nearest=n_nearest, seed=40, run=0))
    assert res["particles"] == n_nearest


@pytest.mark.parametrize("epochs", [0, 1, 2])
def test_epochs(ctx, epochs):
    xy = K.small(8)
    check_run(ctx, "epochs", xy, None, 8, None, dict(epochs=epochs, n_nearest=3, seed=5, run=0))
    res = check_run(ctx, "epochs_init", xy, None, 8, PC.start_tour(8, 2), dict(epochs=epochs, n_nearest=3, seed=5, run=0))
    if epochs == 0:  # the start gbest: the first minimum over the initial tour and 29 shuffles
        assert len(res["improvements"]) == 1


def test_n_1002(ctx):
    check_run(ctx, "n1002", PC.instance(1002), None, 1002, None, dict(epochs=1, n_nearest=3, seed=1002, run=0), seq=PO.swap_sequence_inverse)


def test_largest_n(ctx):
    """n = tl_particle_swarm_max_n with one epoch: the workgroup's LDS to its last byte.  One city more is refused before anything of
    size n is read (the arrays passed hold 52 cities)."""
    from teeline_amd import _capi
    top = ctx.lib.tl_particle_swarm_max_n(ctx.handle)
    assert 4096 < top <= 65535 and plan(ctx, top)[3] >= 1 and plan(ctx, top + 1) == (0, 0, 0, 0)
    check_run(ctx, "largest", PC.instance(top), None, top, None, dict(epochs=1, n_nearest=3, seed=top, run=0), seq=PO.swap_sequence_inverse)
    b = K.tsplib("berlin52")
    out, cost = np.zeros(52, dtype=np.uint32), C.c_float()
    po = _opts(dict(epochs=1, n_nearest=3))
    rc = ctx.lib.tl_particle_swarm(ctx.handle, _vp(b["xy"]), top + 1, None, None, C.byref(po), 1, _vp(out), C.byref(cost), None)
    assert rc == _capi.TL_ERR_UNSUPPORTED and "exceeds the limit" in ctx.lib.tl_last_error(ctx.handle).decode()


def test_small_n_needs_no_device(ctx):
    for n in (0, 1):
        xy = K.small(3)[:n]
        o = dict(epochs=3, n_nearest=3, seed=1, run=0)
        res = PO.solve(xy, None, n, None, **o)
        rc, out, gcost, glog, ln, st, routes, elog = gpu_trace(ctx, xy if n else K.small(3), None, n, None, o)
        assert rc == 0 and out.tolist() == list(range(n)) and bits(gcost) == 0 and ln == 1 and glog.tolist() == PO.log_words(res).tolist()
        assert elog.tolist() == PO.epoch_words(res).tolist() and st["moves"] == 0


def test_plain_entry_defaults_and_truncated_trace(ctx):
    H.plain_entry_defaults_and_truncated_trace(PSO, ctx, GOLDEN)


# ---------------------------------------------------------------- batches
POP = dict(epochs=4, n_nearest=3, seed=31)


def test_batches(ctx):
    H.batches(PSO, ctx, PC, POP)


def test_more_runs_than_one_launch_sequence(ctx):
    """the run is the grid's y: a sequence holds at most 65535 runs; at n = 3 a 65536th run goes in a second one"""
    H.more_runs_than_one_launch_sequence(PSO, ctx, dict(epochs=1, n_nearest=3, seed=3), 2 * (6 * 30 * 60 + 120 + 8 * 30 * 21 + 16 * 30) + 2560)


# ---------------------------------------------------------------- context reuse, errors
def test_context_reuse_larger_then_smaller():
    """stale positions, velocities and logs must not leak: the larger instance leaves its tables where the smaller one's begin"""
    H.context_reuse(PSO, [("trips", PC.instance(300), None, 300, None, dict(epochs=3, n_nearest=3, seed=300, run=0)),
                          ("epochs", K.small(8), None, 8, None, dict(epochs=2, n_nearest=3, seed=5, run=0)), ("gr17_matrix",) + GOLDEN["gr17_matrix"]])


def test_errors(ctx):
    H.common_errors(PSO, ctx, "particles")


# ---------------------------------------------------------------- mirrors
def test_python_mirror_progress_runs_and_pipeline(ctx):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(os.path.join(K.TSPLIB, "berlin52.tsp")).problem()
    xy, _pk, n, init, o = GOLDEN["berlin52"]
    opts = TA.HeuristicOptions(epochs=o["epochs"])
    res = PO.solve_cached(okey("berlin52", n, init, o), prob.xy, None, 52, None, **o)
    msgs = []
    sol = TA.particle_swarm.solve(prob, opts, lambda k, p: msgs.append((k, p)), None, ctx=ctx, seed=1)
    want = PO.messages(res, prob.ids)
    assert [k for k, _ in msgs] == [k for k, _ in want] and sum(k == "EpochUpdate" for k, _ in msgs) == o["epochs"]
    for (k, p), (_k, w) in zip(msgs, want):
        if k == "PathUpdate":
            assert p[0] == w[0] and bits(p[1]) == bits(w[1])
        else:
            assert p == w
    assert sol.route() == prob.ids[res["tour"]].tolist() and bits(sol.total) == bits(res["cost"])
    plain = TA.particle_swarm.solve(prob, opts, None, None, ctx=ctx, seed=1)
    assert plain.route() == sol.route() and plain.stats["moves"] == res["counters"]["improved"]
    short = TA.HeuristicOptions(epochs=5, n_nearest=31)
    so = dict(epochs=5, n_nearest=31, seed=1)
    msgs2 = []
    bestsol = TA.particle_swarm.solve(prob, short, lambda k, p: msgs2.append((k, p)), None, ctx=ctx, seed=1, runs=4)
    singles = [PO.solve_cached(okey("mirror", 52, None, dict(so, run=r)), prob.xy, None, 52, None, **dict(so, run=r)) for r in range(4)]
    r = int(np.argmin([(bits(s["cost"]) << 32) | k for k, s in enumerate(singles)]))
    assert bestsol.stats["run"] == r and bestsol.route() == prob.ids[singles[r]["tour"]].tolist() and bits(bestsol.total) == bits(singles[r]["cost"])
    assert [k for k, _ in msgs2] == [k for k, _ in PO.messages(singles[r])]
    steps = TA.pipeline.steps_for_solve("particle_swarm")
    assert steps == ["shuffle", "particle_swarm"]
    outs = TA.pipeline.run_pipeline_stages(prob, steps, {"particle_swarm": short}, ctx=ctx, lk_seed=3)
    assert [x.name for x in outs] == steps and TA.validate_tour(outs[-1].solution.route(), prob)
    seeded = PO.solve(prob.xy, None, 52, prob.positions_of(outs[0].solution.route()), **dict(so, seed=3))
    assert outs[-1].solution.route() == prob.ids[seeded["tour"]].tolist() and bits(outs[-1].solution.total) == bits(seeded["cost"])
    with pytest.raises(ValueError, match="the seeded particle swarm of this build is `particle_swarm`"):
        TA.pipeline.steps_for_solve("pso")


def test_cli_equals_the_oracle(ctx):
    import re
    import teeline_amd as TA
    from teeline_amd import build
    cli = build.build_cli()
    tsp = os.path.join(K.TSPLIB, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(tsp).problem()
    args0 = ["--epochs", "6", "--seed", "3", "--n-nearest", "31"]
    o = dict(epochs=6, n_nearest=31, seed=3)
    fmt = lambda res: TA.pipeline.format_solution(TA.Solution(res["cost"], prob.ids[res["tour"]], prob)).splitlines()  # noqa: E731
    r = subprocess.run([cli, "solve", "particle_swarm", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    shuffled = TA.pipeline.run_pipeline_stages(prob, ["shuffle"], {}, ctx=ctx, lk_seed=3)[0].solution
    res = PO.solve(prob.xy, None, 52, prob.positions_of(shuffled.route()), **o)
    assert r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "particle_swarm", "--no-seed", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    res = PO.solve(prob.xy, None, 52, None, **o)
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(res)
    r = subprocess.run([cli, "solve", "pso", "-i", tsp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "not accelerated by this build" in r.stderr and "the seeded particle swarm of this build is `particle_swarm`" in r.stderr
    # the C++ mirror's messages: PathUpdate(start) and one per improvement, EpochUpdate per epoch, Done
    r = subprocess.run([cli, "solve", "particle_swarm", "--no-seed", "--progress-digest", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=[0-9a-f]{16} epoch_updates=(\d+)", r.stderr)
    assert r.returncode == 0 and m, r.stderr
    assert [int(v) for v in m.groups()] == [len(res["improvements"]), 0, 1, o["epochs"]]
    r = subprocess.run([cli, "solve", "particle_swarm", "--no-seed", "--runs", "3", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    three = [PO.solve(prob.xy, None, 52, None, **dict(o, run=k)) for k in range(3)]
    best = three[int(np.argmin([(bits(t["cost"]) << 32) | k for k, t in enumerate(three)]))]
    assert r.returncode == 0 and r.stdout.splitlines()[-2:] == fmt(best)
    r = subprocess.run([cli, "pipeline", "--steps=shuffle,particle_swarm,2opt", "-i", tsp] + args0, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = TA.pipeline.run_pipeline_stages(prob, ["shuffle", "particle_swarm", "2opt"], {"particle_swarm": TA.HeuristicOptions(epochs=6, n_nearest=31)}, ctx=ctx,
                                           lk_seed=3)[-1].solution
    assert r.stdout.splitlines()[-2:] == TA.pipeline.format_solution(want).splitlines()


# ---------------------------------------------------------------- jitter build
def test_jitter_build():
    """a handful of the cases above on the race-stress build (-DTL_JITTER: waves leave every barrier far apart): the compaction's
    double-buffered wave counts, the LDS blocks reused within a step, the commit's second pass"""
    jctx = H.jitter(PSO)
    try:
        for name in ("small8_every_condition", "synth130_every_condition"):
            xy, packed, n, init, o, _want = PC.seeded_case(name)
            check_run(jctx, name, xy, packed, n, init, o)
        check_run(jctx, "trips", PC.instance(300), None, 300, None, dict(epochs=3, n_nearest=3, seed=300, run=0))
    finally:
        jctx.close()
