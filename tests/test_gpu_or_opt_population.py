"""GPU parity of tl_or_opt_population (csrc/or_opt_lds.hip: one workgroup per tour, the whole Or-opt descent in LDS) against the
oracle's or_opt (oracle/tl_oracle.c tlo_or_opt, pinned to the reference's goldens): every tour of a batch must be exactly what the
descent gives it alone — route element for element, cost bit for bit, and its move count."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _oracle as O
import _plants as P
from _raw_context import _vp, jitter_context

pytestmark = pytest.mark.gpu



def population(ctx, xy, packed, n, tours, sentinel=None):
    """Raw call: (rc, out [count][n], costs, moves, stats dict)."""
    from teeline_amd import _capi
    count = len(tours)
    init = np.ascontiguousarray(np.asarray(tours, dtype=np.uint32).reshape(count, n)) if count else np.zeros((0, n), np.uint32)
    xy = None if xy is None else np.ascontiguousarray(xy, dtype=np.float32)
    packed = None if packed is None else np.ascontiguousarray(packed, dtype=np.float32)
    fill = 0 if sentinel is None else sentinel
    out = np.full((count, n), fill, dtype=np.uint32)
    costs = np.full(count, np.float32(fill), dtype=np.float32)
    moves = np.full(count, fill, dtype=np.uint32)
    st = _capi.TlStats()
    rc = ctx.lib.tl_or_opt_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(init), count, _vp(out), _vp(costs), _vp(moves), C.byref(st))
    return rc, out, costs, moves, st.as_dict()


_oracle_cache = {}


def oracle(key, xy, packed, n, tour):
    """tlo_or_opt of one start, computed once per process (the jitter test runs the same cases again)."""
    if key not in _oracle_cache:
        rc, route, cost, st = O.or_opt(xy, packed, n, init=tour)
        assert rc == 0
        route.setflags(write=False)
        _oracle_cache[key] = (route, np.float32(cost), st)
    return _oracle_cache[key]


def check_batch(ctx, name, xy, packed, n, tours):
    rc, out, costs, moves, st = population(ctx, xy, packed, n, tours)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    total = passes = 0
    for r, tour in enumerate(tours):
        route, cost, ost = oracle((name, r), xy, packed, n, tour)
        assert out[r].tolist() == route.tolist(), f"{name}: tour {r} differs from the oracle's"
        assert costs[r].tobytes() == cost.tobytes(), f"{name}: tour {r} cost {costs[r]!r} != {cost!r}"
        assert int(moves[r]) == ost["moves"], f"{name}: tour {r} made {moves[r]} moves, the oracle {ost['moves']}"
        total += ost["moves"]
        passes += ost["sweeps"]
    assert st["moves"] == total and st["sweeps"] == passes
    return out, costs, moves, st


# ---------------------------------------------------------------- 1. work edges, coordinates
EDGE_SIZES = [4, 5, 6, 8, 9, 63, 64, 65, 127, 129, 257]


def edge_case(n):
    xy = O.synth_xy(n, seed=n)
    tours = [O.restart_perm(n, 1000 + n, r) for r in range(4)] + [np.arange(n, dtype=np.uint32)]
    return xy, tours


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_work_edges(ctx, n):
    """seg_len gates at n = 4 / 5, the 8-start group edge at 8 / 9, the 63-wide insertion chunk and the 64-lane wave at 63 / 64 / 65,
    two and more chunks at 127 / 129 / 257."""
    import teeline_amd as TA
    xy, tours = edge_case(n)
    out, costs, moves, _ = check_batch(ctx, f"edges{n}", xy, None, n, tours)
    # the host mirror, with ids that are not positions
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    prob = TA.TspProblem(ids, xy)
    sols = TA.or_opt.solve_population(prob, [ids[t].tolist() for t in tours], ctx=ctx)
    for r, s in enumerate(sols):
        assert s.route() == ids[out[r]].tolist() and np.float32(s.total).tobytes() == costs[r].tobytes()
        assert s.stats["moves"] == int(moves[r])


# ---------------------------------------------------------------- 2. ties
LATTICES = [(8, 8), (5, 13), (16, 16)]


def lattice_case(w, h, ulp):
    """An integer lattice (many placements share one delta: the loop-order tie rule decides) or the same lattice with every
    coordinate moved by one ulp (deltas at the rounding limit)."""
    n = w * h
    g = np.array([[x, y] for y in range(h) for x in range(w)], dtype=np.float32)
    if ulp:
        rng = np.random.default_rng(n)
        g = np.nextafter(g, g + rng.choice([-1, 1], (n, 2)).astype(np.float32)).astype(np.float32)
    tours = [O.restart_perm(n, 7, r) for r in range(2 if n > 100 else 3)]
    return np.ascontiguousarray(g), tours


@pytest.mark.parametrize("ulp", [0, 1])
@pytest.mark.parametrize("w,h", LATTICES)
def test_ties(ctx, w, h, ulp):
    xy, tours = lattice_case(w, h, ulp)
    _, _, moves, _ = check_batch(ctx, f"lattice{w}x{h}u{ulp}", xy, None, w * h, tours)
    assert int(moves.min()) > 10


# ---------------------------------------------------------------- 3. apply at every side
APPLY_N = 40
# (seg_len, i, j, reversed): i = 0 (prev = n-1); i + seg_len = n (after_seg wraps to 0); j < i and j >= i + seg_len; j = n-1; the five kinds
APPLY_AIMS = [(1, 0, 5, 0), (2, 0, 20, 1), (3, 0, 25, 1), (3, APPLY_N - 3, 4, 0), (2, APPLY_N - 2, 7, 0), (1, APPLY_N - 1, 12, 0),
              (3, 10, APPLY_N - 1, 1), (1, 17, APPLY_N - 1, 0), (2, 9, APPLY_N - 1, 0), (2, 20, 3, 1), (3, 5, 30, 0), (2, 12, 30, 1)]


def test_apply_aims_cover_every_side():
    aims = APPLY_AIMS
    n = APPLY_N
    assert any(i == 0 for _, i, _, _ in aims) and any(i + L == n for L, i, _, _ in aims)
    assert any(j < i for _, i, j, _ in aims) and any(j >= i + L for L, i, j, _ in aims) and any(j == n - 1 for _, _, j, _ in aims)
    assert {(L, bool(r)) for L, _, _, r in aims} == {(1, False), (2, False), (2, True), (3, False), (3, True)}


@pytest.mark.parametrize("aim", APPLY_AIMS, ids=lambda a: "len%d_i%d_j%d_rev%d" % a)
def test_apply_planted_move(ctx, aim):
    """A constant matrix with the planted move's new edges lowered (tests/_plants.py): the oracle's first move from the start is
    the planted one, and the population's final tours are the oracle's."""
    n = APPLY_N
    plant = P.plant_or(n, "perm", "population_apply", *aim)
    path, m = plant.path(), plant.matrix()
    mv = O.or_opt_find_best_move(None, m, path)
    assert P.coords(plant, mv) == (aim[0], aim[1], aim[2], bool(aim[3]))
    rc, after = O.apply_relocation(path, aim[1], aim[0], aim[2], bool(aim[3]))
    assert rc == 0
    tours = [path, np.arange(n, dtype=np.uint32), after]
    _, _, moves, _ = check_batch(ctx, "apply%s" % (aim,), None, m, n, tours)
    assert int(moves[0]) == int(moves[2]) + 1  # the planted move, then the descent from the tour it leaves


# ---------------------------------------------------------------- 4. isolation
def test_isolation(ctx):
    n = 100
    xy = O.synth_xy(n, seed=41)
    rc, opt, _, _ = O.or_opt(xy, None, n, init=O.restart_perm(n, 5, 0))  # an Or-opt local optimum: 0 moves
    rc, few = O.apply_relocation(opt, 10, 2, 60, True)                   # one segment displaced: a few moves
    many = O.restart_perm(n, 5, 1)
    tours = [opt, few, many, np.arange(n, dtype=np.uint32), opt, many]
    out, costs, moves, st = check_batch(ctx, "isolation", xy, None, n, tours)
    assert int(moves[0]) == 0 and 0 < int(moves[1]) < 10 and int(moves[2]) > 30 and int(moves[4]) == 0
    assert out[0].tolist() == opt.tolist()
    order = [2, 5, 0, 3, 1, 4]
    rc, out2, costs2, moves2, st2 = population(ctx, xy, None, n, [tours[k] for k in order])
    assert rc == 0
    for pos, k in enumerate(order):
        assert out2[pos].tobytes() == out[k].tobytes() and costs2[pos].tobytes() == costs[k].tobytes() and moves2[pos] == moves[k]
    assert st2["moves"] == st["moves"] and st2["sweeps"] == st["sweeps"] and st2["candidates"] == st["candidates"]


# ---------------------------------------------------------------- 5. more tours than CUs
def test_more_tours_than_cus(ctx):
    n = 64
    cus = ctx.device_info()["cus"]
    count = 2 * cus + 3
    xy = O.synth_xy(n, seed=64)
    tours = [O.restart_perm(n, 5, r) for r in range(count)]
    rc, out, costs, moves, st = population(ctx, xy, None, n, tours)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    for lo in range(0, count, cus):
        rc, o2, c2, m2, _ = population(ctx, xy, None, n, tours[lo:lo + cus])
        assert rc == 0
        assert o2.tobytes() == out[lo:lo + cus].tobytes() and c2.tobytes() == costs[lo:lo + cus].tobytes()
        assert m2.tobytes() == moves[lo:lo + cus].tobytes()
    for r in (0, count // 3, 2 * count // 3, count - 1):
        route, cost, ost = oracle(("many", r), xy, None, n, tours[r])
        assert out[r].tolist() == route.tolist() and costs[r].tobytes() == cost.tobytes() and int(moves[r]) == ost["moves"]
    assert st["moves"] == int(moves.astype(np.int64).sum())


# ---------------------------------------------------------------- 6. beyond one workgroup's thread count
def displaced_circle_tour(n, k, seed):
    """The convex order with k segments of 1 to 3 cities taken out and put back elsewhere, some of them reversed."""
    rng = np.random.default_rng(seed)
    t = list(range(n))
    for _ in range(k):
        L = int(rng.integers(1, 4))
        i = int(rng.integers(0, len(t) - L))
        seg = t[i:i + L]
        del t[i:i + L]
        at = int(rng.integers(0, len(t)))
        t[at:at] = seg[::-1] if rng.integers(0, 2) else seg
    return np.array(t, dtype=np.uint32)


def test_beyond_one_workgroups_threads(ctx):
    n = 1100
    a = np.arange(n, dtype=np.float64) * 2 * np.pi / n
    xy = np.ascontiguousarray((np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32) * np.float32(1000)))
    tours = [displaced_circle_tour(n, k, seed) for k, seed in ((3, 1), (5, 2), (8, 3))]
    for r, t in enumerate(tours):
        assert 3 <= oracle(("circle", r), xy, None, n, t)[2]["moves"] <= 20
    check_batch(ctx, "circle", xy, None, n, tours)


# ---------------------------------------------------------------- 7. matrix forms
@pytest.mark.parametrize("name", ["gr17", "ulysses22"])
def test_matrix_forms(ctx, name, tsplib_dir):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(os.path.join(tsplib_dir, f"{name}.tsp")).problem()
    assert prob.explicit_packed() is not None
    n = len(prob)
    tours = [prob.ids.tolist()] + [prob.ids[O.restart_perm(n, 9, r)].tolist() for r in range(3)]
    sols = TA.or_opt.solve_population(prob, tours, ctx=ctx)
    total = 0
    for t, s in zip(tours, sols):
        one = TA.or_opt.solve(prob, None, None, t, ctx=ctx)
        assert s.route() == one.route() and np.float32(s.total).tobytes() == np.float32(one.total).tobytes()
        assert s.stats["moves"] == one.stats["moves"]
        total += one.stats["moves"]
    assert total > 0


def test_berlin52_published_golden(ctx, tsplib_dir, golden_dir):
    import teeline_amd as TA
    with open(os.path.join(golden_dir, "goldens.json")) as fh:
        g = json.load(fh)["berlin52"]["identity_or_opt"]
    prob = TA.tsplib.read_from_file(os.path.join(tsplib_dir, "berlin52.tsp")).problem()
    sols = TA.or_opt.solve_population(prob, [prob.ids.tolist(), prob.ids.tolist()], ctx=ctx)
    for s in sols:
        assert f"{float(s.total):.5f}" == g["cost"] == "7999.91797" and s.route() == g["route_ids"]
        assert s.stats["moves"] == g["stats"]["moves"]
    assert sols[0].stats["sweeps"] == 2 * g["stats"]["sweeps"] and sols[0].stats["candidates"] == 2 * g["stats"]["candidates"]


# ---------------------------------------------------------------- 8. fallback
@pytest.mark.parametrize("n", [65, 129])
def test_forced_scan_fallback_is_identical(ctx, n):
    import teeline_amd as TA
    xy, tours = edge_case(n)
    rc, out, costs, moves, st = population(ctx, xy, None, n, tours)
    assert rc == 0
    with TA.Context(0, TA.TL_FLAG_OR_OPT_FORCE_SCAN) as fctx:
        rc, o2, c2, m2, st2 = population(fctx, xy, None, n, tours)
        assert rc == 0, fctx.lib.tl_last_error(fctx.handle).decode()
    assert o2.tobytes() == out.tobytes() and c2.tobytes() == costs.tobytes() and m2.tobytes() == moves.tobytes()
    assert st2["moves"] == st["moves"] and st2["sweeps"] == st["sweeps"] and st2["candidates"] == st["candidates"]
    assert st2["kernel_ms"] > 0 and st["kernel_ms"] > 0


# ---------------------------------------------------------------- 9. contract edges
def test_contract_edges(ctx):
    import teeline_amd as TA
    from teeline_amd import _capi
    # n < 4: identities, init ignored
    xy3 = np.array([[0, 0], [3, 0], [0, 4]], np.float32)
    rc, out, costs, moves, st = population(ctx, xy3, None, 3, [[2, 0, 1], [1, 2, 0], [0, 0, 0]], sentinel=9)
    assert rc == 0 and out.tolist() == [[0, 1, 2]] * 3 and moves.tolist() == [0, 0, 0]
    assert costs.tobytes() == np.full(3, O.tour_length(xy3, None, np.arange(3)), np.float32).tobytes()
    # count == 0
    rc, *_ = population(ctx, O.synth_xy(10), None, 10, [])
    assert rc == _capi.TL_OK
    # a repeated city in tour 1 of 3: refused, the message names the tour, nothing written
    n = 20
    xy = O.synth_xy(n, seed=3)
    bad = O.restart_perm(n, 1, 1).copy()
    bad[7] = bad[3]
    rc, out, costs, moves, _ = population(ctx, xy, None, n, [O.restart_perm(n, 1, 0), bad, O.restart_perm(n, 1, 2)], sentinel=0xABCD)
    assert rc == _capi.TL_ERR_BADARG
    assert "tour 1" in ctx.lib.tl_last_error(ctx.handle).decode()
    assert (out == 0xABCD).all() and (moves == 0xABCD).all() and (costs == np.float32(0xABCD)).all()
    # tl_two_opt_last_counters after a population call: the previous 2-opt's counters, or a refusal — never anything else
    prob = TA.TspProblem(np.arange(50), O.synth_xy(50, seed=5))
    TA.two_opt.solve(prob, ctx=ctx)
    before = list(ctx.two_opt_last_counters())
    rc, *_ = population(ctx, prob.xy, None, 50, [O.restart_perm(50, 2, r) for r in range(3)])
    assert rc == 0
    try:
        after = list(ctx.two_opt_last_counters())
    except TA.TeelineGpuError as e:
        assert e.code == _capi.TL_ERR_BADARG
    else:
        assert after == before


# ---------------------------------------------------------------- 10. population pipeline
def test_run_population_equals_the_pipeline_per_tour(ctx):
    import teeline_amd as TA
    n = 200
    ids = np.arange(n, dtype=np.int64) + 1
    prob = TA.TspProblem(ids, O.synth_xy(n, seed=200))
    tours = [ids[O.restart_perm(n, 11, r)].tolist() for r in range(4)]
    steps = ["2opt", "or_opt"]
    got = TA.pipeline.run_population(prob, steps, tours, ctx=ctx)
    assert len(got) == 4
    for t, stages in zip(tours, got):
        want = TA.pipeline.run_pipeline_stages(prob, steps, ctx=ctx, init_tour=t)
        assert [s.name for s in stages] == steps == [s.name for s in want]
        for a, b in zip(stages, want):
            assert a.solution.route() == b.solution.route()
            assert np.float32(a.solution.total).tobytes() == np.float32(b.solution.total).tobytes()
        assert stages[1].solution.stats["moves"] == want[1].solution.stats["moves"]


# ---------------------------------------------------------------- 11. jitter build
def test_jitter_build():
    """Cases 1 and 2 on the race-stress build (-DTL_JITTER: waves leave every barrier far apart)."""
    vp, u32 = C.c_void_p, C.c_uint32
    jctx = jitter_context({"tl_or_opt_population": [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp]})
    try:
        for n in EDGE_SIZES:
            xy, tours = edge_case(n)
            check_batch(jctx, f"edges{n}", xy, None, n, tours)
        for w, h in LATTICES:
            for ulp in (0, 1):
                xy, tours = lattice_case(w, h, ulp)
                check_batch(jctx, f"lattice{w}x{h}u{ulp}", xy, None, w * h, tours)
    finally:
        jctx.close()
