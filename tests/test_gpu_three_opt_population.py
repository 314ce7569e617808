"""GPU parity of tl_three_opt_population (csrc/three_opt_pop.hip: one persistent workgroup per tour, the whole 3-opt descent without a
launch per move) against the oracle's three_opt (oracle/tl_oracle.c tlo_three_opt, pinned to the reference's goldens) and, beyond the
sizes the oracle affords, against tl_three_opt on the same context: every tour of a batch must be exactly what the descent gives it
alone — route element for element, cost bit for bit, and its move count.  Every case runs the per-workgroup form
(TL_FLAG_3OPT_POP_FORCE_WG) unless it says otherwise."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _oracle as O
import _plants as P
from _raw_context import _vp, jitter_context

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def wg():
    """A context that runs the per-workgroup form wherever it fits."""
    import teeline_amd as TA
    c = TA.Context(0, TA.TL_FLAG_3OPT_POP_FORCE_WG)
    yield c
    c.close()


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
    rc = ctx.lib.tl_three_opt_population(ctx.handle, _vp(xy), n, _vp(packed), _vp(init), count, _vp(out), _vp(costs), _vp(moves), C.byref(st))
    return rc, out, costs, moves, st.as_dict()


def per_pass(n):
    return n * (n - 1) * (n - 2) // 6 - (n - 2)


_oracle_cache = {}


def oracle(key, xy, packed, n, tour):
    """tlo_three_opt of one start, computed once per process (the jitter test runs the same cases again)."""
    if key not in _oracle_cache:
        rc, route, cost, st = O.three_opt(xy, packed, n, init=tour)
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
    assert st["moves"] == total and st["sweeps"] == passes and st["candidates"] == passes * per_pass(n)
    return out, costs, moves, st


# ---------------------------------------------------------------- 1. work edges, coordinates
EDGE_SIZES = [4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 63, 64, 65, 66, 67, 129]


def edge_case(n):
    xy = O.synth_xy(n, seed=n)
    k = 1 if n >= 129 else 3
    tours = [O.restart_perm(n, 3000 + n, r) for r in range(k)] + [np.arange(n, dtype=np.uint32)]
    return xy, tours


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_work_edges(wg, n):
    """n = 4 … 9: the first sizes with any triple (n = 4: two triples, one of them the i == 0 && k == n-1 skip).  The kernel's own
    seams (three_opt_pop.hip): a unit is 8 consecutive j of one i, so row 0 gets its second chunk at n = 11 (10 | 11); the units are
    dealt round-robin to threads / 64 waves, at most 16, and a tour of 14 has exactly 16 units (13: 14 units on 8 waves, a second
    round; 14: one full round of 16; 15: 18 units, a second round of 16); the lanes run along k from jlo + 1 in strides of 64, so
    the first unit's second stride begins at n = 67 (66 | 67); the rebuild of Dt strides its n + 1 columns by 64 (63 | 64) and the
    wave width itself is 64 | 65.  129: several strides and rounds of everything, more passes."""
    import teeline_amd as TA
    xy, tours = edge_case(n)
    out, costs, moves, _ = check_batch(wg, f"edges{n}", xy, None, n, tours)
    # the host mirror, with ids that are not positions
    ids = np.arange(n, dtype=np.int64) * 3 + 7
    prob = TA.TspProblem(ids, xy)
    sols = TA.three_opt.solve_population(prob, [ids[t].tolist() for t in tours], ctx=wg)
    for r, s in enumerate(sols):
        assert s.route() == ids[out[r]].tolist() and np.float32(s.total).tobytes() == costs[r].tobytes()
        assert s.stats["moves"] == int(moves[r])


# ---------------------------------------------------------------- 2. ties
LATTICES = [(8, 8), (5, 13)]


def lattice_case(w, h, ulp):
    """An integer lattice (many triples share one saving: the loop-order rule decides) or the same lattice with every coordinate
    moved by one ulp (savings at the rounding limit)."""
    n = w * h
    g = np.array([[x, y] for y in range(h) for x in range(w)], dtype=np.float32)
    if ulp:
        rng = np.random.default_rng(n)
        g = np.nextafter(g, g + rng.choice([-1, 1], (n, 2)).astype(np.float32)).astype(np.float32)
    # On the one-ulp 5 x 13 lattice the reference's descent itself does not end from some starts (restart 2 of seed 7 among them:
    # savings that are positive only by rounding lead it round a cycle — the oracle still moves after 1 000 passes); those starts
    # belong to test_pass_cap_names_the_tour, the ones here are starts from which the oracle converges.
    starts = [(7, 0), (7, 1), (8, 0)] if (w, h, ulp) == (5, 13, 1) else [(7, 0), (7, 1), (7, 2)]
    tours = [O.restart_perm(n, seed, r) for seed, r in starts]
    return np.ascontiguousarray(g), tours


@pytest.mark.parametrize("ulp", [0, 1])
@pytest.mark.parametrize("w,h", LATTICES)
def test_ties(wg, w, h, ulp):
    xy, tours = lattice_case(w, h, ulp)
    _, _, moves, _ = check_batch(wg, f"lattice{w}x{h}u{ulp}", xy, None, w * h, tours)
    assert int(moves.min()) > 10


def test_pass_cap_names_the_tour(wg):
    """A start from which the reference's descent cycles for ever (see lattice_case; the oracle is still moving after 1 000 passes):
    the per-workgroup descent stops at its cap of 64 n + 1 024 passes and the entry reports the tour."""
    from teeline_amd import _capi
    xy, tours = lattice_case(5, 13, 1)
    cycling = O.restart_perm(65, 7, 2)
    rc, _, _, st = O.three_opt(xy, None, 65, init=cycling, max_moves=1000)
    assert st["moves"] == 1000
    rc, *_ = population(wg, xy, None, 65, [tours[0], cycling, tours[1]])
    assert rc == _capi.TL_ERR_NO_CONVERGE
    assert "tour 1" in wg.lib.tl_last_error(wg.handle).decode()


# ---------------------------------------------------------------- 3. apply, all seven cases at every side
APPLY_N = 40


def apply_plants():
    """Planted matrices of tests/_plants.py at n = 40: the spans of apply_table3 that exist at this size (both segments long), and
    plants at the sides of the apply step: i = 0, k = n-1, j = i+1 (seg1 one city), k = j+1 (seg2 one city)."""
    n = APPLY_N
    T = [p for p in P.apply_table3(n, "perm") if "_both_" in p.label]
    for case in range(1, 8):
        T.append(P.plant3(n, "perm", f"pop_i0_case{case}", 0, 9 + case, 25 + case, case))
        T.append(P.plant3(n, "perm", f"pop_klast_case{case}", 2 + case, 15 + case, n - 1, case))
        T.append(P.plant3(n, "perm", f"pop_seg1one_case{case}", 4 + case, 5 + case, 30, case))
        if case != 2:  # (5, j, j+1, 2) reverses one city: no move at all
            T.append(P.plant3(n, "perm", f"pop_seg2one_case{case}", 5, 20 + case, 21 + case, case))
    # seg1 of one city with cases 2 and 6: only at i = 0 are they the first of their equivalents in loop order
    T.append(P.plant3(n, "perm", "pop_i0_seg1one_case2", 0, 1, 20, 2))
    T.append(P.plant3(n, "perm", "pop_i0_seg1one_case6", 0, 1, 20, 6))
    return T


APPLY_PLANTS = apply_plants()


def test_apply_plants_cover_every_side():
    """A check of the fixtures, on the oracle alone.  What the oracle finds first on the planted matrices (it decides the expected
    move) covers every case with both segments long and with i = 0; with k = n-1 every case but 2 (reversing path[j+1..n-1] is the
    move case 2 makes at i = 0 on the other part of the tour, which comes first in loop order).  A one-city segment reversed is
    itself, so with seg1 = one city (j = i+1) cases 1, 3, 5, 7 are no move or cases 2, 4, 6 — these three are planted (2 and 6 at
    i = 0, elsewhere the same tour is case 2 of an earlier triple) — and with seg2 = one city (k = j+1) cases 2, 3, 6, 7 are no
    move or cases 1, 4, 5, of which 1 is the 2-opt move the oracle reports at an earlier triple: 4 and 5 are planted."""
    n = APPLY_N
    mvs = [P.oracle_move(p) for p in APPLY_PLANTS]
    assert all(mv is not None for mv in mvs)

    def cases(side):
        return {mv[3] for mv in mvs if side(*mv[:3])}

    assert cases(lambda i, j, k: j - i > 10 and k - j > 10) == set(range(1, 8))
    assert cases(lambda i, j, k: i == 0) == set(range(1, 8))
    assert cases(lambda i, j, k: k == n - 1) >= {1, 3, 4, 5, 6, 7}
    assert cases(lambda i, j, k: j == i + 1) >= {2, 4, 6}
    assert cases(lambda i, j, k: k == j + 1) >= {4, 5}


@pytest.mark.parametrize("plant", APPLY_PLANTS, ids=lambda p: p.label)
def test_apply_planted_move(wg, plant):
    """Batch = [the planted start, the identity, the tour after the oracle's first move]: the descent from the planted start makes
    that move and then the descent of the tour it leaves.  Matrix form."""
    n = APPLY_N
    path, m = plant.path(), plant.matrix()
    mv = P.oracle_move(plant)
    rc, after = O.apply_3opt(path, *mv[:4])
    assert rc == 0
    tours = [path, np.arange(n, dtype=np.uint32), after]
    _, _, moves, _ = check_batch(wg, "apply_" + plant.label, None, m, n, tours)
    assert int(moves[0]) == int(moves[2]) + 1


# ---------------------------------------------------------------- 4. isolation
def test_isolation(wg):
    n = 100
    xy = O.synth_xy(n, seed=41)
    rc, opt, _, _ = O.three_opt(xy, None, n, init=O.restart_perm(n, 5, 0))  # a 3-opt local optimum: 0 moves
    rc, few = O.apply_3opt(opt, 10, 30, 60, 5)                              # one reconnection away: a few moves
    many = O.restart_perm(n, 5, 1)
    tours = [opt, few, many, np.arange(n, dtype=np.uint32), opt, many]
    out, costs, moves, st = check_batch(wg, "isolation", xy, None, n, tours)
    assert int(moves[0]) == 0 and 0 < int(moves[1]) < 10 and int(moves[2]) > 30 and int(moves[4]) == 0
    assert out[0].tolist() == opt.tolist()
    order = [2, 5, 0, 3, 1, 4]
    rc, out2, costs2, moves2, st2 = population(wg, xy, None, n, [tours[k] for k in order])
    assert rc == 0
    for pos, k in enumerate(order):
        assert out2[pos].tobytes() == out[k].tobytes() and costs2[pos].tobytes() == costs[k].tobytes() and moves2[pos] == moves[k]
    assert st2["moves"] == st["moves"] and st2["sweeps"] == st["sweeps"] and st2["candidates"] == st["candidates"]


# ---------------------------------------------------------------- 5. more tours than CUs
def test_more_tours_than_cus(wg):
    n = 52
    cus = wg.device_info()["cus"]
    count = 2 * cus + 3
    xy = O.synth_xy(n, seed=52)
    tours = [O.restart_perm(n, 5, r) for r in range(count)]
    rc, out, costs, moves, st = population(wg, xy, None, n, tours)
    assert rc == 0, wg.lib.tl_last_error(wg.handle).decode()
    for lo in range(0, count, cus):
        rc, o2, c2, m2, _ = population(wg, xy, None, n, tours[lo:lo + cus])
        assert rc == 0
        assert o2.tobytes() == out[lo:lo + cus].tobytes() and c2.tobytes() == costs[lo:lo + cus].tobytes()
        assert m2.tobytes() == moves[lo:lo + cus].tobytes()
    for r in (0, count // 3, 2 * count // 3, count - 1):
        route, cost, ost = oracle(("many", r), xy, None, n, tours[r])
        assert out[r].tolist() == route.tolist() and costs[r].tobytes() == cost.tobytes() and int(moves[r]) == ost["moves"]
    assert st["moves"] == int(moves.astype(np.int64).sum())


# ---------------------------------------------------------------- 6. batches
def test_batches_under_a_work_limit(wg):
    n, count = 65, 8
    xy = O.synth_xy(n, seed=65)
    tours = [O.restart_perm(n, 6, r) for r in range(count)]
    rc, out, costs, moves, st = population(wg, xy, None, n, tours)
    assert rc == 0
    form, threads, batch = C.c_int(), C.c_int(), C.c_uint32()
    limit = 3 * n * (n + 1) * 4 + 100  # three tours' matrices and a little that is not a fourth
    assert wg.lib.tl_three_opt_population_plan(n, count, 256, 163840, limit, wg.flags, C.byref(form), C.byref(threads), C.byref(batch)) == 0
    assert (form.value, batch.value) == (1, 3)
    assert wg.lib.tl_three_opt_population_work_limit(wg.handle, limit) == 0
    try:
        rc, o2, c2, m2, st2 = population(wg, xy, None, n, tours)
        assert rc == 0, wg.lib.tl_last_error(wg.handle).decode()
    finally:
        assert wg.lib.tl_three_opt_population_work_limit(wg.handle, 0) == 0
    assert o2.tobytes() == out.tobytes() and c2.tobytes() == costs.tobytes() and m2.tobytes() == moves.tobytes()
    assert st2["moves"] == st["moves"] and st2["sweeps"] == st["sweeps"] and st2["kernel_ms"] > 0
    for r in (0, 3, 7):  # the first tour, the first of the second batch, the last
        route, cost, ost = oracle(("batches", r), xy, None, n, tours[r])
        assert o2[r].tolist() == route.tolist() and c2[r].tobytes() == cost.tobytes() and int(m2[r]) == ost["moves"]


# ---------------------------------------------------------------- 7. beyond the strides
def circle(n):
    a = np.arange(n, dtype=np.float64) * 2 * np.pi / n
    return np.ascontiguousarray((np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32) * np.float32(1000)))


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


def test_beyond_the_strides_257(wg):
    n = 257
    xy = circle(n)
    tours = [displaced_circle_tour(n, k, seed) for k, seed in ((3, 1), (4, 2), (5, 3))]
    _, _, moves, _ = check_batch(wg, "circle257", xy, None, n, tours)
    assert 1 <= int(moves.min()) and int(moves.max()) <= 20


def test_beyond_the_strides_1100(wg):
    """More cities than a workgroup has threads; the oracle would take a minute here, so the comparison is the header's promise
    itself: tl_three_opt on the same context, which the existing suite pins to the oracle."""
    import teeline_amd as TA
    n = 1100
    prob = TA.TspProblem(np.arange(n), circle(n))
    tours = [displaced_circle_tour(n, k, seed).tolist() for k, seed in ((3, 1), (5, 2))]
    sols = TA.three_opt.solve_population(prob, tours, ctx=wg)
    for t, s in zip(tours, sols):
        one = TA.three_opt.solve(prob, None, None, t, ctx=wg)
        assert s.route() == one.route() and np.float32(s.total).tobytes() == np.float32(one.total).tobytes()
        assert 1 <= s.stats["moves"] == one.stats["moves"] <= 20


# ---------------------------------------------------------------- 8. matrix forms
@pytest.mark.parametrize("name", ["gr17", "ulysses22"])
def test_matrix_forms(wg, name, tsplib_dir):
    import teeline_amd as TA
    prob = TA.tsplib.read_from_file(os.path.join(tsplib_dir, f"{name}.tsp")).problem()
    assert prob.explicit_packed() is not None
    n = len(prob)
    tours = [prob.ids.tolist()] + [prob.ids[O.restart_perm(n, 9, r)].tolist() for r in range(3)]
    sols = TA.three_opt.solve_population(prob, tours, ctx=wg)
    total = 0
    for t, s in zip(tours, sols):
        one = TA.three_opt.solve(prob, None, None, t, ctx=wg)
        assert s.route() == one.route() and np.float32(s.total).tobytes() == np.float32(one.total).tobytes()
        assert s.stats["moves"] == one.stats["moves"]
        total += one.stats["moves"]
    assert total > 0


# ---------------------------------------------------------------- 9. golden
def test_berlin52_published_golden(wg, tsplib_dir, golden_dir):
    import teeline_amd as TA
    with open(os.path.join(golden_dir, "goldens.json")) as fh:
        g = json.load(fh)["berlin52"]["identity_three_opt"]
    prob = TA.tsplib.read_from_file(os.path.join(tsplib_dir, "berlin52.tsp")).problem()
    sols = TA.three_opt.solve_population(prob, [prob.ids.tolist(), prob.ids.tolist()], ctx=wg)
    for s in sols:
        assert f"{float(s.total):.5f}" == g["cost"] == "7716.68701" and s.route() == g["route_ids"]
        assert s.stats["moves"] == g["stats"]["moves"] == 26
    assert sols[0].stats["sweeps"] == 2 * g["stats"]["sweeps"] and sols[0].stats["candidates"] == 2 * g["stats"]["candidates"]


# ---------------------------------------------------------------- 10. the forms agree
@pytest.mark.parametrize("n", [65, 129])
def test_forms_agree(ctx, wg, n):
    import teeline_amd as TA
    xy, tours = edge_case(n)
    rc, out, costs, moves, st = population(wg, xy, None, n, tours)
    assert rc == 0
    with TA.Context(0, TA.TL_FLAG_3OPT_POP_FORCE_SCAN) as fctx:
        rc, o2, c2, m2, st2 = population(fctx, xy, None, n, tours)
        assert rc == 0, fctx.lib.tl_last_error(fctx.handle).decode()
    rc, o3, c3, m3, st3 = population(ctx, xy, None, n, tours)  # no flag: whichever form the plan picks
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    for o, c, m, s in ((o2, c2, m2, st2), (o3, c3, m3, st3)):
        assert o.tobytes() == out.tobytes() and c.tobytes() == costs.tobytes() and m.tobytes() == moves.tobytes()
        assert s["moves"] == st["moves"] and s["sweeps"] == st["sweeps"] and s["candidates"] == st["candidates"]
    assert st2["kernel_ms"] > 0 and st["kernel_ms"] > 0


# ---------------------------------------------------------------- 11. contract edges
def test_contract_edges(ctx, wg):
    import teeline_amd as TA
    from teeline_amd import _capi
    # n < 4: identities, init ignored
    xy3 = np.array([[0, 0], [3, 0], [0, 4]], np.float32)
    rc, out, costs, moves, st = population(wg, xy3, None, 3, [[2, 0, 1], [1, 2, 0], [0, 0, 0]], sentinel=9)
    assert rc == 0 and out.tolist() == [[0, 1, 2]] * 3 and moves.tolist() == [0, 0, 0]
    assert costs.tobytes() == np.full(3, O.tour_length(xy3, None, np.arange(3)), np.float32).tobytes()
    # count == 0
    rc, *_ = population(wg, O.synth_xy(10), None, 10, [])
    assert rc == _capi.TL_OK
    # a repeated city in tour 1 of 3: refused, the message names the tour, nothing written
    n = 20
    xy = O.synth_xy(n, seed=3)
    bad = O.restart_perm(n, 1, 1).copy()
    bad[7] = bad[3]
    rc, out, costs, moves, _ = population(wg, xy, None, n, [O.restart_perm(n, 1, 0), bad, O.restart_perm(n, 1, 2)], sentinel=0xABCD)
    assert rc == _capi.TL_ERR_BADARG
    assert "tour 1" in wg.lib.tl_last_error(wg.handle).decode()
    assert (out == 0xABCD).all() and (moves == 0xABCD).all() and (costs == np.float32(0xABCD)).all()
    # tl_two_opt_last_counters after a population call: the previous 2-opt's counters, or a refusal — never anything else
    prob = TA.TspProblem(np.arange(50), O.synth_xy(50, seed=5))
    TA.two_opt.solve(prob, ctx=wg)
    before = list(wg.two_opt_last_counters())
    rc, *_ = population(wg, prob.xy, None, 50, [O.restart_perm(50, 2, r) for r in range(3)])
    assert rc == 0
    try:
        after = list(wg.two_opt_last_counters())
    except TA.TeelineGpuError as e:
        assert e.code == _capi.TL_ERR_BADARG
    else:
        assert after == before
    assert wg.three_opt_pop_max_n() == ctx.three_opt_pop_max_n() == (wg.device_info()["lds_bytes"] - 264) // 20


# ---------------------------------------------------------------- 12. population pipeline
def test_run_population_equals_the_pipeline_per_tour(wg):
    import teeline_amd as TA
    n = 100
    ids = np.arange(n, dtype=np.int64) + 1
    prob = TA.TspProblem(ids, O.synth_xy(n, seed=100))
    tours = [ids[O.restart_perm(n, 11, r)].tolist() for r in range(4)]
    steps = ["2opt", "3opt", "or_opt"]
    got = TA.pipeline.run_population(prob, steps, tours, ctx=wg)
    assert len(got) == 4
    for t, stages in zip(tours, got):
        want = TA.pipeline.run_pipeline_stages(prob, steps, ctx=wg, init_tour=t)
        assert [s.name for s in stages] == steps == [s.name for s in want]
        for a, b in zip(stages, want):
            assert a.solution.route() == b.solution.route()
            assert np.float32(a.solution.total).tobytes() == np.float32(b.solution.total).tobytes()
        for k in (1, 2):
            assert stages[k].solution.stats["moves"] == want[k].solution.stats["moves"]


# ---------------------------------------------------------------- 13. jitter build
def test_jitter_build():
    """Cases 1 and 2 on the race-stress build (-DTL_JITTER: waves leave every barrier far apart)."""
    from teeline_amd import _capi
    vp, u32 = C.c_void_p, C.c_uint32
    jctx = jitter_context({"tl_three_opt_population": [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp]}, _capi.TL_FLAG_3OPT_POP_FORCE_WG)
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
