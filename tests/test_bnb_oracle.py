"""The branch and bound's contract on the CPU: tl_branch_and_bound_host (the sequential restatement, csrc/tl_api_bnb.hip) against
brute force over every sequence (tests/_bnb_oracle.py: no bound, so an unsafe prune shows), against the plain Python search for its
node counts, and against tests/golden/goldens_bnb.json on the larger cases.

bays29 is not tested: from its NN + 2-opt seed the restatement needs 39 529 865 nodes for the proof (the limit was 300 000)."""
import json
import os

import numpy as np
import pytest

import _bnb_cases as K
import _bnb_oracle as B

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = K.small_cases()
TL_ERR_BADARG, TL_ERR_UNSUPPORTED = -1, -6


def n_of(xy, pk):
    return len(xy) if xy is not None else int(round((1 + (1 + 8 * len(pk)) ** 0.5) / 2))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "goldens_bnb.json")))


@pytest.fixture(scope="module")
def large():
    return K.large_cases()


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_equals_brute_force(case):
    name, xy, pk, start, k = case
    n = n_of(xy, pk)
    D = B.dist_matrix(xy, pk, n)
    route, length, _ = B.brute(D, start, k)
    rc, got, cost, proved, improved, st = K.call(None, xy, pk, n, start=start, K=k)
    assert rc == 0 and proved == 1 and improved == 1
    assert got == route and cost.tobytes() == length.tobytes(), (name, got, cost, route, length)
    # node for node the plain Python search
    droute, dlen, _, nodes, leaves = B.dfs(D, start, k)
    assert droute == route and (st["nodes"], st["leaves"]) == (nodes, leaves) and st["launches"] == 0


def test_both_input_forms_agree():
    xy = K.random_xy(9, 9)
    pk = B.packed_of(B.dist_matrix(xy))
    a, b = K.call(None, xy, None, 9, start=2), K.call(None, None, pk, 9, start=2)
    assert a[:5] == b[:5] and a[5]["nodes"] == b[5]["nodes"]
    # ... and the neighbour order is read from D alone
    a, b = K.call(None, xy, None, 9, K=3), K.call(None, None, pk, 9, K=3)
    assert a[:5] == b[:5]


def test_reference_instances():
    rc, route, cost, proved, _, _ = K.call(None, K.TSP5, None, 5)
    assert rc == 0 and proved == 1 and float(cost) == 4.0 and sorted(route) == list(range(5))
    import _bhk_oracle as H
    rc, route, cost, proved, _, _ = K.call(None, K.TSP8, None, 8)
    _, _, optimal, _ = H.bellman_karp(K.TSP8)
    # both are f32 sums of the same eight edges in different orders: each within 7 x 2^-24 of the real sum
    assert rc == 0 and proved == 1 and abs(float(cost) - float(optimal)) <= 2 * 7 * 2.0 ** -24 * float(optimal)


def test_start_tours():
    # integer distances: every sum is exact, so a rotation of the optimum has the optimum's length bit for bit
    pk = B.packed_of(np.rint(B.dist_matrix(K.random_xy(9, 3))).astype(np.float32))
    xy = None
    D = B.dist_matrix(None, pk, 9)
    route, length, _ = B.brute(D, 0, 0)
    # an optimal start tour comes back as given, in its own rotation
    rot = route[4:] + route[:4]
    rc, got, cost, proved, improved, _ = K.call(None, xy, pk, 9, init=rot)
    assert rc == 0 and proved == 1 and improved == 0 and got == rot
    assert cost.tobytes() == B.tour_length(D, rot).tobytes()
    assert B.brute(D, 0, 0, init=rot)[0] == rot
    # one 2-opt move away: improved, and the result is the contract's
    worse = route[:2] + route[2:6][::-1] + route[6:]
    assert B.tour_length(D, worse) > length
    rc, got, cost, proved, improved, _ = K.call(None, xy, pk, 9, init=worse)
    assert rc == 0 and proved == 1 and improved == 1 and got == route and cost.tobytes() == length.tobytes()
    # a start tour of the optimum's length that is not R: nothing is strictly shorter, so it stays
    mirror = [route[0]] + route[1:][::-1]
    assert B.tour_length(D, mirror).tobytes() == length.tobytes()
    rc, got, _, _, improved, _ = K.call(None, xy, pk, 9, init=mirror)
    assert rc == 0 and improved == 0 and got == mirror


def test_small_sizes():
    xy = K.random_xy(3, 1)
    assert K.call(None, xy, None, 0)[0] == 0
    rc, route, cost, proved, improved, _ = K.call(None, xy, None, 1)
    assert (rc, route, float(cost), proved) == (0, [0], 0.0, 1)
    rc, route, cost, proved, _, _ = K.call(None, xy, None, 2, start=1)
    assert (rc, route, proved) == (0, [1, 0], 1) and cost.tobytes() == B.tour_length(B.dist_matrix(xy[:2]), [1, 0]).tobytes()
    D = B.dist_matrix(xy)
    for start in range(3):
        rc, route, cost, proved, _, _ = K.call(None, xy, None, 3, start=start)
        want = B.brute(D, start, 0)
        assert rc == 0 and proved == 1 and route == want[0] and cost.tobytes() == want[1].tobytes()


def test_error_codes():
    xy = K.random_xy(6, 1)
    assert K.call(None, np.zeros((65, 2), np.float32), None, 65)[0] == TL_ERR_UNSUPPORTED        # n > TL_BNB_MAX_N
    assert K.call(None, xy, None, 6, start=6)[0] == TL_ERR_BADARG                                # start is no position
    assert K.call(None, xy, None, 6, init=[0, 1, 2, 3, 4, 4])[0] == TL_ERR_BADARG                # no permutation
    assert K.call(None, xy, None, 6, init=[0, 1, 2, 3, 4, 6])[0] == TL_ERR_BADARG
    assert K.call(None, None, None, 6)[0] == TL_ERR_BADARG                                       # no input
    pk = B.packed_of(B.dist_matrix(xy))
    for bad in (np.nan, -1.0, -0.0, np.float32(B.F32_MAX), np.inf):
        q = pk.copy()
        q[7] = bad
        assert K.call(None, None, q, 6)[0] == TL_ERR_UNSUPPORTED, bad
    from teeline_amd import _capi
    assert b"NaN, negative or >= f32::MAX" in _capi.load().tl_last_error(None)
    # finite distances whose every tour overflows f32
    assert K.call(None, None, np.full(6, 3e38, np.float32), 4)[0] == TL_ERR_UNSUPPORTED


def test_budget_ends_the_search_with_a_valid_tour(large):
    xy, pk, n, k, start, _ = large["rand33_27"]
    init = K.seed_tour(xy, pk, n, start)
    rc, route, cost, proved, improved, st = K.call(None, xy, pk, n, init=init, max_nodes=50)
    assert rc == 0 and proved == 0 and sorted(route) == list(range(n)) and st["nodes"] <= 50
    assert cost <= B.tour_length(B.dist_matrix(xy), list(init))
    rc, route, cost, proved, _, st = K.call(None, xy, pk, n, max_nodes=5)  # no start tour, no leaf yet
    assert rc == 0 and proved == 0 and route == list(range(n))


def test_larger_cases_equal_the_golden_file(golden, large):
    assert sorted(golden) == sorted(large)
    for name, (xy, pk, n, k, start, seeded) in large.items():
        g = golden[name]
        init = K.seed_tour(xy, pk, n, start) if seeded else None
        rc, route, cost, proved, improved, st = K.call(None, xy, pk, n, init=init, start=start, K=k)
        assert rc == 0 and proved == 1, name
        assert route == g["route"] and B.bits(cost) == g["bits"] and improved == g["improved"], name
        assert (st["nodes"], st["leaves"]) == (g["nodes"], g["leaves"]), name
        assert g["nodes"] <= (1_000_000 if name == "gr17" else 300_000), name
        assert route[0] == start and cost.tobytes() == B.tour_length(B.dist_matrix(xy, pk, n), route).tobytes()


def test_gr17_is_the_published_optimum(golden):
    # EXPLICIT: integer distances, exact sums.  Seeded with the project's own NN and 2-opt on the host; exact solver.
    assert np.uint32(golden["gr17"]["bits"]).view(np.float32) == np.float32(2085.0)


def test_the_python_search_counts_the_golden_nodes(golden, large):
    for name in ("rand20", "k3_n12", "matrix17"):
        xy, pk, n, k, start, seeded = large[name]
        init = K.seed_tour(xy, pk, n, start) if seeded else None
        route, length, improved, nodes, leaves = B.dfs(B.dist_matrix(xy, pk, n), start, k, init)
        g = golden[name]
        assert (route, B.bits(length), nodes, leaves) == (g["route"], g["bits"], g["nodes"], g["leaves"]), name


def test_plan():
    import ctypes as C
    from teeline_amd import _capi
    lib = _capi.load()
    t, w, fd, npl = C.c_int(), C.c_int(), C.c_uint32(), C.c_uint32()
    for n in (4, 20, 33, 64):
        assert lib.tl_branch_and_bound_plan(n, 256, 160 * 1024, C.byref(t), C.byref(w), C.byref(fd), C.byref(npl)) == 0
        assert t.value == 256 and w.value >= 1 and 1 <= fd.value <= n - 2 and npl.value >= 1
        assert 64 * 64 * 4 + 64 * 8 <= 160 * 1024
    assert lib.tl_branch_and_bound_plan(65, 256, 160 * 1024, None, None, None, None) == TL_ERR_UNSUPPORTED
    assert lib.tl_branch_and_bound_plan(20, 0, 160 * 1024, None, None, None, None) == TL_ERR_BADARG


def test_pipeline_names():
    import teeline_amd as TA
    P = TA.pipeline
    assert P.SOLVER_NAMES["branch_and_bound"] == "branch_and_bound" and "branch_bound" not in P.SOLVER_NAMES
    assert P.steps_for_solve("branch_and_bound") == ["nn", "branch_and_bound"]
    assert P.steps_for_solve("branch_and_bound", no_seed=True) == ["branch_and_bound"]
    with pytest.raises(ValueError, match="unknown solver `branch_bound`"):
        P.steps_for_solve("branch_bound")


def test_host_mirror_progress_and_stats():
    import teeline_amd as TA
    xy = K.random_xy(8, 8)
    ids = np.array([7, 3, 9, 1, 12, 5, 8, 2])  # the smallest id is at position 3
    prob = TA.TspProblem(ids, xy)
    msgs = []
    sol = TA.branch_and_bound.solve_host(prob, None, lambda kind, payload: msgs.append((kind, payload)))
    route, length, _ = B.brute(B.dist_matrix(xy), 3, 0)
    assert sol.route() == [int(ids[p]) for p in route] and sol.total.tobytes() == length.tobytes()
    assert [m[0] for m in msgs] == ["PathUpdate", "PathUpdate", "Done"]
    assert msgs[0][1] == (sorted(int(v) for v in ids), 0.0) and msgs[1][1][0] == sol.route()
    assert sol.stats["proved"] == 1 and sol.stats["improved"] == 1 and sol.stats["nodes"] > 0 and sol.stats["leaves"] > 0
    # a HeuristicOptions passes its n_nearest
    sol3 = TA.branch_and_bound.solve_host(prob, TA.HeuristicOptions(n_nearest=3))
    want = B.brute(B.dist_matrix(xy), 3, 3)
    assert sol3.route() == [int(ids[p]) for p in want[0]] and sol3.total.tobytes() == want[1].tobytes()
