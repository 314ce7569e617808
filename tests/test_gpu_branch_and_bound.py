"""The branch and bound on the GPU (-m gpu): tl_branch_and_bound against brute force on the small instances and against the
sequential restatement (tests/golden/goldens_bnb.json, written on the CPU) on the larger ones — routes element for element, lengths
bit for bit, every case proved; the same result under every launch parameter; a budget that ends the search."""
import json
import os

import numpy as np
import pytest

import _bnb_cases as K
import _bnb_oracle as B
from test_bnb_oracle import SMALL, n_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "goldens_bnb.json")))


@pytest.fixture(scope="module")
def large():
    return K.large_cases()


def run_golden(ctx, large, golden, name, **knobs):
    xy, pk, n, k, start, seeded = large[name]
    g = golden[name]
    init = K.seed_tour(xy, pk, n, start) if seeded else None
    rc, route, cost, proved, improved, st = K.call(ctx, xy, pk, n, init=init, start=start, K=k, **knobs)
    assert rc == 0 and proved == 1, (name, knobs, rc, proved, st)
    assert route == g["route"] and B.bits(cost) == g["bits"] and improved == g["improved"], (name, knobs, route, cost)
    assert st["launches"] >= 1 and st["nodes"] > 0 and st["kernel_ms"] > 0 and st["wave_launches"] >= st["idle_wave_launches"], (name, st)
    return st


def test_equals_brute_force_on_the_small_instances(ctx):
    for name, xy, pk, start, k in SMALL:
        n = n_of(xy, pk)
        route, length, _ = B.brute(B.dist_matrix(xy, pk, n), start, k)
        rc, got, cost, proved, improved, st = K.call(ctx, xy, pk, n, start=start, K=k)
        assert rc == 0 and proved == 1 and improved == 1, name
        assert got == route and cost.tobytes() == length.tobytes(), (name, got, cost, route, length)


def test_two_and_three_cities(ctx):
    xy = K.random_xy(3, 1)
    for n in (2, 3):
        for start in range(n):
            got, want = K.call(ctx, xy, None, n, start=start), K.call(None, xy, None, n, start=start)
            assert got[0] == 0 and got[:5] == want[:5] and got[3] == 1


@pytest.mark.parametrize("name", ["rand33_4", "rand33_20", "rand33_27", "rand33_28", "rand33_34", "circle64", "matrix17", "k3_n12"])
def test_equals_the_restatement(ctx, large, golden, name):
    run_golden(ctx, large, golden, name)


def test_n26_equals_the_restatement_and_bellman_karp(ctx, large, golden):
    import ctypes as C
    run_golden(ctx, large, golden, "int26")
    xy, pk, n, *_ = large["int26"]
    out = np.empty(n, dtype=np.uint32)
    cost, optimal, ok = C.c_float(), C.c_float(), C.c_uint32()
    ctx.check(ctx.lib.tl_bellman_karp(ctx.handle, None, pk.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), C.byref(cost),
                                      C.byref(optimal), C.byref(ok), None))
    # integer distances: every sum is exact, so the DP's optimum is the length of the branch and bound's tour
    assert B.bits(optimal.value) == golden["int26"]["bits"]


def test_start_tour_that_is_optimal_comes_back(ctx, large, golden):
    xy, pk, n, *_ = large["int26"]  # integer distances: a rotation of the optimum has its length bit for bit
    opt = golden["int26"]["route"]
    rot = opt[7:] + opt[:7]
    rc, route, cost, proved, improved, _ = K.call(ctx, xy, pk, n, init=rot)
    assert rc == 0 and proved == 1 and improved == 0 and route == rot and B.bits(cost) == golden["int26"]["bits"]


KNOBS = ([dict(nodes_per_launch=v) for v in (1, 7, 0)] + [dict(frontier_depth=v) for v in (1, 2, 4)] + [dict(workgroups=v) for v in (1, 3, 0)]
         + [dict(workgroups=1, frontier_depth=4), dict(nodes_per_launch=7, frontier_depth=1, workgroups=3)])


@pytest.mark.parametrize("knobs", KNOBS, ids=[",".join(f"{k}={v}" for k, v in d.items()) for d in KNOBS])
def test_independent_of_the_knobs(ctx, large, golden, knobs):
    st = run_golden(ctx, large, golden, "rand20", **knobs)
    if knobs.get("nodes_per_launch") == 1:
        assert st["launches"] > 1  # every node crosses a save and a restore
    if knobs.get("workgroups") == 1 and knobs.get("frontier_depth") == 4:
        assert st["queue_start"] > 4  # one workgroup drains a queue longer than its waves


def test_frontier_of_depth_one_is_split_at_launch_boundaries(ctx, large, golden):
    st = run_golden(ctx, large, golden, "rand33_27", frontier_depth=1, nodes_per_launch=64)
    assert st["queue_end"] > st["queue_start"], st


def test_budget_ends_the_search(ctx, large):
    xy, pk, n, k, start, _ = large["rand33_27"]
    init = K.seed_tour(xy, pk, n, start)
    rc, route, cost, proved, improved, st = K.call(ctx, xy, pk, n, init=init, max_nodes=50)
    assert rc == 0 and proved == 0 and sorted(route) == list(range(n)), (rc, proved, st)
    assert cost <= B.tour_length(B.dist_matrix(xy), list(init))
    assert cost.tobytes() == B.tour_length(B.dist_matrix(xy), route).tobytes()


def test_limits_before_anything_is_allocated(ctx):
    assert K.call(ctx, np.zeros((65, 2), np.float32), None, 65)[0] == -6
    assert b"TL_BNB_MAX_N" in ctx.lib.tl_last_error(ctx.handle)
    assert K.call(ctx, K.random_xy(6, 1), None, 6, init=[0, 1, 2, 3, 4, 4])[0] == -1
