"""The neighbour layer at its work edges (-m gpu): the matrix-form NN walk past one wave and past one 1024-stride, the kd-tree build
and walk on signed / equal-comparing / large coordinates and at the level-count edges, the brute-force lists with four and with
sixteen lanes per city at their switch, rounded-distance ties between different squares in both list builders and in the NN
fallback, and every form and host switch of the coordinate-form NN seed.  Everything is compared for EXACT equality with the oracle
or with the numpy float32 reference of tests/_neighbour_cases.py (pinned to the oracle in tests/test_neighbour_cases.py, which
also asserts that every input still holds the edge it is here for): lists element by element, routes as lists, costs as f32 bytes."""
import ctypes as C

import numpy as np
import pytest

import _neighbour_cases as N
import _oracle as O

pytestmark = pytest.mark.gpu


def prob(xy, packed=None):
    import teeline_amd as TA
    ids = np.arange(len(xy))
    dm = None if packed is None else TA.distance_matrix.DistanceMatrix(len(xy), packed, ids, "explicit")
    return TA.TspProblem(ids, xy, dm)


def nn(ctx, xy, k, packed=None):
    import teeline_amd as TA
    sol = TA.nearest_neighbor.solve(prob(xy, packed), TA.HeuristicOptions(n_nearest=k), ctx=ctx)
    return list(sol.route()), np.float32(sol.total).tobytes()


def assert_walk(got, route, cost):
    assert got[0] == route.tolist(), f"walk differs from the oracle's first at step {next(s for s, (a, b) in enumerate(zip(got[0], route.tolist())) if a != b)}"
    assert got[1] == np.float32(cost).tobytes()


@pytest.fixture(scope="module")
def brute():
    import teeline_amd as TA
    with TA.Context(0, TA.TL_FLAG_KNN_BRUTE) as c:
        yield c


def lists(ctx, xy, k):
    import teeline_amd as TA
    return TA.lin_kernighan.build_candidates(prob(xy), k, ctx=ctx)


# ------------------------------------------------------------------------------------------------ A. matrix-form NN walk
@pytest.mark.parametrize("n", N.DM_SIZES)
@pytest.mark.parametrize("kind", N.DM_KINDS)
def test_matrix_nn_walk(ctx, kind, n):
    """k_nn_seed_dm beyond 29 cities: full and partial waves (63/64/65), one full stride and its second trip (1023/1024/1025), a third
    trip (2049, 3000), sixteen waves posting to the 64-bit atomicMin and its double buffer; rows full of ties (b, c, e), negative
    values (d: the ~b branch of the sortable key), +inf (f), and -0.0 against +0.0 (e): the reference compares floats, so the two are
    equal and the lower position wins (tl_oracle.c:510-529) — a key formed from the raw bits puts every -0.0 first."""
    packed = N.dm_packed(kind, n)
    for k in N.dm_ks(n):
        assert_walk(nn(ctx, N.dm_xy(n), k, packed), *N.oracle_dm_walk(kind, n, k))


def test_lk_seeds_from_the_matrix_walk(ctx):
    """The second call site of k_nn_seed_dm (tl_lk with a matrix and no initial tour), n = 1025 on the all-ties matrix (b)."""
    import teeline_amd as TA
    n = 1025
    xy, packed = N.dm_xy(n), N.dm_packed("b", n)
    h = TA.HeuristicOptions(epochs=1, platoo_epochs=10, n_nearest=5)
    sol = TA.lin_kernighan.solve(prob(xy, packed), TA.LKOptions(h, 3), None, None, ctx=ctx, seed=1)
    rc, route, cost, st = O.lin_kernighan(xy, epochs=1, platoo_epochs=10, n_nearest=5, max_depth=3, seed=1, packed=packed)
    assert rc == 0 and list(sol.route()) == route.tolist()
    assert np.float32(sol.total).tobytes() == np.float32(cost).tobytes()
    assert tuple(sol.stats[f] for f in ("sweeps", "candidates", "moves", "reversed")) == tuple(st[f] for f in ("sweeps", "candidates", "moves", "reversed"))


# ------------------------------------------------------------------------------------------------ B. kd-tree lists
def assert_kd_lists(ctx, xy, k):
    got = lists(ctx, xy, k)
    want, _ = O.build_candidates_kdtree(xy, k)  # tie_free may be 0 here: the shared (value, position) rule is the specification
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, f"k={k}: {len(bad)} lists differ, first city {bad[0]}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}"


@pytest.mark.parametrize("n", N.KD_SIZES)
def test_kd_lists_at_the_level_and_block_edges(ctx, n):
    """Trees of 2..9 cities and around 2^8 and 2^10 (levels = the smallest h with 2^h > n, the root at n / 2, 256-lane blocks whose
    tail lanes return early), list lengths on both sides of every k-buffer size (clamped to n - 1 by the library), coordinates in
    all four sign quadrants."""
    for k in N.KD_KS:
        assert_kd_lists(ctx, N.kd_shifted(n), k)


@pytest.mark.parametrize("case", ["signed_zeros", "equal_families", "large_magnitude", "tie_rings"])
def test_kd_lists_on_coordinates_that_stress_the_order(ctx, case):
    """signed_zeros: -0.0 and +0.0 order by position (k_kd_keys canonicalises); equal_families: cmp_coord is Equal for different bit
    patterns, where the walk goes (right, left); large_magnitude: the relative tolerance at 1e6; tie_rings: two squares, one rounded
    distance, inside the list and across its end."""
    if case == "signed_zeros":
        for k in (5, 8):
            assert_kd_lists(ctx, N.kd_signed_zeros(), k)
    elif case == "equal_families":
        for k in (5, 8):
            assert_kd_lists(ctx, N.kd_equal_families(), k)
    elif case == "large_magnitude":
        assert_kd_lists(ctx, N.kd_large_magnitude(), 5)
    else:
        for n, kr in N.RING_KD:
            for k in (5, 8):
                assert_kd_lists(ctx, N.tie_rings(n, kr)[0], k)


# ------------------------------------------------------------------------------------------------ C. brute-force lists
@pytest.mark.parametrize("n,k", [(32769, 3), (32769, 5), (32769, 9), (32769, 17), (32769, 33), (32768, 5)])
def test_brute_lists_at_the_lane_switch(brute, n, k):
    """n = 32 769: four lanes per city, one k per KMAX bucket (k_knn_quad<4|8|16|32|64, 4>); n = 32 768: the sixteen-lane form at its
    upper edge.  1024 sampled rows (0..63, the last 130 with the tail block, a random rest) against the numpy reference."""
    xy, rows, want = N.knn_sampled_reference(n, 3)
    got = lists(brute, xy, k)
    assert got.shape == (n, k)
    bad = np.flatnonzero((got[rows] != want[:, :k]).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} sampled lists differ, first city {rows[bad[0]]}: {got[rows[bad[0]]].tolist()} != {want[bad[0], :k].tolist()}"


@pytest.mark.parametrize("n", [17, 255, 257, 4097])
def test_brute_lists_small_tails_and_rounding_ties(brute, n):
    """The sixteen-lane form's last block (n mod 16 = 1, 15, 1, 1) on the rounding-tie rings — the refusal d < radius, the rlim filter
    on squares and the merge on (rounded distance, position) all meet the same pair — and on a lattice with duplicates."""
    for k in (4, 7, 16):
        for xy in (N.tie_rings(n, k)[0], N.duplicated_lattice(n)):
            got = lists(brute, xy, k)
            want = O.build_candidates(xy, k)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert len(bad) == 0, f"k={k}: {len(bad)} lists differ, first city {bad[0]}: {got[bad[0]].tolist()} != {want[bad[0]].tolist()}"


# ------------------------------------------------------------------------------------------------ E. coordinate-form NN seed
@pytest.mark.parametrize("n,k", [(4096, 3), (4097, 3), (8191, 3), (8192, 3), (8193, 3), (12288, 3), (12289, 3), (16384, 3), (16385, 3), (20000, 2)])
def test_nn_seed_forms_and_host_switches(ctx, n, k):
    """Cities per thread held in registers for the fallback scans: NQ = 4 up to 4096, 8 up to 8192 (first run here), 12, 16 up to
    16 384, then the loop form; the internal list length goes from 4 to 7 at n = 8192 (and down again with what fits the LDS: 6 at
    12 289, the caller's 3 at 16 384); n = 16 385 and n = 20 000 with k = 2 run k_nn_seed<LDS_CAND = true, LDS_XY = false, NQ = 0>."""
    assert_walk(nn(ctx, O.synth_xy(n, seed=n), k), *N.oracle_xy_walk(n, n, k))


@pytest.mark.parametrize("n", [300, 16385])
def test_nn_seed_with_an_empty_frontier(ctx, n):
    """n_nearest = 0: the reference's frontier is empty and every step is the global scan (nearest_neighbor.rs:50-63).  The Python
    mirror validates like HeuristicOptions (n_nearest >= 1), so this goes through the C entry: it serves 0 — with lists of its own up
    to 16 384 cities (the walk does not depend on their length), and as a whole-workgroup fallback scan per step above."""
    xy = O.synth_xy(n, seed=40 + n)
    out = np.empty(n, dtype=np.uint32)
    cost = C.c_float()
    ctx.check(ctx.lib.tl_nearest_neighbor(ctx.handle, xy.ctypes.data_as(C.c_void_p), None, n, 0, out.ctypes.data_as(C.c_void_p), C.byref(cost)))
    rc, route, want = O.nearest_neighbor(xy, None, n, 0)
    assert rc == 0
    assert_walk((out.tolist(), np.float32(cost.value).tobytes()), route, want)


@pytest.mark.parametrize("seed", range(12))
def test_nn_fallback_decided_by_a_rounding_tie(ctx, seed):
    """Register form: the scan's first pass finds the smallest SQUARE, the answer is the lowest position at the smallest ROUNDED
    distance — here a city with a larger square (tests/test_neighbour_cases.py asserts that of every instance)."""
    xy = N.fallback_instance(seed)
    rc, route, cost = O.nearest_neighbor(xy, None, len(xy), 3)
    assert rc == 0 and N.fallback_counter(xy, route, 6)
    assert_walk(nn(ctx, xy, 3), route, cost)


def test_nn_fallback_decided_by_a_rounding_tie_in_the_loop_form(ctx):
    xy = N.fallback_instance(0, N.LOOP_AXIS)
    rc, route, cost = O.nearest_neighbor(xy, None, len(xy), 3)
    assert rc == 0 and N.fallback_counter(xy, route, N.LOOP_AXIS)
    assert_walk(nn(ctx, xy, 3), route, cost)
