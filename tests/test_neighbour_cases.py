"""The inputs of tests/_neighbour_cases.py against the oracle and numpy alone (no GPU): every input family still produces the edge it
was built for — asserted from a counter, not merely aimed at — so a builder that silently stops producing it fails here, on the CPU,
and tests/test_gpu_neighbour_layer.py cannot go green on inputs that no longer decide anything."""
import numpy as np
import pytest

import _neighbour_cases as N
import _oracle as O


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("n", N.DM_SIZES)
@pytest.mark.parametrize("kind", N.DM_KINDS)
def test_matrix_walks_follow_the_float_compare_rule_and_ties_decide(kind, n):
    packed = N.dm_packed(kind, n)
    assert packed.shape == (n * (n - 1) // 2,) and not np.isnan(packed).any()
    for k in N.dm_ks(n):
        c = N.dm_walk_counters(packed, n, N.oracle_dm_walk(kind, n, k)[0])
        print(kind, n, k, c)
        # the walk does not depend on the list length: (distance, position) order with float compares, tl_oracle.c:510-529
        assert c["follows_rule"]
        if kind in "bce":
            assert c["tie_steps"] >= n / 2
        if kind == "e":
            assert c["mixed_zero_steps"] >= 10
            assert c["plus_wins_steps"] >= 10  # steps on which a key that orders -0.0 below +0.0 goes elsewhere
    if kind == "c":
        assert 0.08 < (packed == 0).mean() < 0.12 and not np.signbit(packed).any()
    if kind == "d":
        assert (packed < 0).any() and (packed > 0).any() and (packed != np.rint(packed)).any() and (packed == np.rint(packed)).any()
    if kind == "e":
        assert np.array_equal(packed, N.dm_packed("c", n))  # == : only signs of zeros differ
        assert N.rows_with_plus_zero_before_minus_zero(packed, n) >= 50
    if kind == "f":
        assert 0.005 < np.isinf(packed).mean() < 0.015


# ------------------------------------------------------------------------------------------------ D
RING_TABLE = N.RING_BRUTE + N.RING_KD


def test_the_annulus_gives_rounding_ties():
    pairs = N.tie_pairs()
    assert len(pairs) >= 60  # about 100 of 4000 random offsets
    for big, small in pairs:
        sb, ss = big[0] * big[0] + big[1] * big[1], small[0] * small[0] + small[1] * small[1]
        assert sb > ss and np.sqrt(sb) == np.sqrt(ss) and sb.dtype == np.float32
        assert 4096 <= np.sqrt(ss) < 4104


@pytest.mark.parametrize("n,k", RING_TABLE)
def test_rings_put_a_rounding_tie_into_the_lists(n, k):
    """The thresholds (20 hubs with the pair adjacent among the first k+1 neighbours, 5 with it across the k-th place) hold
    wherever n leaves room for 20 rings of k+1 satellites; a smaller instance must show the tie on every hub it has, and the pair
    across the k-th place on every second hub once a ring can hold k+1 satellites at all (n >= k + 2)."""
    xy, hubs = N.tie_rings(n, k)
    c = N.ring_counters(xy, hubs, k)
    print(n, k, c)
    assert c["hubs"] == max(1, n // (min(k + 1, n - 1) + 1))
    assert c["adjacent"] == c["hubs"]
    assert c["straddling"] >= ((c["hubs"] + 1) // 2 if n >= k + 2 else 0)
    if n >= 20 * (k + 2):
        assert c["adjacent"] >= 20 and c["straddling"] >= 5
    d = np.sqrt(((xy[hubs][:, None, :] - xy[hubs][None, :, :]).astype(np.float64) ** 2).sum(-1))
    assert len(hubs) == 1 or d[d > 0].min() >= 1e5


def test_ring_thresholds_are_met_by_every_instance_with_room():
    assert sum(1 for n, k in RING_TABLE if n >= 20 * (k + 2)) >= 7


# ------------------------------------------------------------------------------------------------ B
def test_kd_clouds_hold_what_they_are_for():
    for n in N.KD_SIZES:
        xy = N.kd_shifted(n)
        if n >= 255:
            quadrants = {(bool(x < 0), bool(y < 0)) for x, y in xy}
            assert len(quadrants) == 4
    assert (N.kd_shifted(2) < 0).any()
    z = N.signed_zero_counts(N.kd_signed_zeros())
    print(z)
    assert z["plus_x"] + z["minus_x"] == 200 and z["plus_y"] + z["minus_y"] == 200
    assert min(z["plus_x"], z["minus_x"], z["plus_y"], z["minus_y"]) >= 60 and min(z["negative"], z["positive"]) >= 300
    xy = N.kd_equal_families()
    ex, ey = N.equal_but_different_pairs(xy[:, 0]), N.equal_but_different_pairs(xy[:, 1])
    print("equal-comparing pairs with different bits:", ex, ey)
    assert xy.shape == (800, 2) and ex >= 200 and ey >= 200
    assert {1.0, 1000.0, 1e6} <= set(np.abs(xy).ravel().tolist())
    big = N.kd_large_magnitude()
    assert big.shape == (1000, 2) and big[:, 0].min() >= 1e6 and big[:, 1].max() <= -1e6 + 1000
    # the oracle's tree is the specification on all of them (tie_free may be 0): it must at least run and return real lists
    for xy, k in ((N.kd_signed_zeros(), 5), (N.kd_equal_families(), 8), (big, 5)):
        lists, _ = O.build_candidates_kdtree(xy, k)
        assert lists.shape == (len(xy), k) and lists.max() < len(xy) and (lists != np.arange(len(xy))[:, None]).all()


def test_cmp_coord_restates_the_oracle():
    # kdtree.rs:301-317 through the one place the oracle exposes it: tie_free of a two-city tree is 0 iff the two x values compare Equal
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(np.inf)), np.nextafter(one, np.float32(-np.inf))
    for a, b in ((one, up), (one, down), (up, down), (np.float32(1000), np.nextafter(np.float32(1000), np.float32(np.inf))),
                 (np.float32(1e6), np.float32(1e6 + 0.125)), (np.float32(-0.0), np.float32(0.0)), (np.float32(-2.0), np.float32(3.0))):
        xy = np.array([[a, 0], [b, 1]], dtype=np.float32)
        _, tie_free = O.build_candidates_kdtree(xy, 1)
        assert (N.cmp_coord(a, b) == 0) == (not tie_free), (a, b)
    assert N.cmp_coord(one, up) == 0 and N.cmp_coord(up, down) != 0  # Equal is not transitive


# ------------------------------------------------------------------------------------------------ C
def test_numpy_list_reference_is_the_oracles_scan():
    xy = O.synth_xy(2000, seed=17)
    rows = N.sample_rows(2000)
    assert set(range(64)) <= set(rows.tolist()) and set(range(2000 - 130, 2000)) <= set(rows.tolist()) and len(rows) == 1024
    want = O.build_candidates(xy, N.KNN_KMAX)
    assert np.array_equal(N.knn_rows_numpy(xy, rows, N.KNN_KMAX), want[rows])
    for xy, k in ((N.tie_rings(257, 7)[0], 7), (N.duplicated_lattice(255), 16)):  # and on ties: (distance, position), lowest first
        assert np.array_equal(N.knn_rows_numpy(xy, np.arange(len(xy)), k), O.build_candidates(xy, k))
    rows = N.sample_rows(32769)
    assert len(rows) == 1024 and set(range(64)) <= set(rows.tolist()) and set(range(32769 - 130, 32769)) <= set(rows.tolist())


def test_duplicated_lattice_has_duplicates():
    for n in (17, 255, 257, 4097):
        xy = N.duplicated_lattice(n)
        assert xy.shape == (n, 2) and len(np.unique(xy, axis=0)) == n - n // 3


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("seed", range(12))
def test_fallback_step_is_decided_by_a_rounding_tie(seed):
    xy = N.fallback_instance(seed)
    rc, route, _ = O.nearest_neighbor(xy, None, len(xy), 3)
    assert rc == 0 and N.fallback_counter(xy, route, 6)


def test_fallback_step_in_the_loop_form_is_decided_by_a_rounding_tie():
    xy = N.fallback_instance(0, N.LOOP_AXIS)
    assert len(xy) > 16384
    rc, route, _ = O.nearest_neighbor(xy, None, len(xy), 3)
    assert rc == 0 and N.fallback_counter(xy, route, N.LOOP_AXIS)
