"""The distance layer's plain restatements (tests/_dm_reference.py) against the C oracle, on the CPU.

tests/test_gpu_distance_layer.py checks the HIP kernels against both; this file shows that the numpy restatement and the oracle
are the same function first (EUC_2D packed / full layout, the sequential tour sum) and that the GEO oracle's host libm agrees with
correctly rounded trig on the inputs where the floor is most sensitive."""
import math

import numpy as np
import pytest

import _dm_reference as R
import _oracle as O


def inputs(n):
    return {"random": O.synth_xy(n, seed=n), "decimal": R.decimal_grid_xy(n, n), "degenerate": R.degenerate_xy(n, n)}


@pytest.mark.parametrize("n", [2, 3, 5, 9, 64, 257, 1025])
def test_euc_packed_full_and_rows_equal_the_oracle(n):
    for name, xy in inputs(n).items():
        packed = O.dm_build_packed(xy)
        ref = R.euc_packed(xy)
        R.assert_bits_equal(ref, packed, f"{name} n={n} packed")
        for i in sorted({1, n // 2, n - 1}):
            R.assert_bits_equal(R.euc_row(xy, i), packed[R.row_offset(i):R.row_offset(i) + i], f"{name} n={n} row {i}")
        full = R.full_from_packed(packed, n)
        R.assert_bits_equal(full, O.dm_expand_full(packed, n), f"{name} n={n} full")
        assert not np.signbit(np.diagonal(full)).any() and not np.diagonal(full).any()


def test_degenerate_inputs_reach_every_special_value():
    # the degenerate set is only worth running if it produces what it claims to: +0.0 (never -0.0) for duplicates and +-0.0
    # coordinates, subnormal and underflowed squares, inf, NaN
    xy = R.degenerate_xy(300, 7)
    d = R.euc_packed(xy)
    assert np.isnan(d).any() and np.isposinf(d).any()
    assert not (np.signbit(d) & (d == 0)).any()
    assert R.euc_dist(xy[30], xy[29]).view(np.uint32) == 0  # kinds[0] at k = 30: duplicate of point 29
    assert R.euc_dist(xy[3], xy[6]).view(np.uint32) == 0    # (0, -0) vs (-0, 0)
    dx = np.float32(xy[9][0] - xy[12][0])                   # kinds[3] vs kinds[4]
    assert 0 < dx * dx < np.finfo(np.float32).tiny
    assert np.float32(xy[12][0]) ** 2 == 0
    assert np.isposinf(R.euc_dist(xy[15], xy[3])) and np.isposinf(R.euc_dist(xy[18], xy[3]))
    assert R.euc_dist(xy[15], xy[3]) == R.euc_dist(xy[3], xy[15])


@pytest.mark.parametrize("n", [2, 3, 17, 1023, 1024, 1025, 2049])
def test_sequential_tour_sum_equals_the_oracle(n):
    rng = np.random.default_rng(n)
    # coordinates over many scales: a different summation order would change the low bits
    xy = (rng.random((n, 2)) * 10.0 ** rng.integers(-3, 5, (n, 1))).astype(np.float32)
    packed = O.dm_build_packed(xy)
    perms = [O.restart_perm(n, 1, 0), np.arange(n, dtype=np.uint32), rng.integers(0, n, n).astype(np.uint32)]  # repeats allowed
    for perm in perms:
        want = O.tour_length(xy, None, perm)
        assert R.tour_length(perm, xy=xy).tobytes() == want.tobytes()
        assert R.tour_length(perm, packed=packed).tobytes() == want.tobytes()
        assert O.tour_length(None, packed, perm).tobytes() == want.tobytes()
    for bad in (np.nan, np.inf):
        p2 = packed.copy()
        p2[len(p2) // 2] = bad
        perm = np.arange(n, dtype=np.uint32)
        assert R.bits_equal(R.tour_length(perm, packed=p2), O.tour_length(None, p2, perm))


def test_sequential_sum_is_not_the_pairwise_sum():
    # the restatement must be order-sensitive where the kernel is: np.sum (pairwise) gives other bits on this tour
    n = 2049
    rng = np.random.default_rng(1)
    xy = (rng.random((n, 2)) * 10.0 ** rng.integers(-3, 5, (n, 1))).astype(np.float32)
    perm = O.restart_perm(n, 1, 0)
    e = R.tour_edges(perm, xy=xy)
    assert R.tour_length(perm, xy=xy).tobytes() != np.sum(e, dtype=np.float32).tobytes()


def test_packed_index_helpers():
    for k in (0, 1, 2, 3, 4, 5, 6, 10**6, 2**31 - 1, 2**31, 2151677200 - 1):
        i, j = R.packed_ij(k)
        assert 0 <= j < i and R.row_offset(i) + j == k
    assert R.row_offset(65601) == 65601 * 65600 // 2 and R.row_offset(65601) > 2**31


def test_geo_oracle_equals_the_host_restatement_on_the_grid():
    rng = np.random.default_rng(11)
    xy = np.concatenate([R.tsplib_grid(rng, 200),
                         np.array([[90.0, 180.0], [-90.0, -180.0], [0.0, 0.0], [-0.3, 179.59], [45.75, -120.99]], np.float32)])
    n = len(xy)
    packed = O.dm_build_packed(xy, geo=True)
    ref = np.empty_like(packed)
    for i in range(1, n):
        for j in range(i):
            ref[R.row_offset(i) + j] = R.geo_host(xy[i], xy[j])[1]
    R.assert_bits_equal(ref, packed, "geo host restatement", R.describe_geo_packed(xy, ref, packed))


def test_geo_near_ties_host_libm_is_correctly_rounded_where_it_matters():
    p, q, gap = R.near_tie_pairs()
    assert len(p) == 2000 and np.all(np.diff(gap) >= 0)
    # deterministic: the same pairs every run
    p2, q2, _ = R.near_tie_pairs()
    assert np.array_equal(p, p2) and np.array_equal(q, q2)
    # the nearest ties lie far above the f64 error scale (~1e-12 here): floor cannot tell the trig implementations apart
    assert 1e-9 < float(gap[0]) < 1e-5, float(gap[0])
    xy = np.empty((2 * len(p), 2), np.float32)
    xy[1::2], xy[0::2] = p, q  # pair k is packed entry (2k+1, 2k)
    packed = O.dm_build_packed(xy, geo=True)
    worst = 0.0
    for k in range(len(p)):
        want = packed[R.row_offset(2 * k + 1) + 2 * k]
        v_mp, r_mp = R.geo_mp(p[k], q[k])
        v_host, r_host = R.geo_host(p[k], q[k])
        assert r_host.tobytes() == want.tobytes(), (k, p[k], q[k], v_host)
        assert r_mp.tobytes() == want.tobytes(), (k, p[k], q[k], v_mp, v_host)
        worst = max(worst, abs(v_mp - v_host))
        assert abs(v_mp - math.floor(v_mp) - 0.5) < 0.5 - 1e-9  # the f64 value itself is no tie either
    assert worst < 1e-8, worst
