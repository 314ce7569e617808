"""CPU tests of the savings restatement tests/_savings_oracle.py (savings.rs:34-163 over graph.rs:98-196): the reference's recorded
number, the hub / cost / -> 2-opt table of three TSPLIB instances, the chunked walk against the literal one, the tie rule, the NaN
rule, the operation order, the shape of tests/golden/goldens_savings.json — and tl_savings_hub (host code of the library, no GPU)
against the numpy hub.  The -m gpu tests hold tl_savings to this oracle."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _oracle as O
import _savings_oracle as S
import _tsplib as T

HERE = os.path.dirname(os.path.abspath(__file__))


def tsp(name):
    return T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))


@pytest.mark.parametrize("name,hub,cost,cost2", [("berlin52", 36, "8378.97363", "8040.27637"), ("a280", 149, "2882.62842", "2799.27539"),
                                                 ("att532", 312, "95440.24219", "92493.13281")])
def test_table_hub_cost_and_two_opt(name, hub, cost, cost2):
    e = tsp(name)
    r, c, h = S.savings(e["xy"], chunk=4096)
    assert h == hub and f"{float(c):.5f}" == cost
    assert sorted(r.tolist()) == list(range(e["n"])) and c.tobytes() == O.tour_length(e["xy"], None, r).tobytes()
    rc, r2, c2, _ = O.two_opt(e["xy"], None, e["n"], init=r)
    assert rc == 0 and f"{float(c2):.5f}" == cost2


def test_berlin52_is_the_references_recorded_number():
    e = tsp("berlin52")
    r, c, h, st = S.savings(e["xy"], with_stats=True)
    assert round(float(c)) == 8379 and float(c) <= 9200.0  # tests/savings_test.rs:66-83: "measured ~8379", ceiling 9200
    assert st["examined"] == 1314                          # of 1326: hub pairs have savings +0.0 and sort last


def test_key_order():
    vals = np.frombuffer(np.array([0x7F800000, 0x3F800000, 0x00000001, 0x00000000, 0x80000000, 0x80000001, 0xBF800000, 0xFF800000],
                                  dtype=np.uint32).tobytes(), dtype=np.float32)  # inf 1 subnormal +0 -0 -subnormal -1 -inf: descending
    k = S.savings_key32(vals)
    assert np.all(k[:-1] < k[1:]) and k[-1] == 0xFF800000
    nans = np.frombuffer(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).tobytes(), dtype=np.float32)
    assert S.savings_key32(nans).tolist() == [int(S.NAN_KEY)] * 4 and S.NAN_KEY > k[-1]
    raw = S.savings_key32(nans, nan_rule=False)  # total_cmp alone: +NaN first, -NaN last
    assert raw[0] < k[0] and raw[1] > k[-1]


def test_hub_pairs_have_zero_savings_and_small_n():
    xy = np.asarray([[0, 0], [5, 0], [10, 0]], dtype=np.float32)
    pk = O.dm_build_packed(xy)
    keys = S.sorted_savings_keys(pk, 3, 0)
    assert len(keys) == 3 and np.all(keys[:-1] < keys[1:])
    i, j = (keys >> np.uint64(16)) & np.uint64(0xFFFF), keys & np.uint64(0xFFFF)
    assert list(zip(i.tolist(), j.tolist())) == [(1, 2), (0, 1), (0, 2)]  # s = 10, then the two hub pairs (+0.0) in (i, j) order
    assert (keys[1] >> np.uint64(32)) == (keys[2] >> np.uint64(32)) == int(S.savings_key32(np.zeros(1, np.float32))[0])
    r, c, h = S.savings(xy[:2])
    assert r.tolist() == [0, 1] and c == np.float32(10.0) and h == 0
    r, c, h = S.savings(xy[:1])
    assert r.tolist() == [0] and c == np.float32(0.0) and h == 0
    r, c, h = S.savings(xy)
    assert sorted(r.tolist()) == [0, 1, 2] and h == 1
    assert S.hub_distances(pk, 3, 1).tolist() == [5.0, 0.0, 5.0]


@pytest.mark.parametrize("n,kind", [(200, "random"), (400, "lattice"), (600, "dups"), (1000, "random")])
def test_chunked_walk_equals_the_literal_walk(n, kind):
    rng = np.random.default_rng(n)
    if kind == "random":
        xy = O.synth_xy(n, seed=n)
    elif kind == "lattice":
        xy = np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(np.float32)
    else:
        xy = np.repeat(rng.random((n // 20, 2)).astype(np.float32), 20, axis=0)
    keys = S.sorted_savings_keys(O.dm_build_packed(xy), n, S.hub_position(xy))
    lit = S.select_edges(n, keys)
    assert lit[1] > 0.9 * len(keys)  # nearly every key is examined: the chunked walk is a necessity here
    for chunk in (7, 256, 4096):
        assert S.select_edges(n, keys, chunk=chunk) == lit


def test_tie_rule_matters_on_a_lattice():
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(np.float32)
    r, c, h = S.savings(g)
    r2, c2, h2 = S.savings(g, tie="ji")
    assert h == h2 and sorted(r2.tolist()) == list(range(400)) and r.tolist() != r2.tolist()


def test_operation_order_matters():
    e = tsp("att532")
    r, c, h = S.savings(e["xy"])
    keys = S.sorted_savings_keys(O.dm_build_packed(e["xy"]), 532, h)
    keys2 = S.sorted_savings_keys(O.dm_build_packed(e["xy"]), 532, h, order="diff_first")
    assert not np.array_equal(keys, keys2)  # dh[i] + (dh[j] - d) rounds differently


def inf_matrix(n, seed):
    rng = np.random.default_rng(seed)
    m = n * (n - 1) // 2
    pk = rng.integers(1, 30, m).astype(np.float32)
    pk[rng.permutation(m)[:m // 4]] = np.float32(np.inf)
    return pk


def test_nan_rule_on_a_matrix_with_inf_entries():
    n = 24
    pk = inf_matrix(n, 5)
    dh = S.hub_distances(pk, n, 0)
    assert np.isinf(dh).any()
    with np.errstate(all="ignore"):
        s = np.concatenate([(dh[:j] + dh[j]) - pk[j * (j - 1) // 2: j * (j - 1) // 2 + j] for j in range(1, n)])
    assert np.isnan(s).any() and np.isneginf(s).any() and np.isposinf(s).any()
    keys = S.sorted_savings_keys(pk, n, 0)
    k32 = (keys >> np.uint64(32)).astype(np.uint32)
    nn = int(np.isnan(s).sum())
    assert np.all(k32[-nn:] == S.NAN_KEY) and np.all(k32[:-nn] < S.NAN_KEY)  # every NaN after every number, -inf included
    low = keys[-nn:] & np.uint64(0xFFFFFFFF)
    assert np.all(low[:-1] < low[1:])                                          # ... in (i, j) order
    # the sign of the NaN must not matter: flip it in the savings and the keys stay
    assert np.array_equal(S.savings_key32(s), S.savings_key32(np.where(np.isnan(s), -s, s)))
    # and the rule decides tours: total_cmp alone with this platform's NaN, or with the other sign, gives other routes
    xy = np.zeros((n, 2), dtype=np.float32)
    r, c, h = S.savings(xy, pk, n, hub=0)
    assert sorted(r.tolist()) == list(range(n))
    differs = 0
    for seed in range(8):
        pk2 = inf_matrix(n, 100 + seed)
        a = S.savings(xy, pk2, n, hub=0)[0].tolist()
        with np.errstate(all="ignore"):
            keys_pos = S.sorted_savings_keys(pk2, n, 0, nan_rule=False)
        k32 = (keys_pos >> np.uint64(32)).astype(np.uint32)
        # force every NaN to +NaN (AArch64 / gfx950 default): it sorts FIRST under total_cmp descending
        neg = k32 > np.uint32(0xFF800000)
        keys_pos = np.sort(np.where(neg, (np.uint64(0x003FFFFF) << np.uint64(32)) | (keys_pos & np.uint64(0xFFFFFFFF)), keys_pos))
        edges, _ = S.select_edges(n, keys_pos)
        differs += S.cycle_to_path(n, edges) != a
    assert differs > 0


def test_golden_file_shape():
    with open(os.path.join(HERE, "golden", "goldens_savings.json")) as fh:
        g = json.load(fh)
    assert set(g) == {"synthetic10000", "synthetic13509"}
    for k, e in g.items():
        assert e["n"] == int(k[len("synthetic"):]) and len(e["route_sha256"]) == 64 and 0 <= e["hub"] < e["n"]
        assert e["hub"] == S.hub_position(O.synth_xy(e["n"]))
        assert f"{float(np.uint32(e['cost_bits']).view(np.float32)):.5f}" == e["cost"]
        assert 0 < e["reference_examined"] <= e["n"] * (e["n"] - 1) // 2


# ---- tl_savings_hub: host code of the library, needs no context and no GPU ----

@pytest.fixture(scope="module")
def lib():
    from teeline_amd import build
    build.build()
    from teeline_amd import _capi
    return _capi.load()


def c_hub(lib, xy):
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    h = C.c_uint32(0xDEADBEEF)
    assert lib.tl_savings_hub(xy.ctypes.data_as(C.c_void_p), len(xy), C.byref(h)) == 0
    return h.value


def test_hub_small_n_ties_and_non_finite(lib):
    assert c_hub(lib, [[3, 4]]) == 0 == S.hub_position([[3, 4]])
    assert c_hub(lib, [[0, 0], [2, 0]]) == 0 == S.hub_position([[0, 0], [2, 0]])           # equal d2: the first wins
    assert c_hub(lib, [[0, 0], [2, 0], [1.5, 0]]) == 2 == S.hub_position([[0, 0], [2, 0], [1.5, 0]])
    sq = [[1, 1], [-1, 1], [-1, -1], [1, -1]]
    assert c_hub(lib, sq) == 0 == S.hub_position(sq)
    assert c_hub(lib, sq[::-1] + [[0, 0]]) == 4
    for bad in (np.nan, np.inf, -np.inf):
        xy = np.asarray([[5, 5], [0, 0], [1, 1], [2, 2]], dtype=np.float32)
        xy[2, 1] = bad
        assert c_hub(lib, xy) == 0 == S.hub_position(xy)
    big = np.full((4, 2), 3e38, dtype=np.float32)  # the sums overflow to inf
    assert c_hub(lib, big) == 0 == S.hub_position(big)
    h = C.c_uint32(7)
    assert lib.tl_savings_hub(None, 0, C.byref(h)) == 0 and h.value == 0
    assert lib.tl_savings_hub(None, 3, C.byref(h)) == -1 and lib.tl_savings_hub(np.zeros(2, np.float32).ctypes.data_as(C.c_void_p), 1, None) == -1


def test_hub_on_circles_round_the_centroid(lib):
    """Near-equal d2 everywhere: a fused dx*dx + dy*dy, or another summation order of the centroid, picks another city."""
    fused_differs = 0
    for seed in range(200):
        rng = np.random.default_rng(seed)
        n = 2 * int(rng.integers(4, 200))
        t = rng.random(n // 2) * 2 * np.pi
        t = np.concatenate([t, t + np.pi])  # antipodal pairs: the centroid is the circle's centre, every d2 is r^2 to rounding
        c, r = rng.random(2) * 1000, 1 + rng.random() * 500
        xy = np.stack([c[0] + r * np.cos(t), c[1] + r * np.sin(t)], 1).astype(np.float32)
        want = S.hub_position(xy)
        assert c_hub(lib, xy) == want, seed
        # what a fused d2 would choose (fma(dx, dx, fl(dy*dy)) through f64: exact product, one rounding)
        cx = np.cumsum(np.concatenate([np.zeros(1, np.float32), xy[:, 0]]), dtype=np.float32)[-1] / np.float32(n)
        cy = np.cumsum(np.concatenate([np.zeros(1, np.float32), xy[:, 1]]), dtype=np.float32)[-1] / np.float32(n)
        dx, dy = xy[:, 0] - cx, xy[:, 1] - cy
        fused = (dx.astype(np.float64) * dx.astype(np.float64) + (dy * dy).astype(np.float64)).astype(np.float32)
        fused_differs += int(np.argmin(fused)) != want
    assert fused_differs > 0, "the clouds do not tell a fused d2 from an unfused one"


def test_hub_sequential_sums_at_n_65535(lib):
    rng = np.random.default_rng(65535)
    xy = (1e6 + rng.random((65535, 2)) * 1e3).astype(np.float32)
    want = S.hub_position(xy)
    assert c_hub(lib, xy) == want
    pair = np.asarray([np.ascontiguousarray(xy[:, k]).sum(dtype=np.float32) for k in (0, 1)]) / np.float32(65535)  # numpy's pairwise sum: another centroid
    seq = np.asarray([np.cumsum(xy[:, k], dtype=np.float32)[-1] for k in (0, 1)]) / np.float32(65535)
    assert not np.array_equal(pair, seq)
    d = xy - pair
    assert int(np.argmin(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])) != want, "the instance does not tell the two summation orders apart"
