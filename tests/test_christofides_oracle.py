"""CPU tests of the Christofides restatement tests/_christofides_oracle.py (christofides.rs:12-241): the issue's table of costs,
-> 2-opt / -> Or-opt ends and tree / odd-vertex / pair counts, the lattice with its massive ties, the inputs on which each pinned
order decides the tour, the pipeline names, the smallest inputs and the shape of tests/golden/goldens_christofides.json.  The
-m gpu tests (test_gpu_christofides.py) hold tl_christofides to this oracle."""
import json
import os

import numpy as np
import pytest

import _christofides_oracle as X
import _oracle as O
import _tsplib as T

HERE = os.path.dirname(os.path.abspath(__file__))


def tsp(name):
    return T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))


def matrix_of(e):
    pk = e["packed"] if e["packed"] is not None else O.dm_build_packed(e["xy"], geo=True)
    return np.ascontiguousarray(pk, dtype=np.float32)


def lattice():
    """7 x 6 unit lattice in row-major order: ties everywhere, in Prim's argmin and in the matching."""
    return np.stack(np.meshgrid(np.arange(7), np.arange(6)), -1).reshape(-1, 2).astype(np.float32)


def star():
    """Three leaves round position 0, one spoke short: the shortest pair of odd vertices (0, 1) is a tree edge, so the multigraph
    holds it twice and the Euler walk must remove ONE occurrence."""
    return np.array([[0, 0], [1, 0], [-10, 10], [-10, -10]], dtype=np.float32)


def all_equal(n):
    return np.zeros((n, 2), np.float32), np.full(n * (n - 1) // 2, 5, np.float32)


def signed_zeros(n, seed=2):
    """An explicit matrix a quarter -0.0, a quarter +0.0, an eighth -1, the rest small integers (as drawn for n = 8, 12, 16 in turn)."""
    rng = np.random.default_rng(seed)
    for m_n in (8, 12, 16):
        m = m_n * (m_n - 1) // 2
        pk = rng.integers(1, 6, m).astype(np.float32)
        idx = rng.permutation(m)
        pk[idx[:m // 4]] = np.float32(-0.0)
        pk[idx[m // 4:m // 2]] = np.float32(0.0)
        pk[idx[m // 2:m // 2 + m // 8]] = -1
        if m_n == n:
            return np.zeros((n, 2), np.float32), pk
    raise ValueError(n)


@pytest.mark.parametrize("name,cost,cost2,cost_or,counts", [
    ("berlin52", "8707.66113", "8128.74512", "8031.55029", (51, 22, 11)),
    ("att48", "41558.89062", None, None, (47, 30, 15)),
    ("a280", "3011.82495", "2731.14819", "2668.86743", (279, 120, 60)),
    ("att532", "102420.89844", None, None, (531, 232, 116))])
def test_table_coordinates(name, cost, cost2, cost_or, counts):
    e = tsp(name)
    r, c, st = X.christofides(e["xy"], with_stats=True)
    assert sorted(r.tolist()) == list(range(e["n"])) and c.tobytes() == O.tour_length(e["xy"], None, r).tobytes()
    assert f"{float(c):.5f}" == cost and (st["mst_edges"], st["k"], len(st["pairs"])) == counts
    if cost2:
        rc, r2, c2, _ = O.two_opt(e["xy"], None, e["n"], init=r)
        assert rc == 0 and f"{float(c2):.5f}" == cost2
        assert f"{float(O.or_opt(e['xy'], None, e['n'], init=r)[2]):.5f}" == cost_or


def test_berlin52_is_the_references_published_number():
    assert f"{float(X.christofides(tsp('berlin52')['xy'])[1]):.2f}" == "8707.66"  # docs/benchmarks.md


@pytest.mark.parametrize("name,cost,counts", [("gr17", 2404.0, (16, 8, 4)), ("bays29", 2389.0, (28, 16, 8)), ("burma14", 4033.0, (13, 6, 3))])
def test_table_matrix_form(name, cost, counts):
    e = tsp(name)
    r, c, st = X.christofides(e["xy"], matrix_of(e), e["n"], with_stats=True)
    assert sorted(r.tolist()) == list(range(e["n"]))
    assert c.tobytes() == np.float32(cost).tobytes() and (st["mst_edges"], st["k"], len(st["pairs"])) == counts


def test_lattice_counts_and_prefix():
    r, c, st = X.christofides(lattice(), with_stats=True)
    assert (st["mst_edges"], st["k"], len(st["pairs"])) == (41, 12, 6)
    assert r[:9].tolist() == [0, 7, 14, 21, 28, 35, 36, 29, 22] and sorted(r.tolist()) == list(range(42))


def _route(xy, pk=None, **kw):
    return X.christofides(xy, pk, len(xy), want_cost=False, **kw)[0].tolist()


def test_each_pinned_order_decides_a_tour():
    """Which input catches which wrong rule (found on the CPU with the oracle's switches):
    last minimum in Prim      the lattice and the all-equal matrix of 6 (Prim's star from 0 becomes a star from elsewhere);
    (j, i) matching ties      the lattice and a280 (a lattice-like drilling pattern);
    total_cmp on +-0          the signed-zero matrices of 8 and 16 (-0.0 would sort before +0.0, in Prim and in the matching);
    remove all occurrences    the 3-leaf star and berlin52 (each has a matched pair that is also a tree edge)."""
    a280 = tsp("a280")["xy"]
    for xy, pk in ((lattice(), None), all_equal(6)):
        assert _route(xy, pk, prim_rule="last") != _route(xy, pk)
    for xy in (lattice(), a280):
        assert _route(xy, tie="ji") != _route(xy)
    for n in (8, 16):
        xy, pk = signed_zeros(n)
        assert _route(xy, pk, zero="total_cmp") != _route(xy, pk)
    for xy in (star(), tsp("berlin52")["xy"]):
        assert _route(xy, euler="all") != _route(xy)
    # the doubled edge is real: the star's first matched pair is the tree edge (1, 0)
    st = X.christofides(star(), with_stats=True)[2]
    assert st["pairs"][0] == (0, 1) and int(st["parent"][1]) == 0


def test_key_order_zero_and_nan():
    vals = np.frombuffer(np.array([0xFF800000, 0xBF800000, 0x80000001, 0x80000000, 0x00000001, 0x3F800000, 0x7F800000],
                                  dtype=np.uint32).tobytes(), dtype=np.float32)  # -inf -1 -subnormal -0 subnormal 1 inf: ascending
    k = X.matching_key32(vals)
    assert np.all(k[:-1] < k[1:]) and k[-1] == 0xFF800000
    assert X.matching_key32(np.float32(-0.0)) == X.matching_key32(np.float32(0.0))
    nans = np.frombuffer(np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).tobytes(), dtype=np.float32)
    assert X.matching_key32(nans).tolist() == [int(X.NAN_KEY)] * 4 and X.NAN_KEY == k[-1] + 1


def test_chunked_matching_equals_the_literal_walk():
    xy = O.synth_xy(600, seed=600)
    pk = O.dm_build_packed(xy)
    parent, _ = X.prim(pk, 600)
    odd = X.odd_vertices(parent, 600)
    keys = X.sorted_pair_keys(pk, odd)
    lit = X.greedy_matching(600, keys, len(odd) // 2, chunk=1)
    for chunk in (7, 64, 4096):
        assert X.greedy_matching(600, keys, len(odd) // 2, chunk=chunk) == lit


def test_not_spanning_names_the_position():
    n = 6
    pk = np.arange(1, n * (n - 1) // 2 + 1, dtype=np.float32)
    for v in range(n):
        if v != 3:
            i, j = min(v, 3), max(v, 3)
            pk[j * (j - 1) // 2 + i] = np.float32(np.nan) if v % 2 else np.float32(np.inf)
    with pytest.raises(X.NotSpanning) as ei:
        X.christofides(np.zeros((n, 2), np.float32), pk, n)
    assert ei.value.position == 3


def test_small_n_is_the_identity():
    xy = np.array([[0, 0], [3, 4], [3, 0]], dtype=np.float32)
    for n in range(4):
        r, c = X.christofides(xy[:n])
        assert r.tolist() == list(range(n))
    assert X.christofides(xy)[1] == np.float32(12.0) and X.christofides(xy[:2])[1] == np.float32(10.0)
    r, c, st = X.christofides(np.array([[0, 0], [1, 0], [2, 0], [1, 1]], dtype=np.float32), with_stats=True)  # n = 4: the smallest real case
    assert sorted(r.tolist()) == [0, 1, 2, 3] and st["mst_edges"] == 3


def test_pipeline_names():
    import teeline_amd as TA
    P = TA.pipeline
    assert P.steps_for_solve("chr") == ["chr"] and P.steps_for_solve("christofides") == ["christofides"]
    assert P.SOLVER_NAMES["chr"] == P.SOLVER_NAMES["christofides"] == "christofides"
    assert "christofides" not in P.AUTO_EXPAND_WITH_NN  # a seed: no NN stage in front
    assert callable(TA.christofides.solve) and TA.host.christofides is TA.christofides


def test_golden_file_shape():
    with open(os.path.join(HERE, "golden", "goldens_christofides.json")) as fh:
        g = json.load(fh)
    assert set(g) == {"synthetic10000", "synthetic13509", "synthetic30000"}
    for k, e in g.items():
        assert e["n"] == int(k[len("synthetic"):]) and len(e["route_sha256"]) == 64
        assert f"{float(np.uint32(e['cost_bits']).view(np.float32)):.5f}" == e["cost"]
        assert e["odd_vertices"] % 2 == 0 and 0 < e["odd_vertices"] <= e["n"]
        assert e["odd_vertices"] // 2 <= e["reference_examined"] <= e["odd_vertices"] * (e["odd_vertices"] - 1) // 2
