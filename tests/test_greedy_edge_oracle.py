"""CPU tests of the greedy-edge restatement tests/_greedy_oracle.py (graph.rs:54-196, greedy_edge.rs:21-65): the reference's
own unit tests restated, its published numbers, the tie rule on a280, the chunked walk against the literal one, and the
shape of tests/golden/goldens_greedy.json.  No GPU; the -m gpu tests hold tl_greedy_edge to this oracle."""
import json
import os

import numpy as np
import pytest

import _greedy_oracle as G
import _oracle as O
import _tsplib as T

HERE = os.path.dirname(os.path.abspath(__file__))


def pts(*p):
    return np.asarray(p, dtype=np.float32)


def degrees(n, edges):
    d = [0] * n
    for u, v in edges:
        d[u] += 1
        d[v] += 1
    return d


def test_sorted_edges_cover_every_pair_in_total_order():
    xy = pts([0, 0], [1, 0], [1, 1], [0, 1])
    keys = G.sorted_edge_keys(O.dm_build_packed(xy), 4)
    assert len(keys) == 6 and np.all(keys[:-1] < keys[1:])
    d = (keys >> np.uint64(32)).astype(np.uint32) & np.uint32(0x7FFFFFFF)
    assert d.view(np.float32)[0] == 1.0
    # ties (i, j) ascending: the four sides of the unit square, then the two diagonals
    i, j = G._ij(keys)
    assert list(zip(i.tolist(), j.tolist())) == [(0, 1), (0, 3), (1, 2), (2, 3), (0, 2), (1, 3)]


def test_total_keys_order():
    vals = np.frombuffer(np.array([0xFFC00001, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000, 0x3F800000, 0x7F800000, 0x7FC00000],
                                  dtype=np.uint32).tobytes(), dtype=np.float32)  # -NaN -inf -1 -0 +0 1 inf NaN
    k = G.total_keys(vals)
    assert np.all(k[:-1] < k[1:])


def test_select_edges_square_and_degree_two():
    xy = pts([0, 0], [1, 0], [1, 1], [0, 1])
    edges, _ = G.select_edges(4, G.sorted_edge_keys(O.dm_build_packed(xy), 4))
    assert len(edges) == 4
    xy = pts([0, 0], [1, 0], [-1, 0], [0, 1], [0, -1])
    edges, _ = G.select_edges(5, G.sorted_edge_keys(O.dm_build_packed(xy), 5))
    assert degrees(5, edges) == [2] * 5


def test_premature_cycle_rejected_closing_edge_accepted():
    xy = pts([0, 0], [1, 0], [2, 0], [1, 1], [10, 0])
    edges, _ = G.select_edges(5, G.sorted_edge_keys(O.dm_build_packed(xy), 5))
    assert len(edges) == 5 and degrees(5, edges) == [2] * 5
    assert sorted(G.cycle_to_path(5, edges)) == list(range(5))
    # (1, 3) finds 1 at degree 2; (2, 3) would close the 4-cycle 2-1-0-3 with 3 edges in: both skipped; 4 closes the tour
    assert edges[:3] == [(0, 1), (1, 2), (0, 3)] and (1, 3) not in edges and (2, 3) not in edges
    assert 4 in edges[-1] and 4 in edges[-2]


def test_random_instances_are_single_cycles():
    rng = np.random.default_rng(0)
    for n in range(3, 40):
        xy = (rng.random((n, 2)) * 10).astype(np.float32)
        edges, _ = G.select_edges(n, G.sorted_edge_keys(O.dm_build_packed(xy), n))
        assert len(edges) == n and degrees(n, edges) == [2] * n
        assert sorted(G.cycle_to_path(n, edges)) == list(range(n))


def test_cycle_to_path_hand_built():
    assert G.cycle_to_path(4, [(0, 1), (1, 2), (2, 3), (3, 0)]) == [0, 1, 2, 3]
    assert sorted(G.cycle_to_path(5, [(0, 2), (2, 4), (4, 1), (1, 3), (3, 0)])) == [0, 1, 2, 3, 4]
    # the first step follows position 0's EARLIER-accepted edge
    assert G.cycle_to_path(4, [(3, 0), (0, 1), (1, 2), (2, 3)]) == [0, 3, 2, 1]
    with pytest.raises(AssertionError):
        G.cycle_to_path(4, [(0, 1), (0, 2), (0, 3), (1, 2)])
    with pytest.raises(AssertionError):
        G.cycle_to_path(6, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3)])


def test_small_n_solve():
    r, c = G.greedy_edge(pts([0, 0], [1, 0]))
    assert r.tolist() == [0, 1] and c == np.float32(2.0)
    r, c = G.greedy_edge(pts([0, 0]))
    assert r.tolist() == [0] and c == np.float32(0.0)
    r, c = G.greedy_edge(pts([0, 0], [1, 0], [0, 1]))
    assert sorted(r.tolist()) == [0, 1, 2]


def test_reported_cost_is_the_recomputed_cost():
    xy = pts([0, 0], [1, 0], [2, 0], [3, 0], [4, 0])
    r, c = G.greedy_edge(xy)
    assert c.tobytes() == O.tour_length(xy, None, r).tobytes()
    assert abs(float(c) - 8.0) < 1e-6


def test_published_numbers_berlin52():
    b = T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", "berlin52.tsp"))
    r, c = G.greedy_edge(b["xy"])
    assert f"{float(c):.5f}" == "9954.06250"                        # docs/benchmarks.md: 9 954.06
    assert G.greedy_edge(b["xy"], tie="ji")[0].tolist() == r.tolist()  # no tie decides berlin52
    rc, r2, c2, _ = O.two_opt(b["xy"], None, 52, init=r)
    assert rc == 0 and f"{float(c2):.5f}" == "8415.54980"          # docs/benchmarks.md: greedy -> 2-opt 8 415.55


def test_tie_rule_decides_a280():
    a = T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", "a280.tsp"))
    assert f"{float(G.greedy_edge(a['xy'])[1]):.5f}" == "2960.47827"
    assert f"{float(G.greedy_edge(a['xy'], tie='ji')[1]):.5f}" == "3184.81030"


def test_matrix_form_uses_the_packed_matrix():
    g = T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", "gr17.tsp"))
    r, c = G.greedy_edge(None, g["packed"], g["n"])
    assert sorted(r.tolist()) == list(range(17))
    assert c.tobytes() == O.tour_length(None, g["packed"], r).tobytes()


@pytest.mark.parametrize("n,kind", [(200, "random"), (400, "lattice"), (600, "dups"), (1000, "random")])
def test_chunked_walk_equals_the_literal_walk(n, kind):
    rng = np.random.default_rng(n)
    if kind == "random":
        xy = O.synth_xy(n, seed=n)
    elif kind == "lattice":
        xy = np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(np.float32)
    else:
        xy = np.repeat(rng.random((n // 20, 2)).astype(np.float32), 20, axis=0)
    keys = G.sorted_edge_keys(O.dm_build_packed(xy), n)
    lit = G.select_edges(n, keys)
    for chunk in (7, 256, 4096):
        assert G.select_edges(n, keys, chunk=chunk) == lit


def test_golden_file_shape():
    with open(os.path.join(HERE, "golden", "goldens_greedy.json")) as fh:
        g = json.load(fh)
    assert set(g) == {"synthetic10000", "synthetic13509"}
    for k, e in g.items():
        assert e["n"] == int(k[len("synthetic"):]) and len(e["route_sha256"]) == 64
        assert f"{float(np.uint32(e['cost_bits']).view(np.float32)):.5f}" == e["cost"]
        assert 0 < e["reference_examined"] <= e["n"] * (e["n"] - 1) // 2
