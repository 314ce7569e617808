"""CPU tests of the Bellman-Held-Karp restatement tests/_bhk_oracle.py (bellman_karp.rs:24-165): the reference's own unit tests
restated, the pinned optima / totals / routes of the small fixtures, the seeded campaign with its one result that is no tour, the
exact walk, the degenerate sizes, the pipeline names and the shape of tests/golden/goldens_bhk.json.  The -m gpu tests
(test_gpu_bhk.py) hold tl_bellman_karp to this oracle."""
import json
import os

import numpy as np
import pytest

import _bhk_oracle as B
import _oracle as O
import _tsplib as T

HERE = os.path.dirname(os.path.abspath(__file__))


def tsp(name):
    return T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))


def matrix_of(e):
    pk = e["packed"] if e["packed"] is not None else O.dm_build_packed(e["xy"], geo=True)
    return np.ascontiguousarray(pk, dtype=np.float32)


def lattice4():
    """4 x 4 unit lattice, row-major: the walk meets ties at four of its steps."""
    return np.array([[c, r] for r in range(4) for c in range(4)], dtype=np.float32)


def doubled6():
    """The first 6 cities of berlin52, each twice: zero distances between the twins."""
    return np.repeat(tsp("berlin52")["xy"][:6], 2, axis=0).astype(np.float32)


TSP5 = np.array([[0, 0], [0, 0.5], [0, 1], [1, 1], [1, 0]], dtype=np.float32)                       # bellman_karp.rs:193-203
TRI = np.array([[0, 0], [3, 0], [0, 4]], dtype=np.float32)                                           # :268-283
EIGHT = np.array([[0, 0], [3, 1], [1, 3], [4, 4], [2, 0.5], [0.5, 2], [3.5, 2.5], [1.5, 4]], dtype=np.float32)  # :237-246


def pinned():
    """name -> (xy, packed, n, optimal, total, route): the issue's table.  The first three are the reference's unit tests, the
    others the values of an independent C restatement."""
    b52 = tsp("berlin52")["xy"]
    rows = {
        "tsp5": (TSP5, None, 5, "4.00000", "4.00000", "4 0 1 2 3"),
        "tri": (TRI, None, 3, "12.00000", "12.00000", "2 0 1"),
        "eight": (EIGHT, None, 8, "13.13949", "13.13949", "7 2 5 0 4 1 6 3"),
        "berlin12": (b52[:12], None, 12, "4056.68066", "4056.68091", "11 3 5 4 0 1 6 2 7 8 9 10"),
        "berlin16": (b52[:16], None, 16, "4990.46045", "4990.46045", "15 0 1 6 2 7 8 9 14 4 5 3 11 10 12 13"),
        "berlin20": (b52[:20], None, 20, "5270.85889", "5270.85938", "19 1 6 16 2 17 0 18 7 8 9 14 4 5 3 11 10 12 13 15"),
        "lattice4": (lattice4(), None, 16, "16.00000", "16.00000", "15 11 7 3 2 1 0 4 5 6 10 9 8 12 13 14"),
        "doubled6": (doubled6(), None, 12, "2315.14673", "2315.14673", "11 6 7 4 5 2 3 0 1 8 9 10"),
    }
    for name, cost, route in (("ring6_explicit", "60.00000", "5 0 1 2 3 4"),
                              ("burma14", "3323.00000", "13 1 0 9 8 10 7 12 6 11 5 4 3 2"),
                              ("gr17", "2085.00000", "16 5 7 6 12 3 0 15 11 8 4 1 9 10 2 14 13")):
        e = tsp(name)
        rows[name] = (e["xy"], matrix_of(e), e["n"], cost, cost, route)
    return rows


PINNED = sorted(pinned())


@pytest.fixture(scope="module")
def rows():
    return pinned()


@pytest.mark.parametrize("name", PINNED)
def test_pinned_instances(rows, name):
    xy, pk, n, optimal, total, route = rows[name]
    ref, ex = B.both(xy, pk, n)
    r, c, o, ok = ref
    assert r.tolist() == [int(v) for v in route.split()]
    assert f"{float(o):.5f}" == optimal and f"{float(c):.5f}" == total and ok == 1
    # the exact walk reads the same table: a permutation from `last` whose own length is the optimum up to the sum's rounding
    xr, xc, xo, xok = ex
    assert xok == 1 and xr[0] == n - 1 and xo.tobytes() == o.tobytes()
    assert abs(float(xc) - float(o)) <= 1e-4 * max(1.0, float(o))


def test_reference_unit_tests_restated():
    # test_solve_returns_all_cities, test_solve_finds_optimal_tour_length, test_route_reconstruction_on_larger_instance,
    # test_solve_with_3_cities (bellman_karp.rs:205-283)
    r, c, o, ok = B.bellman_karp(TSP5)
    assert sorted(r.tolist()) == [0, 1, 2, 3, 4] and abs(float(c) - 4.0) < 1e-3
    r, c, o, ok = B.bellman_karp(EIGHT)
    assert sorted(r.tolist()) == list(range(8)) and ok == 1
    r, c, o, ok = B.bellman_karp(TRI)
    assert sorted(r.tolist()) == [0, 1, 2] and abs(float(c) - 12.0) < 1e-3


def test_total_is_the_routes_length_not_the_optimum(rows):
    xy, pk, n, *_ = rows["berlin12"]
    r, c, o, ok = B.bellman_karp(xy, pk, n)
    assert c.tobytes() == O.tour_length(xy, None, r.astype(np.uint32)).tobytes() and c.tobytes() != o.tobytes()


@pytest.fixture(scope="module")
def campaign():
    return [(xy, *B.both(xy)) for xy in B.campaign()]


def test_campaign_has_exactly_one_result_that_is_no_tour(campaign):
    bad = [k for k, (xy, ref, ex) in enumerate(campaign) if ref[3] == 0]
    assert len(campaign) == 200 and len(bad) == 1
    xy, ref, ex = campaign[bad[0]]
    assert ref[0][0] == len(xy) - 1 and sorted(ref[0].tolist()) != list(range(len(xy)))
    # the exact walk on that instance: a permutation whose length is the optimum up to the tolerance
    assert ex[3] == 1 and abs(float(ex[1]) - float(ex[2])) <= 1e-4 * max(1.0, float(ex[2]))


def test_exact_walk_is_a_permutation_on_the_whole_campaign(campaign):
    for xy, ref, ex in campaign:
        assert ex[3] == 1 and sorted(ex[0].tolist()) == list(range(len(xy))) and ex[0][0] == len(xy) - 1
        assert ex[2].tobytes() == ref[2].tobytes()
        if ref[3]:  # both are optimal tours: equal lengths up to the order of the sum
            assert abs(float(ex[1]) - float(ref[1])) <= 1e-4 * max(1.0, float(ref[1]))


def test_degenerate_sizes():
    xy = np.array([[0, 0], [3, 4]], dtype=np.float32)
    for fn in (B.bellman_karp, B.exact_walk):
        r, c, o, ok = fn(xy[:1])
        assert r.tolist() == [0] and c == np.float32(0.0) and o == B.F32_MAX and ok == 1   # the fold is empty, the walk does not run
        r, c, o, ok = fn(xy)
        assert r.tolist() == [1, 0] and c == np.float32(10.0) and o == np.float32(10.0) and ok == 1
        r, c, o, ok = fn(xy[:0])
        assert len(r) == 0 and c == np.float32(0.0)
    # two cities at one point: optimal = 0 stops the walk before its first step, and [1, 0] is what the zeroed route holds anyway
    r, c, o, ok = B.bellman_karp(np.zeros((2, 2), np.float32))
    assert r.tolist() == [1, 0] and o == np.float32(0.0)


def test_terms_that_are_nan_or_max_are_never_taken():
    n = 9
    rng = np.random.default_rng(9)
    base = rng.integers(1, 50, n * (n - 1) // 2).astype(np.float32)
    want = B.bellman_karp(None, base, n)
    for bad in (np.float32(np.nan), B.F32_MAX):
        pk = base.copy()
        # an edge the optimal tour does not use: poisoning it changes nothing; one it uses: the optimum moves but stays finite
        r = want[0].tolist()
        used = {(min(a, b), max(a, b)) for a, b in zip(r, r[1:] + r[:1])}
        i, j = next((i, j) for j in range(n) for i in range(j) if (i, j) not in used)
        pk[j * (j - 1) // 2 + i] = bad
        got = B.bellman_karp(None, pk, n)
        assert got[0].tolist() == r and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        i, j = sorted(r[1:3])
        pk[j * (j - 1) // 2 + i] = bad
        got = B.bellman_karp(None, pk, n)
        assert got[2] < B.F32_MAX and got[2] >= want[2] and got[3] == 1
        rr = got[0].tolist()
        assert (i, j) not in {(min(a, b), max(a, b)) for a, b in zip(rr, rr[1:] + rr[:1])}


def test_pipeline_names():
    import teeline_amd as TA
    P = TA.pipeline
    assert P.steps_for_solve("bhk") == ["bhk"] and P.steps_for_solve("bellman_karp") == ["bellman_karp"]
    assert P.SOLVER_NAMES["bhk"] == P.SOLVER_NAMES["bellman_karp"] == "bellman_karp"
    assert "bellman_karp" not in P.AUTO_EXPAND_WITH_NN  # mod.rs:2137: no NN stage in front
    assert callable(TA.bellman_karp.solve) and TA.host.bellman_karp is TA.bellman_karp
    assert TA._capi.TL_BHK_MAX_N == 26 and TA._capi.TL_FLAG_BHK_EXACT_WALK == 1 << 25


def test_golden_file_shape():
    with open(os.path.join(HERE, "golden", "goldens_bhk.json")) as fh:
        g = json.load(fh)
    assert "ulysses22" in g and set(g) <= {"ulysses22", "berlin23"}
    u = g["ulysses22"]
    assert u["n"] == 22 and u["optimal"] == "7013.00000"
    assert u["reference_walk"]["route"] == [int(v) for v in "21 3 17 7 0 13 12 11 6 5 14 4 10 8 9 18 19 20 15 2 1 16".split()]
    if "berlin23" in g:
        b = g["berlin23"]
        assert b["optimal"] == "5347.82373" and b["reference_walk"]["cost"] == "5347.82422"
        assert b["reference_walk"]["route"] == [int(v) for v in "22 0 21 17 20 1 6 16 2 18 7 8 9 14 4 5 3 11 10 12 13 15 19".split()]
    for e in g.values():
        for w in ("reference_walk", "exact_walk"):
            r = e[w]
            assert len(r["route"]) == e["n"] and r["route"][0] == e["n"] - 1 and r["is_tour"] in (0, 1)
            assert f"{float(np.uint32(r['cost_bits']).view(np.float32)):.5f}" == r["cost"]
        assert f"{float(np.uint32(e['optimal_bits']).view(np.float32)):.5f}" == e["optimal"]
