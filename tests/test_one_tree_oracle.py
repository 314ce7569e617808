"""The Held-Karp bound on the CPU: the oracle (tests/_one_tree_oracle.py) against ground truth, tl_one_tree_bound_host (the
sequential restatement, csrc/tl_api_onetree.hip) against the oracle bit for bit, the argument rules, the golden file and the mirrors'
names.  DESIGN.md §4.29.

The rounding allowance DESIGN states: the computed L differs from the real-arithmetic 1-tree value of the same tree and pi by at most
A = (n + 1) 2^-52 (sum over the tree's edges |w_e| + 2 sum |pi_i|).  On berlin52 the bound and the f64 length of the tour it proves
are two sums of the same 52 edges in different orders and differ by one unit in the last place (7544.365919113158 against
7544.365919113159), so "equal" is tested within A, not bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _bhk_oracle as B
import _one_tree_cases as K
import _one_tree_oracle as H

HERE = os.path.dirname(os.path.abspath(__file__))


def allowance(res, row, n, root):
    """A of the module text, from the best tree and its pi."""
    pi = res["pi"]
    edges = [(v, int(p)) for v, p in enumerate(res["parent"]) if p != H.NONE] + [(root, int(v)) for v in res["root_nb"]]
    total = sum(abs(float(row(a)[b]) + (pi[a] + pi[b])) for a, b in edges)
    return (n + 1) * 2.0 ** -52 * (total + 2.0 * float(np.abs(pi).sum()))


def small_instances():
    """200 seeded instances, n = 4..9, both input forms."""
    out = []
    for k in range(200):
        n = 4 + k % 6
        xy = K.random_xy(n, k)
        if k % 2:
            out.append((k, None, packed_of_xy(xy), n))
        else:
            out.append((k, xy, None, n))
    return out


def packed_of_xy(xy):
    row = H.rows_of(xy, None, len(xy))
    return np.ascontiguousarray([row(a)[b] for a in range(1, len(xy)) for b in range(a)], dtype=np.float32)


def brute_optimum(row, n):
    """The least f64 tour length over every tour (n <= 9)."""
    import itertools
    D = np.array([row(u).astype(np.float64) for u in range(n)])
    best = np.inf
    for p in itertools.permutations(range(1, n)):
        t = (0,) + p
        best = min(best, sum(D[t[i], t[(i + 1) % n]] for i in range(n)))
    return best


def test_oracle_is_a_lower_bound_on_200_small_instances():
    for k, xy, pk, n in small_instances():
        row = H.rows_of(xy, pk, n)
        upper = K.nn_upper(xy, pk, n)
        res = H.ascent(xy, pk, n, upper=upper, root=k % n, iterations=60)
        # the optimum from the Bellman-Held-Karp oracle (f32 sums: within n 2^-24 of the real sum) and from every permutation in f64
        _, _, optimal, _ = B.bellman_karp(xy, pk, n)
        opt64 = brute_optimum(row, n) if n <= 8 else None
        A = allowance(res, row, n, k % n)
        assert res["bound"] <= float(optimal) * (1.0 + n * 2.0 ** -24) + A, (k, res["bound"], optimal)
        if opt64 is not None:
            assert res["bound"] <= opt64 + A, (k, res["bound"], opt64)
        L0 = H.one_tree(row, n, np.zeros(n), k % n)[0]
        assert res["bound"] >= L0 and res["log"][0][0] == L0, k


def test_berlin52_against_its_optimal_tour():
    xy, pk, n = K.tsp("berlin52")
    row = H.rows_of(xy, pk, n)
    opt_len = H.tour_length_f64(row, K.opt_tour_positions("berlin52"))
    res = H.ascent(xy, pk, n, upper=K.nn_upper(xy, pk, n), iterations=300)
    assert res["bound"] <= opt_len + allowance(res, row, n, 0)
    res = H.ascent(xy, pk, n, upper=1.05 * opt_len)
    assert res["is_tour"] == 1 and res["stop"] == H.STOP_TOUR and sorted(res["tour"]) == list(range(n))
    assert abs(H.tour_length_f64(row, res["tour"]) - res["bound"]) <= allowance(res, row, n, 0)
    assert res["best_iter"] == 159 and f"{res['bound']:.3f}" == "7544.366"  # the figures the specification's prototype gave


def host_equals_oracle(xy, pk, n, what, **kw):
    w = H.ascent(xy, pk, n, **kw)
    rc, got = K.call(None, xy, pk, n, **kw)
    assert rc == 0, what
    K.assert_same(got, w, what)
    return got


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "goldens_one_tree.json")))


def test_host_equals_the_golden_file(golden):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_goldens_one_tree as M
    assert sorted(golden) == sorted(M.CASES)
    for name, kw in M.CASES.items():
        xy, pk, n = K.tsp(name)
        rc, got = K.call(None, xy, pk, n, upper=golden[name]["upper"], **kw)
        assert rc == 0
        assert M.record(got, golden[name]["upper"]) == golden[name], name


def test_host_equals_oracle_on_a_seeded_campaign():
    rng = np.random.default_rng(2028)
    for n in range(3, 41):
        xy = K.random_xy(n, 5)
        pk = packed_of_xy(xy) if n % 3 == 0 else None
        kw = dict(root=int(rng.integers(0, n)), iterations=int(rng.integers(1, 80)), lambda0=float(rng.choice([0.5, 1.0, 2.0, 3.5])),
                  patience=int(rng.integers(1, 12)), upper=K.nn_upper(xy, pk, n) * float(rng.choice([1.0, 1.05, 0.9])))
        host_equals_oracle(None if pk is not None else xy, pk, n, f"n={n}", **kw)


@pytest.mark.parametrize("name", ["grid", "twins", "ring6_explicit", "matrix"])
def test_host_equals_oracle_where_ties_decide(name):
    if name == "grid":
        xy, pk, n = K.unit_grid(6, 5), None, 30
    elif name == "twins":
        xy, pk, n = K.duplicated(24, 3), None, 24
    elif name == "matrix":
        xy, pk, n = None, K.random_matrix(23, 2), 23
    else:
        xy, pk, n = K.tsp(name)
    up = K.nn_upper(xy, pk, n)
    for root in (0, n - 1, 1):  # root 0 is the lowest position: Prim's start moves to 1
        host_equals_oracle(xy, pk, n, f"{name} root {root}", upper=up, root=root, iterations=50)


def test_stop_reasons_on_the_host():
    xy, pk, n = K.random_xy(65, 1), None, 65
    up = K.nn_upper(xy, pk, n)
    assert host_equals_oracle(xy, pk, n, "lambda", upper=up, lambda0=0.05, patience=1, iterations=200)["stop"] == H.STOP_LAMBDA
    assert host_equals_oracle(xy, pk, n, "upper", upper=0.25 * up, iterations=40)["stop"] == H.STOP_UPPER
    assert host_equals_oracle(xy, pk, n, "cap", upper=up, iterations=7)["stop"] == H.STOP_ITERATIONS
    assert host_equals_oracle(K.random_xy(3, 1), None, 3, "n = 3", upper=5000.0)["stop"] == H.STOP_TOUR


def test_small_n():
    xy = K.random_xy(3, 1)
    for n in (0, 1, 2):
        rc, got = K.call(None, xy, None, n, upper=1.0)
        w = H.ascent(xy[:n], None, n, upper=1.0)
        assert rc == 0 and K.bits(got["bound"]) == K.bits(w["bound"]) and got["is_tour"] == 1 and got["tour"] == list(range(n))
        assert got["iterations_run"] == 0 and got["stop"] == 0
    assert K.call(None, xy, None, 2, upper=1.0)[1]["bound"] == 2.0 * float(H.rows_of(xy, None, 3)(0)[1])
    pk = packed_of_xy(xy)
    assert K.bits(K.call(None, None, pk, 2, upper=1.0)[1]["bound"]) == K.bits(2.0 * float(pk[0]))
    got = host_equals_oracle(xy, None, 3, "n = 3", upper=5000.0)
    assert got["iterations_run"] == 1 and got["best_iter"] == 0 and sorted(got["tour"]) == [0, 1, 2]


def test_argument_rules():
    xy = K.random_xy(6, 1)
    ok = dict(upper=3000.0)
    assert K.call(None, xy, None, 6, **ok)[0] == 0
    for bad in (dict(root=6), dict(iterations=0), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda0=np.inf), dict(lambda0=np.nan), dict(patience=0),
                dict(upper=0.0), dict(upper=-5.0), dict(upper=np.inf), dict(upper=np.nan), dict(reserved=1)):
        assert K.call(None, xy, None, 6, **dict(ok, **bad))[0] == K.TL_ERR_BADARG, bad
    assert K.call(None, None, None, 6, **ok)[0] == K.TL_ERR_BADARG
    assert K.call(None, xy, None, 1, root=1, **ok)[0] == K.TL_ERR_BADARG
    pk = packed_of_xy(xy)
    for bad in (np.nan, np.inf, -1.0, -0.0):
        q = pk.copy()
        q[7] = bad
        assert K.call(None, None, q, 6, **ok)[0] == K.TL_ERR_UNSUPPORTED, bad
    for bad in (np.nan, np.inf, 1e19):
        q = xy.copy()
        q[2, 1] = bad
        assert K.call(None, q, None, 6, **ok)[0] == K.TL_ERR_UNSUPPORTED, bad
    from teeline_amd import _capi
    assert b"coordinate" in _capi.load().tl_last_error(None)


def test_plan_max_n_and_work_bytes_need_no_device():
    from teeline_amd import _capi
    lib = _capi.load()
    max_n = lib.tl_one_tree_bound_max_n(K.LDS_BYTES)
    assert max_n == (K.LDS_BYTES - 1024) // 24 and lib.tl_one_tree_bound_max_n(0) == 0
    t, span = C.c_int(), C.c_uint32()
    assert lib.tl_one_tree_bound_plan(max_n, K.LDS_BYTES, C.byref(t), C.byref(span)) == 0 and t.value == 1024 and span.value >= 1
    assert lib.tl_one_tree_bound_plan(max_n + 1, K.LDS_BYTES, C.byref(t), C.byref(span)) == K.TL_ERR_UNSUPPORTED and t.value == 0
    assert lib.tl_one_tree_bound_plan(52, K.LDS_BYTES, C.byref(t), C.byref(span)) == 0 and t.value == 64 and span.value == 16384 // 52
    assert lib.tl_one_tree_bound_plan(52, -1, None, None) == K.TL_ERR_BADARG
    assert lib.tl_one_tree_bound_work_bytes(2, 1, 0) == 0
    assert lib.tl_one_tree_bound_work_bytes(52, 3, 10) >= 3 * (52 * 24 + 10 * 24)


def test_mirror_names_and_gap():
    import teeline_amd as TA
    M = TA.one_tree_bound
    assert callable(M.bound) and callable(M.bound_batch) and callable(M.bound_host)
    assert "one_tree_bound" not in TA.pipeline.SOLVER_NAMES and "bound" not in TA.pipeline.SOLVER_NAMES
    assert M.gap_pct_of(110.0, 100.0) == 10.0
    b = M.Bound(200.0, None, False, None, {}, [], 230.0)
    assert b.gap_pct(210.0) == 5.0 and b.gap_pct(200.0) == 0.0


def test_host_mirror():
    import teeline_amd as TA
    xy, pk, n = K.tsp("berlin52")
    ids = np.arange(1, n + 1)
    row = H.rows_of(xy, pk, n)
    up = 1.05 * H.tour_length_f64(row, K.opt_tour_positions("berlin52"))
    b = TA.one_tree_bound.bound_host(TA.TspProblem(ids, xy), up, log_cap=1000)
    w = H.ascent(xy, pk, n, upper=up)
    assert K.bits(b.bound) == K.bits(w["bound"]) and b.is_tour and b.route == [int(ids[p]) for p in w["tour"]]
    assert b.stats["stop_name"] == "tour" and len(b.log) == 160 and b.pi.tobytes() == w["pi"].tobytes()
