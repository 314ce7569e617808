"""The seeded instances of the branch-and-bound tests and the seed tours they start from."""
import os

import numpy as np

import _bnb_oracle as B
import _oracle as O
import _tsplib as T

HERE = os.path.dirname(os.path.abspath(__file__))

TSP5 = np.array([[0, 0], [0, 0.5], [0, 1], [1, 1], [1, 0]], dtype=np.float32)                                   # branch_bound.rs:323-333
TSP8 = np.array([[0, 0], [3, 1], [1, 3], [4, 4], [2, 0.5], [0.5, 2], [3.5, 2.5], [1.5, 4]], dtype=np.float32)   # :381-400
GRID3 = np.array([[c, r] for r in range(3) for c in range(3)], dtype=np.float32)                                # many equal lengths


def random_xy(n, seed):
    """Uniform integer coordinates in [0, 1000)^2."""
    return np.random.default_rng(1000 * n + seed).integers(0, 1000, size=(n, 2)).astype(np.float32)


def circle_xy(n=64, seed=0, radius=1000.0):
    """n points at seeded irregular angles on a circle, in a seeded order of positions: the optimum is the circle itself."""
    rng = np.random.default_rng(77 + seed)
    ang = rng.uniform(0.0, 2.0 * np.pi, size=n)
    xy = np.stack([radius * np.cos(ang), radius * np.sin(ang)], axis=1).astype(np.float32)
    return xy[rng.permutation(n)]


def tsp(name):
    e = T.parse_tsplib(os.path.join(HERE, "golden", "tsplib", f"{name}.tsp"))
    pk = e["packed"] if e["packed"] is not None else None
    return e["xy"], (None if pk is None else np.ascontiguousarray(pk, dtype=np.float32)), e["n"]


def seed_tour(xy, packed, n, start=0):
    """Nearest neighbour, then 2-opt, both the project's own on the host (the C oracle), rotated to begin at `start`."""
    rc, nn, _ = O.nearest_neighbor(xy, packed, n)
    assert rc == 0
    rc, two, _, _ = O.two_opt(xy, packed, n, init=nn)
    assert rc == 0
    t = [int(v) for v in two]
    k = t.index(start)
    return np.array(t[k:] + t[:k], dtype=np.uint32)


# name -> (xy, packed, n, K, start, seeded): the cases whose expected result is in tests/golden/goldens_bnb.json
def large_cases():
    out = {}
    for s in (4, 20, 27, 28, 34):  # (of the seeds 0..39, those the restatement proves within 300 000 nodes: the golden file has the counts)
        out[f"rand33_{s}"] = (random_xy(33, s), None, 33, 0, 0, True)
    out["circle64"] = (circle_xy(64, 0), None, 64, 0, 0, True)
    xy26 = random_xy(26, 2)  # integer distances: every sum is exact, so tl_bellman_karp's optimum is this tour's length (the GPU test compares)
    out["int26"] = (xy26, B.packed_of(np.rint(B.dist_matrix(xy26)).astype(np.float32)), 26, 0, 0, True)
    out["rand20"] = (random_xy(20, 1), None, 20, 0, 0, True)       # the knob sweep's instance
    xy17 = random_xy(17, 2)
    out["matrix17"] = (xy17, B.packed_of(np.rint(B.dist_matrix(xy17)).astype(np.float32)), 17, 0, 5, False)
    out["k3_n12"] = (random_xy(12, 4), None, 12, 3, 0, False)
    xy, pk, n = tsp("gr17")
    out["gr17"] = (xy, pk, n, 0, 0, True)
    # (bays29 is not here: from its NN + 2-opt seed the restatement needs 39 529 865 nodes for the proof)
    return out


def small_cases():
    """(name, xy, packed, start, K): the brute-force instances, n = 4..9, both input forms, K in {0, 2, 3, n}, a start other than 0."""
    out = []
    for n in range(4, 10):
        xy = random_xy(n, n)
        for K in (0, 2, 3, n):
            out.append((f"rand{n}_K{K}", xy, None, 0, K))
        out.append((f"rand{n}_start", xy, None, n - 2, 0))
        D = B.dist_matrix(random_xy(n, 50 + n))
        out.append((f"matrix{n}", None, B.packed_of(np.rint(D / 10).astype(np.float32)), 1, 0))   # coarse integers: many ties
        out.append((f"matrix{n}_K3", None, B.packed_of(D), 0, 3))
    out.append(("grid3", GRID3, None, 0, 0))
    out.append(("grid3_K3", GRID3, None, 4, 3))
    xy, pk, n = tsp("ring6_explicit")
    out.append(("ring6_explicit", None, pk, 0, 0))
    out.append(("ring6_explicit_K2", None, pk, 3, 2))
    out.append(("tsp5", TSP5, None, 0, 0))
    out.append(("tsp8", TSP8, None, 0, 0))
    return out


def call(ctx, xy, packed, n, init=None, start=0, K=0, max_nodes=0, time_limit_ms=0, nodes_per_launch=0, frontier_depth=0, workgroups=0):
    """tl_branch_and_bound (ctx given) or tl_branch_and_bound_host (ctx None) on positions:
    (rc, route, cost, proved, improved, stats dict).  xy / packed None: a NULL pointer."""
    import ctypes as C
    from teeline_amd import _capi
    lib = _capi.load()
    if xy is not None:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    if packed is not None:
        packed = np.ascontiguousarray(packed, dtype=np.float32)
    if init is not None:
        init = np.ascontiguousarray(init, dtype=np.uint32)
    o = _capi.TlBnbOpts(start, K, max_nodes, time_limit_ms, nodes_per_launch, frontier_depth, workgroups)
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    cost, proved, improved = C.c_float(-1.0), C.c_uint32(7), C.c_uint32(7)
    st = _capi.TlBnbStats()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = (p(xy), p(packed), n, p(init), C.byref(o), p(out), C.byref(cost), C.byref(proved), C.byref(improved), C.byref(st))
    rc = lib.tl_branch_and_bound(ctx.handle, *args) if ctx is not None else lib.tl_branch_and_bound_host(*args)
    return rc, [int(v) for v in out[:n]], np.float32(cost.value), int(proved.value), int(improved.value), st.as_dict()
