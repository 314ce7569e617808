"""Christofides construction on the GPU (-m gpu): tl_christofides against the numpy restatement tests/_christofides_oracle.py
(christofides.rs:12-241 with the orders of DESIGN.md §2) — route element for element, cost bit for bit."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import _christofides_oracle as X
import _greedy_oracle as G
import _oracle as O
import _savings_oracle as S
import _tsplib as T
from test_christofides_oracle import all_equal, lattice, matrix_of, signed_zeros, star

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(ctx, xy, packed=None, n=None):
    """tl_christofides through the C ABI: (rc, route positions, cost, stats dict).  xy None: a NULL pointer."""
    import teeline_amd as TA
    if xy is not None:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        n = len(xy) if n is None else n
    out = np.zeros(max(n, 1), dtype=np.uint32)
    cost = C.c_float()
    st = TA._capi.TlStats()
    rc = ctx.lib.tl_christofides(ctx.handle, None if xy is None else xy.ctypes.data_as(C.c_void_p),
                                 None if packed is None else packed.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p),
                                 C.byref(cost), C.byref(st))
    return rc, out[:n], np.float32(cost.value), st.as_dict()


def check(ctx, xy, packed=None, what=""):
    n = len(xy) if packed is None else int(round((1 + np.sqrt(1 + 8 * len(packed))) / 2))
    rc, route, cost, st = gpu(ctx, xy, packed, n)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    oroute, ocost, ost = X.christofides(xy, packed, n, with_stats=True)
    assert route.tolist() == oroute.tolist(), f"{what}: route differs"
    assert cost.tobytes() == np.float32(ocost).tobytes(), f"{what}: cost {cost!r} against {ocost!r}"
    if n >= 4:
        # the bands hold only pairs of still unmatched vertices: a subset of the pairs the literal walk examines
        assert st["moves"] == n and st["sweeps"] >= 1 and 0 < st["candidates"] <= ost["examined"], (what, st, ost["examined"])
    return route, cost, ost


@pytest.mark.parametrize("name", ["berlin52", "att48", "a280", "att532"])
def test_tsplib_coordinates(ctx, tsplib_dir, name):
    """att532 has 232 odd vertices = 26 796 pairs: more than one band of 16 384 keys."""
    e = T.parse_tsplib(os.path.join(tsplib_dir, f"{name}.tsp"))
    route, cost, ost = check(ctx, e["xy"], what=name)
    pins = {"berlin52": "8707.66113", "att48": "41558.89062", "a280": "3011.82495", "att532": "102420.89844"}
    assert f"{float(cost):.5f}" == pins[name]
    if name == "att532":
        assert ost["k"] * (ost["k"] - 1) // 2 == 26796


@pytest.mark.parametrize("name", ["gr17", "bays29", "burma14", "ring6_explicit"])
def test_matrix_form(ctx, tsplib_dir, name):
    e = T.parse_tsplib(os.path.join(tsplib_dir, f"{name}.tsp"))
    route, cost, _ = check(ctx, e["xy"], matrix_of(e), what=name)
    pins = {"gr17": 2404.0, "bays29": 2389.0, "burma14": 4033.0}
    if name in pins:
        assert cost.tobytes() == np.float32(pins[name]).tobytes()
    # with a matrix the coordinates are not needed at all
    rc, r2, c2, _ = gpu(ctx, None, matrix_of(e), e["n"])
    assert rc == 0 and r2.tolist() == route.tolist() and c2.tobytes() == cost.tobytes()


def test_small_n(ctx):
    xy = np.array([[0, 0], [3, 4], [3, 0], [9, 9]], dtype=np.float32)
    for n in (0, 1, 2, 3):  # christofides.rs:24-30: the identity
        rc, route, cost, st = gpu(ctx, xy[:n], n=n)
        assert rc == 0 and route.tolist() == list(range(n)) and st["sweeps"] == 0
        assert cost.tobytes() == np.float32({0: 0.0, 1: 0.0, 2: 10.0, 3: 12.0}[n]).tobytes()
        if n >= 2:
            rc, route, cost, _ = gpu(ctx, xy[:n], O.dm_build_packed(xy[:n]), n)
            assert rc == 0 and route.tolist() == list(range(n))
    rng = np.random.default_rng(1)
    for n in (4, 5, 6, 7):
        for _ in range(4):
            p = (rng.random((n, 2)) * 100).astype(np.float32)
            check(ctx, p, what=f"n={n}")
            check(ctx, p, O.dm_build_packed(p), what=f"matrix n={n}")
    line = np.stack([np.arange(5), np.zeros(5)], 1).astype(np.float32)  # collinear: the tree is the path, k = 2
    assert check(ctx, line, what="collinear n=5")[2]["k"] == 2


def test_doubled_edge_and_massive_ties(ctx):
    ost = check(ctx, star(), what="3-leaf star")[2]
    assert ost["pairs"][0] == (0, 1) and int(ost["parent"][1]) == 0  # the first matched pair is a tree edge
    route, _, ost = check(ctx, lattice(), what="7 x 6 lattice")
    assert (ost["mst_edges"], ost["k"], len(ost["pairs"])) == (41, 12, 6) and route[:9].tolist() == [0, 7, 14, 21, 28, 35, 36, 29, 22]
    check(ctx, lattice(), O.dm_build_packed(lattice()), what="lattice, matrix form")
    for n in (6, 7, 64, 65, 300):  # Prim builds a star from 0; every matching key ties
        xy, pk = all_equal(n)
        ost = check(ctx, xy, pk, what=f"all-equal matrix n={n}")[2]
        assert np.all(ost["parent"][1:] == 0)
    check(ctx, np.zeros((300, 2), dtype=np.float32), what="300 coincident points")
    rng = np.random.default_rng(4)
    check(ctx, np.repeat((rng.random((40, 2)) * 100).astype(np.float32), 5, axis=0), what="duplicate points")


def test_signed_zero_negative_and_nan_entries(ctx):
    for n in (8, 12, 16):
        xy, pk = signed_zeros(n)
        check(ctx, xy, pk, what=f"signed zeros n={n}")
    rng = np.random.default_rng(3)
    hit = 0
    for n in (9, 17, 64, 200):
        m = n * (n - 1) // 2
        pk = rng.integers(1, 30, m).astype(np.float32)
        idx = rng.permutation(m)
        k = max(1, m // 10)
        pk[idx[:k]] = np.float32(np.nan)
        pk[idx[k:2 * k]] = np.float32(-0.0)
        pk[idx[2 * k:3 * k]] = np.float32(np.inf)
        pk[idx[3 * k:3 * k + 1]] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), dtype=np.float32)  # a negative NaN
        pk[idx[3 * k + 1:4 * k]] = np.float32(-3.0)
        ost = check(ctx, np.zeros((n, 2), np.float32), pk, what=f"explicit n={n}")[2]
        odd = X.odd_vertices(ost["parent"], n)
        d = np.array([pk[j * (j - 1) // 2 + i] for a, i in enumerate(odd) for j in odd[a + 1:]], dtype=np.float32)
        hit += int(np.isnan(d).any())
    assert hit >= 2, "no NaN between two odd vertices in these matrices"


def test_vertex_nothing_reaches_is_refused(ctx):
    import teeline_amd as TA
    n = 40
    pk = O.dm_build_packed(O.synth_xy(n, seed=40)).copy()
    for v in range(n):
        if v != 3:
            i, j = min(v, 3), max(v, 3)
            pk[j * (j - 1) // 2 + i] = np.float32(np.nan) if v % 2 else np.float32(np.inf)
    with pytest.raises(X.NotSpanning) as ei:
        X.christofides(None, pk, n)
    assert ei.value.position == 3
    rc, *_ = gpu(ctx, None, pk, n)
    assert rc == TA._capi.TL_ERR_UNSUPPORTED
    msg = ctx.lib.tl_last_error(ctx.handle).decode()
    assert "tl_christofides" in msg and "position 3 " in msg
    check(ctx, O.synth_xy(n, seed=40), what="the context works afterwards")


@pytest.mark.parametrize("n", [1023, 1024, 1025, 182, 257])
def test_thread_and_tile_edges(ctx, n):
    """1 025: one thread of the tree's workgroup owns two cities.  256 columns and 16 rows make a pair tile."""
    check(ctx, O.synth_xy(n, seed=n), what=f"n={n}")
    check(ctx, O.synth_xy(n, seed=n), O.dm_build_packed(O.synth_xy(n, seed=n)), what=f"matrix n={n}")


@pytest.mark.parametrize("n", [1000, 2000])
def test_synthetic(ctx, n):
    check(ctx, O.synth_xy(n, seed=n), what=f"random n={n}")


@pytest.mark.parametrize("n", [10000, 13509, 30000])
def test_large_against_golden(ctx, golden_dir, n):
    """n = 30 000: Prim's key / parent arrays (6n bytes) no longer fit one workgroup's LDS and live in the workspace."""
    with open(os.path.join(golden_dir, "goldens_christofides.json")) as fh:
        g = json.load(fh)[f"synthetic{n}"]
    rc, route, cost, st = gpu(ctx, O.synth_xy(n))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert G.route_sha256(route) == g["route_sha256"]
    assert int(cost.view(np.uint32)) == g["cost_bits"] and f"{float(cost):.5f}" == g["cost"]
    assert 0 < st["candidates"] <= g["reference_examined"]
    print(f"n={n}: {st['sweeps']} bands, {st['candidates']} pairs examined, kernel {st['kernel_ms']:.1f} ms (tree {st['reversed'] / 1e6:.1f}), "
          f"call {st['total_ms']:.1f} ms")


def test_size_limit(ctx):
    import teeline_amd as TA
    rc, *_ = gpu(ctx, O.synth_xy(65536, seed=7))
    assert rc == TA._capi.TL_ERR_UNSUPPORTED
    msg = ctx.lib.tl_last_error(ctx.handle).decode()
    assert "tl_christofides" in msg and "65536" in msg and "65535" in msg


def test_greedy_edge_and_savings_are_unharmed(ctx):
    """The three constructions share kernels, workspace and context: tl_greedy_edge and tl_savings around a tl_christofides call
    return their unchanged tours."""
    from test_gpu_greedy_edge import gpu as greedy
    from test_gpu_savings import gpu as savings
    xy = O.synth_xy(257, seed=257)
    gw, sw = G.greedy_edge(xy), S.savings(xy)
    for _ in range(2):
        rc, r, c, _st = greedy(ctx, xy)
        assert rc == 0 and r.tolist() == gw[0].tolist() and c.tobytes() == np.float32(gw[1]).tobytes()
        rc, r, c, h, _st = savings(ctx, xy)
        assert rc == 0 and h == sw[2] and r.tolist() == sw[0].tolist() and c.tobytes() == np.float32(sw[1]).tobytes()
        check(ctx, xy, what="christofides between")


def _campaign(seconds, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "probes", "fuzz_campaign_christofides.py"), str(seconds)], env=env,
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) runs, (\d+) mismatches", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) >= 10, r.stdout[-3000:]


def test_jitter_build_campaign():
    """The randomized campaign on the race-stress build (-DTL_JITTER: waves leave every barrier far apart), in a child process."""
    lib = os.path.join(ROOT, "teeline_amd", "libteeline_gpu_jitter.so")
    assert os.path.exists(lib), "built by __graft_entry__.build()"
    _campaign(4, dict(os.environ, TEELINE_GPU_LIB=lib))


def test_product_campaign():
    _campaign(3)


def test_threads_own_contexts_and_busy_shared_context(golden_dir):
    import teeline_amd as TA
    xs = [O.synth_xy(1500, seed=s) for s in (11, 12)]
    want = [X.christofides(x) for x in xs]
    got, errs = [None, None], []

    def run(k):
        try:
            with TA.Context(0) as c:
                for _ in range(3):
                    rc, route, cost, _ = gpu(c, xs[k])
                    assert rc == 0 and route.tolist() == want[k][0].tolist()
                    assert cost.tobytes() == np.float32(want[k][1]).tobytes()
                got[k] = True
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    ts = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs and got == [True, True], errs
    # one shared context, two threads: every call returns the right result or TL_ERR_BUSY (nothing of the context touched), never
    # a wrong one, and the context works afterwards
    small = xs[0][:50].copy()
    small_want = X.christofides(small)
    with open(os.path.join(golden_dir, "goldens_christofides.json")) as fh:
        sha = json.load(fh)["synthetic13509"]["route_sha256"]
    with TA.Context(0) as c:
        big = O.synth_xy(13509)
        started, res = threading.Event(), {}

        def long_call():
            started.set()
            res["r"] = gpu(c, big)

        t = threading.Thread(target=long_call)
        t.start()
        started.wait()
        busy = 0
        while t.is_alive():
            rc, route, cost, _ = gpu(c, small)
            assert rc in (0, TA._capi.TL_ERR_BUSY)
            if rc == 0:
                assert route.tolist() == small_want[0].tolist() and cost.tobytes() == np.float32(small_want[1]).tobytes()
            busy += rc == TA._capi.TL_ERR_BUSY
        t.join()
        rc, route, *_ = res["r"]
        assert rc in (0, TA._capi.TL_ERR_BUSY)
        busy += rc == TA._capi.TL_ERR_BUSY
        assert busy >= 1, "the two threads never met inside the context"
        if rc == 0:
            assert G.route_sha256(route) == sha
        rc, route, *_ = gpu(c, big)
        assert rc == 0 and G.route_sha256(route) == sha


def test_python_solve_progress_and_pipeline(ctx, tsplib_dir):
    import teeline_amd as TA
    e = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))
    prob = TA.TspProblem(e["ids"], e["xy"])
    msgs = []
    sol = TA.christofides.solve(prob, None, lambda k, p: msgs.append((k, p)), [1, 2, 3], ctx=ctx)
    oroute, ocost = X.christofides(e["xy"])
    assert sol.route() == e["ids"][oroute].tolist() and np.float32(sol.total).tobytes() == np.float32(ocost).tobytes()
    assert [k for k, _ in msgs] == ["PathUpdate", "PathUpdate", "Done"]
    assert msgs[0][1] == (e["ids"].tolist(), 0.0) and msgs[1][1] == (sol.route(), float(sol.total)) and msgs[2][1] is None
    assert sol.stats["moves"] == 52 and sol.stats["prim_ms"] > 0
    small, msgs = TA.TspProblem([7, 9, 4], e["xy"][:3]), []  # n < 4: Done alone
    assert TA.christofides.solve(small, None, lambda k, p: msgs.append((k, p)), ctx=ctx).route() == [7, 9, 4] and msgs == [("Done", None)]
    # a GEO problem: every distance is the matrix's
    geo = TA.tsplib.read_from_file(os.path.join(tsplib_dir, "burma14.tsp")).problem()
    b = T.parse_tsplib(os.path.join(tsplib_dir, "burma14.tsp"))
    gr, gc = X.christofides(b["xy"], O.dm_build_packed(b["xy"], geo=True), 14)
    gsol = TA.christofides.solve(geo, ctx=ctx)
    assert gsol.route() == b["ids"][gr].tolist() and np.float32(gsol.total).tobytes() == np.float32(4033.0).tobytes() == np.float32(gc).tobytes()
    # pipelines: `solve chr` runs the construction alone; chr -> 2-opt and chr -> Or-opt against the table
    P = TA.pipeline
    assert P.steps_for_solve("chr") == ["chr"]
    for (steps, pins) in ((["chr", "2opt"], {"berlin52": "8128.74512", "a280": "2731.14819"}),
                          (["christofides", "or_opt"], {"berlin52": "8031.55029", "a280": "2668.86743"})):
        for name, pin in pins.items():
            p = TA.tsplib.read_from_file(os.path.join(tsplib_dir, f"{name}.tsp")).problem()
            out = P.run_pipeline_stages(p, steps, ctx=ctx)
            assert f"{float(out[-1].solution.total):.5f}" == pin, (steps, name)
    out = P.run_pipeline_stages(prob, ["chr", "2opt"], ctx=ctx)
    rc, r2, c2, _ = O.two_opt(e["xy"], None, 52, init=oroute)
    assert out[-1].solution.route() == e["ids"][r2].tolist()


@pytest.fixture(scope="module")
def cli():
    from teeline_amd import build
    return build.build_cli()


def _run_cli(cli, *args):
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr


def test_cli_solve_pipeline_and_listing(cli, tsplib_dir):
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    e = T.parse_tsplib(f)
    croute, _ = X.christofides(e["xy"])
    rc, r2, c2, _ = O.two_opt(e["xy"], None, 52, init=croute)
    ids_c, ids_2 = e["ids"][croute].tolist(), e["ids"][r2].tolist()
    line = lambda ids: "".join(f"{v} " for v in ids) + "\n"  # noqa: E731
    assert _run_cli(cli, "solve", "chr", "-i", f)[0] == "8707.66113 0\n" + line(ids_c)
    assert _run_cli(cli, "solve", "christofides", "-i", f)[0] == "8707.66113 0\n" + line(ids_c)
    out, err = _run_cli(cli, "pipeline", "--steps=christofides,2opt", "-i", f)
    assert out == "8128.74512 0\n" + line(ids_2) and "warning" not in err
    assert _run_cli(cli, "pipeline", "--steps=chr,2opt", "-i", f)[0] == "8128.74512 0\n" + line(ids_2)
    out, err = _run_cli(cli, "pipeline", "--steps=nn,chr", "-i", f)  # pipeline.rs:92-132 has no warning for christofides
    assert out == "8707.66113 0\n" + line(ids_c) and "warning" not in err
    out, _ = _run_cli(cli, "pipeline", "--steps=christofides,lk", "-i", f, "--epochs", "20")
    assert sorted(int(v) for v in out.splitlines()[1].split()) == sorted(e["ids"].tolist())
    assert float(out.split()[0]) <= 8707.66113
    j = json.loads(_run_cli(cli, "solve", "chr", "-i", f, "--output-format", "json")[0])
    assert j["route"] == ids_c and f"{j['cost']:.5f}" == "8707.66113" and j["optimized"] is False
    assert _run_cli(cli, "solvers", "--short")[0].split() == ["nn", "2opt", "3opt", "or-opt", "lk", "shuffle"]


def test_cli_progress_digest_matches_the_python_mirror(cli, ctx, tsplib_dir):
    import teeline_amd as TA
    from test_gpu_cli import _digest
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(f).problem()
    r = subprocess.run([cli, "solve", "chr", "-i", f, "--progress-digest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=([0-9a-f]{16})", r.stderr)
    assert m, r.stderr
    got = []
    TA.christofides.solve(prob, None, lambda kind, payload: got.append((kind, payload)), ctx=ctx)
    n, h = _digest(got)
    assert [int(m.group(1)), int(m.group(2)), int(m.group(3))] == n == [2, 0, 1]
    assert m.group(4) == f"{h:016x}"
