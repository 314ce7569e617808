"""Greedy-edge construction on the GPU (-m gpu): tl_greedy_edge against the numpy restatement tests/_greedy_oracle.py
(graph.rs:54-196, greedy_edge.rs:21-65 with the (i, j)-ascending tie rule) — route element for element, cost as bytes."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _greedy_oracle as G
import _oracle as O
import _tsplib as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(ctx, xy, packed=None, n=None):
    """tl_greedy_edge through the C ABI: (rc, route positions, cost, stats dict)."""
    import teeline_amd as TA
    n = len(xy) if n is None else n
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(max(n, 1), dtype=np.uint32)
    cost = C.c_float()
    st = TA._capi.TlStats()
    rc = ctx.lib.tl_greedy_edge(ctx.handle, xy.ctypes.data_as(C.c_void_p), None if packed is None else packed.ctypes.data_as(C.c_void_p),
                                n, out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(st))
    return rc, out[:n], np.float32(cost.value), st.as_dict()


def check(ctx, xy, packed=None, what=""):
    n = len(xy) if packed is None else int(round((1 + np.sqrt(1 + 8 * len(packed))) / 2))
    rc, route, cost, st = gpu(ctx, xy, packed, n)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    oroute, ocost, ost = G.greedy_edge(xy if packed is None else None, packed, n, with_stats=True)
    assert route.tolist() == oroute.tolist(), f"{what}: route differs"
    assert cost.tobytes() == np.float32(ocost).tobytes(), f"{what}: cost {cost!r} against {ocost!r}"
    if n > 2:
        # the bands hold only edges between cities of degree < 2: a subset of the edges the literal walk examines
        assert st["moves"] == n and st["sweeps"] >= 1 and 0 < st["candidates"] <= ost["examined"], (what, st, ost["examined"])
    return route, cost


@pytest.mark.parametrize("name", ["berlin52", "att48", "a280", "att532"])
def test_tsplib_coordinates(ctx, tsplib_dir, name):
    e = T.parse_tsplib(os.path.join(tsplib_dir, f"{name}.tsp"))
    route, cost = check(ctx, e["xy"], what=name)
    pins = {"berlin52": "9954.06250", "a280": "2960.47827"}  # docs/benchmarks.md 9 954.06; a280 decides ties
    if name in pins:
        assert f"{float(cost):.5f}" == pins[name]


@pytest.mark.parametrize("name", ["gr17", "bays29", "burma14", "ring6_explicit"])
def test_matrix_form(ctx, tsplib_dir, name):
    e = T.parse_tsplib(os.path.join(tsplib_dir, f"{name}.tsp"))
    packed = e["packed"] if e["packed"] is not None else O.dm_build_packed(e["xy"], geo=True)
    check(ctx, e["xy"], np.ascontiguousarray(packed, dtype=np.float32), what=name)


def test_small_n(ctx):
    rng = np.random.default_rng(1)
    for n in (3, 4, 5):
        for _ in range(5):
            check(ctx, (rng.random((n, 2)) * 100).astype(np.float32), what=f"n={n}")
    for n in (1, 2):
        xy = np.array([[0, 0], [3, 4]], dtype=np.float32)[:n]
        rc, route, cost, st = gpu(ctx, xy)
        assert rc == 0 and route.tolist() == list(range(n))
        assert cost.tobytes() == np.float32(0.0 if n == 1 else 10.0).tobytes()


def test_degenerate_inputs(ctx):
    rng = np.random.default_rng(2)
    dup = np.repeat((rng.random((40, 2)) * 50).astype(np.float32), 25, axis=0)       # 1 000 points, 40 places
    check(ctx, dup, what="duplicates")
    check(ctx, np.zeros((300, 2), dtype=np.float32), what="all equal")
    g = np.stack(np.meshgrid(np.arange(37), np.arange(29)), -1).reshape(-1, 2).astype(np.float32)
    check(ctx, g, what="lattice")
    t = np.sort(rng.random(700)).astype(np.float32) * 1000
    check(ctx, np.stack([t, 2 * t], 1).astype(np.float32), what="collinear")


def test_explicit_nan_negative_zero_inf(ctx):
    rng = np.random.default_rng(3)
    for n in (5, 17, 64, 300):
        m = n * (n - 1) // 2
        pk = rng.integers(1, 30, m).astype(np.float32)
        idx = rng.permutation(m)
        k = max(1, m // 10)
        pk[idx[:k]] = np.float32(np.nan)
        pk[idx[k:2 * k]] = np.float32(-0.0)
        pk[idx[2 * k:3 * k]] = np.float32(np.inf)
        pk[idx[3 * k:3 * k + 1]] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), dtype=np.float32)  # a negative NaN
        pk[idx[3 * k + 1:4 * k]] = np.float32(0.0)
        xy = np.zeros((n, 2), dtype=np.float32)
        check(ctx, xy, pk, what=f"explicit n={n}")


@pytest.mark.parametrize("n", [1000, 2000, 5000])
def test_synthetic(ctx, n):
    check(ctx, O.synth_xy(n, seed=n), what=f"random n={n}")
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n].astype(np.float32) * 3
    check(ctx, g, what=f"lattice n={n}")


@pytest.mark.parametrize("n", [10000, 13509])
def test_large_against_golden(ctx, golden_dir, n):
    with open(os.path.join(golden_dir, "goldens_greedy.json")) as fh:
        g = json.load(fh)[f"synthetic{n}"]
    rc, route, cost, st = gpu(ctx, O.synth_xy(n))
    assert rc == 0
    assert G.route_sha256(route) == g["route_sha256"]
    assert int(cost.view(np.uint32)) == g["cost_bits"] and f"{float(cost):.5f}" == g["cost"]
    assert 0 < st["candidates"] <= g["reference_examined"]


def test_size_limit(ctx):
    import teeline_amd as TA
    n = 65535
    xy = O.synth_xy(n, seed=7)
    rc, route, cost, st = gpu(ctx, xy)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert np.array_equal(np.sort(route), np.arange(n, dtype=np.uint32))
    c2 = C.c_float()
    assert ctx.lib.tl_tour_length(ctx.handle, xy.ctypes.data_as(C.c_void_p), None, n, route.ctypes.data_as(C.c_void_p), C.byref(c2)) == 0
    assert cost.tobytes() == np.float32(c2.value).tobytes()
    rc2, route2, cost2, _ = gpu(ctx, xy)
    assert rc2 == 0 and np.array_equal(route, route2) and cost.tobytes() == cost2.tobytes()
    print(f"n={n}: {st['sweeps']} bands, {st['candidates']} edges examined, kernel {st['kernel_ms']:.1f} ms")
    big = O.synth_xy(n + 1, seed=7)
    rc3, *_ = gpu(ctx, big)
    assert rc3 == TA._capi.TL_ERR_UNSUPPORTED


def test_jitter_build_campaign():
    """The randomized campaign on the race-stress build (-DTL_JITTER: waves leave every barrier far apart), in a child process."""
    lib = os.path.join(ROOT, "teeline_amd", "libteeline_gpu_jitter.so")
    assert os.path.exists(lib), "built by __graft_entry__.build()"
    env = dict(os.environ, TEELINE_GPU_LIB=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "probes", "fuzz_campaign_greedy.py"), "10"], env=env,
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    m = re.search(r"(\d+) runs, (\d+) mismatches", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) >= 10, r.stdout[-3000:]


def test_product_campaign():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "probes", "fuzz_campaign_greedy.py"), "8"],
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import re
    m = re.search(r"(\d+) runs, (\d+) mismatches", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) >= 10, r.stdout[-3000:]


def test_threads_own_contexts_and_busy_shared_context():
    import teeline_amd as TA
    xs = [O.synth_xy(3000, seed=s) for s in (11, 12)]
    want = [G.greedy_edge(x) for x in xs]
    got, errs = [None, None], []

    def run(k):
        try:
            with TA.Context(0) as c:
                for _ in range(3):
                    rc, route, cost, _ = gpu(c, xs[k])
                    assert rc == 0 and route.tolist() == want[k][0].tolist() and cost.tobytes() == np.float32(want[k][1]).tobytes()
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
    # a wrong one — whichever thread arrives second is refused — and the context works afterwards
    small = xs[0][:50].copy()
    small_want = G.greedy_edge(small)
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
        rc, route, _, _ = res["r"]
        assert rc in (0, TA._capi.TL_ERR_BUSY)
        busy += rc == TA._capi.TL_ERR_BUSY
        assert busy >= 1, "the two threads never met inside the context"
        with open(os.path.join(ROOT, "tests", "golden", "goldens_greedy.json")) as fh:
            sha = json.load(fh)["synthetic13509"]["route_sha256"]
        if rc == 0:
            assert G.route_sha256(route) == sha
        rc, route, _, _ = gpu(c, big)
        assert rc == 0 and G.route_sha256(route) == sha


def test_python_solve_progress_and_pipeline(ctx, tsplib_dir):
    import teeline_amd as TA
    e = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))
    prob = TA.TspProblem(e["ids"], e["xy"])
    msgs = []
    sol = TA.greedy_edge.solve(prob, None, lambda k, p: msgs.append((k, p)), [1, 2, 3], ctx=ctx)
    oroute, ocost = G.greedy_edge(e["xy"])
    assert sol.route() == e["ids"][oroute].tolist() and np.float32(sol.total).tobytes() == np.float32(ocost).tobytes()
    assert [k for k, _ in msgs] == ["PathUpdate", "PathUpdate", "Done"]
    assert msgs[0][1] == (e["ids"].tolist(), 0.0) and msgs[1][1] == (sol.route(), float(sol.total))
    small, msgs = TA.TspProblem([7, 9], e["xy"][:2]), []
    assert TA.greedy_edge.solve(small, None, lambda k, p: msgs.append((k, p)), ctx=ctx).route() == [7, 9] and msgs == [("Done", None)]
    # pipeline: `solve gec` runs greedy alone; greedy -> 2-opt gives the reference's 8 415.55
    P = TA.pipeline
    assert P.steps_for_solve("gec") == ["gec"] and P.steps_for_solve("greedy_edge") == ["greedy_edge"]
    out = P.run_pipeline_stages(prob, ["greedy_edge", "2opt"], ctx=ctx)
    rc, r2, c2, _ = O.two_opt(e["xy"], None, 52, init=oroute)
    assert f"{float(out[-1].solution.total):.5f}" == "8415.54980"
    assert out[-1].solution.route() == e["ids"][r2].tolist()


@pytest.fixture(scope="module")
def cli():
    from teeline_amd import build
    return build.build_cli()


def _run_cli(cli, *args):
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_solve_and_pipeline(cli, tsplib_dir):
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    e = T.parse_tsplib(f)
    groute, _ = G.greedy_edge(e["xy"])
    rc, r2, c2, _ = O.two_opt(e["xy"], None, 52, init=groute)
    ids_g, ids_2 = e["ids"][groute].tolist(), e["ids"][r2].tolist()
    line = lambda ids: "".join(f"{v} " for v in ids) + "\n"  # noqa: E731
    assert _run_cli(cli, "solve", "gec", "-i", f) == "9954.06250 0\n" + line(ids_g)
    assert _run_cli(cli, "solve", "greedy_edge", "-i", f) == "9954.06250 0\n" + line(ids_g)
    assert _run_cli(cli, "pipeline", "--steps=greedy_edge,2opt", "-i", f) == "8415.54980 0\n" + line(ids_2)
    assert _run_cli(cli, "pipeline", "--steps=gec,2opt", "-i", f) == "8415.54980 0\n" + line(ids_2)
    j = json.loads(_run_cli(cli, "solve", "gec", "-i", f, "--output-format", "json"))
    assert j["route"] == ids_g and f"{j['cost']:.5f}" == "9954.06250" and j["optimized"] is False
    opt = os.path.join(tsplib_dir, "berlin52.opt.tour")
    out = _run_cli(cli, "solve", "gec", "-i", f, "--optimal-tour", opt)
    assert out.startswith("9954.06250 0\n" + line(ids_g))


def test_cli_progress_digest_matches_the_python_mirror(cli, ctx, tsplib_dir):
    import re

    import teeline_amd as TA
    from test_gpu_cli import _digest
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(f).problem()
    r = subprocess.run([cli, "solve", "gec", "-i", f, "--progress-digest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=([0-9a-f]{16})", r.stderr)
    assert m, r.stderr
    got = []
    TA.greedy_edge.solve(prob, None, lambda kind, payload: got.append((kind, payload)), ctx=ctx)
    n, h = _digest(got)
    assert [int(m.group(1)), int(m.group(2)), int(m.group(3))] == n == [2, 0, 1]
    assert m.group(4) == f"{h:016x}"
