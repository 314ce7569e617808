"""Savings construction on the GPU (-m gpu): tl_savings against the numpy restatement tests/_savings_oracle.py (savings.rs:34-163
with the (i, j)-ascending tie rule and the NaN-below-every-number rule) — route element for element, cost and hub bit for bit."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import _greedy_oracle as G
import _oracle as O
import _savings_oracle as S
import _tsplib as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO = 0xFFFFFFFF


def gpu(ctx, xy, packed=None, n=None, hub=AUTO):
    """tl_savings through the C ABI: (rc, route positions, cost, hub used, stats dict).  xy None: a NULL pointer."""
    import teeline_amd as TA
    if xy is not None:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        n = len(xy) if n is None else n
    out = np.zeros(max(n, 1), dtype=np.uint32)
    cost, ghub = C.c_float(), C.c_uint32(0xDEADBEEF)
    st = TA._capi.TlStats()
    rc = ctx.lib.tl_savings(ctx.handle, None if xy is None else xy.ctypes.data_as(C.c_void_p),
                            None if packed is None else packed.ctypes.data_as(C.c_void_p), n, hub, out.ctypes.data_as(C.c_void_p),
                            C.byref(cost), C.byref(ghub), C.byref(st))
    return rc, out[:n], np.float32(cost.value), ghub.value, st.as_dict()


def check(ctx, xy, packed=None, hub=None, what=""):
    n = len(xy) if packed is None else int(round((1 + np.sqrt(1 + 8 * len(packed))) / 2))
    rc, route, cost, ghub, st = gpu(ctx, xy, packed, n, AUTO if hub is None else hub)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    oroute, ocost, ohub, ost = S.savings(xy, packed, n, hub=hub, chunk=4096, with_stats=True)
    assert ghub == ohub, f"{what}: hub {ghub} against {ohub}"
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
    pins = {"berlin52": "8378.97363", "a280": "2882.62842", "att532": "95440.24219"}
    if name in pins:
        assert f"{float(cost):.5f}" == pins[name]


@pytest.mark.parametrize("name", ["gr17", "bays29", "burma14", "ulysses22", "ring6_explicit"])
def test_matrix_form(ctx, tsplib_dir, name):
    """GEO and EXPLICIT give negative savings (hub pairs are not last); the hub still comes from the coordinates the problem carries."""
    e = T.parse_tsplib(os.path.join(tsplib_dir, f"{name}.tsp"))
    packed = e["packed"] if e["packed"] is not None else O.dm_build_packed(e["xy"], geo=True)
    check(ctx, e["xy"], np.ascontiguousarray(packed, dtype=np.float32), what=name)


def test_small_n_and_every_hub_of_three(ctx):
    rng = np.random.default_rng(1)
    for n in (3, 4, 5):
        for _ in range(5):
            check(ctx, (rng.random((n, 2)) * 100).astype(np.float32), what=f"n={n}")
    tri = np.array([[0, 0], [3, 4], [10, 1]], dtype=np.float32)
    for hub in (0, 1, 2):
        check(ctx, tri, hub=hub, what=f"n=3 hub={hub}")
        check(ctx, tri, O.dm_build_packed(tri), hub=hub, what=f"n=3 matrix hub={hub}")
    for n in (0, 1, 2):
        xy = np.array([[0, 0], [3, 4]], dtype=np.float32)[:n]
        rc, route, cost, ghub, st = gpu(ctx, xy, n=n)
        assert rc == 0 and route.tolist() == list(range(n)) and ghub == 0 == S.savings(xy, n=n)[2]
        assert cost.tobytes() == np.float32(10.0 if n == 2 else 0.0).tobytes()


def test_explicit_hub(ctx):
    xy = O.synth_xy(64, seed=64)
    pk = O.dm_build_packed(xy)
    for hub in (0, 63, 31):
        check(ctx, xy, hub=hub, what=f"hub={hub}")
        check(ctx, xy, pk, hub=hub, what=f"matrix hub={hub}")
    # with a matrix and an explicit hub the coordinates are not needed at all
    rc, route, cost, ghub, _ = gpu(ctx, None, pk, 64, hub=31)
    want = S.savings(xy, pk, 64, hub=31)
    assert rc == 0 and ghub == 31 and route.tolist() == want[0].tolist() and cost.tobytes() == np.float32(want[1]).tobytes()


def test_bad_arguments(ctx):
    import teeline_amd as TA
    xy = O.synth_xy(64, seed=64)
    pk = O.dm_build_packed(xy)
    rc, *_ = gpu(ctx, xy, hub=64)
    assert rc == TA._capi.TL_ERR_BADARG and b"hub=64" in ctx.lib.tl_last_error(ctx.handle)
    rc, *_ = gpu(ctx, xy, hub=0xFFFFFFFE)
    assert rc == TA._capi.TL_ERR_BADARG
    rc, *_ = gpu(ctx, None, pk, 64, hub=AUTO)   # AUTO needs the coordinates
    assert rc == TA._capi.TL_ERR_BADARG
    rc, *_ = gpu(ctx, None, None, 64, hub=3)    # no matrix: the distances need them
    assert rc == TA._capi.TL_ERR_BADARG
    check(ctx, xy, what="the context works afterwards")


@pytest.mark.parametrize("n", [16, 17, 181, 182, 255, 256, 257])
def test_band_and_tile_edges(ctx, n):
    """n(n-1)/2 crosses one band of 16 384 keys between 181 and 182; 256 columns and 16 rows make a pair tile."""
    check(ctx, O.synth_xy(n, seed=n), what=f"n={n}")
    check(ctx, O.synth_xy(n, seed=n), O.dm_build_packed(O.synth_xy(n, seed=n)), what=f"matrix n={n}")


def test_massive_ties(ctx):
    check(ctx, np.zeros((300, 2), dtype=np.float32), what="all equal")  # 44 850 keys of +0.0: the threshold refines into i / j
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(np.float32)
    check(ctx, g, what="lattice")
    t = (np.arange(300, dtype=np.float32) - 150) * 7
    line = np.stack([t, 2 * t], 1).astype(np.float32)
    assert S.hub_position(line) in (149, 150)
    check(ctx, line, what="collinear, hub in the middle")


def test_explicit_inf_nan_negative_zero(ctx):
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
        pk[idx[4 * k:4 * k + k // 2]] = np.float32(-np.inf)
        xy = np.stack(np.meshgrid(np.arange(n), np.arange(1)), -1).reshape(-1, 2).astype(np.float32)
        for hub in (None, 0, n - 1):
            check(ctx, xy, pk, hub=hub, what=f"explicit n={n} hub={hub}")
    # inf entries alone: inf - inf savings, the NaN this device makes is positive, x86's is negative — one rule for both
    for n in (24, 100):
        m = n * (n - 1) // 2
        pk = rng.integers(1, 30, m).astype(np.float32)
        pk[rng.permutation(m)[:m // 4]] = np.float32(np.inf)
        check(ctx, np.zeros((n, 2), dtype=np.float32), pk, hub=0, what=f"inf matrix n={n}")


def test_coordinates_with_inf(ctx):
    xy = O.synth_xy(100, seed=4).copy()
    xy[7, 0] = np.float32(np.inf)
    xy[50, 1] = np.float32(-np.inf)
    assert S.hub_position(xy) == 0
    check(ctx, xy, what="inf coordinates")
    check(ctx, xy, hub=7, what="inf coordinates, the hub is one of them")  # dh is inf everywhere but +0.0 at the hub


def test_subnormal_savings_are_not_flushed(ctx):
    rng = np.random.default_rng(6)
    n = 64
    m = n * (n - 1) // 2
    pk = (1e-38 + rng.random(m) * 2e-38).astype(np.float32)
    dh = S.hub_distances(pk, n, 0)
    s = np.concatenate([(dh[:j] + dh[j]) - pk[j * (j - 1) // 2: j * (j - 1) // 2 + j] for j in range(1, n)])
    tiny = np.abs(s[s != 0]) < np.float32(1.17549435e-38)
    assert tiny.sum() > 100, "the instance has no subnormal savings"
    xy = np.zeros((n, 2), dtype=np.float32)
    check(ctx, xy, pk, hub=0, what="subnormal savings")
    # flushed to zero they would all tie and fall to the (i, j) order: another tour
    flushed = np.where(np.abs(pk) < np.float32(1.17549435e-38), np.float32(0.0), pk)
    assert S.savings(xy, flushed, n, hub=0)[0].tolist() != S.savings(xy, pk, n, hub=0)[0].tolist()


@pytest.mark.parametrize("n", [1000, 2000, 5000])
def test_synthetic(ctx, n):
    check(ctx, O.synth_xy(n, seed=n), what=f"random n={n}")


@pytest.mark.parametrize("n", [10000, 13509])
def test_large_against_golden(ctx, golden_dir, n):
    with open(os.path.join(golden_dir, "goldens_savings.json")) as fh:
        g = json.load(fh)[f"synthetic{n}"]
    rc, route, cost, ghub, st = gpu(ctx, O.synth_xy(n))
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle).decode()
    assert ghub == g["hub"]
    assert G.route_sha256(route) == g["route_sha256"]
    assert int(cost.view(np.uint32)) == g["cost_bits"] and f"{float(cost):.5f}" == g["cost"]
    assert 0 < st["candidates"] <= g["reference_examined"]
    print(f"n={n}: {st['sweeps']} bands, {st['candidates']} edges examined, kernel {st['kernel_ms']:.1f} ms")


def test_size_limit(ctx):
    import teeline_amd as TA
    rc, *_ = gpu(ctx, O.synth_xy(65536, seed=7))
    assert rc == TA._capi.TL_ERR_UNSUPPORTED
    msg = ctx.lib.tl_last_error(ctx.handle).decode()
    assert "tl_savings" in msg and "65536" in msg and "65535" in msg


def test_greedy_edge_is_unharmed(ctx):
    """The two constructions share kernels, workspace and context: tl_greedy_edge around a tl_savings call returns the same tour."""
    from test_gpu_greedy_edge import gpu as greedy
    xy = O.synth_xy(257, seed=257)
    want = G.greedy_edge(xy)
    rc, r0, c0, _ = greedy(ctx, xy)
    assert rc == 0 and r0.tolist() == want[0].tolist() and c0.tobytes() == np.float32(want[1]).tobytes()
    check(ctx, xy, what="savings between")
    rc, r1, c1, _ = greedy(ctx, xy)
    assert rc == 0 and r1.tolist() == r0.tolist() and c1.tobytes() == c0.tobytes()


def _campaign(seconds, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "probes", "fuzz_campaign_savings.py"), str(seconds)], env=env,
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) runs, (\d+) mismatches", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) >= 10, r.stdout[-3000:]


def test_jitter_build_campaign():
    """The randomized campaign on the race-stress build (-DTL_JITTER: waves leave every barrier far apart), in a child process."""
    lib = os.path.join(ROOT, "teeline_amd", "libteeline_gpu_jitter.so")
    assert os.path.exists(lib), "built by __graft_entry__.build()"
    _campaign(5, dict(os.environ, TEELINE_GPU_LIB=lib))


def test_product_campaign():
    _campaign(4)


def test_threads_own_contexts_and_busy_shared_context(golden_dir):
    import teeline_amd as TA
    xs = [O.synth_xy(2000, seed=s) for s in (11, 12)]
    want = [S.savings(x, chunk=4096) for x in xs]
    got, errs = [None, None], []

    def run(k):
        try:
            with TA.Context(0) as c:
                for _ in range(3):
                    rc, route, cost, ghub, _ = gpu(c, xs[k])
                    assert rc == 0 and ghub == want[k][2] and route.tolist() == want[k][0].tolist()
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
    small_want = S.savings(small)
    with open(os.path.join(golden_dir, "goldens_savings.json")) as fh:
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
            rc, route, cost, _, _ = gpu(c, small)
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
    sol = TA.savings.solve(prob, None, lambda k, p: msgs.append((k, p)), [1, 2, 3], ctx=ctx)
    oroute, ocost, ohub = S.savings(e["xy"])
    assert sol.route() == e["ids"][oroute].tolist() and np.float32(sol.total).tobytes() == np.float32(ocost).tobytes()
    assert sol.stats["hub"] == ohub == 36
    assert [k for k, _ in msgs] == ["PathUpdate", "PathUpdate", "Done"]
    assert msgs[0][1] == (e["ids"].tolist(), 0.0) and msgs[1][1] == (sol.route(), float(sol.total)) and msgs[2][1] is None
    small, msgs = TA.TspProblem([7, 9], e["xy"][:2]), []
    assert TA.savings.solve(small, None, lambda k, p: msgs.append((k, p)), ctx=ctx).route() == [7, 9] and msgs == [("Done", None)]
    # a GEO problem: the edges are the matrix's, the hub the raw coordinates'
    geo = TA.tsplib.read_from_file(os.path.join(tsplib_dir, "burma14.tsp")).problem()
    b = T.parse_tsplib(os.path.join(tsplib_dir, "burma14.tsp"))
    gr, gc, gh = S.savings(b["xy"], O.dm_build_packed(b["xy"], geo=True), 14)
    gsol = TA.savings.solve(geo, ctx=ctx)
    assert gsol.route() == b["ids"][gr].tolist() and gsol.stats["hub"] == gh and np.float32(gsol.total).tobytes() == np.float32(gc).tobytes()
    # pipeline: `solve sav` runs savings alone; savings -> 2-opt
    P = TA.pipeline
    assert P.steps_for_solve("sav") == ["sav"] and P.steps_for_solve("savings") == ["savings"]
    out = P.run_pipeline_stages(prob, ["savings", "2opt"], ctx=ctx)
    rc, r2, c2, _ = O.two_opt(e["xy"], None, 52, init=oroute)
    assert f"{float(out[-1].solution.total):.5f}" == "8040.27637"
    assert out[-1].solution.route() == e["ids"][r2].tolist()


@pytest.fixture(scope="module")
def cli():
    from teeline_amd import build
    return build.build_cli()


def _run_cli(cli, *args):
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr


def test_cli_solve_pipeline_warning_and_listing(cli, tsplib_dir):
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    e = T.parse_tsplib(f)
    sroute, _, _ = S.savings(e["xy"])
    rc, r2, c2, _ = O.two_opt(e["xy"], None, 52, init=sroute)
    ids_s, ids_2 = e["ids"][sroute].tolist(), e["ids"][r2].tolist()
    line = lambda ids: "".join(f"{v} " for v in ids) + "\n"  # noqa: E731
    assert _run_cli(cli, "solve", "sav", "-i", f)[0] == "8378.97363 0\n" + line(ids_s)
    assert _run_cli(cli, "solve", "savings", "-i", f)[0] == "8378.97363 0\n" + line(ids_s)
    out, err = _run_cli(cli, "pipeline", "--steps=savings,2opt", "-i", f)
    assert out == "8040.27637 0\n" + line(ids_2) and "warning" not in err
    assert _run_cli(cli, "pipeline", "--steps=sav,2opt", "-i", f)[0] == "8040.27637 0\n" + line(ids_2)
    out, err = _run_cli(cli, "pipeline", "--steps=nn,savings", "-i", f)
    assert out == "8378.97363 0\n" + line(ids_s)
    assert "warning: savings at stage 1 discards the warm-start seed from the previous stage (it always rebuilds from scratch)\n" in err
    j = json.loads(_run_cli(cli, "solve", "sav", "-i", f, "--output-format", "json")[0])
    assert j["route"] == ids_s and f"{j['cost']:.5f}" == "8378.97363" and j["optimized"] is False
    assert _run_cli(cli, "solvers", "--short")[0].split() == ["nn", "2opt", "3opt", "or-opt", "lk", "shuffle"]


def test_cli_progress_digest_matches_the_python_mirror(cli, ctx, tsplib_dir):
    import teeline_amd as TA
    from test_gpu_cli import _digest
    f = os.path.join(tsplib_dir, "berlin52.tsp")
    prob = TA.tsplib.read_from_file(f).problem()
    r = subprocess.run([cli, "solve", "sav", "-i", f, "--progress-digest"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = re.search(r"progress: path_updates=(\d+) city_changes=(\d+) done=(\d+) digest=([0-9a-f]{16})", r.stderr)
    assert m, r.stderr
    got = []
    TA.savings.solve(prob, None, lambda kind, payload: got.append((kind, payload)), ctx=ctx)
    n, h = _digest(got)
    assert [int(m.group(1)), int(m.group(2)), int(m.group(3))] == n == [2, 0, 1]
    assert m.group(4) == f"{h:016x}"
