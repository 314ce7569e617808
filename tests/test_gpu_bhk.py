"""The Bellman-Held-Karp exact solver on the GPU (-m gpu): tl_bellman_karp against the numpy restatement tests/_bhk_oracle.py
(bellman_karp.rs:24-165) — route element for element, out_cost byte for byte, out_optimal with == (the sign of a zero is the one
thing the parallel minimum may change), is_tour and the stats formulas exactly; both walks."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _bhk_oracle as B
import _oracle as O
import _tsplib as T
from test_bhk_oracle import PINNED, matrix_of, pinned
from test_christofides_oracle import all_equal, signed_zeros

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(ctx, xy, packed=None, n=None):
    """tl_bellman_karp through the C ABI: (rc, route positions, cost, optimal, is_tour, stats dict).  xy None: a NULL pointer."""
    import teeline_amd as TA
    if xy is not None:
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        n = len(xy) if n is None else n
    out = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    cost, optimal, ok = C.c_float(-1.0), C.c_float(-1.0), C.c_uint32(7)
    st = TA._capi.TlStats()
    rc = ctx.lib.tl_bellman_karp(ctx.handle, None if xy is None else xy.ctypes.data_as(C.c_void_p),
                                 None if packed is None else packed.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p),
                                 C.byref(cost), C.byref(optimal), C.byref(ok), C.byref(st))
    return rc, out[:n], np.float32(cost.value), np.float32(optimal.value), int(ok.value), st.as_dict()


@pytest.fixture(scope="module")
def xctx():
    """A context whose walk is the exact one (TL_FLAG_BHK_EXACT_WALK)."""
    import teeline_amd as TA
    c = TA.Context(0, TA._capi.TL_FLAG_BHK_EXACT_WALK)
    yield c
    c.close()


def same(got, want, n, what):
    rc, route, cost, optimal, ok, st = got
    wroute, wcost, woptimal, wok = want
    assert rc == 0, what
    assert route.tolist() == [int(v) for v in wroute], f"{what}: route differs"
    assert cost.tobytes() == np.float32(wcost).tobytes(), f"{what}: cost {cost!r} against {wcost!r}"
    assert optimal == np.float32(woptimal), f"{what}: optimal {optimal!r} against {woptimal!r}"
    assert ok == wok, f"{what}: is_tour"
    k = n - 1
    assert st["sweeps"] == max(0, k - 1) and st["moves"] == n, (what, st)
    assert st["candidates"] == (k * (k - 1) * 2 ** (k - 2) if k >= 2 else 0), (what, st)
    if n >= 2:
        assert st["kernel_ms"] > 0 and st["reversed"] / 1e6 <= st["kernel_ms"] <= st["total_ms"], (what, st)


def check(ctx, xctx, xy, packed=None, n=None, what="", want=None):
    """Both walks against the oracle (one table serves both)."""
    n = (len(xy) if n is None else n)
    ref, ex = want or B.both(xy, packed, n)
    same(gpu(ctx, xy, packed, n), ref, n, what)
    same(gpu(xctx, xy, packed, n), ex, n, what + " (exact walk)")
    return ref, ex


def test_small_sizes_and_no_layer_cases(ctx, xctx):
    xy = np.array([[0, 0], [3, 4], [3, 0], [9, 9]], dtype=np.float32)
    for c in (ctx, xctx):
        rc, route, cost, optimal, ok, st = gpu(c, xy[:0], n=0)          # nothing written but the cost
        assert rc == 0 and cost == np.float32(0.0) and st["sweeps"] == 0 and st["moves"] == 0
        assert gpu(c, None, None, 0)[0] == 0
        rc, route, cost, optimal, ok, st = gpu(c, xy[:1])               # the fold is empty, the walk does not run
        assert rc == 0 and route.tolist() == [0] and cost == np.float32(0.0) and optimal == B.F32_MAX and ok == 1
    for n in (1, 2, 3, 4):                                              # k = 1: no layer; k = 2: one
        check(ctx, xctx, xy[:n], what=f"n={n}")
        pk = O.dm_build_packed(xy[:n]) if n >= 2 else np.zeros(1, np.float32)
        check(ctx, xctx, xy[:n], pk, n, what=f"matrix n={n}")
        check(ctx, xctx, None, pk, n, what=f"matrix alone n={n}", want=B.both(xy[:n], pk, n))
    assert gpu(ctx, xy[:2])[1].tolist() == [1, 0] and gpu(ctx, xy[:2])[2] == np.float32(10.0)
    check(ctx, xctx, np.zeros((2, 2), np.float32), what="two cities at one point")   # optimal 0: the walk stops before its first step
    rng = np.random.default_rng(1)
    for n in (3, 4, 5, 6, 7):
        p = (rng.random((n, 2)) * 100).astype(np.float32)
        check(ctx, xctx, p, what=f"random n={n}")


@pytest.mark.parametrize("name", PINNED)
def test_pinned_instances(ctx, xctx, name):
    xy, pk, n, optimal, total, route = pinned()[name]
    ref, ex = check(ctx, xctx, xy, pk, n, what=name)
    assert ref[0].tolist() == [int(v) for v in route.split()] and f"{float(ref[2]):.5f}" == optimal and f"{float(ref[1]):.5f}" == total
    if pk is not None:  # with a matrix the coordinates are not needed at all
        same(gpu(ctx, None, pk, n), ref, n, name + ", xy NULL")


def _golden_walks(g):
    w = lambda e, o: (e["route"], np.uint32(e["cost_bits"]).view(np.float32), o, e["is_tour"])  # noqa: E731
    o = np.uint32(g["optimal_bits"]).view(np.float32)
    return w(g["reference_walk"], o), w(g["exact_walk"], o)


def test_ulysses22_against_golden(ctx, xctx, tsplib_dir, golden_dir):
    """The largest parity case: k = 21, a table of 2^21 rows = 268 MB."""
    with open(os.path.join(golden_dir, "goldens_bhk.json")) as fh:
        g = json.load(fh)["ulysses22"]
    e = T.parse_tsplib(os.path.join(tsplib_dir, "ulysses22.tsp"))
    ref, ex = check(ctx, xctx, e["xy"], matrix_of(e), 22, what="ulysses22", want=_golden_walks(g))
    assert f"{float(ref[2]):.5f}" == "7013.00000"


def test_berlin23_against_golden(ctx, xctx, tsplib_dir, golden_dir):
    with open(os.path.join(golden_dir, "goldens_bhk.json")) as fh:
        g = json.load(fh)["berlin23"]
    xy = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))["xy"][:23]
    ref, ex = check(ctx, xctx, xy, what="berlin52[:23]", want=_golden_walks(g))
    assert f"{float(ref[2]):.5f}" == "5347.82373" and f"{float(ref[1]):.5f}" == "5347.82422"


@pytest.mark.parametrize("n", [16, 17, 18])
def test_half_wave_boundary(ctx, xctx, n):
    """Two subsets share a wave, one per half; k = 15, 16, 17 puts the last city of a subset on the last lane below, at and above
    the 16-lane mark of a half."""
    rng = np.random.default_rng(n)
    xy = (rng.random((n, 2)) * 1000).astype(np.float32)
    check(ctx, xctx, xy, what=f"random n={n}")


def test_seeded_campaign_and_its_one_result_that_is_no_tour(ctx, xctx):
    bad = []
    for k, xy in enumerate(B.campaign()):
        ref, ex = check(ctx, xctx, xy, what=f"campaign {k}")
        assert ex[3] == 1
        if not ref[3]:
            bad.append(k)
            rc, route, cost, optimal, ok, st = gpu(ctx, xy)   # TL_OK all the same, the oracle's positions and cost
            assert rc == 0 and ok == 0 and route.tolist() == ref[0].tolist() and cost.tobytes() == ref[1].tobytes()
            assert sorted(route.tolist()) != list(range(len(xy)))
    assert len(bad) == 1


def test_ties_zeros_negative_nan_and_max_entries(ctx, xctx):
    for n in (6, 12):
        xy, pk = all_equal(n)
        check(ctx, xctx, xy, pk, n, what=f"all-equal matrix n={n}")
    stopped = 0
    for n in (8, 12, 16):  # negative entries, left <= 0.0 ending the walk early, zeros of both signs in the table
        xy, pk = signed_zeros(n)
        ref, ex = check(ctx, xctx, xy, pk, n, what=f"signed zeros n={n}")
        stopped += int(not ref[3])
    assert stopped >= 1, "no walk of these matrices ended early"
    rng = np.random.default_rng(9)
    base = rng.integers(1, 50, 36).astype(np.float32)
    for bad in (np.float32(np.nan), B.F32_MAX):
        for where in (3, 17, 30):
            pk = base.copy()
            pk[where] = bad
            check(ctx, xctx, None, pk, 9, what=f"n=9 with {bad!r} at {where}", want=B.both(None, pk, 9))
    pk = np.full(36, np.float32(np.nan))  # no finite tour at all: optimal stays f32::MAX, both contexts return the reference walk
    ref, ex = check(ctx, xctx, None, pk, 9, what="all NaN", want=B.both(None, pk, 9))
    assert ref[2] == B.F32_MAX and ex[0].tolist() == ref[0].tolist()


def _free_bytes():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_the_limit(tsplib_dir):
    """n = 27 is refused before anything is allocated: a fresh context's workspace would have to grow by the 8 GiB table."""
    import teeline_amd as TA
    xy = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))["xy"][:27]
    with TA.Context(0) as c:
        assert gpu(c, xy[:5])[0] == 0
        before = _free_bytes()
        rc = gpu(c, xy)[0]
        after = _free_bytes()
        assert rc == TA._capi.TL_ERR_UNSUPPORTED
        msg = c.lib.tl_last_error(c.handle).decode()
        assert "tl_bellman_karp" in msg and "n=27" in msg and "26" in msg
        assert before - after < (1 << 32), "the refused call allocated"
        assert gpu(c, None, O.dm_build_packed(xy), 27)[0] == TA._capi.TL_ERR_UNSUPPORTED
        rc, route, *_ = gpu(c, xy[:5])
        assert rc == 0 and sorted(route.tolist()) == [0, 1, 2, 3, 4]


def test_top_of_the_range_on_a_circle():
    """n = 26, the exact walk: 2^25 rows of 128 bytes = 4 GiB, so a row's byte offset needs more than 32 bits from k = 25 on.  26
    points in strictly convex position (a circle of radius 1000, irregular gaps between 0.5 and 1.5 times the mean): the optimum is
    the hull order, unique up to direction, so no oracle run is needed."""
    import teeline_amd as TA
    n = 26
    rng = np.random.default_rng(26)
    gaps = rng.uniform(0.5, 1.5, n)
    ang = np.cumsum(gaps) / gaps.sum() * 2 * np.pi
    assert np.all(np.diff(ang) > 0)
    xy = np.ascontiguousarray(1000.0 * np.stack([np.cos(ang), np.sin(ang)], 1), dtype=np.float32)
    with TA.Context(0, TA._capi.TL_FLAG_BHK_EXACT_WALK) as c:
        rc, route, cost, optimal, ok, st = gpu(c, xy)
        assert rc == 0, c.lib.tl_last_error(c.handle).decode()
        print(f"n=26: kernel {st['kernel_ms']:.1f} ms (layers {st['reversed'] / 1e6:.1f}), call {st['total_ms']:.1f} ms")
        assert ok == 1 and route[0] == 25
        assert route.tolist() in ([25] + list(range(25)), [25] + list(range(24, -1, -1)))
        want = C.c_float()
        assert c.lib.tl_tour_length(c.handle, xy.ctypes.data_as(C.c_void_p), None, n, route.ctypes.data_as(C.c_void_p), C.byref(want)) == 0
        assert cost.tobytes() == np.float32(want.value).tobytes()
        assert abs(float(optimal) - float(cost)) <= 1e-4 * float(cost)
        assert st["sweeps"] == 24 and st["candidates"] == 25 * 24 * 2 ** 23 and st["moves"] == 26


@pytest.fixture(scope="module")
def cli():
    from teeline_amd import build
    return build.build_cli()


def _run_cli(cli, *args):
    r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr


def test_cli_solve_and_pipeline(cli, tsplib_dir):
    line = lambda ids: "".join(f"{v} " for v in ids) + "\n"  # noqa: E731
    pins = {"burma14": ("3323.00000", "13 1 0 9 8 10 7 12 6 11 5 4 3 2"), "gr17": ("2085.00000", "16 5 7 6 12 3 0 15 11 8 4 1 9 10 2 14 13")}
    for name, (cost, route) in pins.items():
        f = os.path.join(tsplib_dir, f"{name}.tsp")
        ids = T.parse_tsplib(f)["ids"][[int(v) for v in route.split()]].tolist()
        want = f"{cost} 0\n" + line(ids)
        out, err = _run_cli(cli, "pipeline", "--steps=bhk", "-i", f)
        assert out == want and "warning" not in err
        out, err = _run_cli(cli, "solve", "bhk", "-i", f, "--stats")     # no nn stage in front (mod.rs:2137)
        assert out == want and err.count("stage ") == 1 and "stage bellman_karp:" in err
        assert _run_cli(cli, "solve", "bellman_karp", "-i", f)[0] == want
        out, err = _run_cli(cli, "pipeline", "--steps=nn,2opt,bhk", "-i", f)  # the seed is ignored
        assert out == want
        out, err = _run_cli(cli, "pipeline", "--steps=bhk,2opt", "-i", f)     # pipeline.rs:112-118
        assert "BellmanKarp at stage 0 ignores the warm-start seed" in err
        xout, _ = _run_cli(cli, "solve", "bhk", "--exact-walk", "-i", f)
        assert xout.split()[0] == cost and sorted(int(v) for v in xout.splitlines()[1].split()) == sorted(ids)
    assert _run_cli(cli, "solve", "bhk", "-i", os.path.join(tsplib_dir, "burma14.tsp"))[0] == \
        "3323.00000 0\n14 2 1 10 9 11 8 13 7 12 6 5 4 3 \n"
    r = subprocess.run([cli, "solve", "bhk", "-i", os.path.join(tsplib_dir, "berlin52.tsp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "TL_BHK_MAX_N" in r.stderr and r.stdout == ""


def test_python_solve_progress_and_pipeline(ctx, tsplib_dir):
    import teeline_amd as TA
    e = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))
    prob = TA.TspProblem(e["ids"][:12], e["xy"][:12])
    ref, ex = B.both(e["xy"][:12])
    msgs = []
    sol = TA.bellman_karp.solve(prob, None, lambda k, p: msgs.append((k, p)), [1, 2, 3], ctx=ctx)
    assert sol.route() == e["ids"][ref[0]].tolist() and np.float32(sol.total).tobytes() == ref[1].tobytes()
    assert sol.stats["optimal"] == ref[2] and sol.stats["is_tour"] == 1 and sol.stats["sweeps"] == 10 and sol.stats["layers_ms"] > 0
    assert f"{float(sol.stats['optimal']):.5f}" == "4056.68066" and f"{float(sol.total):.5f}" == "4056.68091"
    # bellman_karp.rs:48-52, :81-84: k CityChanges in position order, PathUpdate(route, 0.0), Done
    assert [k for k, _ in msgs] == ["CityChange"] * 11 + ["PathUpdate", "Done"]
    assert [p for k, p in msgs[:11]] == e["ids"][:11].tolist() and msgs[11][1] == (sol.route(), 0.0) and msgs[12][1] is None
    xsol = TA.bellman_karp.solve(prob, ctx=ctx, exact_walk=True)
    assert xsol.route() == e["ids"][ex[0]].tolist() and np.float32(xsol.total).tobytes() == ex[1].tobytes() and xsol.stats["is_tour"] == 1
    P = TA.pipeline
    assert P.steps_for_solve("bhk") == ["bhk"]
    for name, pin in (("burma14", "3323.00000"), ("gr17", "2085.00000")):
        p = TA.tsplib.read_from_file(os.path.join(tsplib_dir, f"{name}.tsp")).problem()
        out = P.run_pipeline_stages(p, ["bhk"], ctx=ctx)
        assert f"{float(out[-1].solution.total):.5f}" == pin
        seeded = P.run_pipeline_stages(p, ["nn", "2opt", "bellman_karp"], ctx=ctx)
        assert seeded[-1].solution.route() == out[-1].solution.route()
    # the campaign's one result that is no tour: the pipeline refuses it, as the reference's does; the exact walk passes
    for xy in B.campaign():
        if not B.bellman_karp(xy)[3]:
            break
    bad = TA.TspProblem(np.arange(1, len(xy) + 1), xy)
    assert TA.bellman_karp.solve(bad, ctx=ctx).stats["is_tour"] == 0
    with pytest.raises(RuntimeError, match="invalid tour"):
        P.run_pipeline_stages(bad, ["bhk"], ctx=ctx)
    assert TA.validate_tour(P.run_pipeline_stages(bad, ["bhk"], ctx=ctx, exact_walk=True)[-1].solution.route(), bad)


def test_no_heuristic_beats_the_optimum(ctx, xctx, tsplib_dir):
    """nn -> 2opt -> or_opt through the existing entries never costs less than the exact walk's tour."""
    import teeline_amd as TA
    b52 = T.parse_tsplib(os.path.join(tsplib_dir, "berlin52.tsp"))
    probs = [TA.tsplib.read_from_file(os.path.join(tsplib_dir, f"{name}.tsp")).problem() for name in ("burma14", "gr17", "ulysses22")]
    probs += [TA.TspProblem(b52["ids"][:m], b52["xy"][:m]) for m in (12, 16, 20)]
    for p in probs:
        exact = TA.bellman_karp.solve(p, ctx=xctx)
        assert exact.stats["is_tour"] == 1
        heur = TA.pipeline.run_pipeline_stages(p, ["nn", "2opt", "or_opt"], ctx=ctx)[-1].solution
        assert float(heur.total) >= float(exact.total), (len(p), heur.total, exact.total)
