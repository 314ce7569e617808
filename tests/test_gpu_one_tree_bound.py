"""tl_one_tree_bound on the device (-m gpu) against tests/_one_tree_oracle.py, bit for bit: bound, best_iter, iterations run, stop
reason, is_tour and tour, pi, parents, root neighbours and every log row."""
import functools

import numpy as np
import pytest

import _one_tree_cases as K
import _one_tree_oracle as H

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def instance(name):
    """(xy, packed, n, upper): upper is the nearest-neighbour tour's length unless the case says otherwise."""
    kind, _, arg = name.partition(":")
    if kind == "rand":
        n = int(arg)
        xy, pk = K.random_xy(n, 1), None
    elif kind == "matrix":
        n = int(arg)
        xy, pk = None, K.random_matrix(n, 2)
    elif kind == "grid":
        xy, pk = K.unit_grid(9, 8), None
        n = 72
    elif kind == "twins":
        n = int(arg)
        xy, pk = K.duplicated(n, 3), None
    else:
        xy, pk, n = K.tsp(kind)
    return xy, pk, n, K.nn_upper(xy, pk, n)


@functools.lru_cache(maxsize=None)
def want(name, root=0, iterations=40, lambda0=2.0, patience=10, upper_scale=1.0):
    xy, pk, n, upper = instance(name)
    return H.ascent(xy, pk, n, upper=upper * upper_scale, root=root, iterations=iterations, lambda0=lambda0, patience=patience)


def check(ctx, name, iters_per_launch=0, **kw):
    xy, pk, n, upper = instance(name)
    kw.setdefault("iterations", 40)
    w = want(name, **kw)
    scale = kw.pop("upper_scale", 1.0)
    rc, got = K.call(ctx, xy, pk, n, upper=upper * scale, iters_per_launch=iters_per_launch, **kw)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle)
    K.assert_same(got, w, name)
    return got


# 3, 4, 5; around a wave; around the workgroup's 1024 threads; 2049 gives thread 0 three positions
@pytest.mark.parametrize("n,iterations", [(3, 40), (4, 40), (5, 40), (63, 40), (64, 40), (65, 40), (1023, 3), (1024, 3), (1025, 3), (2049, 2)])
def test_sizes(ctx, n, iterations):
    import ctypes as C
    t = C.c_int()
    assert ctx.lib.tl_one_tree_bound_plan(n, ctx.device_info()["lds_bytes"], C.byref(t), None) == 0
    assert t.value == min(1024, (n + 63) // 64 * 64)  # the sizes above are chosen around these
    check(ctx, f"rand:{n}", iterations=iterations)


def test_largest_n_and_one_more(ctx):
    max_n = int(ctx.lib.tl_one_tree_bound_max_n(ctx.device_info()["lds_bytes"]))
    assert max_n == (ctx.device_info()["lds_bytes"] - 1024) // 24 and 4096 <= max_n <= 65535
    check(ctx, f"rand:{max_n}", iterations=2)
    xy = K.random_xy(max_n + 1, 1)
    rc, _ = K.call(ctx, xy, None, max_n + 1, upper=1.0, iterations=2)
    assert rc == K.TL_ERR_UNSUPPORTED and b"above" in ctx.lib.tl_last_error(ctx.handle)


@pytest.mark.parametrize("name", ["matrix:70", "ring6_explicit", "gr17"])
def test_matrix_form(ctx, name):
    check(ctx, name)


@pytest.mark.parametrize("name", ["grid", "twins:66"])
def test_ties_go_to_the_lower_position(ctx, name):
    got = check(ctx, name)
    assert got["iterations_run"] >= 1


@pytest.mark.parametrize("root", [0, 1, 64])  # root 0 moves Prim's start to position 1
def test_roots(ctx, root):
    check(ctx, "rand:65", root=root)
    check(ctx, "grid", root=min(root, 71))


@pytest.mark.parametrize("span", [1, 7, 0])
def test_a_result_never_depends_on_the_span(ctx, span):
    check(ctx, "berlin52", iters_per_launch=span, iterations=40)
    check(ctx, "matrix:70", iters_per_launch=span, iterations=40)


def berlin_upper():
    xy, pk, n, _ = instance("berlin52")
    return 1.05 * H.tour_length_f64(H.rows_of(xy, pk, n), K.opt_tour_positions("berlin52"))


def test_stop_tour_found(ctx):
    xy, pk, n, _ = instance("berlin52")
    up = berlin_upper()
    w = H.ascent(xy, pk, n, upper=up)
    rc, got = K.call(ctx, xy, pk, n, upper=up)
    assert rc == 0
    K.assert_same(got, w, "berlin52 to the tour")
    assert got["stop"] == H.STOP_TOUR and got["is_tour"] == 1 and sorted(got["tour"]) == list(range(n)) and got["tour"][0] == 0
    assert got["iterations_run"] == 160 and f"{got['bound']:.3f}" == "7544.366"
    # n = 3: the 1-tree is a tour at k = 0
    g3 = check(ctx, "rand:3")
    assert g3["stop"] == H.STOP_TOUR and g3["iterations_run"] == 1 and sorted(g3["tour"]) == [0, 1, 2]


def test_stop_lambda_exhausted(ctx):
    got = check(ctx, "rand:65", lambda0=0.05, patience=1, iterations=200)
    assert got["stop"] == H.STOP_LAMBDA and got["iterations_run"] < 200


def test_stop_upper_reached(ctx):
    got = check(ctx, "rand:65", upper_scale=0.25)
    assert got["stop"] == H.STOP_UPPER and got["iterations_run"] == 1


def test_stop_iteration_cap(ctx):
    got = check(ctx, "rand:65", iterations=7)
    assert got["stop"] == H.STOP_ITERATIONS and got["iterations_run"] == 7


@pytest.mark.parametrize("jobs", [1, 2, 257])  # 257: one more than the CUs, a second pass
def test_job_counts(ctx, jobs):
    xy, pk, n, upper = instance("rand:16")
    kinds = [dict(root=j % 16, lambda0=(2.0, 1.0, 0.5)[j % 3], patience=(10, 3)[j % 2], iterations=25) for j in range(jobs)]
    rc, got, best = K.call_batch(ctx, xy, pk, n, [dict(upper=upper, **k) for k in kinds])
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle)
    for j, k in enumerate(kinds):
        K.assert_same(got[j], want("rand:16", **k), f"job {j}")
    bounds = [g["bound"] for g in got]
    assert best == bounds.index(max(bounds))


def test_jobs_that_stop_at_different_iterations(ctx):
    """A finished job must not disturb a running one: the jobs stop at the tour (k = 159), at the cap (7), at upper (1), by lambda."""
    xy, pk, n, _ = instance("berlin52")
    up = berlin_upper()
    sets = [dict(upper=up, iterations=1000), dict(upper=up, iterations=7), dict(upper=0.25 * up, iterations=1000),
            dict(upper=up, iterations=300, lambda0=0.05, patience=1), dict(upper=up, iterations=90, root=51)]
    rc, got, best = K.call_batch(ctx, xy, pk, n, sets)
    assert rc == 0
    for j, s in enumerate(sets):
        K.assert_same(got[j], H.ascent(xy, pk, n, **s), f"job {j}")
    assert [g["stop"] for g in got[:4]] == [H.STOP_TOUR, H.STOP_ITERATIONS, H.STOP_UPPER, H.STOP_LAMBDA]
    assert len({g["iterations_run"] for g in got}) == len(got)
    assert best == 0


def test_optional_outputs_and_a_short_log(ctx):
    import ctypes as C
    from teeline_amd import _capi
    xy, pk, n, upper = instance("rand:65")
    w = want("rand:65")
    o = _capi.TlOneTreeOpts(0, 40, 10, 0, 2.0, upper, 0)
    res = _capi.TlOneTreeResult()
    st = _capi.TlStats()
    assert ctx.lib.tl_one_tree_bound(ctx.handle, xy.ctypes.data_as(C.c_void_p), None, n, C.byref(o), C.byref(res), None, None, None, None, 0, C.byref(st)) == 0
    assert K.bits(res.bound) == K.bits(w["bound"]) and st.sweeps == w["iterations_run"] and st.kernel_ms > 0
    rc, got = K.call(ctx, xy, pk, n, upper=upper, iterations=40, log_cap=5)
    assert rc == 0 and len(got["log"]) == 5
    for a, b in zip(got["log"], w["log"][:5]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_stale_workspace_then_two_opt(ctx):
    """A context used by the bound and then by tl_two_opt gives the latter's usual result."""
    import _oracle as O
    import teeline_amd as TA
    check(ctx, "matrix:70")
    check(ctx, "rand:1025", iterations=3)
    xy = O.synth_xy(300, seed=4)
    sol = TA.two_opt.solve(TA.TspProblem(np.arange(300), xy), ctx=ctx)
    rc, route, cost, _ = O.two_opt(xy, None, 300)
    assert list(sol.route()) == route.tolist() and np.float32(sol.total).tobytes() == np.float32(cost).tobytes()


def test_a_busy_context_refuses_the_bound(ctx):
    """While one thread is inside tl_two_opt (an n = 10^4 descent) a second thread's tl_one_tree_bound on the same context is TL_ERR_BUSY."""
    import threading
    import time

    import _oracle as O
    import teeline_amd as TA
    n = 10000
    prob = TA.TspProblem(np.arange(n), O.synth_xy(n))
    init = [int(v) for v in O.restart_perm(n, 12345, 2)]
    t = threading.Thread(target=lambda: TA.two_opt.solve(prob, None, None, init, ctx=ctx))
    xy, pk, m, upper = instance("rand:16")
    codes = []
    t.start()
    t0 = time.time()
    while t.is_alive() and time.time() - t0 < 30:
        codes.append(K.call(ctx, xy, pk, m, upper=upper, iterations=5)[0])
    t.join()
    assert TA._capi.TL_ERR_BUSY in codes and set(codes) <= {0, TA._capi.TL_ERR_BUSY}, codes[:20]
    check(ctx, "rand:16", iterations=25)
