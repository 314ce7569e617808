"""tl_alpha_candidates on the device (-m gpu) against tests/_alpha_oracle.py, bit for bit: rows, alphas, parents and root neighbours
(DESIGN.md §4.32)."""
import ctypes as C
import functools

import numpy as np
import pytest

import _alpha_cases as AC
import _alpha_oracle as A
import _one_tree_cases as K

pytestmark = pytest.mark.gpu


def check(ctx, name, root, pi_kind, k, threads=0):
    xy, pk, n = AC.instance(name)
    rc, got, st = AC.call(ctx, xy, pk, n, AC.pi_of(name, pi_kind), root, k, threads)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle)
    AC.assert_same(got, AC.want(name, root, pi_kind, k), f"{name} root {root} k {k} threads {threads}")
    return got, st


@pytest.mark.parametrize("name,root,pi_kind,k", AC.CASES)
def test_device_equals_the_oracle(ctx, name, root, pi_kind, k):
    xy, pk, n = AC.instance(name)
    got, _ = check(ctx, name, root, pi_kind, k)
    AC.assert_properties(got, n, root, name)


# past one pass of a 256-thread workgroup (the plan's) and of a 1024-thread one; 1002: the largest size of the suite
@pytest.mark.parametrize("name,threads", [("rand:257", 0), ("rand:257", 256), ("rand:1025", 1024), ("rand:1025", 0), ("synth:1002", 0)])
def test_past_one_pass_of_the_workgroup(ctx, name, threads):
    t = C.c_int()
    n = AC.instance(name)[2]
    assert ctx.lib.tl_alpha_candidates_plan(n, 5, ctx.device_info()["lds_bytes"], C.byref(t), None) == 0 and t.value == 256
    got, st = check(ctx, name, 0, "zero", 5, threads)
    AC.assert_properties(got, n, 0, name)
    assert st.kernel_ms > 0 and st.candidates == n * (n - 1) and st.sweeps >= 2


@pytest.mark.parametrize("threads", [64, 128, 512, 1024])
def test_a_result_never_depends_on_the_threads(ctx, threads):
    check(ctx, "rand:257", 5, "zero", 7, threads)
    check(ctx, "line:65", 0, "zero", 5, threads)
    check(ctx, "ulysses22", 0, "ascent", 5, threads)


@functools.lru_cache(maxsize=None)
def ascent_on_device(ctx, name, root, iterations):
    xy, pk, n = AC.instance(name)
    rc, b = K.call(ctx, xy, pk, n, upper=K.nn_upper(xy, pk, n), root=root, iterations=iterations)
    assert rc == 0
    return b


@pytest.mark.parametrize("name,root,iterations", [("berlin52", 0, 1000), ("berlin52", 51, 60), ("a280", 0, 100)])
def test_the_ascents_tree_is_rebuilt_from_its_pi(ctx, name, root, iterations):
    """With the out_pi of tl_one_tree_bound: the parents and root neighbours equal that call's, and the rows the oracle's under that pi."""
    xy, pk, n = AC.instance(name)
    b = ascent_on_device(ctx, name, root, iterations)
    rc, got, _ = AC.call(ctx, xy, pk, n, b["pi"], root, 5)
    assert rc == 0, ctx.lib.tl_last_error(ctx.handle)
    assert np.array_equal(got["parent"], b["parent"]) and tuple(got["root_nb"]) == tuple(b["root_nb"])
    AC.assert_same(got, A.candidates(xy, pk, n, b["pi"], root, 5), name)
    AC.assert_properties(got, n, root, name)


def test_optional_outputs_and_trivial_sizes(ctx):
    xy, pk, n = AC.instance("rand:20")
    rc, got, _ = AC.call(ctx, xy, pk, n, None, 0, 5, outputs=False)
    assert rc == 0 and np.array_equal(got["cand"], AC.want("rand:20", 0, "zero", 5)["cand"])
    assert np.isnan(got["alpha"]).all() and (got["parent"] == 0xABABABAB).all()
    for m in (1, 2):
        rc, got, _ = AC.call(ctx, xy[:m], None, m, None, m - 1, 5)
        assert rc == 0
        AC.assert_same(got, A.candidates(xy[:m], None, m, None, m - 1, 5), f"n = {m}")


def test_errors(ctx):
    err = lambda: ctx.lib.tl_last_error(ctx.handle)  # noqa: E731
    xy, pk, n = AC.instance("rand:20")
    assert AC.call(ctx, xy, pk, n, None, 0, 65)[0] == AC.TL_ERR_UNSUPPORTED and b"64" in err()
    assert AC.call(ctx, xy, pk, n, None, 0, 0)[0] == AC.TL_ERR_BADARG
    assert AC.call(ctx, xy, pk, n, None, 20, 5)[0] == AC.TL_ERR_BADARG and b"root" in err()
    assert AC.call(ctx, xy, pk, n, None, 0, 5, threads=100)[0] == AC.TL_ERR_BADARG and b"threads" in err()
    max_n = int(ctx.lib.tl_alpha_candidates_max_n(ctx.device_info()["lds_bytes"]))
    assert max_n == (ctx.device_info()["lds_bytes"] - 1024) // 24
    # one more than the limit, with ONE city's coordinates behind the pointer: refused before anything of size n is read
    assert AC.call(ctx, xy[:1], None, max_n + 1, None, 0, 5)[0] == AC.TL_ERR_UNSUPPORTED and b"above" in err()
    for bad in (np.nan, np.inf, 2.0 ** 1021):
        pi = np.zeros(n)
        pi[11] = bad
        assert AC.call(ctx, xy, pk, n, pi, 0, 5)[0] == AC.TL_ERR_UNSUPPORTED and b"penalty" in err()
    check(ctx, "rand:20", 0, "zero", 5)  # the context is as good as before


def test_stale_workspace_then_the_bound(ctx):
    """A context used by the lists and then by tl_one_tree_bound gives the latter's usual result, and the other way round."""
    import _one_tree_oracle as H
    check(ctx, "synth:1002", 0, "zero", 5)
    xy, pk, n = AC.instance("rand:30")
    up = K.nn_upper(xy, pk, n)
    rc, got = K.call(ctx, xy, pk, n, upper=up, iterations=20)
    assert rc == 0
    K.assert_same(got, H.ascent(xy, pk, n, upper=up, iterations=20), "rand:30")
    check(ctx, "rand:30", 29, "ascent", 7)


def test_a_busy_context_refuses_the_lists(ctx):
    """While one thread is inside tl_two_opt (an n = 10^4 descent) a second thread's tl_alpha_candidates on the same context is TL_ERR_BUSY."""
    import threading
    import time

    import _oracle as O
    import teeline_amd as TA
    n = 10000
    prob = TA.TspProblem(np.arange(n), O.synth_xy(n))
    init = [int(v) for v in O.restart_perm(n, 12345, 2)]
    t = threading.Thread(target=lambda: TA.two_opt.solve(prob, None, None, init, ctx=ctx))
    xy, pk, m = AC.instance("rand:20")
    codes = []
    t.start()
    t0 = time.time()
    while t.is_alive() and time.time() - t0 < 30:
        codes.append(AC.call(ctx, xy, pk, m, None, 0, 5)[0])
    t.join()
    assert AC.TL_ERR_BUSY in codes and set(codes) <= {0, AC.TL_ERR_BUSY}, codes[:20]
    check(ctx, "rand:20", 0, "zero", 5)
