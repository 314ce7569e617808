"""tl_alpha_candidates_host, the sequential restatement (no device), against tests/_alpha_oracle.py bit for bit: rows, alphas, parents
and root neighbours; the host-only queries; tl_lk_candidates' declaration."""
import ctypes as C
import os

import numpy as np
import pytest

import _alpha_cases as AC
import _one_tree_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from teeline_amd import build
    build.build()
    from teeline_amd import _capi
    return _capi.load()


@pytest.mark.parametrize("name,root,pi_kind,k", AC.CASES)
def test_host_equals_the_oracle(lib, name, root, pi_kind, k):
    xy, pk, n = AC.instance(name)
    rc, got, _ = AC.call(None, xy, pk, n, AC.pi_of(name, pi_kind), root, k)
    assert rc == 0, lib.tl_last_error(None)
    AC.assert_same(got, AC.want(name, root, pi_kind, k), name)
    AC.assert_properties(got, n, root, name)


def test_the_ascents_tree_is_rebuilt_from_its_pi(lib):
    """For the out_pi of a tl_one_tree_bound(_host) call the rebuilt parents and root neighbours equal that call's."""
    for name, root in (("rand:30", 0), ("rand:30", 12), ("ulysses22", 3)):
        xy, pk, n = AC.instance(name)
        rc, b = K.call(None, xy, pk, n, upper=K.nn_upper(xy, pk, n), root=root, iterations=20)
        assert rc == 0
        rc, got, _ = AC.call(None, xy, pk, n, b["pi"], root, 5)
        assert rc == 0
        assert np.array_equal(got["parent"], b["parent"]) and tuple(got["root_nb"]) == tuple(b["root_nb"]), name


def test_optional_outputs_and_trivial_sizes(lib):
    xy, pk, n = AC.instance("rand:20")
    rc, got, _ = AC.call(None, xy, pk, n, None, 0, 5, outputs=False)
    assert rc == 0 and np.array_equal(got["cand"], AC.want("rand:20", 0, "zero", 5)["cand"])
    assert np.isnan(got["alpha"]).all() and (got["parent"] == 0xABABABAB).all()
    for m in (1, 2):
        rc, got, _ = AC.call(None, xy[:m], None, m, None, m - 1, 5)
        w = AC.A.candidates(xy[:m], None, m, None, m - 1, 5)
        assert rc == 0
        AC.assert_same(got, w, f"n = {m}")


def test_errors(lib):
    xy, pk, n = AC.instance("rand:20")
    assert AC.call(None, xy, pk, n, None, 20, 5)[0] == AC.TL_ERR_BADARG and b"root" in lib.tl_last_error(None)
    assert AC.call(None, xy, pk, n, None, 0, 0)[0] == AC.TL_ERR_BADARG
    assert AC.call(None, xy, pk, n, None, 0, 65)[0] == AC.TL_ERR_UNSUPPORTED and b"64" in lib.tl_last_error(None)
    assert AC.call(None, xy[:1], None, 70000, None, 0, 5)[0] == AC.TL_ERR_UNSUPPORTED  # refused before anything of size n is read
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 1021):
        pi = np.zeros(n)
        pi[7] = bad
        assert AC.call(None, xy, pk, n, pi, 0, 5)[0] == AC.TL_ERR_UNSUPPORTED and b"penalty" in lib.tl_last_error(None)
    bad_xy = xy.copy()
    bad_xy[3, 1] = np.inf
    assert AC.call(None, bad_xy, None, n, None, 0, 5)[0] == AC.TL_ERR_UNSUPPORTED
    m = np.asarray(AC.instance("ring6_explicit")[1]).copy()
    m[2] = -0.0
    assert AC.call(None, None, m, 6, None, 0, 5)[0] == AC.TL_ERR_UNSUPPORTED
    assert lib.tl_alpha_candidates_host(None, None, 5, None, 0, 5, None, None, None, None) == AC.TL_ERR_BADARG


def test_plan_and_max_n(lib):
    lds = K.LDS_BYTES
    assert lib.tl_alpha_candidates_max_n(lds) == min((lds - 1024) // 24, (lds - 1024) // 16) == lib.tl_one_tree_bound_max_n(lds)
    assert lib.tl_alpha_candidates_max_n(0) == 0
    t, used = C.c_int(-1), C.c_uint32(7)
    assert lib.tl_alpha_candidates_plan(1002, 5, lds, C.byref(t), C.byref(used)) == 0 and t.value == 256 and used.value == 16 * 1002 + 0
    assert lib.tl_alpha_candidates_plan(65, 5, lds, C.byref(t), C.byref(used)) == 0 and t.value == 128 and used.value == 16 * 65
    assert lib.tl_alpha_candidates_plan(2, 5, lds, C.byref(t), C.byref(used)) == 0 and t.value == 0
    assert lib.tl_alpha_candidates_plan(7000, 5, lds, C.byref(t), None) == AC.TL_ERR_UNSUPPORTED
    assert lib.tl_alpha_candidates_plan(100, 65, lds, None, None) == AC.TL_ERR_UNSUPPORTED
    assert lib.tl_alpha_candidates_plan(100, 0, lds, None, None) == AC.TL_ERR_BADARG
    assert lib.tl_alpha_candidates_plan(100, 5, -1, None, None) == AC.TL_ERR_BADARG


def test_the_header_states_the_order_rule():
    text = open(os.path.join(ROOT, "include", "teeline_gpu.h")).read()
    assert "ALPHA CHOOSES THE SET, DISTANCE ORDERS IT" in text and "int tl_lk_candidates(tl_ctx *ctx, const uint32_t *cand, uint32_t n, uint32_t k);" in text
    spec = open(os.path.join(ROOT, "teeline_amd", "csrc", "alpha_spec.h")).read()
    assert "alpha >= +0.0 always" in spec and "bit for bit" in spec
