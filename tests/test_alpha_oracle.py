"""tests/_alpha_oracle.py, the statement of record of DESIGN.md §4.32, against a brute-force path maximum (n <= 12), and the properties
every alpha table has."""
import numpy as np
import pytest

import _alpha_cases as AC
import _alpha_oracle as A


def offdiag(M):
    n = len(M)
    return M[~np.eye(n, dtype=bool)]


@pytest.mark.parametrize("name,root,pi_kind", [("rand:3", 0, "zero"), ("rand:4", 3, "zero"), ("rand:5", 2, "zero"), ("rand:8", 0, "zero"),
                                               ("rand:12", 0, "zero"), ("rand:12", 11, "zero"), ("rand:12", 5, "ascent"), ("line:12", 0, "zero"),
                                               ("line:12", 6, "zero"), ("star:5", 0, "zero"), ("star:5", 2, "zero"), ("twins:12", 4, "zero"),
                                               ("grid:4x3", 0, "zero"), ("grid:4x3", 7, "ascent"), ("ring6_explicit", 0, "zero"),
                                               ("ring6_explicit", 3, "ascent")])
def test_table_equals_the_walk_along_every_path(name, root, pi_kind):
    xy, pk, n = AC.instance(name)
    pi = AC.pi_of(name, pi_kind)
    got, W, par, nb = A.table(xy, pk, n, pi, root)
    want, W2, par2, nb2 = A.brute_table(xy, pk, n, pi, root)
    assert np.array_equal(par, par2) and nb == nb2 and W.tobytes() == W2.tobytes()
    assert offdiag(got).tobytes() == offdiag(want).tobytes()
    assert (offdiag(got) >= 0).all() and not np.signbit(offdiag(got)).any()
    assert offdiag(got).tobytes() == offdiag(got.T.copy()).tobytes()


def test_ordered_is_the_number_order():
    x = np.array([-np.inf, -3.5, -0.0, 0.0, 5e-324, 1.0, np.inf])
    o = A.ordered(x)
    assert o[2] == o[3] and (np.diff(o.astype(object)) >= 0).all() and len(set(o.tolist())) == 6


@pytest.mark.parametrize("name,root,pi_kind,k", AC.CASES)
def test_rows_and_properties(name, root, pi_kind, k):
    xy, pk, n = AC.instance(name)
    w = AC.want(name, root, pi_kind, k)
    kk = min(k, n - 1)
    assert w["cand"].shape == (n, kk)
    for i in range(n):
        assert i not in w["cand"][i] and len(set(w["cand"][i].tolist())) == kk
    AC.assert_properties(w, n, root, name)


def test_rows_are_the_sorted_table():
    """Row i by a plain Python sort of (alpha, w, j) as numbers."""
    name, root = "grid:5x4", 19
    xy, pk, n = AC.instance(name)
    T, W, _, _ = A.table(xy, pk, n, None, root)
    w = AC.want(name, root, "zero", 8)
    for i in range(n):
        keys = sorted((float(T[i, j]), float(W[i, j]), j) for j in range(n) if j != i)
        assert [j for _, _, j in keys[:8]] == w["cand"][i].tolist()


def test_trivial_sizes():
    for n in (1, 2):
        w = A.candidates(np.zeros((n, 2), dtype=np.float32), None, n, None, 0, 5)
        assert w["cand"].shape == (n, n - 1) and w["root_nb"] == (A.NONE, A.NONE)
    assert A.candidates(np.array([[0, 0], [3, 4]], dtype=np.float32), None, 2, None, 1, 5)["cand"].tolist() == [[1], [0]]
