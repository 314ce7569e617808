"""Lin–Kernighan from planted start tours (-m gpu): the search starts from a tour whose FIRST move is a chain of a known number of
exchanges (tests/_lk_chain_cases.py; tests/test_lk_chain_cases.py certifies the tours on the CPU).  The runs from the nearest-neighbour
seed elsewhere in the suite apply chains of one or two exchanges and never more than six.

Against O.lin_kernighan from the same tour: the tour element for element, the cost bits, scans / searches / moves / exchanged edges.

THE RULE OF THIS FILE.  tl_lk has not returned within minutes from filed cases run through the chip-wide scans of the deep build
(lk_deep.hip, max_depth >= 7; seen with first chains of twelve and more exchanges, cause not found — DESIGN.md §4.10).  Until the cause
is known, no run here enters those scans.  A (case, max_depth) pair is run in a form iff
  - max_depth <= 6: the register build (lk.hip), in every form — first chains of 1..6 exchanges, 6 being the most its arrays hold; or
  - the LDS-resident form applies (lk_ils_qcap > 0: k = 3 at max_depth 7 among the filed cases), under TL_FLAG_LK_ILS_LDS with and
    without speculation: k_lk_ils of the deep build with a first chain of 7 exchanges, at n = 100 and at n = 1600, and the chain of 6
    of small-d06 once more.
Left for the day the cause is known: every case at max_depth 16, d >= 8 at all, the deep build in the chip-wide, one-workgroup, flat,
chip-step and classic-view forms, the lattice.  The default context at n = 1600 is not run either (the chip-step kernel of both builds
is launched by the one host loop from which a run did not return).

Forms (product-library flags only): spec TL_FLAG_LK_ILS_LDS; seq | TL_FLAG_LK_NO_SPECULATION; chip TL_FLAG_LK_CHIP_WIDE (fused pick at
k <= 9, the flat form with kept sub-chains at k = 10); one TL_FLAG_LK_ONE_WORKGROUP."""
import ctypes as C

import numpy as np
import pytest

import _lk_chain_cases as L
import _oracle as O

pytestmark = pytest.mark.gpu

FORMS = ["spec", "seq", "chip", "one"]
REGISTER = [(c, depth) for c in L.group("small", "wide") for depth in c.depths if depth <= 6]          # d = 1..6 at max_depth = d
LDS_DEEP = [(c, depth) for c in L.load() for depth in c.depths if depth >= 7 and L.takes_lds_form(c.n, c.k, depth)]
assert sorted(c.d for c, _ in REGISTER) == [1, 2, 3, 4, 5, 6, 6] and all(c.d == depth for c, depth in REGISTER)
assert sorted((c.d, depth, c.n >= 1500) for c, depth in LDS_DEEP) == [(6, 7, False), (7, 7, False), (7, 7, True)]  # all k = 3


@pytest.fixture(scope="module")
def forms():
    import teeline_amd as TA
    TA._capi.load()
    c = {"spec": TA.Context(0, TA.TL_FLAG_LK_ILS_LDS), "seq": TA.Context(0, TA.TL_FLAG_LK_ILS_LDS | TA.TL_FLAG_LK_NO_SPECULATION),
         "chip": TA.Context(0, TA.TL_FLAG_LK_CHIP_WIDE), "one": TA.Context(0, TA.TL_FLAG_LK_ONE_WORKGROUP)}
    yield c
    for v in c.values():
        v.close()


def gpu_lk(ctx, case, max_depth, epochs=0, platoo_epochs=10, seed=1, packed=None, trace=False):
    """tl_lk (trace: tl_lk_trace) from the case's tour: (route, cost, stats[, snapshots])."""
    from teeline_amd import _capi
    xy, _, tour = case.build()
    n = case.n
    init = np.ascontiguousarray(tour, dtype=np.uint32)
    out = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    cost, st = C.c_float(), _capi.TlStats()
    o = _capi.TlLkOpts(epochs, platoo_epochs, case.k, max_depth)
    args = (ctx.handle, xy.ctypes.data_as(C.c_void_p), n, None if packed is None else packed.ctypes.data_as(C.c_void_p),
            init.ctypes.data_as(C.c_void_p), C.byref(o), seed, out.ctypes.data_as(C.c_void_p), C.byref(cost), C.byref(st))
    if not trace:
        ctx.check(ctx.lib.tl_lk(*args))
        return out, np.float32(cost.value), st.as_dict()
    cap = epochs + 1
    snaps = np.full((cap, n), 0xFFFFFFFF, dtype=np.uint32)
    dists = np.zeros(cap, dtype=np.float32)
    ln = C.c_uint32()
    ctx.check(ctx.lib.tl_lk_trace(*args, snaps.ctypes.data_as(C.c_void_p), dists.ctypes.data_as(C.c_void_p), cap, C.byref(ln)))
    assert ln.value <= cap
    return out, np.float32(cost.value), st.as_dict(), [(snaps[m], dists[m]) for m in range(ln.value)]


def assert_same(g, o, what):
    route, cost, st = g[:3]
    rc, oroute, ocost, ost = o[:4]
    assert rc == 0 and route.tolist() == oroute.tolist(), f"{what}: tour differs from the oracle"
    assert np.float32(cost).tobytes() == np.float32(ocost).tobytes(), what
    assert (st["sweeps"], st["candidates"], st["moves"], st["reversed"]) == (ost["sweeps"], ost["candidates"], ost["moves"], ost["reversed"]), what


def assert_same_trace(g, o, what):
    assert_same(g, o, what)
    assert len(g[3]) == len(o[4]) >= 1, what
    for (gp, gd), (op, od) in zip(g[3], o[4]):
        assert gp.tolist() == op.tolist() and np.float32(gd).tobytes() == np.float32(od).tobytes(), what


def test_the_restated_lds_rule_is_the_librarys(forms):
    # LDS_DEEP is chosen with L.ils_qcap, a restatement of lk_ils_qcap (lk.hip): against the library's own function (the two builds'
    # namespaces) for every filed (n, k, max_depth) and this device's LDS size — a change of the product's rule fails here instead of
    # quietly turning the LDS runs below into chip-wide ones
    ctx = forms["spec"]
    lds = ctx.device_info()["lds_bytes"]
    assert lds == L.LDS_BYTES
    fn = {}
    for deep, name in ((False, "_ZN2tl11lk_ils_qcapEjjjm"), (True, "_ZN10tl_lk_deep11lk_ils_qcapEjjjm")):
        fn[deep] = getattr(ctx.lib, name)
        fn[deep].restype, fn[deep].argtypes = C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t]
    for c in L.load():
        for depth in range(1, L.MAX_DEPTH + 1):
            assert fn[depth > 6](c.n, c.k, depth, lds) == L.ils_qcap(c.n, c.k, depth, lds), (c.id, depth)
    assert all(L.ils_qcap(c.n, c.k, depth, lds) > 0 for c, depth in LDS_DEEP)


@pytest.mark.parametrize("form", FORMS)
def test_first_chain_of_one_to_six_exchanges_in_the_register_build(forms, form):
    for case, depth in REGISTER:
        o = case.oracle(depth)
        assert o[3]["moves"] == case.pass_moves[depth]  # the fixture's own record: the pass the CPU test certified
        assert_same(gpu_lk(forms[form], case, depth), o, f"{case.id} max_depth {depth} {form}")


@pytest.mark.parametrize("form", ["spec", "seq"])
def test_first_chain_of_six_and_seven_exchanges_in_the_lds_form_of_the_deep_build(forms, form):
    # k_lk_ils from lk_deep.hip, level queues with keys of 7 digits: n = 100 (4 waves) and n = 1600 (16 waves, chunks of pairs, 241 moves)
    for case, depth in LDS_DEEP:
        o = case.oracle(depth)
        assert o[3]["moves"] == case.pass_moves[depth]
        assert_same(gpu_lk(forms[form], case, depth), o, f"{case.id} max_depth {depth} {form}")


# the subset that also goes through tl_lk_trace, with and without epochs: d = 6 in the register build, d = 7 in the deep LDS form
SUBSET = {"spec": [(L.pick("small", 6), 6)] + LDS_DEEP, "seq": [(L.pick("small", 6), 6)] + LDS_DEEP,
          "chip": [(L.pick("small", 6), 6), (L.pick("wide", 6), 6)]}


@pytest.mark.parametrize("form", list(SUBSET))
def test_trace_reports_the_tour_after_the_first_pass(forms, form):
    for case, depth in SUBSET[form]:
        g = gpu_lk(forms[form], case, depth, trace=True)
        assert len(g[3]) == 1
        assert_same_trace(g, case.oracle(depth), f"{case.id} max_depth {depth} {form}")


@pytest.mark.parametrize("form", list(SUBSET))
def test_epochs_kick_the_tour_the_chain_left(forms, form):
    # three epochs, none of them the last of a plateau: the speculative form runs them as one batch from the tour the first pass left
    for case, depth in SUBSET[form]:
        kw = dict(epochs=3, platoo_epochs=3, seed=5)
        o = case.oracle(depth, **kw)
        assert o[3]["sweeps"] >= case.oracle(depth)[3]["sweeps"] + 3  # the first pass and three passes more
        assert_same_trace(gpu_lk(forms[form], case, depth, trace=True, **kw), o, f"{case.id} max_depth {depth} {form} with epochs")


@pytest.mark.parametrize("form", ["spec", "chip"])
def test_explicit_matrix_reports_the_total(forms, form):
    # the search is Euclidean over the coordinates; the total goes through the matrix (lin_kernighan.rs:99).  d = 7 in the deep LDS form,
    # d = 6 chip-wide
    case, depth = (L.pick("small", 7), 7) if form == "spec" else (L.pick("small", 6), 6)
    assert (case, depth) in REGISTER + LDS_DEEP
    xy = case.build()[0]
    packed = O.dm_build_packed(xy)
    rc, oroute, ocost, ost = O.lin_kernighan(xy, init=case.tour, epochs=0, n_nearest=case.k, max_depth=depth, packed=packed)
    g = gpu_lk(forms[form], case, depth, packed=packed)
    assert_same(g, (rc, oroute, ocost, ost), f"{case.id} max_depth {depth} {form} explicit matrix")
    assert oroute.tolist() == case.oracle(depth)[1].tolist()
    assert np.float32(g[1]).tobytes() == np.float32(O.tour_length(None, packed, oroute)).tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_context_reuse_leaves_no_stale_chain_slots(forms, form):
    # the longest chain the form's build is run with here, then a smaller instance whose only move is one exchange, then the first again
    ctx = forms[form]
    deep = (L.pick("small", 7), 7) if form in ("spec", "seq") else (L.pick("small", 6), 6)
    shallow = (L.pick("small", 1), 1)
    assert deep in REGISTER + LDS_DEEP and shallow in REGISTER and shallow[0].n <= deep[0].n
    for case, depth in (deep, shallow, deep):
        assert_same(gpu_lk(ctx, case, depth), case.oracle(depth), f"{case.id} max_depth {depth} {form} on a reused context")
