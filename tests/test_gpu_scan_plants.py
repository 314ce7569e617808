"""GPU tests (-m gpu): the 3-opt and Or-opt scans and their pick / apply kernels on planted winners (tests/_plants.py).  An
explicit matrix that is one constant but for a handful of entries puts the best move on a chosen seam of the work division: a
chunk's first or last j, lane 63 / 64, the second trip along k, the wrap column, a block beyond the pick kernel's first trip,
the last group of segment starts, a slab boundary.  The oracle decides the expected move (tests/test_scan_plants_oracle.py
proves, without a GPU, that every seam is where some plant's oracle winner lies); the comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _plants as P

pytestmark = pytest.mark.gpu


def problem(packed, n):
    import teeline_amd as TA
    return TA.TspProblem(np.arange(n), np.zeros((n, 2), np.float32), TA.distance_matrix.DistanceMatrix(n, packed, np.arange(n), "explicit"))


def gpu_move(ctx, scan, packed, path):
    import teeline_amd as TA
    mod = TA.three_opt if scan == "3" else TA.or_opt
    return mod.find_best_move(problem(packed, len(path)), path, ctx=ctx)


def same_move(scan, got, want):
    if got is None or want is None:
        return got is None and want is None
    if scan == "3":   # (i, j, k, case, savings)
        return tuple(got[:4]) == tuple(want[:4]) and np.float32(got[4]).tobytes() == np.float32(want[4]).tobytes()
    return np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes() and tuple(got[1:]) == tuple(want[1:])  # (delta, i, j, seg_len, reversed)


@pytest.mark.parametrize("scan,n,kind", P.all_tables(), ids=lambda v: str(v))
def test_planted_winners_match_the_oracle(ctx, scan, n, kind):
    bad = []
    for p in P.table(scan, n, kind):
        got, want = gpu_move(ctx, scan, p.matrix(), p.path()), P.oracle_move(p)
        if not same_move(scan, got, want):
            bad.append((p.id, p.aims, got, want))
        if len(p.aims) > 1:
            # the tie without its first member: the next one in loop order, the same bits
            first = min(range(len(p.aims)), key=lambda a: P._loop_key(p, p.aims[a]))
            got, want = gpu_move(ctx, scan, p.matrix(drop=(first,)), p.path()), P.oracle_move(p, drop=(first,))
            if not same_move(scan, got, want):
                bad.append((p.id + " minus its first", p.aims, got, want))
    assert not bad, bad


@pytest.mark.parametrize("scan,n,kind", P.all_tables(), ids=lambda v: str(v))
def test_nothing_is_reported_where_nothing_may_be(ctx, scan, n, kind):
    # the skipped triple i == 0 && k == n-1, a masked lane's k <= j, a wrapping row, j == prev, j inside the segment: the aim carries
    # the plant's best arithmetic, and neither the oracle nor the scan may report it
    for p in P.table(scan, n, kind):
        if p.neg:
            got = gpu_move(ctx, scan, p.matrix(), p.path())
            assert got is None or P._loop_key(p, P.coords(p, got))[:3] != P._loop_key(p, p.aims[0])[:3], (p.id, got)


@pytest.mark.parametrize("n", sorted(set(P.SIZES3) | set(P.SIZES_OR)))
def test_the_constant_matrix_has_no_move(ctx, n):
    # also the masks' plainest check: a lane at k == j, or at j == prev, computes a gain out of d(c, c) = 0
    m = P.constant_matrix(n)
    for kind in P.KINDS:
        if n in P.SIZES3:
            assert gpu_move(ctx, "3", m, P.tour(n, kind)) is None
        if n in P.SIZES_OR:
            assert gpu_move(ctx, "or", m, P.tour(n, kind)) is None


@pytest.mark.parametrize("n", P.THRESHOLD_SIZES)
def test_or_opt_threshold_at_its_edge(ctx, n):
    # or_opt.rs:86 best_delta = -1e-3, strict: delta -2^-9 is a move, delta -2^-10 is none
    for kind in P.KINDS:
        for p in P.threshold_plants(n, kind):
            got, want = gpu_move(ctx, "or", p.matrix(), p.path()), P.oracle_move(p)
            assert same_move("or", got, want), (p.id, got, want)
            if "take" in p.label:
                assert got is not None and P.value_bits(p, got) == P.THRESHOLD_TAKEN_BITS, (p.id, got)
            else:
                assert got is None, (p.id, got)


def trace(ctx, scan, p, log_cap=64):
    """tl_three_opt_trace / tl_or_opt_trace on the plant: (tour, cost, moves, log)."""
    from teeline_amd import _capi
    n = p.n
    out = np.empty(n, dtype=np.uint32)
    c, st, ln = C.c_float(), _capi.TlStats(), C.c_uint32()
    log = np.full((log_cap, 4), 0xFFFFFFFF, dtype=np.uint32)
    pk, ip = np.ascontiguousarray(p.matrix()), np.ascontiguousarray(p.path(), dtype=np.uint32)
    xy = np.zeros((n, 2), np.float32)
    fn = ctx.lib.tl_three_opt_trace if scan == "3" else ctx.lib.tl_or_opt_trace
    ctx.check(fn(ctx.handle, xy.ctypes.data_as(C.c_void_p), n, pk.ctypes.data_as(C.c_void_p), ip.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(c),
                 C.byref(st), log.ctypes.data_as(C.c_void_p), log_cap, C.byref(ln)))
    assert ln.value == st.moves <= log_cap
    return out, np.float32(c.value), int(ln.value), log[:ln.value].tolist()


def check_replay(scan, p, out, cost, moves, log):
    """The move log replayed with the oracle's apply from the start tour gives the returned tour, element for element; the cost is
    the oracle's tour length of it, bit for bit; the first move is the plant; the descent ends within APPLY_MAX_MOVES."""
    assert 1 <= moves <= P.APPLY_MAX_MOVES, (p.id, moves, log)
    assert tuple(log[0]) == ((p.aims[0] if scan == "3" else (p.aims[0][1], p.aims[0][2], p.aims[0][0], int(p.aims[0][3])))), (p.id, log[0])
    t = np.array(p.path(), dtype=np.uint32)
    for w in log:
        rc, t = O.apply_3opt(t, *w) if scan == "3" else O.apply_relocation(t, w[0], w[2], w[1], w[3])
        assert rc == 0, (p.id, w)
    assert out.tolist() == t.tolist(), p.id
    assert cost.tobytes() == O.tour_length(None, p.matrix(), out).tobytes(), p.id


@pytest.mark.parametrize("span", ["long_l1", "long_l2", "both"])
@pytest.mark.parametrize("n", P.APPLY_SIZES)
def test_three_opt_apply_cases_1_to_7(ctx, n, span):
    # n = 256 stages the move in LDS, 257 in the workspace; at n = 1100 the moved span l1 + l2 exceeds the pick kernel's 1024 threads
    # (long_l1: l1 = 1030, l2 = 5; long_l2: the reverse; both: 600 + 450)
    for kind in P.KINDS:
        for p in P.apply_table3(n, kind):
            if span in p.label:
                i, j, k, case = p.aims[0]
                assert n < 1100 or k - i > 1024
                check_replay("3", p, *trace(ctx, "3", p))


@pytest.mark.parametrize("n", P.APPLY_SIZES)
def test_or_opt_apply_every_kind_both_sides(ctx, n):
    # lengths 1-3, forward and reversed, j < i and j >= i + len; the oracle's Or-opt is quadratic, so the whole descent is compared outright
    for kind in P.KINDS:
        for p in P.apply_table_or(n, kind):
            out, cost, moves, log = trace(ctx, "or", p)
            check_replay("or", p, out, cost, moves, log)
            rc, oout, ocost, ost = O.or_opt(None, p.matrix(), n, init=p.path())
            assert rc == 0 and out.tolist() == oout.tolist() and cost.tobytes() == np.float32(ocost).tobytes() and moves == ost["moves"], p.id
