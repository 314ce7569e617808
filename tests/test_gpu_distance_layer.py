"""The distance layer on the GPU (-m gpu): csrc/dm_build.hip through tl_dm_build, tl_dm_build_dev, tl_dm_is_euc2d and
tl_tour_length, against the C oracle and the numpy restatement (tests/_dm_reference.py), bit for bit (NaN payloads aside).

A  packed EUC_2D at the blocked kernel's edges (partial 4-row blocks, the ilast clamp, slabs on the diagonal, clamped loads)
B  packed GEO beyond one 4 096-column slab, over the whole globe and at the floor's nearest ties; ulysses22 through the mirror
C  TL_DM_FULL, both distance kinds; packed and full builds side by side
D  tl_dm_build_dev on caller tensors and a caller stream; its argument checks
E  tl_dm_is_euc2d (bit flips at slab and row edges, the NaN and -0.0 rules) and tl_tour_length (chunk edges, NaN / inf)
F  packed offsets above 2^31 elements (n = 65 601) and a full matrix of more than 2^31 entries (n = 46 341)
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _dm_reference as R
import _oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 0xDEADBEEF  # a negative finite float: no distance is ever negative


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def gpu_dm(ctx, xy, geo=False, layout=0):
    xy = np.ascontiguousarray(xy, dtype=F32)
    n = xy.shape[0]
    out = np.empty(n * (n - 1) // 2 if layout == 0 else n * n, dtype=F32)
    out.view(np.uint32)[:] = SENTINEL
    ctx.check(ctx.lib.tl_dm_build(ctx.handle, _p(xy), n, 1 if geo else 0, layout, _p(out), None))
    return out if layout == 0 else out.reshape(n, n)


def check_geo(got, want, xy, what):
    R.assert_bits_equal(got, want, what, R.describe_geo_packed(xy, got.reshape(-1), want.reshape(-1)))


@functools.lru_cache(maxsize=None)
def near_ties():
    return R.near_tie_pairs()


@functools.lru_cache(maxsize=6)
def geo_case(n):
    """A mixed GEO instance of n points and the oracle's packed matrix (cached: the oracle needs ~3 s at n = 8 193)."""
    xy = R.geo_mix(n, seed=n, ties=near_ties()[:2] if n >= 4096 else None)
    return xy, O.dm_build_packed(xy, geo=True)


def euc_inputs(n):
    return {"random": O.synth_xy(n, seed=n), "decimal": R.decimal_grid_xy(n, n), "degenerate": R.degenerate_xy(n, n)}


# ---- A: packed EUC_2D ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(2, 10)) + list(range(1023, 1030)) + [2049, 4097, 5000])
def test_packed_euc2d_at_block_and_slab_edges(ctx, n):
    for name, xy in euc_inputs(n).items():
        got = gpu_dm(ctx, xy)
        R.assert_bits_equal(got, O.dm_build_packed(xy), f"{name} n={n} vs oracle")
        R.assert_bits_equal(got, R.euc_packed(xy), f"{name} n={n} vs numpy")
        assert not (got.view(np.uint32) == 0x80000000).any(), "-0.0 in a packed matrix"
    if n >= 31:  # the degenerate input's duplicate (k = 30 repeats 29) and +-0.0 pair (3, 6) give +0.0, never -0.0
        got = gpu_dm(ctx, R.degenerate_xy(n, n))
        assert got.view(np.uint32)[R.row_offset(30) + 29] == 0 and got.view(np.uint32)[R.row_offset(6) + 3] == 0


# ---- B: packed GEO -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(2, 10)))
def test_packed_geo_small_every_category(ctx, n):
    rng = np.random.default_rng(100 + n)
    for name, xy in R.geo_categories(rng, n).items():
        check_geo(gpu_dm(ctx, xy, geo=True), O.dm_build_packed(xy, geo=True), xy, f"{name} n={n}")


@pytest.mark.parametrize("n", [4095, 4096, 4097, 4098, 8193])
def test_packed_geo_beyond_one_slab(ctx, n):
    xy, want = geo_case(n)
    check_geo(gpu_dm(ctx, xy, geo=True), want, xy, f"mixed GEO n={n}")


def test_packed_geo_near_ties(ctx):
    # the 2 000 grid pairs (of 2e6 drawn) whose RRR * acos(...) + 1 lies nearest an integer, as pairs (2k + 1, 2k) of one matrix
    p, q, gap = near_ties()
    xy = np.empty((2 * len(p), 2), F32)
    xy[1::2], xy[0::2] = p, q
    got, want = gpu_dm(ctx, xy, geo=True), O.dm_build_packed(xy, geo=True)
    check_geo(got, want, xy, f"near ties (nearest {float(gap[0]):.3g} from an integer)")
    # in a column slab >= 1 as well: geo_case(8193) holds them at (4096 + 2000 + k, 4096 + k)
    xy8 = geo_case(8193)[0]
    base = 8193 // 2
    assert np.array_equal(xy8[base:base + len(p)], q) and np.array_equal(xy8[base + len(p):base + 2 * len(p)], p)


def test_ulysses22_matrix_nn_seed_and_two_opt_through_the_mirror(ctx, tsplib_dir):
    import teeline_amd as TA
    d = TA.tsplib.read_from_file(os.path.join(tsplib_dir, "ulysses22.tsp"))
    assert d.distance_type == "geo" and len(d) == 22
    prob = d.problem(ctx=ctx)
    n, xy = len(d), d.xy
    packed = O.dm_build_packed(xy, geo=True)
    check_geo(prob.distances.items, packed, xy, "ulysses22")
    for k in (1, 3, 5):
        sol = TA.nearest_neighbor.solve(prob, TA.HeuristicOptions(n_nearest=k), ctx=ctx)
        rc, route, c = O.nearest_neighbor(None, packed, n, k)
        assert rc == 0 and list(sol.route()) == d.ids[route].tolist()
        assert np.float32(sol.total).tobytes() == np.float32(c).tobytes()
        sol2 = TA.two_opt.solve(prob, None, None, list(sol.route()), ctx=ctx)
        rc, route2, c2, st = O.two_opt(xy, packed, n, init=route)
        assert rc == 0 and list(sol2.route()) == d.ids[route2].tolist()
        assert np.float32(sol2.total).tobytes() == np.float32(c2).tobytes()
        assert np.float32(sol2.total).tobytes() == O.tour_length(None, packed, route2).tobytes()


# ---- C: TL_DM_FULL -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 1025, 4097, 4098, 8193])
def test_full_layout_both_kinds(ctx, n):
    cases = [("euc2d", R.degenerate_xy(n, n + 1), False)]
    if n < 4096:
        cases.append(("geo", R.geo_mix(n, seed=n), True))
    else:
        cases.append(("geo", geo_case(n)[0], True))
    for name, xy, geo in cases:
        want_packed = geo_case(n)[1] if (geo and n >= 4096) else O.dm_build_packed(xy, geo=geo)
        got = gpu_dm(ctx, xy, geo=geo, layout=1)
        diag = np.diagonal(got)
        assert (diag.view(np.uint32) == 0).all(), f"{name} n={n}: diagonal is not +0.0"
        R.assert_bits_equal(got, O.dm_expand_full(want_packed, n), f"{name} n={n} full vs expanded oracle")
        if geo:  # orientation: (i, j) is geo_dist(xy[max], xy[min]); spot-check a few against the packed entry
            for i, j in ((1, 0), (0, 1), (n - 1, 0), (0, n - 1)):
                if i != j:
                    hi, lo = max(i, j), min(i, j)
                    assert got[i, j].tobytes() == want_packed[R.row_offset(hi) + lo].tobytes()


@pytest.mark.parametrize("n", [1025, 4097])
def test_packed_and_full_builds_leave_each_other_intact(ctx, n):
    for geo in (False, True):
        xy = geo_case(n)[0] if geo and n >= 4096 else (R.geo_mix(n, seed=n) if geo else R.degenerate_xy(n, 3))
        want = geo_case(n)[1] if geo and n >= 4096 else O.dm_build_packed(xy, geo=geo)
        p1 = gpu_dm(ctx, xy, geo=geo)
        f1 = gpu_dm(ctx, xy, geo=geo, layout=1)
        p2 = gpu_dm(ctx, xy, geo=geo)
        f2 = gpu_dm(ctx, xy, geo=geo, layout=1)
        for got in (p1, p2):
            R.assert_bits_equal(got, want, f"geo={geo} n={n} packed")
        for got in (f1, f2):
            R.assert_bits_equal(got, R.full_from_packed(want, n), f"geo={geo} n={n} full")


# ---- D: tl_dm_build_dev --------------------------------------------------------------------------------------------------
GUARD = 4096  # floats of sentinel before and after every device output


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev_buffer(torch, elems):
    return torch.full((elems + 2 * GUARD,), SENTINEL - 2**32, dtype=torch.int32, device="cuda")


def _guards_ok(host_u32, elems):
    return (host_u32[:GUARD] == SENTINEL).all() and (host_u32[GUARD + elems:] == SENTINEL).all()


@pytest.mark.parametrize("n", list(range(2, 10)) + [1023, 1024, 1025, 1029, 2049, 4097, 4098])
def test_dev_build_on_a_caller_stream_writes_exactly_its_matrix(ctx, n):
    """Both kinds, both layouts into guarded, sentinel-filled device buffers on a non-default stream: every entry written, nothing
    outside it, the same bits as tl_dm_build; one packed and one full matrix side by side on the same context."""
    torch = _torch()
    xy = R.geo_mix(n, seed=7 * n)
    xy[: min(n, 4)] = xy[0]  # a duplicate run at the start of the matrix
    d_xy = torch.from_numpy(xy).to("cuda")
    s = torch.cuda.Stream()
    for geo in (False, True):
        elems = {0: n * (n - 1) // 2, 1: n * n}
        bufs = {lay: _dev_buffer(torch, elems[lay]) for lay in (0, 1)}
        s.wait_stream(torch.cuda.current_stream())
        for lay in (0, 1):
            ptr = C.c_void_p(bufs[lay].data_ptr() + 4 * GUARD)
            ctx.check(ctx.lib.tl_dm_build_dev(ctx.handle, C.c_void_p(d_xy.data_ptr()), n, int(geo), lay, ptr,
                                              C.c_void_p(s.cuda_stream)))
        s.synchronize()
        assert ctx.last_kernel_ms() >= 0.0
        for lay in (0, 1):
            host = bufs[lay].cpu().numpy().view(np.uint32)
            assert _guards_ok(host, elems[lay]), f"geo={geo} layout={lay} n={n}: write outside the matrix"
            got = host[GUARD:GUARD + elems[lay]].view(F32)
            R.assert_bits_equal(got, gpu_dm(ctx, xy, geo=geo, layout=lay).reshape(-1), f"geo={geo} layout={lay} n={n} dev vs host")


def test_dev_build_rejects_bad_arguments_and_writes_nothing(ctx):
    torch = _torch()
    from teeline_amd import _capi
    n = 1025
    d_xy = torch.from_numpy(O.synth_xy(n, seed=1)).to("cuda")
    elems = n * n
    buf = _dev_buffer(torch, elems)
    torch.cuda.synchronize()
    out = C.c_void_p(buf.data_ptr() + 4 * GUARD)
    xyp = C.c_void_p(d_xy.data_ptr())
    L, h = ctx.lib, ctx.handle
    s = torch.cuda.Stream()
    for args in [(None, n, 0, 0, out), (xyp, n, 0, 0, None), (xyp, 1, 0, 0, out), (xyp, 0, 1, 1, out), (xyp, n, 2, 0, out),
                 (xyp, n, 0, 2, out), (xyp, n, -1, 0, out), (xyp, n, 1, -1, out)]:
        rc = L.tl_dm_build_dev(h, args[0], args[1], args[2], args[3], args[4], C.c_void_p(s.cuda_stream))
        assert rc == _capi.TL_ERR_BADARG, (args[1:4], rc)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a rejected call wrote to its output"


# ---- E: tl_dm_is_euc2d, tl_tour_length -----------------------------------------------------------------------------------
def is_euc2d(ctx, xy, packed):
    out = C.c_int(-1)
    ctx.check(ctx.lib.tl_dm_is_euc2d(ctx.handle, _p(np.ascontiguousarray(xy, F32)), _p(packed), len(xy), C.byref(out)))
    assert out.value in (0, 1)
    return bool(out.value)


@pytest.mark.parametrize("n", [1025, 4098])
def test_is_euc2d_detects_one_bit_at_every_edge(ctx, n):
    xy = O.synth_xy(n, seed=n)
    packed = O.dm_build_packed(xy)
    assert is_euc2d(ctx, xy, packed)
    m = len(packed)
    places = {"first": 0, "last": m - 1}
    for i in (1, 2, 3, 4, 5, 1023, 1024, 1025, n - 2, n - 1):
        if i < n:
            places[f"end of row {i}"] = R.row_offset(i) + i - 1
            places[f"start of row {i}"] = R.row_offset(i)
    for i in (4096, 4097):
        for j in (4095, 4096):
            if j < i < n:
                places[f"({i}, {j})"] = R.row_offset(i) + j
    u = packed.view(np.uint32)
    for name, k in places.items():
        for bit in (0, 22, 31):
            u[k] ^= np.uint32(1 << bit)
            assert not is_euc2d(ctx, xy, packed), f"n={n}: flip of bit {bit} at {name} (index {k}) not detected"
            u[k] ^= np.uint32(1 << bit)
    assert is_euc2d(ctx, xy, packed)


def test_is_euc2d_nan_payloads_match_and_negative_zero_does_not(ctx):
    n = 4098
    xy = O.synth_xy(n, seed=3)
    xy[4097] = (np.nan, 1.0)   # the whole last row, two column slabs, is NaN ...
    xy[100] = (2.0, np.nan)    # ... and column 100 of every later row
    xy[7] = xy[5]              # a duplicate: entry (7, 5) is +0.0
    packed = O.dm_build_packed(xy)
    assert np.isnan(packed).sum() > n
    assert is_euc2d(ctx, xy, packed)
    u = packed.view(np.uint32)
    nan = np.isnan(packed)
    u[nan] ^= np.uint32(0x00000001)  # other payloads, still NaN
    u[np.flatnonzero(nan)[::2]] ^= np.uint32(0x80000000)  # and the other sign on half of them
    assert np.isnan(packed[nan]).all()
    assert is_euc2d(ctx, xy, packed), "a NaN entry with another payload must still read as EUC_2D"
    k = R.row_offset(7) + 5
    assert u[k] == 0
    u[k] = 0x80000000  # -0.0 where the computed distance is +0.0: the bits differ, so not EUC_2D (the conservative answer)
    assert not is_euc2d(ctx, xy, packed)


def gpu_tour_length(ctx, perm, xy=None, packed=None):
    perm = np.ascontiguousarray(perm, dtype=np.uint32)
    out = C.c_float()
    ctx.check(ctx.lib.tl_tour_length(ctx.handle, _p(None if xy is None else np.ascontiguousarray(xy, F32)), _p(packed),
                                     len(perm), _p(perm), C.byref(out)))
    return F32(out.value)


def multiscale_xy(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 2)) * 10.0 ** rng.integers(-3, 5, (n, 1))).astype(F32)


def chunk_reversed_sum(edges):
    """The edge sum with each 1 024-wide chunk summed back to front: what a kernel that sums a chunk out of order returns."""
    total = F32(edges[0])
    for s in range(1, len(edges), 1024):
        for v in edges[s:s + 1024][::-1]:
            total = F32(total + v)
    return total


@pytest.mark.parametrize("n", [2, 3, 1023, 1024, 1025, 2048, 2049])
def test_tour_length_at_chunk_edges(ctx, n):
    xy = multiscale_xy(n, n)
    packed = O.dm_build_packed(xy)
    rng = np.random.default_rng(n)
    perms = {"restart": O.restart_perm(n, 1, 0), "identity": np.arange(n, dtype=np.uint32),
             "repeats": rng.integers(0, max(2, n // 3), n).astype(np.uint32)}
    for name, perm in perms.items():
        want = R.tour_length(perm, xy=xy)
        g_xy, g_dm = gpu_tour_length(ctx, perm, xy=xy), gpu_tour_length(ctx, perm, packed=packed)
        assert g_xy.tobytes() == want.tobytes(), (name, g_xy, want)
        assert g_dm.tobytes() == want.tobytes(), (name, g_dm, want)
        assert R.tour_length(perm, packed=packed).tobytes() == want.tobytes()
    if n >= 1025:  # the inputs are order-sensitive: any other order inside a chunk gives other bits
        e = R.tour_edges(perms["restart"], xy=xy)
        assert chunk_reversed_sum(e).tobytes() != R.tour_length(perms["restart"], xy=xy).tobytes()


def test_tour_length_nan_inf_and_bad_positions(ctx):
    from teeline_amd import _capi
    for n in (3, 1025, 2049):
        xy = multiscale_xy(n, 5)
        perm = O.restart_perm(n, 1, 0)
        packed = O.dm_build_packed(xy)
        for bad in (np.nan, np.inf):
            p2 = packed.copy()
            a, b = int(perm[n // 2]), int(perm[n // 2 + 1])
            p2[R.row_offset(max(a, b)) + min(a, b)] = bad
            got, want = gpu_tour_length(ctx, perm, packed=p2), R.tour_length(perm, packed=p2)
            assert R.bits_equal(got, want) and (np.isnan(got) if bad != bad else np.isposinf(got)), (n, bad, got, want)
        x2 = xy.copy()
        x2[perm[n - 1]] = (np.nan, 0.0)
        got = gpu_tour_length(ctx, perm, xy=x2)
        assert np.isnan(got) and R.bits_equal(got, R.tour_length(perm, xy=x2))
        x2 = xy.copy()
        x2[perm[0]] = (3e38, 0.0)
        x2[perm[1]] = (-3e38, 0.0)
        got = gpu_tour_length(ctx, perm, xy=x2)
        assert np.isposinf(got) and R.bits_equal(got, R.tour_length(perm, xy=x2))
        for form in ("xy", "dm"):
            p3 = perm.copy()
            p3[n - 1] = n
            out = C.c_float(12345.0)
            rc = ctx.lib.tl_tour_length(ctx.handle, _p(xy) if form == "xy" else None, _p(packed) if form == "dm" else None,
                                        n, _p(p3), C.byref(out))
            assert rc == _capi.TL_ERR_BADARG and out.value == 12345.0, (form, rc)


def test_tour_length_million_cities(ctx):
    n = 10**6
    xy = multiscale_xy(n, 9)
    perm = O.restart_perm(n, 1, 0)
    want = R.tour_length(perm, xy=xy)
    assert gpu_tour_length(ctx, perm, xy=xy).tobytes() == want.tobytes()
    assert O.tour_length(xy, None, perm).tobytes() == want.tobytes()


# ---- F: 64-bit offsets ---------------------------------------------------------------------------------------------------
BIG_HOST_GB = 40


def _host_available_gb():
    with open("/proc/meminfo") as fh:
        for line in fh:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / 2**20
    return 0.0


def _need_host_memory():
    avail = _host_available_gb()
    if avail < BIG_HOST_GB:
        pytest.skip(f"needs {BIG_HOST_GB} GB of available host memory for two 8.6 GB matrices, {avail:.1f} GB available")


def test_packed_offsets_above_2_31_elements():
    _need_host_memory()
    import teeline_amd as TA
    n = 65601
    m = n * (n - 1) // 2
    assert m > 2**31
    xy = O.synth_xy(n, seed=65601)
    with TA.Context(0) as big:  # its own context: the 8.6 GB device buffer goes with it
        out = np.empty(m, dtype=F32)
        big.check(big.lib.tl_dm_build(big.handle, _p(xy), n, 0, 0, _p(out), None))
        for i in (1, 2, 4097, 46341, 65535, 65536, 65537, 65600):
            R.assert_bits_equal(out[R.row_offset(i):R.row_offset(i) + i], R.euc_row(xy, i), f"row {i}")
        R.assert_bits_equal(out[-1:], R.euc_dist(xy[n - 1], xy[n - 2]).reshape(1), "last element")
        assert is_euc2d(big, xy, out)
        out.view(np.uint32)[-1] ^= np.uint32(1)
        assert not is_euc2d(big, xy, out), "a flip of the last element's low bit went unnoticed"
        out.view(np.uint32)[-1] ^= np.uint32(1)
        perm = O.restart_perm(n, 1, 0)
        want = R.tour_length(perm, xy=xy)
        assert R.tour_length(perm, packed=out).tobytes() == want.tobytes()
        assert gpu_tour_length(big, perm, packed=out).tobytes() == want.tobytes()
        assert gpu_tour_length(big, perm, xy=xy).tobytes() == want.tobytes()
        del out


def test_full_layout_above_2_31_entries():
    _need_host_memory()
    import teeline_amd as TA
    n = 46341
    assert n * n > 2**31
    xy = O.synth_xy(n, seed=46341)
    with TA.Context(0) as big:
        out = np.empty(n * n, dtype=F32)
        big.check(big.lib.tl_dm_build(big.handle, _p(xy), n, 0, 1, _p(out), None))
        full = out.reshape(n, n)
        for i in (0, 1, 2, 23170, 46339, 46340):
            want = R.euc_dist(xy[i], xy)
            want[i] = 0.0
            R.assert_bits_equal(full[i], want, f"full row {i}")
        del full, out
