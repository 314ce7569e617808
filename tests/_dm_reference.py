"""Plain restatements of the distance layer (csrc/dm_build.hip) for the tests.  TEST INFRASTRUCTURE ONLY.

EUC_2D (kdtree.rs:291-295): f32 dx, dy, f32 products, f32 sum, correctly rounded sqrt — in numpy, which does f32 arithmetic in
f32.  The sqrt is taken twice, as np.sqrt on f32 and as the f64 sqrt rounded to f32 (exact: 53 >= 2 * 24 + 2 bits), and the two
must agree.  GEO (distance_matrix.rs:59-75): the C oracle is the parity reference (it calls the host libm, as the reference
does); geo_mp here evaluates the same f64 formula with cos and acos correctly rounded, so that a failing comparison can say
which side left the correctly rounded result.

Comparisons are on f32 bit patterns; the only exception is NaN, where two NaNs count as equal whatever their payloads (the rule
of k_dm_compare_packed_rows).
"""
import math

import numpy as np

F32 = np.float32
GEO_RRR = 6378.388
GEO_PI = 3.14159265358979323846264338327950288  # std::f64::consts::PI, as an f64


# ---- layout --------------------------------------------------------------------------------------------------------------
def row_offset(i):
    """First packed index of row i of the strict lower triangle (distance_matrix.rs:177-191), as a Python int."""
    i = int(i)
    return i * (i - 1) // 2


def packed_ij(k):
    """(i, j), j < i, of packed index k."""
    k = int(k)
    i = (1 + math.isqrt(1 + 8 * k)) // 2
    while row_offset(i) > k:
        i -= 1
    while row_offset(i + 1) <= k:
        i += 1
    return i, k - row_offset(i)


# ---- comparison rule -----------------------------------------------------------------------------------------------------
def mismatches(got, want):
    """Flat indices where the f32 bit patterns differ, two NaNs counting as equal."""
    g = np.ascontiguousarray(got, dtype=F32).reshape(-1)
    w = np.ascontiguousarray(want, dtype=F32).reshape(-1)
    assert g.shape == w.shape, f"shape {g.shape} != {w.shape}"
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    return np.flatnonzero(bad)


def bits_equal(got, want):
    return mismatches(got, want).size == 0


def assert_bits_equal(got, want, what="", describe=None, limit=5):
    """Bit-for-bit equality under the NaN rule.  describe(flat_index) -> str adds a line per mismatch shown."""
    bad = mismatches(got, want)
    if bad.size == 0:
        return
    g = np.ascontiguousarray(got, dtype=F32).reshape(-1)
    w = np.ascontiguousarray(want, dtype=F32).reshape(-1)
    lines = [f"{what}: {bad.size} of {g.size} entries differ"]
    for k in bad[:limit].tolist():
        line = f"  [{k}] got {g[k]!r} ({int(g.view(np.uint32)[k]):#010x}) want {w[k]!r} ({int(w.view(np.uint32)[k]):#010x})"
        if describe is not None:
            line += "  " + describe(k)
        lines.append(line)
    raise AssertionError("\n".join(lines))


# ---- EUC_2D --------------------------------------------------------------------------------------------------------------
def euc_dist(a, b):
    """d(a, b) per kdtree.rs:291-295, a and b f32 arrays [..., 2] (broadcast): dx = a.x - b.x, dy = a.y - b.y."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32)
    with np.errstate(all="ignore"):
        dx = a[..., 0] - b[..., 0]
        dy = a[..., 1] - b[..., 1]
        s = dx * dx + dy * dy
        r = np.sqrt(s)
        r64 = np.sqrt(s.astype(np.float64)).astype(F32)
    assert r.dtype == F32 and bits_equal(r, r64), "np.sqrt(f32) and the f64 sqrt rounded to f32 disagree"
    return r


def euc_row(xy, i):
    """Packed row i: d(xy[i], xy[j]) for j < i."""
    xy = np.asarray(xy, dtype=F32)
    return euc_dist(xy[i], xy[:i])


def euc_packed(xy):
    xy = np.asarray(xy, dtype=F32)
    n = xy.shape[0]
    out = np.empty(n * (n - 1) // 2, dtype=F32)
    for i in range(1, n):
        out[row_offset(i):row_offset(i) + i] = euc_row(xy, i)
    return out


def full_from_packed(packed, n):
    """TL_DM_FULL from a packed matrix: (i, j) is the packed entry at (max, min), the diagonal is +0.0 (no arithmetic, so -0.0
    and NaN payloads pass through unchanged)."""
    packed = np.asarray(packed, dtype=F32)
    full = np.zeros((n, n), dtype=F32)
    for i in range(1, n):
        row = packed[row_offset(i):row_offset(i) + i]
        full[i, :i] = row
        full[:i, i] = row
    return full


def euc_full(xy):
    return full_from_packed(euc_packed(xy), np.asarray(xy).shape[0])


def degenerate_xy(n, seed):
    """Random points with duplicates, +-0.0 coordinates, magnitudes whose squares are subnormal or overflow, NaN and +-inf."""
    rng = np.random.default_rng(seed)
    xy = (rng.random((n, 2)) * 1000).astype(np.float32)
    kinds = [
        lambda k: xy[k - 1] if k else xy[k],                                    # duplicate of the previous point
        lambda k: np.array([0.0, -0.0], np.float32),
        lambda k: np.array([-0.0, 0.0], np.float32),
        lambda k: (rng.random(2) * 3e-21).astype(np.float32),                   # squares subnormal (or 0)
        lambda k: (rng.random(2) * 3e-23).astype(np.float32),                   # squares below the subnormal range
        lambda k: (rng.random(2) * 4e19 + 1.9e19).astype(np.float32),          # squares overflow to inf
        lambda k: np.array([-3.0e38, 3.0e38], np.float32),                      # dx itself overflows
        lambda k: np.array([np.nan, 1.0], np.float32),
        lambda k: np.array([np.inf, 2.0], np.float32),
        lambda k: np.array([3.0, -np.inf], np.float32),
    ]
    for k in range(0, n, 3):
        xy[k] = kinds[(k // 3) % len(kinds)](k)
    return xy


def decimal_grid_xy(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 100000, (n, 2)) / 100.0).astype(np.float32)


# ---- tour length ---------------------------------------------------------------------------------------------------------
def tour_edges(perm, xy=None, packed=None):
    """Edge lengths in the reference's summation order (distance_matrix.rs:235-245): the closing edge d(last, first) first,
    then d(w0, w1) along the tour.  Equal positions give 0.0 (:178-180, :198-200)."""
    perm = np.asarray(perm, dtype=np.int64)
    p = np.concatenate([perm[-1:], perm[:-1]])
    q = np.concatenate([perm[:1], perm[1:]])
    if packed is not None:
        hi, lo = np.maximum(p, q), np.minimum(p, q)
        e = np.asarray(packed, dtype=F32)[np.where(hi == lo, 0, hi * (hi - 1) // 2 + lo)]
    else:
        xy = np.asarray(xy, dtype=F32)
        e = euc_dist(xy[p], xy[q])
    return np.where(p == q, F32(0.0), e).astype(F32)


def tour_length(perm, xy=None, packed=None):
    """The sequential f32 sum of tour_edges (np.add.accumulate, not np.sum: that one sums pairwise)."""
    if len(perm) < 2:
        return F32(0.0)
    return np.add.accumulate(tour_edges(perm, xy, packed), dtype=F32)[-1]


# ---- GEO -----------------------------------------------------------------------------------------------------------------
def geo_to_rad(x):
    """distance_matrix.rs:59-75: truncf and the fraction in f32, the rest in f64 (Python floats), in the reference's order."""
    x = F32(x)
    deg = np.trunc(x)
    mn = float(x - deg)
    return GEO_PI * (float(deg) + 5.0 * mn / 3.0) / 180.0


def geo_host(p, q):
    """geo_distance(p, q) with the host libm (math.cos / math.acos): (f64 value before floor, f32 result)."""
    lat1, lon1, lat2, lon2 = geo_to_rad(p[0]), geo_to_rad(p[1]), geo_to_rad(q[0]), geo_to_rad(q[1])
    q1, q2, q3 = math.cos(lon1 - lon2), math.cos(lat1 - lat2), math.cos(lat1 + lat2)
    v = GEO_RRR * math.acos(0.5 * ((1.0 + q1) * q2 - (1.0 - q1) * q3)) + 1.0
    return v, F32(math.floor(v))


def _cr(f, x):
    import mpmath
    from mpmath.libmp import to_float
    with mpmath.workprec(256):
        return to_float(f(mpmath.mpf(x))._mpf_, rnd="n")


def geo_mp(p, q):
    """geo_distance(p, q) from the same f64 inputs with cos and acos correctly rounded to f64 (mpmath):
    (f64 value of RRR * acos(...) + 1 before floor, f32 result)."""
    import mpmath
    lat1, lon1, lat2, lon2 = geo_to_rad(p[0]), geo_to_rad(p[1]), geo_to_rad(q[0]), geo_to_rad(q[1])
    q1, q2, q3 = _cr(mpmath.cos, lon1 - lon2), _cr(mpmath.cos, lat1 - lat2), _cr(mpmath.cos, lat1 + lat2)
    arg = 0.5 * ((1.0 + q1) * q2 - (1.0 - q1) * q3)
    if not -1.0 <= arg <= 1.0:
        return math.nan, F32(math.nan)
    v = GEO_RRR * _cr(mpmath.acos, arg) + 1.0
    return v, F32(math.floor(v))


def describe_geo_packed(xy, got, want):
    """describe() for assert_bits_equal on a packed GEO matrix: the two points, both bit patterns and the mpmath value."""
    xy = np.asarray(xy, dtype=F32)

    def d(k):
        i, j = packed_ij(k)
        v, r = geo_mp(xy[i], xy[j])
        return (f"(i={i}, j={j}) p={xy[i].tolist()} q={xy[j].tolist()} gpu={int(F32(got[k]).view(np.uint32)):#010x} "
                f"oracle={int(F32(want[k]).view(np.uint32)):#010x} mpmath: {v!r} -> {float(r)!r}")
    return d


def tsplib_grid(rng, size, lat_deg=90, lon_deg=180):
    """TSPLIB GEO coordinates DDD.MM with MM < 60 over the whole globe (negative values included), as f32 [size, 2]."""
    def draw(top):
        deg = rng.integers(0, top + 1, size)
        mm = rng.integers(0, 60, size)
        sign = np.where(rng.random(size) < 0.5, -1.0, 1.0)
        return (sign * (deg * 100 + mm) / 100.0).astype(F32)
    return np.stack([draw(lat_deg), draw(lon_deg)], axis=1)


def near_tie_pairs(keep=2000, draws=2_000_000, seed=20240601):
    """A deterministic set of GEO pairs on the TSPLIB grid whose RRR * acos(...) + 1 lies nearest an integer, i.e. where the
    floor is most sensitive to the trig: draws `draws` grid pairs, evaluates them in long double, keeps the `keep` nearest.
    Returns (p [keep, 2] f32, q [keep, 2] f32, distance of each to the nearest integer, in long double)."""
    rng = np.random.default_rng(seed)
    p = tsplib_grid(rng, draws)
    q = tsplib_grid(rng, draws)
    same = np.all(p == q, axis=1)
    ld = np.longdouble

    def rad(x):
        deg = np.trunc(x)
        mn = (x - deg).astype(ld)
        return ld(GEO_PI) * (deg.astype(ld) + ld(5.0) * mn / ld(3.0)) / ld(180.0)

    lat1, lon1, lat2, lon2 = rad(p[:, 0]), rad(p[:, 1]), rad(q[:, 0]), rad(q[:, 1])
    q1, q2, q3 = np.cos(lon1 - lon2), np.cos(lat1 - lat2), np.cos(lat1 + lat2)
    arg = np.clip(ld(0.5) * ((1 + q1) * q2 - (1 - q1) * q3), -1, 1)
    v = ld(GEO_RRR) * np.arccos(arg) + 1
    gap = np.abs(v - np.rint(v))
    gap[same] = np.inf
    order = np.argpartition(gap, keep)[:keep]
    order = order[np.lexsort((order, gap[order]))]
    return p[order], q[order], gap[order]


def geo_special():
    """Grid points at the edges of the formula's domain: poles, the antimeridian, signed zero, minute fields >= .60 (accepted:
    5 * min / 3 is simply more than a degree)."""
    return np.array([[90.0, 180.0], [-90.0, -180.0], [90.0, -180.0], [-90.0, 180.0], [0.0, 180.0], [0.0, -180.0],
                     [-0.0, 0.0], [0.0, -0.0], [12.75, -45.99], [-45.99, 12.75], [89.6, 179.99], [-89.99, -179.6],
                     [0.6, -0.99], [-0.3, 179.59], [45.0, 0.6], [90.99, 180.99]], dtype=F32)


def geo_antipodal(rng, count):
    """Pairs (lat, lon), (-lat, lon -+ 180) on the grid: the acos argument is near -1."""
    a = tsplib_grid(rng, count, 89, 179)
    b = np.stack([-a[:, 0], np.where(a[:, 1] > 0, a[:, 1] - F32(180), a[:, 1] + F32(180))], axis=1).astype(F32)
    out = np.empty((2 * count, 2), F32)
    out[0::2], out[1::2] = a, b
    return out


def geo_ulp_clusters(rng, count):
    """Each grid point followed by copies offset by 1 to 8 f32 ulps in lat, lon or both: the acos argument is near +1."""
    base = tsplib_grid(rng, count)
    out = []
    for b in base:
        out.append(b)
        for k in range(1, 9):
            c = b.copy()
            axis = k % 3
            for ax in ((0,), (1,), (0, 1))[axis]:
                for _ in range(k):
                    c[ax] = np.nextafter(c[ax], F32(np.inf) if k % 2 else F32(-np.inf))
            out.append(c)
    return np.asarray(out, dtype=F32)


def geo_categories(rng, n):
    """n points of each GEO input category."""
    def take(a):
        return np.resize(a, (n, 2)).astype(F32)
    grid = tsplib_grid(rng, n)
    return {
        "grid": grid,
        "special": take(geo_special()),
        "random": ((rng.random((n, 2)) - 0.5) * np.array([200.0, 400.0])).astype(F32),
        "identical": take(np.repeat(grid[:max(1, n // 3)], 3, axis=0)),
        "antipodal": take(geo_antipodal(rng, n // 2 + 1)),
        "ulp_clusters": take(geo_ulp_clusters(rng, n // 9 + 1)),
    }


def geo_mix(n, seed, ties=None):
    """n GEO points: every category in blocks, shuffled block-wise, so that all of them meet in one matrix.  ties = (p, q): the
    near-tie pairs; pair k lands at rows (n_half + k, n_half + len(p) + k) if that fits, i.e. in a column slab >= 1 for n > 8192,
    and the first half of them also at (2k + 1, 2k)."""
    rng = np.random.default_rng(seed)
    cats = geo_categories(rng, n)
    blocks = []
    for name in cats:
        for s in range(0, n, 64):
            blocks.append(cats[name][s:s + 64])
    order = rng.permutation(len(blocks))
    xy = np.concatenate([blocks[k] for k in order])[:n].copy()
    if ties is not None:
        p, q = ties
        m = len(p)
        h = m // 2
        xy[1:2 * h:2], xy[0:2 * h:2] = p[:h], q[:h]
        base = n // 2
        if base >= 2 * h and base + 2 * m <= n:
            xy[base + m:base + 2 * m], xy[base:base + m] = p, q
    return xy
