"""Inputs for the neighbour layer (kdtree.hip, nn_knn.hip, the host decisions of tl_api_lk.hip) and, per input family, a counter of
the property the input exists to exercise.  TEST INFRASTRUCTURE ONLY (no tests here): tests/test_neighbour_cases.py asserts the
counters against the oracle alone, tests/test_gpu_neighbour_layer.py runs the inputs through the library.

Everything is plain numpy in float32 with every operation rounded (nothing fused), the oracle's arithmetic (oracle/tl_oracle.c
tlo_dist: dx*dx + dy*dy, then the correctly rounded sqrt).  Every builder is cached and hands out read-only arrays."""
import functools

import numpy as np

import _oracle as O

F32 = np.float32
EPS = F32(1.1920929e-07)  # f32::EPSILON, kdtree.rs:301-317


def _ro(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def sq_and_dist(xy, c):
    """Row c of squared and of rounded distances, float32 throughout."""
    xy = np.asarray(xy, dtype=F32)
    dx = xy[:, 0] - xy[c, 0]
    dy = xy[:, 1] - xy[c, 1]
    sq = dx * dx + dy * dy
    return sq, np.sqrt(sq)


# ------------------------------------------------------------------------------------------------
# A. packed matrices for the matrix-form NN walk (k_nn_seed_dm)
# ------------------------------------------------------------------------------------------------
DM_SIZES = (63, 64, 65, 1023, 1024, 1025, 2049, 3000)  # one partial wave .. three trips of the p += 1024 stride
DM_KINDS = ("a", "b", "c", "d", "e", "f")
# NaN entries are out of scope: the reference's min_by / k-buffer leave their order unspecified (partial_cmp), and the 2-opt NaN-row
# test (tests/test_gpu_distance_layer.py) starts from a tour of its own, never from this walk.


def dm_ks(n):
    return (1, 3, 5) if n == 1025 else (1, 3)


@functools.lru_cache(maxsize=None)
def dm_xy(n):
    return _ro(O.synth_xy(n, seed=700 + n))


@functools.lru_cache(maxsize=None)
def dm_packed(kind, n):
    """(a) Euclidean matrix of a synth_xy cloud; (b) integers 1..5: every row full of ties; (c) = (b) with ~10 % zeros; (d) negative to
    positive, integers and non-integers; (e) = (c) with the sign of half the zeros flipped; (f) = (a) with ~1 % +inf."""
    m = n * (n - 1) // 2
    rng = np.random.default_rng([ord(kind), n])
    if kind == "a":
        out = O.dm_build_packed(dm_xy(n))
    elif kind == "b":
        out = np.random.default_rng([ord("b"), n]).integers(1, 6, m).astype(F32)
    elif kind == "c":
        out = dm_packed("b", n).copy()
        out[np.random.default_rng([ord("c"), n]).random(m) < 0.10] = F32(0.0)
    elif kind == "d":
        ints = rng.integers(-3, 4, m).astype(F32)
        reals = (rng.random(m) * 5.0 - 2.5).astype(F32)
        out = np.where(rng.random(m) < 0.5, ints, reals).astype(F32)
    elif kind == "e":
        out = dm_packed("c", n).copy()
        zeros = np.flatnonzero(out == 0)
        out[zeros[rng.random(len(zeros)) < 0.5]] = F32(-0.0)
    elif kind == "f":
        out = dm_packed("a", n).copy()
        out[rng.random(m) < 0.01] = F32(np.inf)
    else:
        raise KeyError(kind)
    return _ro(np.ascontiguousarray(out, dtype=F32))


def rows_with_plus_zero_before_minus_zero(packed, n):
    """Rows of the full matrix (diagonal left out) in which some +0.0 sits at a lower position than some -0.0."""
    full = O.dm_expand_full(packed, n)
    zero = full == 0
    np.fill_diagonal(zero, False)
    neg = np.signbit(full)
    plus, minus = zero & ~neg, zero & neg
    pos = np.arange(n)
    first_plus = np.where(plus, pos, n).min(axis=1)
    last_minus = np.where(minus, pos, -1).max(axis=1)
    return int((first_plus < last_minus).sum())


def dm_walk_counters(packed, n, route):
    """Replays a walk over the matrix in numpy: every step must take the lowest position among the unvisited cities whose distance
    COMPARES equal to the minimum (+0.0 == -0.0).  Returns the counters of the steps on which that rule decided:
      tie_steps         two or more unvisited cities share the minimum
      mixed_zero_steps  ... and the shared minimum holds both +0.0 and -0.0
      plus_wins_steps   ... and the lowest position holds +0.0 (an order on the bit patterns would take a -0.0 instead)
      follows_rule      the walk is the rule's walk"""
    full = O.dm_expand_full(packed, n)
    route = np.asarray(route, dtype=np.int64)
    open_ = np.ones(n, dtype=bool)
    open_[route[0]] = False
    out = dict(tie_steps=0, mixed_zero_steps=0, plus_wins_steps=0, follows_rule=bool(route[0] == 0))
    for s in range(1, n):
        row = full[route[s - 1]]
        m = row[open_].min()
        tied = np.flatnonzero(open_ & (row == m))
        if tied[0] != route[s]:
            out["follows_rule"] = False
        if len(tied) >= 2:
            out["tie_steps"] += 1
            neg = np.signbit(row[tied])
            if m == 0 and neg.any() and not neg.all():
                out["mixed_zero_steps"] += 1
                out["plus_wins_steps"] += int(not neg[0])
        open_[route[s]] = False
    return out


# ------------------------------------------------------------------------------------------------
# D. rounding ties: different squares, one rounded distance
# ------------------------------------------------------------------------------------------------
# Integer offsets v with |v| in [4096, 4104) have float32 squares two apart (2^24 <= |v|^2 < 2^25) while the float32 distances
# are 2^-11 apart: the root's slope 1 / (2 * 4096) turns a step of 2 into half an ulp, so about every second pair of neighbouring
# squares rounds to one distance.
@functools.lru_cache(maxsize=None)
def tie_pairs():
    """[(offset with the larger square, offset with the smaller square)], same rounded length; integer offsets as float32 [2]."""
    rng = np.random.default_rng(4096)
    r = 4096.0 + 8.0 * rng.random(4000)
    phi = 2.0 * np.pi * rng.random(4000)
    v = np.unique(np.stack([np.rint(r * np.cos(phi)), np.rint(r * np.sin(phi))], 1), axis=0).astype(F32)
    sq = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    d = np.sqrt(sq)
    keep = (d >= 4096) & (d < 4104)
    v, sq, d = v[keep], sq[keep], d[keep]
    order = np.lexsort((sq, d))
    v, sq, d = v[order], sq[order], d[order]
    pairs = []
    t = 0
    while t + 1 < len(v):
        if d[t] == d[t + 1] and sq[t] != sq[t + 1]:
            pairs.append((v[t + 1].copy(), v[t].copy()))  # sorted by square inside one distance: t + 1 has the larger one
            t += 2
        else:
            t += 1
    return pairs


RING_BRUTE = [(n, k) for n in (17, 255, 257, 4097) for k in (4, 7, 16)]  # (n, list length) run through the brute-force builder
RING_KD = [(280, 5), (400, 8)]                                           # ... and through the kd-tree
HUB_PITCH = 131072.0  # hubs this far apart (>= 1e5): a ring's cities have all their neighbours inside the ring


def _grid(count):
    """`count` integer grid points around the origin (all four sign quadrants), as float32 [count, 2] times HUB_PITCH."""
    w = int(np.ceil(np.sqrt(count)))
    g = np.arange(count)
    return (np.stack([g % w - w // 2, g // w - w // 2], 1) * HUB_PITCH).astype(F32)


def _fillers(rng, count, lo, hi):
    r = lo + (hi - lo) * rng.random(count)
    phi = 2.0 * np.pi * rng.random(count)
    return np.stack([np.rint(r * np.cos(phi)), np.rint(r * np.sin(phi))], 1).astype(F32)


@functools.lru_cache(maxsize=None)
def tie_rings(n, k):
    """(xy, hubs): n cities; hub h is followed by its ring of min(k + 1, what is left) satellites, one tie pair among them.  On even
    hubs the pair takes the k-th and (k+1)-th place of the hub's neighbours (it straddles the end of a list of k), on odd hubs an
    earlier place; within a pair the city with the LARGER square has the LOWER position.  What n leaves over after the rings are
    lone cities on the same grid.  Coordinates are integers below 2^24: every difference is exact."""
    kk = min(k, n - 1)
    ring = min(kk + 1, n - 1)
    n_hubs = max(1, n // (ring + 1))
    lone = n - n_hubs * (ring + 1)
    centres = _grid(n_hubs + lone)
    pairs = tie_pairs()
    rng = np.random.default_rng([n, k])
    xy, hubs = [], []
    for h in range(n_hubs):
        big, small = pairs[(h * 7 + n) % len(pairs)]
        straddle = h % 2 == 0 and ring == kk + 1
        place = kk if straddle else 1 + (h // 2) % max(1, ring - 1)   # 1-based place of the pair's first city
        near = _fillers(rng, place - 1, 2000.0, 4000.0)
        far = _fillers(rng, ring - 2 - (place - 1), 4200.0, 6000.0)
        rest = rng.permutation(np.concatenate([near, far]))
        slots = np.sort(rng.choice(ring, 2, replace=False))            # where the pair sits among the ring's positions
        sat = np.empty((ring, 2), F32)
        sat[slots[0]], sat[slots[1]] = big, small
        sat[np.setdiff1d(np.arange(ring), slots)] = rest
        hubs.append(len(xy))
        xy.append(centres[h])
        xy.extend(centres[h] + sat)
    xy.extend(centres[n_hubs:])
    xy = np.ascontiguousarray(np.array(xy, dtype=F32).reshape(-1, 2))
    assert xy.shape == (n, 2) and np.abs(xy).max() < 2 ** 24
    return _ro(xy, np.array(hubs, dtype=np.int64))


def ring_counters(xy, hubs, k):
    """adjacent: hubs whose first k+1 neighbours in (distance, position) order hold, next to each other, two cities at one rounded
    distance with different squares; straddling: ... at the k-th and (k+1)-th place, the larger square first (the lower position)."""
    n = len(xy)
    kk = min(k, n - 1)
    adjacent = straddling = 0
    for h in hubs:
        sq, d = sq_and_dist(xy, h)
        order = np.argsort(d, kind="stable")
        order = order[order != h][:kk + 1]
        hit = np.flatnonzero((d[order][:-1] == d[order][1:]) & (sq[order][:-1] != sq[order][1:]))
        adjacent += int(len(hit) > 0)
        straddling += int(any(t == kk - 1 and sq[order][t] > sq[order][t + 1] for t in hit))
    return dict(adjacent=adjacent, straddling=straddling, hubs=len(hubs))


@functools.lru_cache(maxsize=None)
def duplicated_lattice(n):
    """A shuffled integer lattice whose last third repeats earlier points: equal squares and zero distances."""
    m = n - n // 3
    w = int(np.ceil(np.sqrt(m)))
    g = np.stack([np.arange(m) % w, np.arange(m) // w], 1).astype(F32)
    g = g[np.random.default_rng(n).permutation(m)]
    return _ro(np.ascontiguousarray(np.concatenate([g, g[:n - m]])))


# ------------------------------------------------------------------------------------------------
# B. clouds for the kd-tree lists
# ------------------------------------------------------------------------------------------------
KD_SIZES = (2, 3, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025)  # around 2^h (the level count), the 256-lane blocks and their tails
KD_KS = (1, 5, 8, 9, 16, 17)                                    # both sides of every KMAX bucket edge up to 32


@functools.lru_cache(maxsize=None)
def kd_shifted(n):
    """synth_xy moved by (-500, -500): all four sign quadrants (the ~b branch of the sortable key)."""
    return _ro(O.synth_xy(n, seed=900 + n) - F32(500.0))


@functools.lru_cache(maxsize=None)
def kd_signed_zeros(n=600):
    """A third of the x and a third of the y coordinates are exactly +0.0 or -0.0, mixed; the rest are signed."""
    rng = np.random.default_rng(600)
    xy = (rng.random((n, 2)) * 1000.0 - 500.0).astype(F32)
    for c in range(2):
        idx = rng.permutation(n)[:n // 3]
        xy[idx, c] = np.where(rng.random(len(idx)) < 0.5, F32(0.0), F32(-0.0))
    return _ro(np.ascontiguousarray(xy))


def signed_zero_counts(xy):
    z, neg = xy == 0, np.signbit(xy)
    return dict(plus_x=int((z & ~neg)[:, 0].sum()), minus_x=int((z & neg)[:, 0].sum()), plus_y=int((z & ~neg)[:, 1].sum()),
                minus_y=int((z & neg)[:, 1].sum()), negative=int((xy < 0).sum()), positive=int((xy > 0).sum()))


@functools.lru_cache(maxsize=None)
def kd_equal_families(n=800):
    """Coordinates from families {v, nextafter(v, +inf), nextafter(v, -inf)} at |v| in {1, 1000, 1e6} (times 1, 1.25, 1.5, 1.75, both
    signs): many pairs compare Equal under the relative tolerance of kdtree.rs:301-317 while being different floats."""
    rng = np.random.default_rng(800)
    base = np.array([s * m * f for m in (1.0, 1000.0, 1e6) for s in (1.0, -1.0) for f in (1.0, 1.25, 1.5, 1.75)], dtype=F32)
    fam = np.stack([base, np.nextafter(base, F32(np.inf)), np.nextafter(base, F32(-np.inf))], 1)
    xy = fam[rng.integers(0, len(base), (n, 2)), rng.integers(0, 3, (n, 2))]
    return _ro(np.ascontiguousarray(xy, dtype=F32))


def cmp_coord(a, b):
    """kdtree.rs:301-317 in float32: -1 Less, 0 Equal, +1 Greater with tol = max(|a|, |b|) * f32::EPSILON."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    tol = np.maximum(np.abs(a), np.abs(b)) * EPS
    return np.where(np.abs(a - b) <= tol, 0, np.where(a < b, -1, 1))


def equal_but_different_pairs(v):
    """City pairs whose coordinate values differ in bits yet compare Equal."""
    v = np.asarray(v, dtype=F32)
    c = cmp_coord(v[:, None], v[None, :])
    diff = bits(v)[:, None] != bits(v)[None, :]
    return int(np.triu((c == 0) & diff, 1).sum())


@functools.lru_cache(maxsize=None)
def kd_large_magnitude(n=1000):
    """A cloud offset to (1e6, -1e6): the float32 grid there is 1/16, the tolerance about two grid steps."""
    return _ro(np.ascontiguousarray(O.synth_xy(n, seed=31) + np.array([1e6, -1e6], dtype=F32)))


# ------------------------------------------------------------------------------------------------
# C. numpy reference for sampled rows of the brute-force lists
# ------------------------------------------------------------------------------------------------
KNN_KMAX = 33


def sample_rows(n, count=1024):
    """Rows 0..63, the last 130 (the tail block, where most lanes have c >= n) and a random rest."""
    fixed = np.unique(np.concatenate([np.arange(min(64, n)), np.arange(max(0, n - 130), n)]))
    rest = np.setdiff1d(np.arange(n), fixed)
    rest = rest[np.random.default_rng(n).permutation(len(rest))[:max(0, count - len(fixed))]]
    return np.sort(np.concatenate([fixed, rest]))


def knn_rows_numpy(xy, rows, k):
    """Lists of `rows`: float32 squares dx*dx + dy*dy, np.sqrt in float32, self dropped, stable sort by (distance, position), first k.
    (Only the cities no farther than the (k+2)-th smallest distance are sorted: the first k of the whole row are among them.)"""
    xy = np.asarray(xy, dtype=F32)
    out = np.empty((len(rows), k), dtype=np.uint32)
    for t, c in enumerate(rows):
        _, d = sq_and_dist(xy, c)
        near = np.flatnonzero(d <= np.partition(d, k + 1)[k + 1]) if len(d) > k + 2 else np.arange(len(d))  # ascending positions
        order = near[np.argsort(d[near], kind="stable")]
        out[t] = order[order != c][:k]
    return out


@functools.lru_cache(maxsize=None)
def oracle_dm_walk(kind, n, k):
    """(route, cost) of the oracle's walk over dm_packed(kind, n): computed once, shared, left unchanged."""
    rc, route, cost = O.nearest_neighbor(None, dm_packed(kind, n), n, k)
    assert rc == 0
    return _ro(route), cost


@functools.lru_cache(maxsize=None)
def oracle_xy_walk(n, seed, k):
    rc, route, cost = O.nearest_neighbor(O.synth_xy(n, seed=seed), None, n, k)
    assert rc == 0
    return _ro(route), cost


@functools.lru_cache(maxsize=None)
def knn_sampled_reference(n, seed):
    """(xy, rows, lists [len(rows), 33]) of a synth_xy cloud: the lists for a shorter k are their first k columns."""
    xy = O.synth_xy(n, seed=seed)
    rows = sample_rows(n)
    return _ro(xy, rows, knn_rows_numpy(xy, rows, KNN_KMAX))


# ------------------------------------------------------------------------------------------------
# E. NN seed: a fallback scan that a rounding tie decides
# ------------------------------------------------------------------------------------------------
LOOP_AXIS = 16390  # with its ring beyond 16 384 cities: the fallback scans run in the loop form (NQ = 0)


@functools.lru_cache(maxsize=None)
def fallback_instance(seed, axis=6):
    """Cities 0..axis-1 on the x axis at unit spacing — the walk is 0 -> 1 -> ... -> axis-1 and the last city's short list is
    exhausted — and one ring centred on the last city, nothing else.  The ring's nearest two cities are a tie pair, the larger
    square at the lower position."""
    rng = np.random.default_rng([seed, axis])
    pairs = tie_pairs()
    big, small = pairs[(seed * 11 + axis) % len(pairs)]
    far = _fillers(rng, 6, 4200.0, 6000.0)
    slots = np.sort(rng.choice(8, 2, replace=False))
    ring = np.empty((8, 2), F32)
    ring[slots[0]], ring[slots[1]] = big, small
    ring[np.setdiff1d(np.arange(8), slots)] = far
    line = np.stack([np.arange(axis), np.zeros(axis)], 1).astype(F32)
    return _ro(np.ascontiguousarray(np.concatenate([line, line[-1] + ring]), dtype=F32))


def fallback_counter(xy, route, axis):
    """The step that leaves the axis, replayed: True iff the walk came along the axis, the minimum rounded distance from its end is
    shared by two unvisited cities with different squares, the lower position has the larger square (so the smallest square is NOT
    the answer) and the walk took the lower position."""
    route = np.asarray(route, dtype=np.int64)
    if route[:axis].tolist() != list(range(axis)):
        return False
    sq, d = sq_and_dist(xy, axis - 1)
    rest = np.arange(axis, len(xy))
    tied = rest[d[rest] == d[rest].min()]
    return bool(len(tied) == 2 and sq[tied[0]] > sq[tied[1]] and rest[np.argmin(sq[rest])] == tied[1] and route[axis] == tied[0])
