"""Instances and two numpy restatements for TL_MODE_BEST_SWEEP (two_opt_best.hip).  TEST INFRASTRUCTURE ONLY (no tests here).

The oracle (oracle/tl_oracle.c tlo_two_opt_best) costs O(moves * n^2 / 2), so every start is a few moves away from a best-sweep fixed
point: a fixed point with a handful of position ranges reversed ("plants").  Two families:

  snake     a unit lattice walked boustrophedon (partial last row allowed): every tour edge is 1 and any two cities are >= 1 apart, so
            no 2-opt move improves.  City ids are shuffled.  Distances are square roots of integers: ties everywhere.
  uniform   O.synth_xy points, the REF_ORDER local optimum from the NN seed (the same candidate set and the same `neu < cur` rule as
            best-sweep, so a fixed point of it too).  Real geometry for the L0 pruning.

ref_best_sweep is the plain specification (every candidate of every sweep); model_best_sweep restates the kernel's own scheme — row
cache, column-restricted rescan, tile groups with L0 liveness, tile rebuild, packed key — line by line, records which branch every row
took, and can carry exactly one planted error (DEFECTS).  THE ORACLE DECIDES what is expected; the model only says which path was taken."""
import functools

import numpy as np

import _oracle as O

F32 = np.float32
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)  # two_opt_best.hip:24   kNoKey64
MAX_N = 65535                          # tl_api_two_opt.hip:782


# ------------------------------------------------------------------------------------------------
# instances
# ------------------------------------------------------------------------------------------------
def snake_width(n):
    return 257 if n > 16384 else 65  # 65535 = 255 x 257; the small snakes' rows (65) do not line up with the 64-column tiles


@functools.lru_cache(maxsize=None)
def _snake_base(n):
    w = snake_width(n)
    k = np.arange(n)
    r, c = k // w, k % w
    lattice = np.stack([np.where(r % 2 == 0, c, w - 1 - c), r], 1).astype(F32)
    tour = O.restart_perm(n, 4096 + n, 0)  # position k holds city tour[k]: a position is not a city
    xy = np.empty((n, 2), F32)
    xy[tour] = lattice
    return xy, tour


@functools.lru_cache(maxsize=None)
def _uniform_base(n, seed):
    xy = O.synth_xy(n, seed=seed)
    rc, nn, _ = O.nearest_neighbor(xy, None, n, 3)
    rc2, opt, _, _ = O.two_opt(xy, None, n, init=nn)
    assert rc == 0 and rc2 == 0
    return xy, opt


def plant(tour, plants):
    tour = np.array(tour, dtype=np.uint32)
    for a, b in plants:
        assert 1 <= a < b <= len(tour) - 2, (a, b)  # the undoing move (a-1, b) is a candidate of the open path
        tour[a:b + 1] = tour[a:b + 1][::-1].copy()
    return tour


def snake(n, plants=()):
    xy, tour = _snake_base(n)
    return xy, plant(tour, plants)


def uniform(n, seed, plants=()):
    xy, tour = _uniform_base(n, seed)
    return xy, plant(tour, plants)


class Case:
    def __init__(self, family, n, plants, what, seed=0):
        self.family, self.n, self.plants, self.what, self.seed = family, n, tuple(plants), what, seed
        self.id = f"{family}{n}" + (f"s{seed}" if family == "uniform" else "") + "-" + what.split(":")[0].replace(" ", "_")

    def build(self):
        xy, tour = snake(self.n, self.plants) if self.family == "snake" else uniform(self.n, self.seed, self.plants)
        xy.setflags(write=False)
        tour.setflags(write=False)
        return xy, tour


# Position ranges [a, b] reversed in this order; the move that undoes one alone is (i, j) = (a-1, b).
CASES = [
    Case("snake", 4098, [(4095, 4096), (3000, 4096), (100, 163)], "first group-1 column: j = 4096 = n-2 at n = 4098, then the last row i = n-4"),
    Case("snake", 4160, [(64, 200), (4157, 4158), (4100, 4158), (2000, 3100)], "n mod 64 = 0: both ends in group 1, j = n-2, i = n-4, js - is > 1024"),
    Case("snake", 4161, [(1000, 2000), (1500, 2500), (4097, 4159), (228, 569), (570, 639)], "n mod 64 = 1: crossing plants, adjacent plants (column is)"),
    Case("snake", 4223, [(128, 181), (4, 12), (140, 155), (128, 163), (125, 143), (4220, 4221), (4100, 4221)], "n mod 64 = 63: a knot of five plants where a tie decides the path"),
    Case("snake", 4224, [(3000, 4150), (4100, 4200), (192, 1300), (192, 700), (4221, 4222)], "five plants, two overlapping: i < 4096 <= j and both >= 4096"),
    Case("snake", 4224, [(128, 1381), (330, 1381), (2500, 2565), (2630, 2695)], "twenty touched tiles: plants that share their right end, twin plants (tie between rows)"),
    Case("snake", 300, [(64, 106), (212, 241), (256, 264), (64, 138), (64, 74)], "small: nested plants that share their left end (column js)"),
    Case("snake", 300, [(131, 184), (151, 262)], "small tie: 33 columns of the winning row tie"),
    Case("uniform", 400, [(14, 191), (192, 325)], "small: adjacent plants, the tile of is after a move", seed=286),
    Case("uniform", 700, [(128, 321), (192, 447), (128, 447)], "small: the tile of js after a move", seed=5),
    Case("uniform", 4200, [(2744, 3623), (1613, 1817), (258, 981), (679, 1638), (1792, 2888), (909, 1176), (986, 2361), (2783, 3529), (832, 1834),
                           (2729, 4124)], "ten random reversals", seed=1),
    Case("uniform", 4200, [(204, 1123), (3147, 4119), (2886, 3407), (2354, 2725), (570, 1875), (770, 1589), (599, 1934), (2695, 3790)],
         "eight random reversals", seed=2),
    Case("uniform", 4200, [(520, 1829), (342, 982), (2940, 3515), (1260, 2586), (2471, 2760), (1814, 3197), (904, 1525), (2236, 2613), (879, 2270),
                           (869, 2317), (2101, 3539), (2468, 3109)], "twelve random reversals", seed=3),
    Case("uniform", 8300, [(3424, 4264), (5810, 6760), (4157, 4664), (5389, 6864), (2586, 3521), (7000, 8250)], "third tile group", seed=4),
]

GOLDEN_CASE = Case("snake", 65535, [(65532, 65533), (65000, 65533), (40000, 50000), (20000, 36000)], "golden: i and j beyond 32767, j = n-2, i = n-4")


def case_table():
    return list(CASES)


# ------------------------------------------------------------------------------------------------
# f32 arithmetic in the oracle's operation order (oracle/tl_oracle.c tlo_dist: dx*dx + dy*dy, then the correctly rounded sqrt)
# ------------------------------------------------------------------------------------------------
def _sqd(p, q):
    dx = p[..., 0] - q[..., 0]
    dy = p[..., 1] - q[..., 1]
    return dx * dx + dy * dy  # float32 arrays: every operation rounds to f32, nothing is fused


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def cost_bits(xy, tour):
    return int(np.float32(O.tour_length(xy, None, tour)).view(np.uint32))


# ------------------------------------------------------------------------------------------------
# the plain specification
# ------------------------------------------------------------------------------------------------
def ref_best_sweep(xy, tour, max_sweeps=None, rows_per_chunk=256):
    """tlo_two_opt_best restated: per sweep every (i, j), j in [i+2, n-2], decided in f32; improving iff neu < cur; the winner has the
    lowest delta = neu - cur, then the lowest (i, j); swap_2opt(i+1, j).  Returns a dict: tour, cost_bits, sweeps, moves, reversed,
    move_list [(i, j, delta bits)], ties [(rows whose best delta equals the winner's, columns of the winning row that do)]."""
    xy = np.ascontiguousarray(xy, dtype=F32)
    tour = np.array(tour, dtype=np.uint32)
    n = len(tour)
    sweeps = moves = reversed_ = 0
    move_list, ties = [], []
    while max_sweeps is None or sweeps < max_sweeps:
        sweeps += 1
        P = xy[tour]
        edge = np.sqrt(_sqd(P[:-1], P[1:]))  # edge[k] = D(p[k], p[k+1])
        rowmin = np.full(n, np.inf, F32)
        rowarg = np.zeros(n, np.int64)
        rowcnt = np.zeros(n, np.int64)
        for i0 in range(0, n - 3, rows_per_chunk):
            i = np.arange(i0, min(i0 + rows_per_chunk, n - 3))
            j = np.arange(i0 + 2, n - 1)
            neu = np.sqrt(_sqd(P[i][:, None, :], P[j][None, :, :])) + np.sqrt(_sqd(P[i + 1][:, None, :], P[j + 1][None, :, :]))
            cur = edge[i][:, None] + edge[j][None, :]
            delta = np.where((j[None, :] >= i[:, None] + 2) & (neu < cur), neu - cur, F32(np.inf))
            arg = delta.argmin(1)  # the first of equal minima: the lowest j
            rowmin[i] = delta[np.arange(len(i)), arg]
            rowarg[i] = j[arg]
            rowcnt[i] = (delta == rowmin[i][:, None]).sum(1)
        bi = int(rowmin.argmin())  # the first of equal minima: the lowest i
        if not rowmin[bi] < np.inf:
            break
        bj = int(rowarg[bi])
        move_list.append((bi, bj, int(_bits(rowmin[bi:bi + 1])[0])))
        ties.append((int((rowmin == rowmin[bi]).sum()), int(rowcnt[bi])))
        tour[bi + 1:bj + 1] = tour[bi + 1:bj + 1][::-1].copy()
        moves += 1
        reversed_ += bj - bi
    return {"tour": tour, "cost_bits": cost_bits(xy, tour), "sweeps": sweeps, "moves": moves, "reversed": reversed_,
            "move_list": move_list, "ties": ties}


# ------------------------------------------------------------------------------------------------
# the kernel's scheme, restated
# ------------------------------------------------------------------------------------------------
DEFECTS = {
    "a": "a tie goes to the highest (i, j)",
    "b": "key without the ~: the smallest |delta| wins",
    "c": "rows in [is, js] keep their cached key",
    "d": "rows < is always take min(cached, partial), even when the cached column is in [is, js]",
    "e": "rows < is keep the cached key, no partial rescan",
    "f": "partial range [is+1, js]",
    "g": "partial range [is, js-1]",
    "h": "a row's scan stops after its first tile group",
    "i": "decode mask 0x7FFF on i",
    "j": "decode mask 0x7FFF on j",
    "k": "tile (lo-1)>>6 not rebuilt after a move (the rebuild starts at lo>>6)",
    "l": "tile hi>>6 not rebuilt (the rebuild ends before it)",
    "m": "the rebuild covers only the first 16 touched tiles (no stride loop)",
}
# (None is equivalent on all inputs, so none was removed; tests/test_best_sweep_cases.py says which case kills each.  k is the rare one: only
#  lane 63 of tile (lo-1)>>6 has a new e, so only a winner at column exactly `is`, live through box_lb(b, box) < msq alone, with the edge
#  (p[is], p[is+1]) made longer by the move, can tell — found by filtering adjacent plant pairs of uniform tours on that geometry.)

# the branch a row took in a sweep (record["branch"][sweep][row])
BR_NONE, BR_AFRESH, BR_KEPT, BR_CACHED_COL_IN_RANGE, BR_PARTIAL_WINS, BR_PARTIAL_LOSES = 0, 1, 2, 3, 4, 5


class WildMove(Exception):
    """A defect decoded a move that is no candidate (the kernel would index out of range): the run differs from the oracle's."""


def _box_lb(p, box):
    """two_opt_common.h:102-115  box_lb: d = max(lo - p, p - hi, 0) per axis, d.x^2 + d.y^2.  p [R, 2], box [T, 4] -> [R, T]."""
    ux = box[None, :, 0] - p[:, None, 0]  # :105   u = lo - p
    uy = box[None, :, 1] - p[:, None, 1]
    vx = p[:, None, 0] - box[None, :, 2]  # :105   v = p - hi
    vy = p[:, None, 1] - box[None, :, 3]
    dx = np.maximum(np.maximum(ux, vx), F32(0))  # :111-112 (taken on the bit patterns there: the same for non-NaN values)
    dy = np.maximum(np.maximum(uy, vy), F32(0))
    return dx * dx + dy * dy  # :113-114


class _Model:
    def __init__(self, xy, tour, defect):
        assert defect is None or defect in DEFECTS
        self.defect = defect
        self.n = n = len(tour)
        assert 4 <= n <= MAX_N
        self.xy = np.ascontiguousarray(xy, dtype=F32)
        self.n_pad = ((n + 64 + 63) // 64) * 64                    # tl_api_two_opt.hip:227
        self.ntile = self.n_pad >> 6                               # two_opt_best.hip:39
        self.ntile_cap = (((self.n_pad >> 6) + 63) // 64) * 64     # tl_api_two_opt.hip:227
        self.perm = np.array(tour, dtype=np.uint32)
        self.P = np.zeros((self.n_pad + 1, 2), F32)                # two_opt_best.hip:43   k < n ? xy[perm[k]] : (0, 0), k <= npad
        self.P[:n] = self.xy[self.perm]
        inf = F32(np.inf)
        self.tbox = np.tile(np.array([inf, inf, -inf, -inf], F32), (self.ntile_cap, 1))  # two_opt_best.hip:50   pad tiles: the empty box
        self.tmsq = np.full(self.ntile_cap, -1.0, F32)                                   # two_opt_best.hip:51
        self.build_tile_meta(np.arange(self.ntile))                                      # two_opt_best.hip:47   t < ntile
        self.rowkey = np.full(n, NOKEY, np.uint64)
        self.mv, self.is_, self.js = 0, 0, 0  # A.move: zeroed with the counters (tl_api_two_opt.hip:793,799)
        self.sweeps = self.moves = self.reversed = 0
        self.move_list = []
        self.record = {"branch": [], "g0": [], "g1": [], "partial_col": []}

    # -- two_opt_common.h:76-94
    def build_tile_meta(self, ts):
        if len(ts) == 0:
            return
        j = (ts[:, None] << 6) + np.arange(64)[None, :]            # :78
        valid = j + 2 <= self.n                                    # :79   j <= n-2
        c, e = self.P[j], self.P[j + 1]                            # :80
        inf = F32(np.inf)
        self.tbox[ts, 0] = np.where(valid, np.minimum(c[..., 0], e[..., 0]), inf).min(1)   # :83
        self.tbox[ts, 1] = np.where(valid, np.minimum(c[..., 1], e[..., 1]), inf).min(1)
        self.tbox[ts, 2] = np.where(valid, np.maximum(c[..., 0], e[..., 0]), -inf).max(1)  # :84
        self.tbox[ts, 3] = np.where(valid, np.maximum(c[..., 1], e[..., 1]), -inf).max(1)
        self.tmsq[ts] = np.where(valid, _sqd(c, e), F32(0)).max(1)                         # :85-86   invalid lanes: 0

    # -- the packed key, two_opt_best.hip:90
    def pack(self, delta, i, j):
        d = _bits(delta).astype(np.uint64)
        if self.defect != "b":
            d = d ^ np.uint64(0xFFFFFFFF)                          # ~delta bits
        ij = (i.astype(np.uint64) << np.uint64(16)) | j.astype(np.uint64)
        if self.defect == "a":
            ij = ij ^ np.uint64(0xFFFFFFFF)                        # the highest (i, j) has the lowest key
        return (d << np.uint64(32)) | ij

    def unpack(self, key):
        ij = int(key) & 0xFFFFFFFF
        if self.defect == "a":
            ij ^= 0xFFFFFFFF
        return (ij >> 16) & 0xFFFF, ij & 0xFFFF                    # two_opt_best.hip:166

    def key_col(self, keys):
        ij = keys & np.uint64(0xFFFFFFFF)
        if self.defect == "a":
            ij = ij ^ np.uint64(0xFFFFFFFF)
        return (ij & np.uint64(0xFFFF)).astype(np.int64)           # two_opt_best.hip:124   cj = ck & 0xFFFF

    # -- two_opt_best.hip:57-96  bs_row_best for the rows `rows`, columns [jlo, jhi]; also the first and last tile group each row visits
    def row_best(self, rows, jlo, jhi, chunk_elems=1 << 22):
        n, P = self.n, self.P
        best = np.full(len(rows), NOKEY, np.uint64)                # :60
        g0 = np.full(len(rows), -1, np.int64)
        g1 = np.full(len(rows), -1, np.int64)
        if len(rows) == 0:
            return best, g0, g1
        jmin = np.maximum(rows + 2, jlo)                           # :64
        jmax = np.minimum(n - 2, jhi) + 0 * rows                   # :64
        ok = jmin <= jmax                                          # :65
        tmin, tmax = jmin >> 6, jmax >> 6                          # :66
        g0[ok] = tmin[ok] >> 6                                     # :67   g = tmin >> 6 ...
        g1[ok] = (tmin[ok] >> 6) if self.defect == "h" else (tmax[ok] >> 6)  # :67   ... <= tmax >> 6
        if not ok.any():
            return best, g0, g1
        tl = np.arange(int(g0[ok].min()) << 6, (int(g1[ok].max()) + 1) << 6)  # :68   tl = (g << 6) + lane, every group some row visits
        box, msq = self.tbox[tl], self.tmsq[tl]                    # :69-70   (an index beyond ntile_cap raises here)
        step = max(1, chunk_elems // len(tl))
        for r0 in range(0, len(rows), step):
            sl = slice(r0, min(r0 + step, len(rows)))
            i = rows[sl]
            a, b = P[i], P[i + 1]                                  # :61
            sqab = _sqd(a, b)                                      # :62
            grp = tl[None, :] >> 6
            live = (ok[sl, None] & (grp >= g0[sl, None]) & (grp <= g1[sl, None])             # :67   the groups of this row's loop
                    & (tl[None, :] >= tmin[sl, None]) & (tl[None, :] <= tmax[sl, None])      # :71
                    & ((_box_lb(a, box) < sqab[:, None]) | (_box_lb(b, box) < msq[None, :])))  # :71   L0
            r, t = np.nonzero(live)                                # :72-75   the live tiles of each row
            if len(r) == 0:
                continue
            j = (tl[t][:, None] << 6) + np.arange(64)[None, :]     # :76
            c, e = P[j], P[j + 1]                                  # :77
            ar, br = a[r][:, None, :], b[r][:, None, :]
            sqce, s1, s2 = _sqd(c, e), _sqd(ar, c), _sqd(br, e)    # :78
            # (L1 :79 and L2 :82-84 only discard what cannot improve; they keep no state and are not restated)
            neu = np.sqrt(s1) + np.sqrt(s2)                        # :86
            cur = np.sqrt(sqab[r])[:, None] + np.sqrt(sqce)        # :87
            imp = (j >= jmin[sl][r][:, None]) & (j <= jmax[sl][r][:, None]) & (neu < cur)   # :79, :88
            key = np.where(imp, self.pack(neu - cur, np.broadcast_to(i[r][:, None], j.shape), j), NOKEY)  # :89-90
            np.minimum.at(best, r0 + r, key.min(1))                # :91, :95
        return best, g0, g1

    # -- two_opt_best.hip:106-141  k_bs_scan, all rows of one sweep; returns the sweep's best key (:138-139 and :150-158 are a plain minimum)
    def scan(self):
        n, d = self.n, self.defect
        rows = np.arange(n - 3)                                    # :114   i + 3 < n
        branch = np.full(n, BR_NONE, np.int8)
        G0 = np.full(n, -1, np.int64)
        G1 = np.full(n, -1, np.int64)
        pcol = np.full(n, -1, np.int64)
        is_, js = self.is_, self.js                                # :116
        if self.mv == 0:                                           # :117
            fresh, kept, front = rows, rows[:0], rows[:0]
        else:
            fresh = rows[(rows >= is_) & (rows <= js)]             # :117
            kept = rows[rows > js]                                 # :120
            front = rows[rows < is_]                               # :122
        if d == "c" and self.mv != 0:
            kept, fresh = np.concatenate([fresh, kept]), rows[:0]
        best, G0[fresh], G1[fresh] = self.row_best(fresh, 0, n)    # :118
        self.rowkey[fresh] = best                                  # :119
        branch[fresh] = BR_AFRESH
        branch[kept] = BR_KEPT                                     # :121
        if len(front):
            ck = self.rowkey[front]                                # :123
            cj = self.key_col(ck)                                  # :124
            inr = (ck != NOKEY) & (cj >= is_) & (cj <= js)         # :125
            if d in ("d", "e"):
                inr[:] = False
            full, part = front[inr], front[~inr]
            best, G0[full], G1[full] = self.row_best(full, 0, n)   # :126
            self.rowkey[full] = best                               # :131
            branch[full] = BR_CACHED_COL_IN_RANGE
            if d == "e":
                branch[part] = BR_KEPT
            else:
                plo, phi = (is_ + 1 if d == "f" else is_), (js - 1 if d == "g" else js)
                pk, G0[part], G1[part] = self.row_best(part, plo, phi)   # :128
                ckp = self.rowkey[part]
                wins = pk < ckp
                self.rowkey[part] = np.where(wins, pk, ckp)        # :129, :131
                branch[part] = np.where(wins, BR_PARTIAL_WINS, BR_PARTIAL_LOSES)
                pcol[part[wins]] = self.key_col(pk[wins])
        for k, v in (("branch", branch), ("g0", G0), ("g1", G1), ("partial_col", pcol)):
            self.record[k].append(v)
        return self.rowkey[:n - 3].min() if n > 3 else NOKEY

    # -- two_opt_best.hip:143-188  k_bs_apply
    def apply(self, best):
        n, d = self.n, self.defect
        self.sweeps += 1                                           # :161, :181
        if best == NOKEY:                                          # :159
            return False
        is_, js = self.unpack(best)                                # :166
        if d == "i":
            is_ &= 0x7FFF
        if d == "j":
            js &= 0x7FFF
        lo, hi = is_ + 1, js                                       # :167
        if not (lo <= hi and hi <= n - 2):
            raise WildMove((is_, js))
        self.P[lo:hi + 1] = self.P[lo:hi + 1][::-1].copy()         # :170-177   swap_2opt(path, i+1, j) on P and perm
        self.perm[lo:hi + 1] = self.perm[lo:hi + 1][::-1].copy()
        t0, t1 = (lo - 1) >> 6, hi >> 6                            # :179   t = ((lo-1) >> 6) + wave; t <= (hi >> 6); t += 16
        if d == "k":
            t0 = lo >> 6
        ts = np.arange(t0, t1 + (0 if d == "l" else 1))
        if d == "m":
            ts = ts[:16]
        self.build_tile_meta(ts)
        self.moves += 1                                            # :182
        self.reversed += js - is_                                  # :183
        self.mv, self.is_, self.js = 1, is_, js                    # :184-186
        self.move_list.append((is_, js))
        return True


def model_best_sweep(xy, tour, defect=None, max_sweeps=None):
    """The kernel's scheme.  Returns the same dict as ref_best_sweep (without ties) plus record: per sweep, for every row, the branch
    it took (BR_*), the first and last tile group its scan visited (g0, g1; -1: no scan) and, where a partial rescan won, its column.
    A run that a defect drives off the candidate set, or past max_sweeps, ends with wild / capped set: it differs from the oracle."""
    m = _Model(xy, tour, defect)
    wild = capped = False
    try:
        while m.apply(m.scan()):
            if max_sweeps is not None and m.sweeps >= max_sweeps:
                capped = True
                break
    except WildMove:
        wild = True
    return {"tour": m.perm, "cost_bits": cost_bits(m.xy, m.perm), "sweeps": m.sweeps, "moves": m.moves, "reversed": m.reversed,
            "move_list": m.move_list, "record": m.record, "wild": wild, "capped": capped}


def oracle_best_sweep(xy, tour):
    rc, route, cost, st = O.two_opt(xy, None, len(tour), init=np.asarray(tour, dtype=np.uint32), best=True)
    assert rc == 0
    return {"tour": route, "cost_bits": int(np.float32(cost).view(np.uint32)), "sweeps": st["sweeps"], "moves": st["moves"],
            "reversed": st["reversed"], "candidates": st["candidates"]}


def same_result(x, y):
    return (not x.get("wild") and not x.get("capped") and not y.get("wild") and not y.get("capped")
            and np.array_equal(x["tour"], y["tour"]) and all(x[k] == y[k] for k in ("cost_bits", "sweeps", "moves", "reversed")))
