"""Planted winners for the 3-opt and Or-opt scans.  TEST INFRASTRUCTURE ONLY (no tests here).

A plant is an explicit packed matrix that is one constant (10) everywhere except a handful of entries, chosen so that the
move at chosen coordinates is the best one: 3-opt (i, j, k, case), Or-opt (seg_len, i, j, reversed).  All values but one
(the case-1, case-7 and last-row plants, see edits3_case1, edits3_case7, edits3_last_row) are small integers, so every f32 sum is exact and the comparison with the oracle is bit
for bit.  THE ORACLE DECIDES what the expected move is; the plant only aims.  seams3() / seams_or() restate the kernels'
work division and say on which seams of it a move lies; hit_table() runs the oracle over the tables and lists, per seam,
the plants whose ORACLE WINNER lies on it (for the seams whose point is that nothing may be reported — a skipped triple,
a wrapping row, an excluded j — the plants that aim there and whose oracle winner lies elsewhere)."""
import functools

import numpy as np

import _oracle as O

CONST = 10.0

# ------------------------------------------------------------------------------------------------
# the work division, restated
# ------------------------------------------------------------------------------------------------
K_T3 = 256          # three_opt.hip:30   kT3, threads per scan workgroup (a lane strides k by it, :109)
PICK = 1024         # three_opt.hip:195, or_opt.hip:197   the pick kernels stride the partials by 1024
K_OR_WAVES = 4      # or_opt.hip:22
K_OR_IR = 8         # or_opt.hip:23
K_OR_TARGET = 4096  # or_opt.hip:24


def jc(n):
    return 4 if n <= 256 else 16  # tl_api_scans.hip:90   const uint32_t jc = n <= 256 ? 4u : 16u;


def three_opt_prefix(n):
    pre, acc = [], 0
    for i in range(n - 2):                      # tl_api_scans.hip:93   for (i = 0; i + 2 < n; ++i)
        pre.append(acc)                         # tl_api_scans.hip:94   prefix[i] = acc;
        acc += (n - 2 - i + jc(n) - 1) // jc(n)  # tl_api_scans.hip:95   acc += ((n - 2u - i) + jc - 1u) / jc;
    return pre, acc                             # tl_api_scans.hip:98   *nblocks = acc;


def three_opt_blocks(n):
    return three_opt_prefix(n)[1]


def three_opt_where(n, i, j, k):
    """Where the scan meets the triple: block, jlo / jhi of its chunk, and the lane and trip of column k."""
    J = jc(n)
    c = (j - (i + 1)) // J
    jlo = i + 1 + c * J            # three_opt.hip:98    jlo = i + 1 + (blockIdx.x - chunk_prefix[i]) * jc
    jhi = min(jlo + J, n - 1)      # three_opt.hip:99-100
    off = k - (jlo + 1)            # three_opt.hip:109   for (k = jlo + 1 + tid; k < n; k += kT3)
    return {"block": three_opt_prefix(n)[0][i] + c, "jlo": jlo, "jhi": jhi, "off": off, "tid": off % K_T3, "trip": off // K_T3,
            "chunks_in_row": (n - 2 - i + J - 1) // J, "chunk": c}


def or_opt_grid_x(n):
    return ((n + K_OR_IR - 1) // K_OR_IR + K_OR_WAVES - 1) // K_OR_WAVES  # or_opt.hip:41


def or_opt_chunks(n):
    total, groups = (n + 62) // 63, (n + K_OR_IR - 1) // K_OR_IR  # or_opt.hip:44
    slabs = (K_OR_TARGET + groups - 1) // groups                  # or_opt.hip:45
    slabs = min(slabs, total)                                     # or_opt.hip:46
    slabs = max(slabs, 1)                                         # or_opt.hip:47
    return (total + slabs - 1) // slabs                           # or_opt.hip:48


def or_opt_grid_y(n):
    return ((n + 62) // 63 + or_opt_chunks(n) - 1) // or_opt_chunks(n)  # or_opt.hip:50


def or_opt_where(n, i, j):
    slab = or_opt_chunks(n) * 63                # or_opt.hip:82    jlo = blockIdx.y * (chunks * 63u)
    by, bx = j // slab, i // (K_OR_IR * K_OR_WAVES)  # or_opt.hip:81    i0 = (blockIdx.x * kOrWaves + wave) * kOrIR
    return {"bx": bx, "by": by, "wave": (i // K_OR_IR) % K_OR_WAVES, "r": i % K_OR_IR, "chunk": (j % slab) // 63, "lane": j % 63,
            "partial": by * or_opt_grid_x(n) + bx}  # or_opt.hip:168   partials + 2 * (blockIdx.y * gridDim.x + blockIdx.x)


# what the issue states about the sizes, checked instead of trusted
assert jc(256) == 4 and jc(257) == 16
assert three_opt_blocks(300) > 2048 and three_opt_blocks(256) > 2048 and three_opt_blocks(257) > 2048
assert or_opt_chunks(2040) == 2 and or_opt_grid_x(2040) == 64 and or_opt_grid_y(2040) == 17
# (n = 2040 has a second chunk per wave AND more than 1024 partials; the first such size is 2017, where ceil(n/63) reaches 33)
assert min(m for m in range(4, 2041) if or_opt_chunks(m) >= 2 and or_opt_grid_x(m) * or_opt_grid_y(m) > PICK) == 2017


# ------------------------------------------------------------------------------------------------
# matrices
# ------------------------------------------------------------------------------------------------
def tri(p, q):
    hi, lo = max(p, q), min(p, q)
    return hi * (hi - 1) // 2 + lo  # distance_matrix.rs:177-191 (oracle/tl_oracle.c tlo_dm_lookup)


def constant_matrix(n):
    return np.full(n * (n - 1) // 2, CONST, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def tour(n, kind):
    """'id': the identity; 'perm': a seeded shuffle, so that a position is not a city."""
    p = np.arange(n, dtype=np.uint32) if kind == "id" else O.restart_perm(n, 20 + n, 0)
    p.setflags(write=False)
    return p


class Plant:
    """scan: '3' or 'or'; aims: the planted moves (more than one: a tie), each with the edits only it needs; neg: the name of
    the must-not-be-reported seam the (single) aim sits on, or None."""

    def __init__(self, scan, n, kind, label, aims, edits, neg=None):
        self.scan, self.n, self.kind, self.label, self.aims, self.edits, self.neg = scan, n, kind, label, aims, edits, neg
        self.id = f"{scan}-n{n}-{kind}-{label}"

    def path(self):
        return tour(self.n, self.kind)

    def matrix(self, drop=()):
        """The packed matrix; drop: indices of aims whose edits are left out (their entries stay as the other aims set them)."""
        m = constant_matrix(self.n)
        for a, ed in enumerate(self.edits):
            if a not in drop:
                for p, q, v in ed:
                    m[tri(p, q)] = v
        return m


def _new_edges3(case):
    # three_opt.rs:170-180 (oracle/tl_oracle.c tlo_reconnection_costs): the three edges of each reconnection
    return {1: ("ac", "bd", "ef"), 2: ("ab", "ce", "df"), 3: ("ac", "be", "df"), 4: ("ad", "be", "cf"), 5: ("ad", "ce", "bf"),
            6: ("ae", "bd", "cf"), 7: ("ae", "cd", "bf")}[case]


def edits3(n, path, i, j, k, case, value=1.0):
    """Lower the edges that reconnection `case` of (i, j, k) adds to `value`.  Pairs that are one city twice (j = i+1 makes
    b == c) or one of the three tour edges are left alone.  k <= j is allowed: the ghost plants aim at what a lane computes
    where it is masked."""
    v = {"a": int(path[i]), "b": int(path[i + 1]), "c": int(path[j]), "d": int(path[j + 1]), "e": int(path[k]), "f": int(path[(k + 1) % n])}
    old = {frozenset((v["a"], v["b"])), frozenset((v["c"], v["d"])), frozenset((v["e"], v["f"]))}
    out = []
    for e in _new_edges3(case):
        p, q = v[e[0]], v[e[1]]
        if p != q and frozenset((p, q)) not in old:
            out.append((p, q, value))
    return out


def edits3_case7(n, path, i, j, k):
    """Case 7 (ae + cd + bf) is the 2-opt move on (i, k) whatever j is, so with exact sums (i, i+1, k) ties with it, comes
    first, and reads as case 6 there (b == c).  It can only win by rounding: with cd = 10 + 2^-19 and ef = 12 + 2^-19,
    orig = (10 + cd) + ef = 32 + 2^-18 is exact at (i, j, k), while at every other j' it is 32 + 2^-19, a tie that rounds to
    even, 32.  Savings 20 + 2^-19 here, 20 there.  This is the one plant whose sums are not all exact: it also pins the
    association (x + y) + z."""
    a, b, c, d, e, f = (int(path[t]) for t in (i, i + 1, j, j + 1, k, (k + 1) % n))
    t = float(np.float32(2.0 ** -19))
    return [(a, e, 1.0), (b, f, 1.0), (c, d, CONST + t), (e, f, 12.0 + t)]


def edits_or(n, path, seg_len, i, j, rev, value=1.0):
    """Lower d(x, first), d(last, y) (swapped when reversed) and d(prev, after) to `value`, leaving alone pairs that are one
    city twice or a tour edge next to the segment or (x, y)."""
    prev, after = int(path[(i - 1) % n]), int(path[(i + seg_len) % n])
    first, last = int(path[i % n]), int(path[(i + seg_len - 1) % n])
    x, y = int(path[j]), int(path[(j + 1) % n])
    old = {frozenset((prev, first)), frozenset((last, after)), frozenset((x, y))}
    pairs = [(x, last), (first, y)] if rev else [(x, first), (last, y)]
    out = []
    for p, q in pairs + [(prev, after)]:
        if p != q and frozenset((p, q)) not in old:
            out.append((p, q, value))
    return out


def edits3_case1(n, path, i, j, k):
    """Case 1 (ac + bd + ef) is the 2-opt move on (i, j) whatever k is; (i, i+1, j) makes the same move as case 6, ties with
    exact sums and comes first.  The rounding plant: cd = 10 + 3 * 2^-20 makes ab + cd = 20 + 1.5 * 2^-19 a tie that rounds up to
    20 + 2^-18, and with ef = 12 + 2^-19 the next sum, 32 + 1.5 * 2^-18, is a tie that rounds up again: savings
    18 + 3 * 2^-19 here, 18 + 2 * 2^-19 at every equivalent, whose sums meet cd last or ef not at all."""
    a, b, c, d, e, f = (int(path[t]) for t in (i, i + 1, j, j + 1, k, (k + 1) % n))
    return [(a, c, 1.0), (b, d, 1.0), (c, d, CONST + 3 * 2.0 ** -20), (e, f, 12.0 + 2.0 ** -19)]


def edits3_last_row(n, path):
    """i = n-3 leaves one triple, (n-3, n-2, n-1), and its only move swaps b and d: cases 4-7 alike, and the same tour as
    case 2 of (i', n-3, n-1) for every i' >= 1, which comes first.  So this row, too, wins by rounding only, with the
    construction of edits3_case1 on the edges bd and df: savings 22 + 2 * 2^-19 here, 22 at the equivalents.  ab is raised to
    12 because (n-4, n-2, n-1) moves d in front of a with both cheap edges and the same rounding, for 20 + 4 * 2^-19."""
    a, b, d, f = (int(path[t]) for t in (n - 3, n - 2, n - 1, 0))
    return [(a, d, 1.0), (b, f, 1.0), (a, b, 12.0), (b, d, CONST + 3 * 2.0 ** -20), (d, f, 12.0 + 2.0 ** -19)]


def plant3(n, kind, label, i, j, k, case, neg=None, raised=(), exact=False):
    """raised: tour positions t whose removed edge (path[t], path[t+1]) goes up to 12, where lowering alone leaves a tie;
    exact: cases 1 and 7 with integer entries only (the oracle's earlier equivalent wins)."""
    p = tour(n, kind)
    if i == n - 3 and not exact:
        ed = edits3_last_row(n, p)
    elif case in (1, 7) and not exact and not neg:
        ed = (edits3_case1 if case == 1 else edits3_case7)(n, p, i, j, k)
    else:
        ed = edits3(n, p, i, j, k, case)
    ed = ed + [(int(p[t]), int(p[(t + 1) % n]), 12.0) for t in raised]
    return Plant("3", n, kind, label, [(i, j, k, case)], [ed], neg)


def tie3(n, kind, label, aims):
    p = tour(n, kind)
    return Plant("3", n, kind, label, list(aims), [edits3(n, p, *a) for a in aims])


def plant_or(n, kind, label, seg_len, i, j, rev, neg=None, raised=()):
    """raised: tour positions t whose removed edge (path[t], path[t+1]) goes up to 12, where lowering alone leaves a tie."""
    p = tour(n, kind)
    ed = edits_or(n, p, seg_len, i, j, rev) + [(int(p[t]), int(p[(t + 1) % n]), 12.0) for t in raised]
    return Plant("or", n, kind, label, [(seg_len, i, j, bool(rev))], [ed], neg)


def tie_or(n, kind, label, aims):
    p = tour(n, kind)
    aims = [(a[0], a[1], a[2], bool(a[3])) for a in aims]
    return Plant("or", n, kind, label, aims, [edits_or(n, p, *a) for a in aims])


# ------------------------------------------------------------------------------------------------
# seams
# ------------------------------------------------------------------------------------------------
def seams3(n, i, j, k, case):
    """The seams of the 3-opt work division on which the move (i, j, k, case) lies; each name carries the jc of its size."""
    w = three_opt_where(n, i, j, k)
    J, s = jc(n), set()
    if j == w["jlo"]:
        s.add("j_first_in_chunk")
    if j == w["jhi"] - 1 and w["jhi"] - w["jlo"] > 1:
        s.add("j_last_in_chunk")             # three_opt.hip:121 reloads the same row
    if w["chunk"] == w["chunks_in_row"] - 1 and w["jhi"] - w["jlo"] < J:
        s.add("j_in_short_last_chunk")
    if j == n - 2:
        s.add("j_eq_n-2")
    if k == j + 1:
        s.add("k_eq_j+1")
    if w["jlo"] + 1 <= k <= w["jhi"] - 1:
        s.add("k_in_own_chunk_j_range")      # this lane is masked (j < k, three_opt.hip:143) for the chunk's later j
    if w["jhi"] + 1 <= k <= min(w["jhi"] + J, n - 1) - 1 and w["chunk"] + 1 < w["chunks_in_row"]:
        s.add("k_in_next_chunk_j_range")     # the next chunk's lane of this column is masked there
    if w["trip"] == 0 and w["tid"] in (63, 64):
        s.add(f"k_lane_{w['tid']}")
    if w["off"] in (255, 256):
        s.add(f"k_off_{w['off']}")           # the last column of a lane's first trip, the first of its second
    if k == n - 1 and i > 0:
        s.add("k_wrap_column")
    if i == 0:
        s.add("i_eq_0")
    if i == n - 3:
        s.add("i_eq_n-3")
    if w["block"] == 0:
        s.add("first_block")
    if w["block"] == three_opt_blocks(n) - 1:
        s.add("last_block")
    if w["block"] >= PICK:
        s.add("block_ge_1024")
    if w["block"] >= 2 * PICK:
        s.add("block_ge_2048")
    s.add(f"case_{case}")
    return {f"{x}@jc{J}" for x in s}


# must-not-be-reported seams (hit by a plant that aims there and whose oracle winner lies elsewhere)
NEG3 = ("skip_i0_k_n-1", "ghost_k_le_j")
# k_off_255 / k_off_256 need n >= 259, which is jc = 16 only; blocks >= 1024 need n >= 256
SEAMS3 = sorted({f"{s}@jc{J}" for J in (4, 16) for s in
                 ("j_first_in_chunk", "j_last_in_chunk", "j_in_short_last_chunk", "j_eq_n-2", "k_eq_j+1", "k_in_own_chunk_j_range",
                  "k_in_next_chunk_j_range", "k_lane_63", "k_lane_64", "k_wrap_column", "i_eq_0", "i_eq_n-3", "first_block",
                  "last_block", "block_ge_1024", "block_ge_2048") + NEG3 + tuple(f"case_{c}" for c in range(1, 8))}
                | {"k_off_255@jc16", "k_off_256@jc16"})
TIES3 = ("tie_two_lanes_one_wave", "tie_two_waves_one_block", "tie_two_blocks", "tie_two_pick_trips", "tie_k_and_k+256_one_lane")


def tie_class3(n, a, b):
    wa, wb = three_opt_where(n, *a[:3]), three_opt_where(n, *b[:3])
    if wa["block"] != wb["block"]:
        return "tie_two_pick_trips" if wa["block"] // PICK != wb["block"] // PICK else "tie_two_blocks"
    if wa["tid"] == wb["tid"]:
        return "tie_k_and_k+256_one_lane" if abs(wa["trip"] - wb["trip"]) == 1 else None
    return "tie_two_lanes_one_wave" if wa["tid"] // 64 == wb["tid"] // 64 else "tie_two_waves_one_block"


def seams_or(n, seg_len, i, j, rev):
    w = or_opt_where(n, i, j)
    s = set()
    if w["r"] in (0, 7):
        s.add(f"r_eq_{w['r']}")
    if i in (31, 32):
        s.add(f"i_eq_{i}")
    if n % 8 and i // K_OR_IR == (n - 1) // K_OR_IR and n in (63, 65, 127):
        s.add(f"last_group_n{n}")            # or_opt.hip:110 pm clamps at n-1
    if i + seg_len == n:
        s.add(f"i+len_eq_n_len{seg_len}")
    if w["lane"] == 0 and j == 0:
        s.add("j_lane_0")
    if w["lane"] == 62:
        s.add("j_lane_62")                   # y comes from helper lane 63 (or_opt.hip:113)
    if w["lane"] == 0 and j >= 63:
        s.add("j_first_lane_of_next_chunk")
    if j == n - 1:
        s.add("j_eq_n-1")                    # y is the wrap, P[0] (or_opt.hip:105)
    if (j + 2) % n == i:
        s.add("j_eq_i-2")                    # y is prev, next to the excluded j == prev
    if j == i + seg_len:
        s.add("j_eq_i+len")
    slab = or_opt_chunks(n) * 63
    if or_opt_grid_y(n) > 1 and (j + 1) % slab == 0 and j + 1 < n:
        s.add("j_last_of_slab")
    if j and j % slab == 0:
        s.add("j_first_of_slab")
    if n == 2040 and w["chunk"] == 1:
        s.add("second_chunk_n2040")
    if w["partial"] >= PICK:
        s.add("partial_ge_1024")
    s.add(f"kind_len{seg_len}_{'rev' if rev else 'fwd'}")
    return s


NEG_OR = ("wrapping_row", "j_eq_prev", "j_inside_segment")
SEAMS_OR = sorted(("r_eq_0", "r_eq_7", "i_eq_31", "i_eq_32", "last_group_n63", "last_group_n65", "last_group_n127", "i+len_eq_n_len1",
                   "i+len_eq_n_len2", "i+len_eq_n_len3", "j_lane_0", "j_lane_62", "j_first_lane_of_next_chunk", "j_eq_n-1", "j_eq_i-2",
                   "j_eq_i+len", "j_last_of_slab", "j_first_of_slab", "second_chunk_n2040", "partial_ge_1024", "kind_len1_fwd",
                   "kind_len2_fwd", "kind_len2_rev", "kind_len3_fwd", "kind_len3_rev") + NEG_OR)
TIES_OR = ("tie_two_lanes_one_wave", "tie_two_waves_one_block", "tie_two_blocks", "tie_two_pick_trips", "tie_fwd_and_rev")


def tie_class_or(n, a, b):
    wa, wb = or_opt_where(n, a[1], a[2]), or_opt_where(n, b[1], b[2])
    if a[:3] == b[:3] and a[3] != b[3]:
        return "tie_fwd_and_rev"
    if wa["partial"] != wb["partial"]:
        return "tie_two_pick_trips" if wa["partial"] // PICK != wb["partial"] // PICK else "tie_two_blocks"
    if wa["wave"] != wb["wave"]:
        return "tie_two_waves_one_block"
    return "tie_two_lanes_one_wave" if (wa["chunk"], wa["lane"]) != (wb["chunk"], wb["lane"]) else None


# ------------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------------
SIZES3 = (7, 64, 256, 257, 300)
SIZES_OR = (5, 9, 63, 64, 65, 127, 256, 257, 300, 2040)
KINDS = ("id", "perm")


def _first_row_with_prefix(n, at_least):
    pre = three_opt_prefix(n)[0]
    return next(i for i in range(n - 2) if pre[i] >= at_least)


@functools.lru_cache(maxsize=None)
def table3(n, kind):
    """The 3-opt plants of one size and tour; three-edge cases 3-6 take turns where the seam does not ask for a case."""
    J, T = jc(n), []
    turn = [0]

    def add(label, i, j, k, case=None, neg=None, **kw):
        if case is None:
            case = 3 + turn[0] % 4
            turn[0] += 1
        assert 0 <= i and i + 2 < n and (neg == "ghost_k_le_j" or i < j < k < n) and j + 1 < n, (label, n, i, j, k)
        T.append(plant3(n, kind, label, i, j, k, case, neg, **kw))

    if n == 7:
        add("first_block", 0, 2, 4)
        add("i0_k_eq_j+1", 0, 1, 2, 4)
        add("short_chunk", 0, 5, 6, 3, neg="skip_i0_k_n-1")
        add("row1_short_chunk", 1, 3, 5)
        add("row1_wrap", 1, 3, 6)
        add("row2_last_j", 2, 5, 6, 4)
        add("last_block", 4, 5, 6, 4)
        add("case1", 0, 3, 5, 1)
        add("case2", 0, 2, 5, 2)
        add("case7", 1, 3, 5, 7)
        return tuple(T)
    i0 = 5
    jl = [i0 + 1 + c * J for c in range(4)]  # jlo of row i0's chunks 0..3
    if n == 300:
        # an oracle scan takes 0.2 s here: n = 257 carries the jc = 16 seams, this size what needs a second trip along k
        add("k_off255", i0, jl[1] + 1, jl[1] + 1 + 255)
        add("k_off256", i0, jl[1] + 2, jl[1] + 1 + 256)
        add("k_off256_last_j", i0, jl[1] + J - 1, jl[1] + 1 + 256)
        add("k_off256_first_block", 0, 2, 2 + 256)
        add("wrap_column_second_trip", 3, 6, n - 1)
        add("skip", 0, 3, n - 1, 3, neg="skip_i0_k_n-1")
        add("last_block", n - 3, n - 2, n - 1, 4)
        add("block_ge_2048", _first_row_with_prefix(n, 2 * PICK), n - 9, n - 4)
        add("case1", 4, n // 2, n - 7, 1)
        add("case7", i0 + 2, n // 3, n - 6, 7)
        add("case1_exact", 7, n // 2, n - 3, 1, exact=True)
        add("case7_exact", 8, n // 2, n - 3, 7, exact=True)
        T.append(tie3(n, kind, "tie_k_k+256", [(3, 9, 20, 3), (3, 9, 276, 3)]))
        T.append(tie3(n, kind, "tie_k_k+256_waves", [(3, 9, 30, 5), (3, 9, 30 + 256, 5), (3, 9, 100, 5)]))
        T.append(tie3(n, kind, "tie_blocks_i", [(2, 20, 30, 5), (40, 50, 60, 5)]))
        return tuple(T)
    add("first_block_i0", 0, 2, 4)
    add("j_first", i0, jl[2], jl[2] + 10)
    add("j_last", i0, jl[2] + J - 1, jl[2] + J + 9)
    r = next(i for i in range(6, 40) if (n - 2 - i) % J == 2)  # a row whose last chunk holds two j
    add("short_chunk_first_j", r, n - 3, n - 1)
    add("short_chunk_last_j", r + 1 if (n - 3 - r) % J == 1 else r, n - 2, n - 1, 4)
    add("k_eq_j+1", i0, jl[1] + 1, jl[1] + 2)
    add("k_own_chunk", i0, jl[1], jl[1] + 2)
    add("k_next_chunk", i0, jl[1] + J - 2, jl[1] + J + 2)
    add("ghost", i0, jl[1] + 3, jl[1] + 1, 6, neg="ghost_k_le_j")
    add("ghost_next_chunk", i0, jl[2] + 2, jl[2] + 1, 4, neg="ghost_k_le_j")
    if n >= 256:
        add("k_lane63", i0, jl[1] + 1, jl[1] + 1 + 63)
        add("k_lane64", i0, jl[1] + 2, jl[1] + 1 + 64)
        for b in (PICK, 2 * PICK):
            i = _first_row_with_prefix(n, b)
            add(f"block_ge_{b}", i, i + 2, i + 4)
        add("block_1024_far_k", _first_row_with_prefix(n, PICK) + 1, n - 5, n - 2)
    add("wrap_column", i0, jl[3] + 1, n - 1)
    add("wrap_column_row1", 1, n // 2, n - 1)
    add("skip", 0, 3, n - 1, 3, neg="skip_i0_k_n-1")
    add("skip_long", 0, n // 2, n - 1, 5, neg="skip_i0_k_n-1")
    add("i0_mid", 0, n // 3, n // 2)
    add("last_block", n - 3, n - 2, n - 1, 4)
    add("row_n-4", n - 4, n - 3, n - 1, 4)
    add("case1", 4, n // 2, n - 7, 1)
    add("case1_k_eq_j+1", 0, n // 2, n // 2 + 1, 1)
    add("case1_exact", 7, n // 2, n - 3, 1, exact=True)     # the oracle's earlier equivalent wins: a tie in loop order
    add("case7_exact", 8, n // 2, n - 3, 7, exact=True)
    add("case2", 0, n // 3, n - 4, 2)
    add("case2_aimed_late", 9, n // 3, n - 4, 2)
    add("case7", i0 + 2, n // 3, n - 6, 7)
    add("case7_far", 20, 30, 40, 7)
    for c in (3, 4, 5, 6):
        add(f"case{c}", 11, 11 + n // 4, 11 + n // 2, c)
    # ties: equal winners, the oracle keeps the first in loop order
    a, b, c = jl[1] + 1, jl[1] + 9, 3
    T.append(tie3(n, kind, "tie_lanes", [(i0 + 1, a, b, c), (i0 + 1, a, b + 3, c)]))
    if n >= 256:
        T.append(tie3(n, kind, "tie_waves", [(i0 + 1, a, b, c), (i0 + 1, a, b + 100, c), (i0 + 1, a, b + 200, c)]))
    T.append(tie3(n, kind, "tie_blocks_j", [(i0 + 1, a, n - 9, 4), (i0 + 1, a + J, n - 9, 4)]))
    T.append(tie3(n, kind, "tie_blocks_i", [(2, 20, 30, 5), (40, 50, 60, 5), (41, 45, 49, 5)]))
    if n >= 256:
        i = _first_row_with_prefix(n, PICK + 7)
        blk = three_opt_prefix(n)[0][i] - PICK        # the block the same pick thread reads one trip earlier
        pre = three_opt_prefix(n)[0]
        ie = max(t for t in range(n - 2) if pre[t] <= blk)
        je = ie + 1 + (blk - pre[ie]) * J
        T.append(tie3(n, kind, "tie_pick_trips", [(ie, je + 1, je + 5, 6), (i, i + 2, i + 5, 6)]))
    return tuple(T)


@functools.lru_cache(maxsize=None)
def table_or(n, kind):
    T = []
    turn = [0]
    kinds = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)]

    def add(label, i, j, seg_len=None, rev=None, neg=None, raised=()):
        if seg_len is None:
            seg_len, rev = kinds[turn[0] % 5]
            turn[0] += 1
        assert 0 <= i < n and 0 <= j < n, (label, n, i, j)
        T.append(plant_or(n, kind, label, seg_len, i, j, rev, neg, raised))

    if n == 5:
        add("len1_end", 4, 1, 1, 0)
        add("len2_end", 3, 0, 2, 1)
        add("len3", 1, 4, 3, 0)
        add("len1_j_n-1", 1, 4, 1, 0)
        add("wrap_row", 4, 1, 2, 0, neg="wrapping_row")
        return tuple(T)
    if n == 9:
        add("r0", 0, 4)
        add("r7", 7, 3)
        add("group2", 8, 4, 1, 0)
        add("len2_end", 7, 2, 2, 1)
        add("len3_end", 6, 2, 3, 1)
        add("j_n-1", 3, 8, 2, 0)
        add("j_i-2", 5, 3, 3, 0)
        add("j_i+len", 2, 4, 2, 1)
        add("wrap_row", 7, 3, 3, 0, neg="wrapping_row")
        add("j_prev", 4, 3, 2, 1, neg="j_eq_prev")
        add("j_inside", 4, 5, 3, 0, neg="j_inside_segment")
        return tuple(T)
    slab = or_opt_chunks(n) * 63
    if n == 2040:
        # an oracle scan takes half a second here: only what needs this size (a second chunk per wave, partials beyond 1024)
        add("chunk2_first_lane", 100, 63)
        add("chunk2_lane62", 102, 125, 3, 1)
        add("chunk2_far_slab", 1000, 7 * slab + 70)
        add("partial_1024", 10, 2020)
        add("partial_1087_j_n-1", 2037, n - 1, 2, 1)
        T.append(tie_or(n, kind, "tie_pick_trips", [(2, 70, 5, 0), (2, 70, 2020, 0)]))
        return tuple(T)
    add("r0", 8, 20)
    add("r7", 15, 30)
    add("i31", 31, 50)
    add("i32", 32, 10)
    add("i31_len3", 31, 12, 3, 1)          # a segment that straddles the block boundary
    g = (n - 1) // 8 * 8                   # the last group's first start
    add("last_group_first", g, 5, 1, 0)
    add("last_group_len2", n - 2, 7, 2, 1)
    add("end_len1", n - 1, 3, 1, 0)
    add("end_len2", n - 2, 9, 2, 0)
    add("end_len3", n - 3, 11, 3, 1)
    add("end_len3_fwd", n - 3, 21, 3, 0)
    add("wrap_row_len2", n - 1, 6, 2, 0, neg="wrapping_row")
    add("wrap_row_len3", n - 2, 6, 3, 1, neg="wrapping_row")
    add("j_lane0", 20, 0)
    add("j_lane0_len1", 21, 0, 1, 0)
    add("j_lane62", 20, 62)
    add("j_lane62_rev", 17, 62, 3, 1)
    if n > 64:
        add("j_63", 20, 63)
        add("j_63_len3", 9, 63, 3, 0)
    if n == 64:
        add("j_63", 20, 63, 2, 0)
    add("j_n-1", 25, n - 1)
    add("j_n-1_len1", 26, n - 1, 1, 0)
    add("j_n-1_rev", 27, n - 1, 2, 1)
    add("j_i-2", 40, 38)                   # (1, i-1, i+len-1) is the same tour and comes first: a tie the oracle resolves
    # only across the wrap is j = i-2 the first of its equivalents; j = n-3 shares the cheap edge, so (x, y) is raised too
    add("j_i-2_wrap_len1", 0, n - 2, 1, 0, raised=(n - 2,))
    add("j_i-2_wrap_len2", 0, n - 2, 2, 1, raised=(n - 2,))
    add("j_i-2_len1", 41, 39, 1, 0)
    add("j_i+len", 44, 46, 2, 1)
    add("j_i+len_len1", 45, 46, 1, 0)
    add("j_i+len_len3", 33, 36, 3, 0)
    add("j_prev", 30, 29, 2, 1, neg="j_eq_prev")
    add("j_prev_len3", 30, 29, 3, 0, neg="j_eq_prev")
    add("j_inside", 30, 31, 3, 1, neg="j_inside_segment")
    add("j_inside_last", 30, 32, 3, 0, neg="j_inside_segment")
    for s, r in kinds:
        add(f"kind_{s}_{r}", 50, 12 + s, s, r)
    if or_opt_grid_y(n) > 1:
        add("slab_last", 12, slab - 1)
        add("slab_first", 13, slab)
        add("slab_last_len1", 14, slab - 1, 1, 0)
        add("slab_first_rev", 15, slab, 2, 1)
    # ties
    T.append(tie_or(n, kind, "tie_lanes", [(2, 16, 30, 0), (2, 16, 40, 0)]))
    T.append(tie_or(n, kind, "tie_lanes_rows", [(3, 17, 33, 1), (3, 21, 43, 1)]))
    T.append(tie_or(n, kind, "tie_waves", [(1, 35, 10, 0), (1, 43, 20, 0), (1, 59, 25, 0)]))
    if n >= 127:
        T.append(tie_or(n, kind, "tie_blocks_x", [(2, 36, 50, 1), (2, 100, 50 + 3, 1)]))
    if or_opt_grid_y(n) > 1 and n >= 127:
        T.append(tie_or(n, kind, "tie_blocks_y", [(3, 37, 2, 0), (3, 37, slab + 10, 0)]))
    T.append(tie_or(n, kind, "tie_fwd_rev_len2", [(2, 52, 20, 0), (2, 52, 20, 1)]))
    T.append(tie_or(n, kind, "tie_fwd_rev_len3", [(3, 24, 48, 0), (3, 24, 48, 1)]))
    return tuple(T)


def threshold_plants(n, kind):
    """or_opt.rs:86 best_delta = -1e-3: one edge d(x, first) at 10 - 2^-9 gives delta -0.001953125 (taken), at 10 - 2^-10 it
    gives -0.0009765625 (not taken).  (-10 + v) + 10 - 10 is exact in f32 for both."""
    p, out = tour(n, kind), []
    spots = [(1, 2, 5), (2, 1, 6), (3, 0, 4)] if n < 64 else [(1, 8, 20), (2, 31, 62), (3, 32, n - 1), (1, n - 1, 3), (2, 40, 0)]
    for t, (seg_len, i, j) in enumerate(spots):
        for name, v in (("take", CONST - 2.0 ** -9), ("leave", CONST - 2.0 ** -10)):
            out.append(Plant("or", n, kind, f"threshold_{name}_{t}", [(seg_len, i, j, False)],
                             [[(int(p[j]), int(p[i]), float(np.float32(v)))]]))
    return out


THRESHOLD_SIZES = (9, 64, 300)
THRESHOLD_TAKEN_BITS = int(np.float32(-0.001953125).view(np.uint32))


# the apply tables: log[0] of a traced descent must be the plant itself, so case 2 sits at i = 0, where it is the first of its
# equivalents in loop order, and cases 1 and 7 are the rounding plants
def apply_table3(n, kind):
    """Cases 1-7; at n >= 1100 the moved span l1 + l2 exceeds 1024: long l1 with short l2, the reverse, and both long."""
    T = []
    if n >= 1100:
        spans = {"long_l1": (1030, 5), "long_l2": (5, 1030), "both": (600, 450)}
    else:
        spans = {"long_l1": (n - 40, 5), "long_l2": (5, n - 40), "both": (n // 2, n // 3)}
    for name, (l1, l2) in spans.items():
        for case in range(1, 8):
            i = 0 if case == 2 else 3
            j = i + l1
            k = j + l2
            T.append(plant3(n, kind, f"apply_{name}_case{case}", i, j, k, case))
    return T


def apply_table_or(n, kind):
    T = []
    for seg_len, rev in [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1)]:
        T.append(plant_or(n, kind, f"apply_len{seg_len}_{rev}_j_lt_i", seg_len, n - 20 - seg_len, 7 + seg_len, rev))
        T.append(plant_or(n, kind, f"apply_len{seg_len}_{rev}_j_ge_i", seg_len, 11 + seg_len, n - 9 - seg_len, rev))
    return T


APPLY_SIZES = (256, 257, 1100)
# moves after which every planted descent has ended.  The oracle gives 1 for the exact plants and at most 2 for the case-7
# rounding plant at n = 300 (tests/test_scan_plants_oracle.py asserts it there); the GPU test holds n = 1100 to the same count.
APPLY_MAX_MOVES = 2


# ------------------------------------------------------------------------------------------------
# the oracle's answers (computed once per process, shared by the CPU and the GPU tests)
# ------------------------------------------------------------------------------------------------
_cache = {}


def oracle_move(plant, drop=()):
    """3-opt: (i, j, k, case, savings) or None; Or-opt: (delta, i, j, seg_len, reversed) or None."""
    key = (plant.id, tuple(drop))
    if key not in _cache:
        fn = O.three_opt_find_best_move if plant.scan == "3" else O.or_opt_find_best_move
        _cache[key] = fn(None, plant.matrix(drop), plant.path())
    return _cache[key]


def coords(plant, mv):
    """The move as the plant's aim tuple: (i, j, k, case) or (seg_len, i, j, reversed)."""
    if mv is None:
        return None
    return tuple(mv[:4]) if plant.scan == "3" else (mv[3], mv[1], mv[2], bool(mv[4]))


def value_bits(plant, mv):
    return int(np.float32(mv[4] if plant.scan == "3" else mv[0]).view(np.uint32))


def _loop_key(plant, aim):
    return aim[:3] if plant.scan == "3" else aim  # 3-opt: (i, j, k); Or-opt: (seg_len, i, j, forward before reversed)


def plant_hits(plant):
    """The seams this plant hits, as decided by the oracle's winner."""
    mv = oracle_move(plant)
    win = coords(plant, mv)
    if plant.neg:
        # nothing may be reported at the aim
        hit = win is None or _loop_key(plant, win)[:3] != _loop_key(plant, plant.aims[0])[:3]
        return {plant.neg + (f"@jc{jc(plant.n)}" if plant.scan == "3" else "")} if hit else set()
    if len(plant.aims) > 1:
        # a tie: the winner is the first aim in loop order, and without that aim's own entries the next one wins with the same bits
        order = sorted(range(len(plant.aims)), key=lambda a: _loop_key(plant, plant.aims[a]))
        if win != plant.aims[order[0]]:
            return set()
        nxt = oracle_move(plant, drop=(order[0],))
        if coords(plant, nxt) != plant.aims[order[1]] or value_bits(plant, nxt) != value_bits(plant, mv):
            return set()
        cls = (tie_class3 if plant.scan == "3" else tie_class_or)(plant.n, plant.aims[order[0]], plant.aims[order[1]])
        return {cls} if cls else set()
    if win is None:
        return set()
    return seams3(plant.n, *win) if plant.scan == "3" else seams_or(plant.n, *win)


def all_tables():
    return [("3", n, k) for n in SIZES3 for k in KINDS] + [("or", n, k) for n in SIZES_OR for k in KINDS]


def table(scan, n, kind):
    return table3(n, kind) if scan == "3" else table_or(n, kind)


def hit_table(scan):
    """{seam: [ids of the plants whose oracle winner lies on it]} over every table of the scan."""
    names = (SEAMS3 + list(TIES3)) if scan == "3" else (SEAMS_OR + list(TIES_OR))
    hits = {s: [] for s in names}
    for sc, n, kind in all_tables():
        if sc == scan:
            for p in table(sc, n, kind):
                for s in plant_hits(p):
                    hits.setdefault(s, []).append(p.id)
    return hits
