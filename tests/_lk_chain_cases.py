"""Start tours whose FIRST Lin–Kernighan move is a chain of a known number of exchanges.  TEST INFRASTRUCTURE ONLY (no tests here).

The LK tests that start from the nearest-neighbour seed apply chains of one or two exchanges and, rarely, of up to six: the NN tour is
close to a local optimum.  A pass from a random permutation applies chains of every length up to max_depth = 16, and the tour just
before such a move, given as the initial tour, has that move as the first one of its pass (city_ids is then that tour, as in
find_lk_move on a flat tour).  tests/golden/make_goldens_lk_chains.py searches such tours with the oracle alone and files them in
tests/golden/goldens_lk_chains.json; tests/test_lk_chain_cases.py certifies them on the CPU; tests/test_gpu_lk_chains.py runs the GPU
search from them (and says which cases it holds back).

A case:  id, group, instance (a recipe, below), k (n_nearest), d (exchanges of the first chain = (len(chain) - 2) // 2), pass_moves
(keyed by the max_depth values to run at: d itself — the chain fills exactly what the option allows — and 16; for d = 6 the values 6
and 7, the last length of the register build and the same chain in the deep build; the value is the number of moves of the oracle's
whole pass from the tour at that max_depth), start (where the generator found it: restart_perm seed and the move's index in the replayed pass) and the tour, as a list.

Groups:
  small    64 <= n <= 400, k <= 9 (k (k+1)^2 <= 1024: the chip-wide scan takes its fused-pick form), one case for every d in 1..16
  wide     10 <= k <= 16 (the flat scan form with kept sub-chains): d = 6, d = 7 and one d >= 10
  lattice  a unit lattice, every candidate list holds ties: d >= 7
  large    n = 1600 (the chip-wide step kernel): d = 6, 7, 8 and one d >= 12
The LDS-resident form (k_lk_ils) applies only where k^(max_depth-1) nodes fit a level queue (ils_qcap below); elsewhere the same
flags run the chip-wide scans.  So the small and the large group each hold a d >= 7 case with k = 3, run at max_depth = d.

Instances are uniform points (O.synth_xy) and lattices only.  The GPU scans search every pair of a window, not only the pairs up to
the first hit as the oracle does, and on clustered points with k = 8 a single pair's search, which the oracle never reaches, can cost
10^6 nodes (counted on the CPU for one such tour: 1.5 * 10^6 at n = 400, against at most 3 * 10^4 on every tour filed here)."""
import functools
import json
import os

import numpy as np

import _oracle as O

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "goldens_lk_chains.json")
MAX_DEPTH = 16  # TL_LK_MAX_DEPTH of the deep build (lk_deep.hip)
LARGE_N = 1600  # >= 1500: the chip-wide step kernel


# ------------------------------------------------------------------------------------------------
# instances, by recipe
# ------------------------------------------------------------------------------------------------
def lattice_xy(side, seed):
    """side x side unit lattice, the cities numbered by O.restart_perm(side^2, seed, 0)."""
    g = np.stack(np.meshgrid(np.arange(side, dtype=F32), np.arange(side, dtype=F32)), -1).reshape(-1, 2)
    return np.ascontiguousarray(g[O.restart_perm(side * side, seed, 0)])


def instance_xy(recipe):
    kind = recipe["kind"]
    if kind == "uniform":
        return O.synth_xy(recipe["n"], seed=recipe["seed"])
    if kind == "lattice":
        return lattice_xy(recipe["side"], recipe["seed"])
    raise ValueError(kind)


def instance_n(recipe):
    return recipe["side"] ** 2 if recipe["kind"] == "lattice" else recipe["n"]


@functools.lru_cache(maxsize=None)
def _instance(recipe_json, k):
    xy = instance_xy(json.loads(recipe_json))
    cand, _ = O.build_candidates_kdtree(xy, k)  # the reference's lists (kd-tree order among equal distances)
    cand = np.ascontiguousarray(cand)
    xy.setflags(write=False)
    cand.setflags(write=False)
    return xy, cand


def instance(recipe, k):
    """(xy, kd-tree candidate lists), read-only and shared."""
    return _instance(json.dumps(recipe, sort_keys=True), k)


# ------------------------------------------------------------------------------------------------
# the first move
# ------------------------------------------------------------------------------------------------
def exchanges(chain):
    return 0 if chain is None else (len(chain) - 2) // 2


def first_chain(xy, tour, cand, max_depth):
    return O.find_lk_move(xy, np.asarray(tour, dtype=np.uint32), cand, max_depth)


def case_depths(d):
    return [6, 7] if d == 6 else sorted({d, MAX_DEPTH})


# ------------------------------------------------------------------------------------------------
# which runs the LDS-resident form (k_lk_ils) takes
# ------------------------------------------------------------------------------------------------
LDS_BYTES = 160 * 1024  # one CU of gfx950


def ils_qcap(n, k, max_depth, lds_budget=LDS_BYTES):
    """lk.hip lk_ils_qcap restated: the records per level queue of k_lk_ils, or 0 where the form does not apply.  The host
    (tl_api_lk.hip) then runs the chip-wide scans instead, also under TL_FLAG_LK_ILS_LDS and at n <= 700.  The widest queued level of
    ONE pair's search, k^(max_depth-1) nodes, must fit a queue: at max_depth >= 7 that leaves k = 2 (up to 11) and k = 3 (7 alone)."""
    build_depth = 6 if max_depth <= 6 else MAX_DEPTH                      # lk.hip / lk_deep.hip: TL_LK_MAX_DEPTH
    if n < 4 or n > 65535 or k == 0 or k > 16 or max_depth == 0:
        return 0
    bits = 1
    while (1 << bits) < k + 1:                                            # ils_bits
        bits += 1
    if bits * max_depth > 64:
        return 0

    def up16(v):
        return (v + 15) & ~15

    fixed = up16(n * 8) + up16(n * k * 2) + up16(n * k * 4) + up16(n * 4) + 7 * up16(n * 2) + 1024 * 8  # ils_fixed_bytes
    fixed += (1024 // 64) * (2 * (build_depth + 2)) * 16 + 1024           # kIlsStatic: per-wave segment tables of kLkMaxSeg entries
    if fixed >= lds_budget:
        return 0
    rec = (4 + max_depth) * 4
    qcap = (lds_budget - fixed) // (2 * rec)
    need = 1
    for _ in range(1, max_depth):
        need *= k
        if need > qcap:
            return 0
    cap = max(need, 512)
    if n * 4 > 2 * cap * rec:
        cap = (n * 4 + 2 * rec - 1) // (2 * rec)
    qcap = min(qcap, cap, 2048)
    return 0 if qcap < 64 or 2 * qcap * rec < n * 4 else qcap


def takes_lds_form(n, k, max_depth):
    return ils_qcap(n, k, max_depth) > 0


# ------------------------------------------------------------------------------------------------
# the fixtures
# ------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, rec):
        self.rec = rec
        self.id, self.group, self.recipe, self.k, self.d = rec["id"], rec["group"], rec["instance"], rec["k"], rec["d"]
        self.pass_moves = {int(k): v for k, v in rec["pass_moves"].items()}
        self.depths = sorted(self.pass_moves)
        self.n = instance_n(self.recipe)
        self.tour = np.array(rec["tour"], dtype=np.uint32)
        self.tour.setflags(write=False)

    def build(self):
        xy, cand = instance(self.recipe, self.k)
        return xy, cand, self.tour

    def oracle(self, max_depth, epochs=0, platoo_epochs=10, seed=1, packed=None):
        """The oracle's run from the tour, computed once per argument set and shared: (rc, route, cost, stats, snapshots)."""
        key = (max_depth, epochs, platoo_epochs, seed, packed is not None)
        memo = self.__dict__.setdefault("_memo", {})
        if key not in memo:
            xy = self.build()[0]
            r = O.lin_kernighan_trace(xy, init=self.tour, epochs=epochs, platoo_epochs=platoo_epochs, n_nearest=self.k, max_depth=max_depth,
                                      seed=seed, packed=packed, cap=epochs + 1)
            r[1].setflags(write=False)
            memo[key] = r
        return memo[key]


@functools.lru_cache(maxsize=None)
def load():
    with open(GOLDEN) as fh:
        return tuple(Case(rec) for rec in json.load(fh)["cases"])


def group(*names):
    return [c for c in load() if c.group in names]


def pick(grp, d):
    """The case of a group with exactly d exchanges (the first, if several)."""
    return next(c for c in load() if c.group == grp and c.d == d)


def missing_requirements(records):
    """What the required-cases list (module docstring) still lacks in `records` (dicts as filed): a list of sentences, empty if met."""
    miss = []
    by = {}
    for r in records:
        by.setdefault(r["group"], []).append(r)
        n, k, d = instance_n(r["instance"]), r["k"], r["d"]
        ok = {"small": 64 <= n <= 400 and k <= 9 and k * (k + 1) ** 2 <= 1024 and r["instance"]["kind"] != "lattice",
              "wide": 64 <= n <= 400 and 10 <= k <= 16 and k * (k + 1) ** 2 > 1024,
              "lattice": 64 <= n <= 400 and k <= 9 and r["instance"]["kind"] == "lattice",
              "large": n == LARGE_N and k <= 9}.get(r["group"], False)
        if not ok:
            miss.append(f"{r['id']}: n = {n}, k = {k} do not fit group {r['group']}")
        if not 1 <= d <= MAX_DEPTH or sorted(int(q) for q in r["pass_moves"]) != case_depths(d):
            miss.append(f"{r['id']}: d = {d} with depths {sorted(r['pass_moves'])}")
    ds = {g: sorted(r["d"] for r in rs) for g, rs in by.items()}
    for d in range(1, MAX_DEPTH + 1):
        if d not in ds.get("small", []):
            miss.append(f"small: no case with d = {d}")
    for d in (6, 7):
        if d not in ds.get("wide", []):
            miss.append(f"wide: no case with d = {d}")
    if not any(d >= 10 for d in ds.get("wide", [])):
        miss.append("wide: no case with d >= 10")
    if not any(d >= 7 for d in ds.get("lattice", [])):
        miss.append("lattice: no case with d >= 7")
    for d in (6, 7, 8):
        if d not in ds.get("large", []):
            miss.append(f"large: no case with d = {d}")
    if not any(d >= 12 for d in ds.get("large", [])):
        miss.append("large: no case with d >= 12")
    # (not in the issue's list: without these no chain of the deep build would pass through k_lk_ils at all)
    for g in ("small", "large"):
        if not any(r["d"] >= 7 and takes_lds_form(instance_n(r["instance"]), r["k"], r["d"]) for r in by.get(g, [])):
            miss.append(f"{g}: no case with d >= 7 whose run at max_depth = d takes the LDS-resident form (k = 3, d = 7 or k = 2, d <= 11)")
    return miss
