"""Instances the ant colony tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import numpy as np

import _sa_cases as K

CHUNK = 64  # cities per tile of the construct kernel (csrc/ant_colony.hip: kAcoChunk)
OPT = dict(alpha=1.0, beta=2.0, evaporation_rate=0.5, num_ants=25)


def start_tour(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def instance(n):
    return K.tsplib("berlin52")["xy"] if n == 52 else K.small(n) if n <= 8 else K.synth(n, 900 + n)


# name -> (xy, packed, n, init or None, dict(epochs, alpha, beta, evaporation_rate, num_ants, seed, run)): what goldens_aco.json freezes
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    return {
        "berlin52": (b["xy"], None, 52, None, dict(OPT, epochs=12, seed=1, run=0)),
        "berlin52_init_run2": (b["xy"], None, 52, np.arange(52, dtype=np.uint32), dict(OPT, epochs=12, seed=2, run=2)),
        "gr17_matrix": (g["xy"], g["packed"], 17, None, dict(OPT, epochs=20, seed=4, run=0)),
        "small5": (K.small(5), None, 5, None, dict(OPT, epochs=15, num_ants=6, seed=5, run=0)),
        "small8_init": (K.small(8), None, 8, start_tour(8, 8), dict(OPT, epochs=20, num_ants=8, alpha=1.5, beta=2.5, evaporation_rate=0.3, seed=8, run=0)),
        "synth65_init": (K.synth(65, 65), None, 65, start_tour(65, 65), dict(OPT, epochs=4, num_ants=65, seed=65, run=0)),
    }


# alpha = 20 on berlin52 with an initial tour: tau0 = 25 / cost ~ 1e-3, tau^20 underflows to 0: every selection takes the eta path
UNDERFLOW = dict(OPT, epochs=2, alpha=20.0, seed=3, run=0)
# 400 coincident cities, beta = 6: eta = (1e6)^6 = 1e36, and more than 340 of them sum past f32's maximum: the first candidate
COINCIDENT = dict(OPT, epochs=2, beta=6.0, num_ants=3, seed=9, run=0)
COINCIDENT_N = 400


def check_conditions(name, n, res, opts):
    """what each golden case is there for, asserted on the oracle's record: no case passes vacuously"""
    assert len(res["epochs"]) == opts["epochs"] and res["counters"]["tours"] == opts["epochs"] * opts["num_ants"]
    assert res["counters"]["improved"] >= 1 and len(res["routes"]) == 1 + res["counters"]["improved"], name
    assert sorted(res["tour"].tolist()) == list(range(n))
    assert res["counters"]["fallbacks"] == 0, name  # ordinary parameters never leave the primary weights
    if name == "synth65_init":
        assert opts["num_ants"] > 64  # two groups of ants


def selection_rows(n, seed):
    """(weights, eta, visited, r1, r2, what) for the selection self-test at n cities: random rows, targets in the first and the last
    chunk, exact ties, a zero-weight first city at r1 = 0, exhaustion, all visited but one, the eta path, the first-candidate path"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    e = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    none = np.zeros(n, dtype=np.uint32)
    some = (rng.uniform(size=n) < 0.4).astype(np.uint32)
    some[int(rng.integers(n))] = 0
    rows = []
    for vis in (none, some):
        for r1 in (0.0, 1e-7, 0.25, 0.5, 0.999, float(np.float32(1.0 - 2.0 ** -24))):
            rows.append((w, e, vis, r1, 0.5, "random"))
    rows.append((w, e, some, 1.0, 0.5, "r1 = 1: the walk is exhausted, the last unvisited city"))
    rows.append((w, e, none, 2.0, 0.5, "exhausted, nothing visited"))
    tail = some.copy()
    tail[n - 1] = 1
    if (tail == 0).any():
        rows.append((w, e, tail, 1.5, 0.5, "exhausted with city n - 1 visited"))
    one = np.ones(n, dtype=np.uint32)
    one[n // 2] = 0
    rows.append((w, e, one, 0.3, 0.5, "all visited but one"))
    ties = np.full(n, 0.25, dtype=np.float32)  # exact sums: the prefix hits r1 total exactly, the strict test moves on
    for r1 in (0.0, 0.25, 0.5, 0.75):
        rows.append((ties, e, none, r1, 0.5, "exact ties"))
    z = w.copy()
    z[0] = 0.0
    rows.append((z, e, none, 0.0, 0.5, "a zero-weight first city at r1 = 0"))
    zero = np.zeros(n, dtype=np.float32)
    for r2 in (0.0, 0.4, 0.9999, 1.0):
        rows.append((zero, e, some, 0.5, r2, "primary all zero: the eta path"))
    nanw = w.copy()
    nanw[n - 1] = np.nan
    rows.append((nanw, e, none, 0.5, 0.5, "a NaN weight: the eta path"))
    big = np.full(n, 3e38, dtype=np.float32)
    rows.append((big if n > 1 else nanw, np.full(n, np.inf, dtype=np.float32), some, 0.5, 0.5, "both sums non-finite: the first candidate"))
    rows.append((zero, zero, some, 0.5, 0.5, "both sums zero: the first candidate"))
    return rows


# the reference's own unit vectors for select_next (ant_colony.rs:336-355): (primary, fallback, r1, r2, chosen)
REFERENCE_SELECT = [
    ([1.0, 3.0], [1.0, 1.0], 0.5, 0.5, 1),
    ([0.0, 0.0], [1.0, 3.0], 0.5, 0.5, 1),
    ([0.0, float("nan")], [0.0, 0.0], 0.5, 0.5, 0),
]
