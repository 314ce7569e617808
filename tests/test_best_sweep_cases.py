"""The best-sweep case table of tests/_best_sweep_cases.py against the oracle alone (no GPU): the plain numpy specification, the
restated kernel scheme and tlo_two_opt_best agree on every case; every seam of the kernel that tests/test_gpu_best_sweep.py means to
pin is reached by some case (asserted from the model's branch record and the reference's move list — not merely aimed at); and every
planted defect of the model changes the result of some case, so a kernel with that defect could not pass the GPU comparison."""
import functools
import json
import os

import numpy as np
import pytest

import _best_sweep_cases as B

CASES = {c.id: c for c in B.case_table()}
assert len(CASES) == len(B.case_table())


@functools.lru_cache(maxsize=None)
def runs(cid):
    """(xy, start, oracle, reference, model) of a case: computed once, shared, left unchanged."""
    xy, tour = CASES[cid].build()
    return xy, tour, B.oracle_best_sweep(xy, tour), B.ref_best_sweep(xy, tour), B.model_best_sweep(xy, tour)


@pytest.mark.parametrize("cid", list(CASES))
def test_reference_model_and_oracle_agree(cid):
    assert CASES[cid].n <= 8300
    xy, tour, o, r, m = runs(cid)
    assert o["moves"] >= 2 and o["sweeps"] == o["moves"] + 1
    for name, x in (("reference", r), ("model", m)):
        assert x["tour"].tolist() == o["tour"].tolist(), name
        assert (x["cost_bits"], x["sweeps"], x["moves"], x["reversed"]) == (o["cost_bits"], o["sweeps"], o["moves"], o["reversed"]), name
    assert m["move_list"] == [(i, j) for i, j, _ in r["move_list"]]


def seams(cid):
    """The seams a case reaches, from the reference's moves and the model's record."""
    xy, tour, o, r, m = runs(cid)
    n, hit, rec = CASES[cid].n, set(), m["record"]
    for (i, j, _), (rows_tied, cols_tied) in zip(r["move_list"], r["ties"]):
        hit |= {name for name, yes in (
            ("move with i < 4096 <= j", i < 4096 <= j), ("move with i and j >= 4096", i >= 4096), ("move with j = n-2", j == n - 2),
            ("move with i = n-4", i == n - 4), ("move at j = 4096 at n = 4098", n == 4098 and j == 4096), ("move with js - is > 1024", j - i > 1024),
            ("move with is>>6 != (is+1)>>6", i >> 6 != (i + 1) >> 6), ("move with j >= 8192", j >= 8192),
            ("tie between two rows", rows_tied > 1), ("tie inside the winning row", cols_tied > 1)) if yes}
    for s in range(1, len(rec["branch"])):
        is_, js = m["move_list"][s - 1]  # the move this sweep's scan was told of
        br, pc, g0, g1 = rec["branch"][s], rec["partial_col"][s], rec["g0"][s], rec["g1"][s]
        hit |= {name for name, yes in (
            ("row in [is, js] decided afresh", (br == B.BR_AFRESH).any()), ("row > js keeps its key", (br == B.BR_KEPT).any()),
            ("row < is rescanned over [is, js]", ((br == B.BR_PARTIAL_WINS) | (br == B.BR_PARTIAL_LOSES)).any()),
            ("cached column in [is, js]", (br == B.BR_CACHED_COL_IN_RANGE).any()), ("partial rescan wins at column is", (pc == is_).any()),
            ("partial rescan wins at column js", (pc == js).any()), ("partial rescan loses to the cached key", (br == B.BR_PARTIAL_LOSES).any()),
            ("partial rescan begins in a later tile group", ((g0 >= 1) & (br >= B.BR_PARTIAL_WINS)).any())) if yes}
    g0, g1 = rec["g0"][0], rec["g1"][0]
    hit |= {name for name, yes in (("scan over two tile groups", (g1 > g0).any()), ("scan over three tile groups", (g1 > g0 + 1).any()),
                                   ("scan that begins in a later tile group", (g0 >= 1).any())) if yes}
    return hit


WANTED = ["move with i < 4096 <= j", "move with i and j >= 4096", "move with j = n-2", "move with i = n-4", "move at j = 4096 at n = 4098",
          "move with js - is > 1024", "move with is>>6 != (is+1)>>6", "row in [is, js] decided afresh", "row > js keeps its key",
          "row < is rescanned over [is, js]", "cached column in [is, js]", "partial rescan wins at column is", "partial rescan wins at column js",
          "partial rescan loses to the cached key", "tie between two rows", "tie inside the winning row",
          # beyond the issue's list: the tile-group loop itself
          "scan over two tile groups", "scan over three tile groups", "scan that begins in a later tile group",
          "partial rescan begins in a later tile group", "move with j >= 8192"]


def test_every_seam_is_reached_by_some_case():
    first = {}
    for cid in CASES:
        for s in sorted(seams(cid)):
            first.setdefault(s, cid)
    print(json.dumps(first, indent=1))
    missed = [s for s in WANTED if s not in first]
    assert not missed, f"no case reaches: {missed}"


def test_the_sizes_the_issue_names_are_in_the_table():
    ns = [c.n for c in CASES.values()]
    assert {4098, 4160, 4161, 4223, 4224, 8300} <= set(ns)
    assert sum(1 for c in CASES.values() if c.family == "uniform" and 4100 <= c.n <= 4300 and 8 <= len(c.plants) <= 12) >= 3
    assert all(b - a <= 1500 for c in CASES.values() if c.family == "uniform" for a, b in c.plants)


# the case tried first for each defect (any case may kill it; the assertion is over the whole table)
FIRST_TRY = {"a": "snake4223", "f": "snake4161", "g": "snake300", "h": "snake4098", "k": "uniform400", "l": "uniform700", "m": "snake4224-twenty"}


@pytest.mark.parametrize("defect", list(B.DEFECTS))
def test_every_defect_changes_some_result(defect, golden_dir):
    """Every planted defect gives a result that differs from the oracle's in (tour, cost bits, sweeps, moves, reversed) on some case.
    Defects i and j (a 15-bit decode mask) cannot show below n = 32 768: the n = 65 535 golden kills them — make_goldens_best_sweep.py
    ran the model with each against the oracle there; here the golden's recorded moves are decoded with the mask."""
    if defect in ("i", "j"):
        with open(os.path.join(golden_dir, "goldens_best_sweep.json")) as fh:
            moves = json.load(fh)["snake65535_best_sweep"]["moves"]
        k = 0 if defect == "i" else 1
        assert any((mv[k] & 0x7FFF) != mv[k] for mv in moves)
        print(defect, "killed by the n = 65535 golden")
        return
    order = sorted(CASES, key=lambda cid: (not cid.startswith(FIRST_TRY.get(defect, "snake300")), CASES[cid].n))
    for cid in order:
        xy, tour, o, r, m = runs(cid)
        if not B.same_result(B.model_best_sweep(xy, tour, defect=defect, max_sweeps=o["sweeps"] + 1), o):
            print(defect, "killed by", cid)
            return
    pytest.fail(f"defect {defect} ({B.DEFECTS[defect]}) changes no case's result")
