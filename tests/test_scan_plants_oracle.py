"""The planted-winner tables of tests/_plants.py against the oracle alone (no GPU): every seam of the 3-opt and Or-opt work
division that tests/test_gpu_scan_plants.py means to pin must be the place of at least one plant's ORACLE winner — not merely
aimed at.  Without this the GPU tests could pass while missing their targets."""
import numpy as np
import pytest

import _oracle as O
import _plants as P


@pytest.mark.parametrize("scan,n,kind", P.all_tables(), ids=lambda v: str(v))
def test_every_plant_has_an_oracle_answer(scan, n, kind):
    # fills the shared cache table by table, and holds the oracle's winners to what a plant can mean: a valid move, strictly better
    # than nothing, and never at a must-not-be-reported aim
    for p in P.table(scan, n, kind):
        mv = P.oracle_move(p)
        win = P.coords(p, mv)
        if p.neg:
            assert P.plant_hits(p), (p.id, "the oracle reports the aim", win)
            continue
        assert mv is not None, p.id
        if scan == "3":
            i, j, k, case = win
            assert 0 <= i < j < k < n and j <= n - 2 and not (i == 0 and k == n - 1) and 1 <= case <= 7 and mv[4] > 0
        else:
            seg_len, i, j, rev = win
            assert 1 <= seg_len <= 3 and i + seg_len <= n and j != (i - 1) % n and not i <= j < i + seg_len and mv[0] < np.float32(-1e-3)


@pytest.mark.parametrize("scan", ["3", "or"])
def test_every_seam_is_hit_by_an_oracle_winner(scan):
    hits = P.hit_table(scan)
    print({s: v[:3] for s, v in hits.items()})
    missed = [s for s, v in hits.items() if not v]
    assert not missed, f"no plant's oracle winner lies on: {missed}"
    # the tables aim; a plant whose winner moved elsewhere stays in the GPU comparison as a tie or ordering case
    wanted = set(P.SEAMS3) | set(P.TIES3) if scan == "3" else set(P.SEAMS_OR) | set(P.TIES_OR)
    assert wanted <= set(hits)


@pytest.mark.parametrize("n", sorted(set(P.SIZES3) | set(P.SIZES_OR) | {1100}))
def test_the_constant_matrix_has_no_move(n):
    m = P.constant_matrix(n)
    for kind in P.KINDS:
        if n <= 300:
            assert O.three_opt_find_best_move(None, m, P.tour(n, kind)) is None
        assert O.or_opt_find_best_move(None, m, P.tour(n, kind)) is None


@pytest.mark.parametrize("n", P.THRESHOLD_SIZES)
def test_or_opt_threshold_plants(n):
    # or_opt.rs:86: -2^-9 is below -1e-3 and is taken, -2^-10 is not
    for kind in P.KINDS:
        for p in P.threshold_plants(n, kind):
            mv = P.oracle_move(p)
            if "take" in p.label:
                assert mv is not None and P.value_bits(p, mv) == P.THRESHOLD_TAKEN_BITS, p.id
            else:
                assert mv is None, p.id


@pytest.mark.parametrize("span", ["long_l1", "long_l2", "both"])
def test_apply_plants_win_and_end_at_once_3opt(span):
    # the construction the GPU test traces at n = 1100, at the size the oracle affords: the plant is the first move and the descent
    # ends within APPLY_MAX_MOVES
    n = 300
    for p in P.apply_table3(n, "perm"):
        if span in p.label:
            assert P.coords(p, P.oracle_move(p)) == p.aims[0], p.id
            rc, out, cost, st = O.three_opt(None, p.matrix(), n, init=p.path())
            assert rc == 0 and 1 <= st["moves"] <= P.APPLY_MAX_MOVES, (p.id, st)


@pytest.mark.parametrize("n", P.APPLY_SIZES)
def test_apply_plants_win_and_end_at_once_or_opt(n):
    for kind in P.KINDS:
        for p in P.apply_table_or(n, kind):
            assert P.coords(p, P.oracle_move(p)) == p.aims[0], p.id
            rc, out, cost, st = O.or_opt(None, p.matrix(), n, init=p.path())
            assert rc == 0 and st["moves"] == 1, (p.id, st)
