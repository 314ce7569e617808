#!/usr/bin/env python3
"""Regenerates tests/golden/goldens_lk_chains.json: start tours whose first Lin–Kernighan move is a chain of a known number of
exchanges (tests/_lk_chain_cases.py says what a case holds and which cases are required).  CPU only, the oracle only.

Search: oracle passes from O.restart_perm starts over kd-tree candidate lists at max_depth 16, replayed move by move with
O.find_lk_move / O.apply_lk_chain.  The tour before a move of d exchanges is a candidate for d.  Per (group, d) the candidates are
ranked: first those whose run at max_depth = d takes the LDS-resident form (L.takes_lds_form: few do, and only they pass a deep
chain through k_lk_ils), then a remaining pass of at most 64 moves, then the smaller instance (the file stays small), then the shorter remainder.
(The replay takes city_ids = the current tour at every move; the real pass keeps the start's.  The replayed remainder therefore only
ranks; what is filed as pass_moves is the move count of O.lin_kernighan from the tour, per max_depth.)

A candidate is filed only if the oracle confirms it: O.find_lk_move from the tour returns the same chain of d exchanges at each of
the case's max_depth values (a depth-first search cut at d visits a subset of the same nodes in the same order, but an EARLIER pair
whose first chain at depth 16 is deeper than d and no tour may close a shorter, valid one under the cut: checked, not assumed).

A replayed pass is given up after PASS_SECONDS of wall clock (none of the plan's is, as measured; a guard) and contributes
nothing: its remainder is unknown.  Which passes that hits depends on the machine, so a regenerated file may choose other tours; it
must pass tests/test_lk_chain_cases.py all the same.  The script fails if a required case is missing.

Usage: python tests/golden/make_goldens_lk_chains.py      (measured: 61 s of one core)
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import _lk_chain_cases as L  # noqa: E402
import _oracle as O  # noqa: E402

PASS_SECONDS = 5.0
SHORT_PASS = 64
KEEP = 12  # ranked candidates kept per (group, d)


def plan():
    """(group, recipe, k, start seed), in a fixed order."""
    for n in (64, 100, 150, 200, 300, 400):
        for k in (3, 4, 5, 8):
            for seed in (1, 2, 3, 4, 5, 6, 7, 8):
                for s in (1, 2, 3, 4):
                    yield "small", {"kind": "uniform", "n": n, "seed": seed}, k, s
    for n in (64, 100, 150, 200):
        for k in (10, 12, 16):
            for seed in (1, 2, 3):
                for s in (1, 2, 3):
                    yield "wide", {"kind": "uniform", "n": n, "seed": seed}, k, s
    for side in (8, 10, 12, 15, 20):
        for k in (5, 6, 8):
            for seed in (1, 2, 3):
                for s in (1, 2, 3):
                    yield "lattice", {"kind": "lattice", "side": side, "seed": seed}, k, s
    for seed, k, s in ((3, 8, 7), (2, 5, 6), (1, 5, 1), (1, 8, 2), (4, 5, 3), (4, 8, 4)) + tuple((seed, 3, s) for seed in (1, 2, 3, 4) for s in (1, 2, 3)):
        yield "large", {"kind": "uniform", "n": L.LARGE_N, "seed": seed}, k, s


def replay(xy, cand, start):
    """The pass from `start`, move by move: [(exchanges, tour before the move)], and whether it ran to its end."""
    tour = np.array(start, dtype=np.uint32)
    out = []
    t0 = time.time()
    while True:
        chain = O.find_lk_move(xy, tour, cand, L.MAX_DEPTH)
        if chain is None:
            return out, True
        out.append((L.exchanges(chain), tour))
        tour = O.apply_lk_chain(tour, chain)
        if time.time() - t0 > PASS_SECONDS:
            return out, False


def confirm(xy, cand, tour, d):
    """The same chain of d exchanges at each max_depth of the case, and a shorter permutation after it."""
    chains = [O.find_lk_move(xy, tour, cand, depth) for depth in L.case_depths(d)]
    if any(c is None or L.exchanges(c) != d or c != chains[0] for c in chains):
        return False
    after = O.apply_lk_chain(tour, chains[0])
    return O.validate_tour(after) and float(O.tour_length(xy, None, tour)) - float(O.tour_length(xy, None, after)) > 1e-6


def main():
    t_start = time.time()
    pool = {}  # (group, d) -> [(rank key, recipe, k, start seed, step, tour)]
    skipped = []
    for grp, recipe, k, s in plan():
        xy, cand = L.instance(recipe, k)
        n = len(xy)
        moves, whole = replay(xy, cand, O.restart_perm(n, s, 0))
        if not whole:
            skipped.append((recipe, k, s, len(moves)))
            continue  # (the remainder of an unfinished pass is unknown)
        for step, (d, tour) in enumerate(moves):
            rest = len(moves) - step
            lds = L.takes_lds_form(n, k, d) and (grp == "small" or d >= 7)  # (at n = 1600 these passes are long: for the deep build only)
            key = (not lds, rest > SHORT_PASS, n, rest, step)
            lst = pool.setdefault((grp, d), [])
            if len(lst) < KEEP or key < lst[-1][0]:
                lst.append((key, recipe, k, s, step, tour))
                lst.sort(key=lambda e: e[0])
                del lst[KEEP:]

    def best(grp, d):
        for key, recipe, k, s, step, tour in pool.get((grp, d), []):
            xy, cand = L.instance(recipe, k)
            if confirm(xy, cand, tour, d):
                return key, recipe, k, s, step, tour
        return None

    def deepest(grp, lo):
        found = [(d, best(grp, d)) for d in range(L.MAX_DEPTH, lo - 1, -1)]
        found = [(d, b) for d, b in found if b is not None]
        short = [(d, b) for d, b in found if not b[0][1]]
        return (short or found or [(None, None)])[0][0]

    wanted = [("small", d) for d in range(1, L.MAX_DEPTH + 1)]
    wanted += [("wide", 6), ("wide", 7), ("wide", deepest("wide", 10))]
    wanted += [("lattice", deepest("lattice", 7))]
    wanted += [("large", 6), ("large", 7), ("large", 8), ("large", deepest("large", 12))]
    records = []
    for grp, d in wanted:
        b = None if d is None else best(grp, d)
        if b is None:
            continue  # missing_requirements names it below
        key, recipe, k, s, step, tour = b
        xy, cand = L.instance(recipe, k)
        pass_moves = {}
        for depth in L.case_depths(d):
            rc, route, cost, st = O.lin_kernighan(xy, init=tour, epochs=0, n_nearest=k, max_depth=depth)
            assert rc == 0 and O.validate_tour(route)
            pass_moves[str(depth)] = st["moves"]
        records.append({"id": f"{grp}-d{d:02d}", "group": grp, "instance": recipe, "k": k, "d": d,
                        "pass_moves": pass_moves, "start": {"seed": s, "step": step}, "tour": [int(v) for v in tour]})
    miss = L.missing_requirements(records)
    found = {g: sorted(d for gg, d in pool if gg == g) for g in ("small", "wide", "lattice", "large")}
    assert not miss, "the search missed required cases:\n  " + "\n  ".join(miss) + f"\n(lengths met, unconfirmed: {found})"
    with open(L.GOLDEN, "w") as fh:  # one case per line, no blanks: the tours are most of the file
        fh.write('{"cases":[\n' + ",\n".join(json.dumps(r, separators=(",", ":"), sort_keys=True) for r in records) + "\n]}\n")
    for r in records:
        print(r["id"], r["instance"], "k", r["k"], "pass moves", r["pass_moves"], "from", r["start"])
    for sk in skipped:
        print("given up after", PASS_SECONDS, "s:", sk)
    print(f"{len(records)} cases, {os.path.getsize(L.GOLDEN)} bytes, {time.time() - t_start:.0f} s")


if __name__ == "__main__":
    main()
