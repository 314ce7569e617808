"""The planted Lin–Kernighan start tours of tests/golden/goldens_lk_chains.json against the oracle alone (no GPU): from every stored
tour the first move of a pass is a chain of exactly the recorded number of exchanges, the same chain at each recorded max_depth, and
applying it gives a shorter permutation; the set holds every required case (tests/_lk_chain_cases.py).  This certifies what
tests/test_gpu_lk_chains.py relies on: that a GPU form which matches the oracle from these tours has found, validated and applied a
chain of that length."""
import numpy as np
import pytest

import _lk_chain_cases as L
import _oracle as O

CASES = {c.id: c for c in L.load()}
assert len(CASES) == len(L.load())


def test_the_fixture_set_holds_every_required_case():
    assert L.missing_requirements([c.rec for c in L.load()]) == []
    assert sorted(c.d for c in L.group("small")) == list(range(1, L.MAX_DEPTH + 1))


@pytest.mark.parametrize("cid", list(CASES))
def test_the_first_move_is_a_chain_of_the_recorded_length(cid):
    c = CASES[cid]
    xy, cand, tour = c.build()
    assert len(xy) == c.n == len(tour) and cand.shape == (c.n, c.k)
    assert O.validate_tour(tour)
    assert c.depths == L.case_depths(c.d) and c.d in c.depths
    chains = [L.first_chain(xy, tour, cand, depth) for depth in c.depths]
    for depth, chain in zip(c.depths, chains):
        assert chain is not None and L.exchanges(chain) == c.d and len(chain) == 2 * c.d + 2, (depth, chain)
        assert len(set(chain)) == len(chain)  # 2 d + 2 cities: what the chain arrays and slots of the build must hold
        assert chain == chains[0], f"max_depth {depth} finds another chain than max_depth {c.depths[0]}"
    after = O.apply_lk_chain(tour, chains[0])
    assert O.validate_tour(after)
    assert float(O.tour_length(xy, None, tour)) - float(O.tour_length(xy, None, after)) > 1e-6


@pytest.mark.parametrize("cid", list(CASES))
def test_the_whole_pass_is_as_long_as_recorded(cid):
    # the GPU tests run the whole pass: its length is what keeps them short (tens of moves; a few hundred at n = 1600)
    c = CASES[cid]
    for depth in c.depths:
        rc, route, cost, st, snaps = c.oracle(depth)
        assert rc == 0 and O.validate_tour(route)
        assert st["moves"] == c.pass_moves[depth] >= 1 and st["sweeps"] == st["moves"] + 1
        assert st["reversed"] >= c.d  # the exchanged edges of the first chain alone
        assert len(snaps) == 1 and snaps[0][0].tolist() == route.tolist()
    assert max(c.pass_moves.values()) <= (400 if c.group == "large" else 256)
