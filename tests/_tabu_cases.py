"""Instances the tabu-search tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import _sa_cases as K


# name -> (xy, packed, n, init or None, epochs, seed, chain): what goldens_tabu.json freezes.  Every case starts from city order.
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    out = {f"small{n}": (K.small(n), None, n, None, 200, 5, 0) for n in (2, 3, 4, 5, 8)}
    out["gr17_matrix"] = (g["xy"], g["packed"], 17, None, 400, 4, 0)
    out["grid4x4"] = (K.grid(4, 4), None, 16, None, 400, 6, 0)
    out["berlin52"] = (b["xy"], None, 52, None, 600, 1, 0)
    return out


HIT_CASES = ("small3", "small4", "small5", "small8", "gr17_matrix", "grid4x4")  # cases whose list refuses at least one improving candidate


def check_conditions(name, n, epochs, log, cnt):
    """what each golden case is there for, asserted on the oracle's counters: no case passes vacuously"""
    assert len(log) == epochs + 1
    if name in HIT_CASES:
        assert cnt["hits"] >= 1, (name, cnt)
    elif name == "small2":
        assert cnt["forced"] == epochs + 1 == 201 and cnt["hits"] == 0, cnt
    elif name == "berlin52":
        assert cnt["forced"] >= 1 and cnt["bests"] >= 1, cnt
    else:
        raise AssertionError(f"no conditions stated for {name}")
