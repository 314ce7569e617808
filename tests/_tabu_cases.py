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


# ---------------------------------------------------------------- lists longer than one look-up round
CUS, LDS_BYTES, WORK = K.CUS, K.LDS_BYTES, 8 << 30  # the device the sizes below were chosen for; the GPU tests read theirs from device_info


def opt_start(xy):
    """a 2-opt local optimum (the plain-C oracle's descent from city order): no reversal shortens it, so early epochs reach deep attempts"""
    import numpy as np

    import _oracle as O
    n = len(xy)
    rc, route, _cost, _st = O.two_opt(xy, None, n, init=np.arange(n, dtype=np.uint32))
    assert rc == 0
    return np.asarray(route, dtype=np.uint32)


# One wave per chain (more chains than CUs) looks 64 listed routes up per round: n -> seed of a chain from opt_start whose list, longer
# than that and wrapped, refuses a candidate because of a route in the second round.  Picked on the CPU with the oracle, scanning
# seeds from 1 upward (such refusals are rare: n = 68 has its first at seed 458); check_wrapped_ring states what for.
WRAP_EPOCHS = 160
WRAP_SEEDS = {66: 242, 67: 67, 68: 458, 69: 72, 70: 18}


def wrap_chain(n):
    """(key, xy, packed, n, init, epochs, seed) of the chain above, as check_chain takes them"""
    xy = K.synth(n, n)
    return f"wrap{n}", xy, None, n, opt_start(xy), WRAP_EPOCHS, WRAP_SEEDS[n]


def check_wrapped_ring(n, width, log, rec):
    """on the oracle's record: (a) a refusal whose every matching listed route sits at a ring index >= width, beyond the look-up's first
    round; (b) after the ring has wrapped (epoch > n) an improving candidate is checked against the list and taken; (c) a refusal
    after the wrap"""
    assert n > width and rec["list_len"][n - 1:] == [n] * (len(log) - n + 1)
    assert any(idx and min(idx) >= width for _e, _a, idx in rec["refusals"]), rec["refusals"]
    assert any(e > n and a < n and rec["checked"][e] >= 1 for e, (a, *_x) in enumerate(log))
    assert any(e > n for e, _a, _idx in rec["refusals"]), rec["refusals"]


# A single chain (four waves) looks 256 listed routes up per round: from city order at n = 300 improving candidates are still found, and
# so looked up, when the list is longer than that; the ring wraps at epoch 300.
LONG_N, LONG_EPOCHS, LONG_SEED = 300, 330, 1


def long_chain():
    return f"long{LONG_N}", K.synth(LONG_N, LONG_N), None, LONG_N, None, LONG_EPOCHS, LONG_SEED


def check_long_list(n, width, log, rec):
    assert n > width and rec["list_len"][n - 1:] == [n] * (len(log) - n + 1)
    beyond = [e for e in range(len(log)) if rec["list_len"][e] > width and rec["checked"][e] >= 1]
    assert len(beyond) >= 10 and any(e > n for e in beyond), "no look-up in a list longer than one round, or none after the wrap"
