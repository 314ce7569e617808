"""Instances and schedules the simulated-annealing tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import os

import numpy as np

import _sa_oracle as SA
import _tsplib

TSPLIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsplib")

# (epochs, cooling_rate, min_temperature, max_temperature)
HOT = dict(epochs=300, cooling_rate=1e-4, min_temperature=9.99e8, max_temperature=1e9)      # nearly every epoch accepted
COLD = dict(epochs=4000, cooling_rate=0.5, min_temperature=1e-7, max_temperature=1e-6)       # improvements only; `epochs` drives the loop
SHORT = dict(epochs=0, cooling_rate=1e-2, min_temperature=1e-3, max_temperature=1000.0)     # the default shape, 1 375 epochs
EMPTY = dict(epochs=0, cooling_rate=1e-4, min_temperature=1e6, max_temperature=0.0)         # the reference test's own combination


def with_epochs(k):
    """exactly k epochs (k >= 1), hot enough that worsening moves are taken: the temperature leaves the loop to `epochs`"""
    return dict(epochs=k, cooling_rate=0.5, min_temperature=400.0, max_temperature=500.0) if k else dict(EMPTY)


def tsplib(name):
    return _tsplib.parse_tsplib(os.path.join(TSPLIB, f"{name}.tsp"))


def synth(n, seed):
    """n points on a 0.25 grid in [0, 1000)^2, splitmix64-driven (exact in f32)"""
    v = np.array([SA.draw(seed, 7, k, 0) >> 40 for k in range(2 * n)], dtype=np.float64)
    return np.ascontiguousarray((np.floor(v / (1 << 24) * 4000.0) / 4.0).astype(np.float32).reshape(n, 2))


def grid(w, h):
    return np.ascontiguousarray(np.array([[x, y] for y in range(h) for x in range(w)], dtype=np.float32))


def small(n):
    return synth(n, 100 + n)


# name -> (xy, packed, n, init or None, opts, seed, chain): what goldens_sa.json freezes
def golden_cases():
    b = tsplib("berlin52")
    g = tsplib("gr17")
    out = {
        "berlin52_short": (b["xy"], None, 52, None, SHORT, 1, 0),
        "berlin52_hot": (b["xy"], None, 52, None, HOT, 2, 0),
        "berlin52_cold_chain3": (b["xy"], None, 52, None, COLD, 3, 3),
        "gr17_short": (g["xy"], g["packed"], 17, None, SHORT, 4, 0),
    }
    for n in (2, 3, 4, 5):
        out[f"small{n}_hot"] = (small(n), None, n, None, dict(HOT, epochs=120), 5, 0)
    return out


# ---------------------------------------------------------------- cases past one pass of a workgroup's loops
CUS, LDS_BYTES = 256, 160 * 1024  # the device the sizes below were chosen for; the GPU tests read theirs from device_info
LONG_EPOCHS = 60
# n -> (seed, the chain between chain 0 and the last one that is checked against the oracle).  One wave per chain (more chains than
# CUs): a reversal of more than 128 elements takes the reversal loops into a second trip.  Picked on the CPU with the oracle;
# check_long_reversals states what for.
LONG_POP = {130: (131, 58), 200: (200, 128)}
LONG_SINGLE = (1500, 14)  # (n, seed): four waves, reversals of more than 512 elements


def long_opts(epochs=LONG_EPOCHS):
    return dict(HOT, epochs=epochs)


def long_chain(n, seed, chain):
    """(key, xy, packed, n, init, opts, seed, chain) of a chain of the cases above, as SA.solve_cached takes them"""
    return (f"long{n}", seed, chain), synth(n, n), None, n, None, long_opts(), seed, chain


def check_long_reversals(trace, n, nt, same_move=False):
    """What a case past one trip is there for, on the oracle's accept trace, for a workgroup of nt threads: an accepted reversal of
    more than 2 nt elements, long enough for a second trip of the loop that swaps the positions (i = tid, tid + nt, ... while
    2 i + 1 < t - f + 1) and, where n leaves room for it, of the loop that swaps the edges (2 i + 1 < t - f); and an accepted move with
    from = 0 or to = n - 1, which rebuilds the closing edge.  same_move: one move that is both."""
    lens = [t - f + 1 for _e, f, t, _c in trace]
    assert any(ln > 2 * nt for ln in lens), "no accepted reversal of more than 2 nt elements"
    assert any(2 * nt + 1 < ln for ln in lens), "the position loop never takes a second trip"
    if n > 2 * nt + 2:
        assert any(2 * nt + 1 < ln - 1 for ln in lens), "the edge loop never takes a second trip"
    assert any(f == 0 or t == n - 1 for _e, f, t, _c in trace), "no accepted move rebuilds the closing edge"
    if same_move:
        assert any(t - f + 1 > 2 * nt + 2 and (f == 0 or t == n - 1) for _e, f, t, _c in trace), "no long reversal that rebuilds the closing edge"


# schedules cut into pieces (the tuning build's TL_SA_CHUNK): piece lengths that are no multiple of the window of 256, one window, one more
PIECES = (100, 256, 257)


def piece_cases(piece):
    """name -> (xy, n, init, opts, seed) of the single chains run in pieces of `piece` epochs"""
    b = tsplib("berlin52")["xy"]
    return {
        "berlin52_short": (b, 52, None, SHORT, 1),
        "berlin52_hot": (b, 52, None, HOT, 2),
        f"last_piece_of_one_{piece}": (b, 52, None, dict(HOT, epochs=2 * piece + 1), 21),  # its one epoch is accepted
    }


PIECE_POP_SEED = 31


def piece_start_tours():
    rng = np.random.default_rng(5)
    return np.stack([rng.permutation(52) for _ in range(3)]).astype(np.uint32)
