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
