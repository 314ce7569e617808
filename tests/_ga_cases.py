"""Instances the genetic-algorithm tests share (goldens, oracle tests, GPU tests).  Test infrastructure."""
import numpy as np

import _sa_cases as K


def start_tour(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


# name -> (xy, packed, n, init or None, epochs, mutation_probability, n_elite, seed, run): what goldens_ga.json freezes
def golden_cases():
    b = K.tsplib("berlin52")
    g = K.tsplib("gr17")
    out = {
        "berlin52": (b["xy"], None, 52, None, 50, 0.5, 3, 1, 0),
        "berlin52_init_run2": (b["xy"], None, 52, np.arange(52, dtype=np.uint32), 50, 0.001, 3, 2, 2),
        "gr17_matrix": (g["xy"], g["packed"], 17, None, 50, 0.5, 3, 4, 0),
        "small7": (K.small(7), None, 7, None, 50, 1.0, 0, 7, 0),
        "small8_init": (K.small(8), None, 8, start_tour(8, 8), 50, 0.5, 3, 8, 0),
        "synth65_init": (K.synth(65, 65), None, 65, start_tour(65, 65), 20, 0.5, 3, 65, 0),
    }
    return out


def equal_matrix(n):
    """every distance 1: every tour has length n, every fitness ties"""
    return np.ones(n * (n - 1) // 2, dtype=np.float32)


def check_conditions(name, n, epochs, trace, cnt):
    """what each golden case is there for, asserted on the oracle's counters: no case passes vacuously"""
    assert len(trace) == epochs
    assert cnt["children"] == 2 * max(0, n // 2 - {"small7": 0}.get(name, 3)) * epochs
    assert cnt["improved"] >= 1, (name, cnt)
    if name == "small7":
        assert cnt["mutations"] == cnt["children"]
    elif name == "berlin52_init_run2":
        assert 0 < cnt["mutations"] < cnt["children"] // 50
    else:
        assert cnt["children"] // 4 < cnt["mutations"] < 3 * cnt["children"] // 4, (name, cnt)
    if name in ("berlin52", "synth65_init"):  # a mutated best: its recomputed length is not 1 / fitness
        assert any(np.float32(1.0) / f != c for _b, f, c, _l in trace), name


# ---------------------------------------------------------------- past two compaction rounds, past one thread per individual
CUS, LDS_BYTES, WORK = K.CUS, K.LDS_BYTES, 8 << 30  # the device the sizes below were chosen for; the GPU tests read theirs from device_info
CROSS_SIZES = (511, 512, 513, 769, 1025, 4097)      # and tl_genetic_algorithm_max_n
WIDE = dict(n=520, epochs=2, p=0.5, e=3, seed=520)   # three compaction rounds per child on 256 threads
RANK = dict(n=1030, epochs=1, p=0.5, e=3, seed=1030)  # more individuals than the 1024 threads that rank them; the next generation has n - 3


def instance(n):
    return K.synth(n, 700 + n)


def crossover_segments(n):
    """(from, to) of the crossover self-test at n > 8: the wave-edge list the small sizes use, segments that start or end on the
    workgroup's widths and their neighbours, the whole route and single positions at both ends"""
    pairs = [(0, n - 1), (0, 0), (n - 1, n - 1), (0, 1), (n - 2, n - 1), (0, n - 2), (1, n - 1), (n // 2, n // 2), (1, n - 2), (62, 64), (63, 63), (0, 63)]
    for v in (255, 256, 257, 511, 512):
        pairs += [(v, n - 1), (0, v), (v, v), (v, v + 300), (v - 200, v), (1, v), (v, n - 2)]
    out = []
    for lo, hi in pairs:
        if 0 <= lo <= hi < n and (lo, hi) not in out:
            out.append((lo, hi))
    return out


def rounds(n, threads):
    """trips of the compaction loop (one per `threads` positions): the two sets of wave counts alternate, set 0 is used again in the third"""
    return -(-n // threads)
