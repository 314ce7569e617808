"""Writes goldens_tabu.json from tests/_tabu_oracle.py: draw values, and best tours, costs (as f32 bit patterns), counters and a hash
of the per-epoch log of the cases in tests/_tabu_cases.py.  Run from the repository root: python tests/golden/make_goldens_tabu.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _tabu_cases as TC  # noqa: E402
import _tabu_oracle as TO  # noqa: E402

OUT = os.path.join(HERE, "goldens_tabu.json")

DRAWS = [(0, 0, 2, 0, 0, 0), (1, 0, 52, 0, 0, 0), (1, 0, 52, 0, 52, 21), (1, 3, 52, 10000, 52, 21), (2 ** 64 - 1, 2 ** 32 - 1, 13650, 2 ** 32 - 2, 13650, 31),
         (0x0123456789ABCDEF, 17, 1002, 99, 640, 5)]


def bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def log_words(log):
    """the log as the library writes it: 4 u32 per epoch"""
    return np.array([[a, f, t, bits(c)] for a, f, t, c in log], dtype=np.uint32).reshape(-1, 4)


def log_hash(log):
    return hashlib.sha256(log_words(log).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "cases": {}}
    for seed, chain, n, epoch, attempt, slot in DRAWS:
        g["draws"].append([str(seed), chain, n, epoch, attempt, slot, str(TO.draw(seed, chain, n, epoch, attempt, slot))])
    for name, (xy, packed, n, init, epochs, seed, chain) in TC.golden_cases().items():
        tour, cost, log, cnt = TO.solve(xy, packed, n, init, epochs=epochs, seed=seed, chain=chain)
        TC.check_conditions(name, n, epochs, log, cnt)
        g["cases"][name] = {"tour": [int(v) for v in tour], "cost_bits": bits(cost), "counters": cnt, "log_sha256": log_hash(log),
                            "log_head": log_words(log)[:8].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
