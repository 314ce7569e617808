"""Writes goldens_sa.json from tests/_sa_oracle.py: draw values, schedule lengths, and final tours, costs (as f32 bit patterns) and
accepted epochs of the cases in tests/_sa_cases.py.  Run from the repository root: python tests/golden/make_goldens_sa.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _sa_cases as K  # noqa: E402
import _sa_oracle as SA  # noqa: E402

OUT = os.path.join(HERE, "goldens_sa.json")


def bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def main():
    g = {"draws": [], "schedules": [], "cases": {}}
    for seed, chain, epoch, slot in [(0, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 22), (1, 3, 138148, 21), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 31),
                                     (0x0123456789ABCDEF, 17, 99, 5)]:
        g["draws"].append([str(seed), chain, epoch, slot, str(SA.draw(seed, chain, epoch, slot))])
    for o in (SA.DEFAULTS, K.HOT, K.COLD, K.SHORT, K.EMPTY, K.with_epochs(1), K.with_epochs(65),
              dict(epochs=200_000, cooling_rate=1e-4, min_temperature=1e-3, max_temperature=1000.0)):
        g["schedules"].append([o, len(SA.schedule(**o))])
    for name, (xy, packed, n, init, opts, seed, chain) in K.golden_cases().items():
        tour, cost, trace = SA.solve(xy, packed, n, init, seed=seed, chain=chain, **opts)
        g["cases"][name] = {"tour": [int(v) for v in tour], "cost_bits": bits(cost),
                            "trace": [[int(e), int(f), int(t), bits(c)] for e, f, t, c in trace]}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
