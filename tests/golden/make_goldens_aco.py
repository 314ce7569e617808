"""Writes goldens_aco.json from tests/_aco_oracle.py: draw values, aco_pow vectors (as f32 bit patterns), and best tours, costs,
counters and a hash of the per-epoch trace and of the route log of the cases in tests/_aco_cases.py.
Run from the repository root: python tests/golden/make_goldens_aco.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _aco_cases as AC  # noqa: E402
import _aco_oracle as ACO  # noqa: E402

OUT = os.path.join(HERE, "goldens_aco.json")

# (seed, run, event, slot)
DRAWS = [(0, 0, 0, 0), (1, 0, ACO.event(0, 25, 0, 52, 1), 1), (1, 0, ACO.event(149, 25, 24, 52, 51), 2), (1, 3, ACO.shuffle_event(51), 26),
         (2 ** 64 - 1, 2 ** 32 - 1, ACO.event(2 ** 32 - 1, 4096, 4095, 10000, 9999), 2), (0x0123456789ABCDEF, 17, ACO.event(7, 64, 63, 1002, 0), 0)]
# (x, a)
POWS = [(0.0, 0.0), (0.0, 1.5), (float("inf"), 0.5), (3.0, 1.0), (3.0, 2.0), (1e-3, 20.0), (1e6, 6.0), (1e6, 6.5), (2.0, 0.5), (0.5, 0.5), (1.4142135, 3.3),
         (0.70710677, 3.3), (1e-30, 1.5), (1e-40, 0.5), (123.456, 2.5), (1.0, 5.9), (0.99999994, 6.0), (1.0000001, 6.0), (7.5e-4, 1.3), (1e-6, 6.0)]


def bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "pow": [], "cases": {}}
    for seed, run, event, slot in DRAWS:
        g["draws"].append([str(seed), run, str(event), slot, str(ACO.draw(seed, run, event, slot))])
    for x, a in POWS:
        g["pow"].append([bits(x), bits(a), bits(ACO.pow_scalar(x, a))])
    for name, (xy, packed, n, init, o) in AC.golden_cases().items():
        res = ACO.solve(xy, packed, n, init, **o)
        AC.check_conditions(name, n, res, o)
        g["cases"][name] = {"tour": [int(v) for v in res["tour"]], "cost_bits": bits(res["cost"]), "counters": {k: int(v) for k, v in res["counters"].items()},
                            "log_sha256": sha(ACO.log_words(res, o["num_ants"])), "routes_sha256": sha(ACO.route_words(res, n)),
                            "log_head": ACO.log_words(res, o["num_ants"])[:2].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
