"""Writes goldens_gsa.json from tests/_gsa_oracle.py: draw values, g, pull lengths, masses with their ranking, and best tours, costs,
counters, the improvement log and a hash of the per-epoch record of the cases in tests/_gsa_cases.py.  The goldens are this
project's oracle output: nothing of the reference's can be frozen, its RNG is unseeded.
Run from the repository root: python tests/golden/make_goldens_gsa.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _gsa_cases as GC  # noqa: E402
import _gsa_oracle as GO  # noqa: E402

OUT = os.path.join(HERE, "goldens_gsa.json")

# (seed, run, event, slot)
DRAWS = [(0, 0, 0, 0), (1, 0, GO.event(0, 25, 1, 2), 0), (1, 0, GO.event(9999, 25, 24, 23), 0), (1, 3, GO.init_event(52, 24, 51), 26),
         (2 ** 64 - 1, 2 ** 32 - 1, GO.event(2 ** 32 - 2, 4096, 4095, 4094), 0), (0x0123456789ABCDEF, 17, GO.event(7, 65, 64, 3), 0)]
G_OF = [(0, 0), (0, 1), (0, 10000), (1, 10000), (9999, 10000), (3, 8), (7, 8), (2 ** 32 - 2, 2 ** 32 - 2)]
PULLS = [(0.0, 20.0, 1.0), (0.5, 20.0, 0.05), (0.4999999, 20.0, 0.05), (0.999999, 20.0, 1.0), (0.3, 7.357588823428847, 0.2), (0.125, 20.0, 1.0), (0.9, 12.0, 0.04)]
COSTS = [[10.0, 9.0, 8.0, 7.0, 6.0], [5.0] * 6, [3.0, 1.0, 3.0, 1.0, 2.0, 2.0, 2.0], [1.0, 1.0 + 2.0 ** -23, 1.0]]


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "g": [], "pulls": [], "masses": [], "cases": {}}
    for seed, run, event, slot in DRAWS:
        g["draws"].append([str(seed), run, str(event), slot, str(GO.draw(seed, run, event, slot))])
    for e, total in G_OF:
        g["g"].append([e, total, str(GO.f64_bits(GO.g_of(e, total)))])
    for r, gg, m in PULLS:
        g["pulls"].append([r, gg, m, GO.pull_swaps(r, gg, m)])
    for costs in COSTS:
        m, rank, _u = GO.masses_of(costs)
        g["masses"].append([costs, [str(GO.f64_bits(x)) for x in m], rank])
    for name, (xy, packed, n, init, o) in GC.golden_cases().items():
        res = GO.solve(xy, packed, n, init, **o)
        GC.check_conditions(name, n, res, o)
        g["cases"][name] = {"tour": [int(v) for v in res["tour"]], "cost_bits": GO.bits(res["cost"]), "counters": {k: int(v) for k, v in res["counters"].items()},
                            "log": GO.log_words(res).tolist(), "routes_sha256": sha(GO.route_words(res, n)), "epochs_sha256": sha(GO.epoch_words(res)),
                            "epochs_head": GO.epoch_words(res)[:1].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
