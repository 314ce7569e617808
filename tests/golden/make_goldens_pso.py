"""Writes goldens_pso.json from tests/_pso_oracle.py: draw values, rounding and weight vectors, and best tours, costs, counters, the
improvement log and a hash of the per-epoch record of the cases in tests/_pso_cases.py.  The goldens are this project's oracle
output: nothing of the reference's can be frozen, its RNG is unseeded.
Run from the repository root: python tests/golden/make_goldens_pso.py"""
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _pso_cases as PC  # noqa: E402
import _pso_oracle as PO  # noqa: E402

OUT = os.path.join(HERE, "goldens_pso.json")

# (seed, run, event, slot)
DRAWS = [(0, 0, 0, 0), (1, 0, PO.step_event(0, 30, 1), 1), (1, 0, PO.step_event(9999, 30, 29), 0), (1, 3, PO.init_event(52, 29, 51), 26),
         (2 ** 64 - 1, 2 ** 32 - 1, PO.step_event(2 ** 32 - 2, 4096, 4095), 1), (0x0123456789ABCDEF, 17, PO.init_event(1002, 64, 1), 26)]
KEEPS = [0.0, 0.49999999999999994, 0.5, 1.4999999999999998, 1.5, 2.5, 4.5, 0.9 * 5, 0.65 * 10, 1.5 * 0.9999999999999999 * 7, 17.0, 1e9 + 0.5, -0.5]
WEIGHTS = [(0, 0), (0, 1), (0, 10000), (9999, 10000), (1, 3), (2, 3), (7, 8), (39, 40)]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "keeps": [], "weights": [], "cases": {}}
    for seed, run, event, slot in DRAWS:
        g["draws"].append([str(seed), run, str(event), slot, str(PO.draw(seed, run, event, slot))])
    for x in KEEPS:
        g["keeps"].append([str(f64_bits(x)), PO.keep(x)])
    for e, of in WEIGHTS:
        g["weights"].append([e, of, str(f64_bits(PO.weight(e, of)))])
    for name, (xy, packed, n, init, o) in PC.golden_cases().items():
        res = PO.solve(xy, packed, n, init, **o)
        PC.check_conditions(name, n, res, o)
        g["cases"][name] = {"tour": [int(v) for v in res["tour"]], "cost_bits": PO.bits(res["cost"]), "counters": {k: int(v) for k, v in res["counters"].items()},
                            "log": PO.log_words(res).tolist(), "routes_sha256": sha(PO.route_words(res, n)), "epochs_sha256": sha(PO.epoch_words(res)),
                            "epochs_head": PO.epoch_words(res)[:1].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
