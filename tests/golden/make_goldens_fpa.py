"""Writes goldens_fpa.json from tests/_fpa_oracle.py: draw values, partners, prefix lengths, and best tours, costs, counters, the
improvement log and a hash of the per-epoch record of the cases in tests/_fpa_cases.py.  The goldens are this project's oracle
output: nothing of the reference's can be frozen, its RNG is unseeded.
Run from the repository root: python tests/golden/make_goldens_fpa.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _fpa_cases as FC  # noqa: E402
import _fpa_oracle as FO  # noqa: E402

OUT = os.path.join(HERE, "goldens_fpa.json")

# (seed, run, event, slot)
DRAWS = [(0, 0, 0, 0), (1, 0, FO.event(0, 25, 1), 13), (1, 0, FO.event(9999, 25, 24), 15), (1, 3, FO.init_event(52, 24, 51), 26),
         (2 ** 64 - 1, 2 ** 32 - 1, FO.event(2 ** 32 - 2, 4096, 4095), 14), (0x0123456789ABCDEF, 17, FO.event(7, 65, 64), 12)]
LENGTHS = [(0.0, 7), (0.25, 8), (0.2500000001, 8), (1.0, 8), (2.0, 7), (1e300, 7), (0.3, 0), (0.999999, 1)]


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "partners": [], "lengths": [], "cases": {}}
    for seed, run, event, slot in DRAWS:
        g["draws"].append([str(seed), run, str(event), slot, str(FO.draw(seed, run, event, slot))])
    key = FO.chain_key(77, 5)
    for N in (25, 26, 64):
        g["partners"].append([N, [list(FO.partners(key, FO.event(3, N, i), i, N)) for i in range(N)]])
    for x, ln in LENGTHS:
        g["lengths"].append([x, ln, FO.global_swaps(x, ln), FO.local_swaps(x, ln)])
    for name, (xy, packed, n, init, o) in FC.golden_cases().items():
        res = FO.solve(xy, packed, n, init, **o)
        FC.check_conditions(name, n, res, o)
        g["cases"][name] = {"tour": [int(v) for v in res["tour"]], "cost_bits": FO.bits(res["cost"]), "counters": {k: int(v) for k, v in res["counters"].items()},
                            "log": FO.log_words(res).tolist(), "routes_sha256": sha(FO.route_words(res, n)), "epochs_sha256": sha(FO.epoch_words(res)),
                            "epochs_head": FO.epoch_words(res)[:1].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
