"""Writes goldens_som.json from tests/_som_oracle.py: city draws, schedules, h values, small start rings, and the tour, cost, hashes of
the (city, bmu) log and of the final ring, and the checkpoint records of the cases named in tests/_som_cases.py (GOLDEN).  The goldens
are this project's oracle output: nothing of the reference's can be frozen, its RNG is unseeded and its exp is libm's.
Run from the repository root: python tests/golden/make_goldens_som.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _som_cases as SC  # noqa: E402
import _som_oracle as SO  # noqa: E402

OUT = os.path.join(HERE, "goldens_som.json")

# (seed, run, epoch, n)
DRAWS = [(0, 0, 1, 2), (1, 0, 1, 52), (1, 0, 100_000, 52), (1, 3, 7, 1002), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 2, 65536), (0x0123456789ABCDEF, 17, 9, 13)]
# (epoch, epochs, M, learning_rate, radius_fraction)
SCHEDULES = [(1, 1, 2, 0.8, 0.1), (1, 100_000, 416, 0.8, 0.1), (50_000, 100_000, 416, 0.8, 0.1), (100_000, 100_000, 8016, 0.8, 0.1), (7, 25, 20, 0.8, 0.1),
             (18, 25, 20, 0.8, 0.1), (3, 11, 21, 1.0, 1.0), (1, 10, 65536, 0.5, 1.0)]
# (d, two_sigma_sq): both sides of y = -8 and of h = 1e-3
H_OF = [(0.0, 2.0), (3.0, 2.0), (4.0, 2.0), (5.0, 2.0), (3.7, 2.0), (3.8, 2.0), (np.nextafter(4.0, 5.0), 2.0), (100_000.0, 2.0), (41.0, 3461.12), (166.0, 3461.12),
         (167.0, 3461.12)]
RINGS = [1, 2, 3, 4, 7, 12]


def main():
    g = {"draws": [], "schedules": [], "h": [], "rings": [], "cases": {}}
    for seed, run, t, n in DRAWS:
        g["draws"].append([str(seed), run, t, n, SO.city_of(SO.chain_key(seed, run), t, n)])
    for t, epochs, M, lr, rf in SCHEDULES:
        eta, sigma, tss, radius = SO.schedule(t, epochs, M, lr, rf)
        g["schedules"].append([t, epochs, M, lr, rf, str(SO.f64_bits(eta)), str(SO.f64_bits(sigma)), str(SO.f64_bits(tss)), radius])
    for d, tss in H_OF:
        ok, h = SO.h_of(d, tss)
        g["h"].append([str(SO.f64_bits(d)), tss, int(ok), str(SO.f64_bits(h))])
    for M in RINGS:
        g["rings"].append([M, [str(SO.f64_bits(v)) for v in SO.ring_init(0.5, 0.25, M).T.reshape(-1)]])
    cases = SC.cases()
    for name in SC.GOLDEN:
        xy, packed, n, o, want = cases[name]
        res = SO.solve(xy, packed, n, **o)
        SC.check_conditions(name, res, o, want)
        g["cases"][name] = SC.case_record(res)
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
