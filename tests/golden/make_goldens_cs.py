"""Writes goldens_cs.json from tests/_cs_oracle.py: draw values, Lévy steps on word tuples (edge words included) with their flight
lengths, and best tours, costs, counters, the improvement log and a hash of the per-epoch record of the cases in tests/_cs_cases.py.
The goldens are this project's oracle output: nothing of the reference's can be frozen, its RNG is unseeded.
Run from the repository root: python tests/golden/make_goldens_cs.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _cs_cases as CC  # noqa: E402
import _cs_oracle as CO  # noqa: E402

OUT = os.path.join(HERE, "goldens_cs.json")

# (seed, run, event, slot)
DRAWS = [(0, 0, 0, 0), (1, 0, CO.base(0, 25, 1, 52), 12), (1, 0, CO.base(9999, 25, 24, 52) + 26, 1), (1, 3, CO.init_event(52, 24, 51), 26),
         (2 ** 64 - 1, 2 ** 32 - 1, CO.base(2 ** 32 - 2, 4096, 4095, 16000) + 16000, 2), (0x0123456789ABCDEF, 17, CO.base(7, 65, 64, 1002), 13)]


def edge_words():
    """u1 = 0 (the floor), u1 = 1 - 2^-53 (v tiny), u2 = 1/4 and 3/4 (v exactly zero: one resample, all four, the value after the last)"""
    top, q1, q3, mid = CO.word_of_uniform(2 ** 53 - 1), CO.word_of_uniform(2 ** 51), CO.word_of_uniform(3 * 2 ** 51), CO.word_of_uniform(12345678901234)
    ok = [mid, CO.word_of_uniform(2 ** 50)]  # a pair whose normal is not zero
    rows = [[0, mid, mid, mid] + ok * 4,
            [mid, mid, top, mid] + ok * 4,
            [mid, mid, mid, q1] + ok * 4,
            [mid, mid, mid, q3] + [mid, q1] + ok * 3,
            [mid, mid, mid, q1] + [mid, q3] * 3 + ok,
            [mid, mid, mid, q1] + [mid, q3] * 4,
            [0, 0, 0, 0] + [0] * 8,
            [mid, q1, mid, mid] + ok * 4]
    return np.asarray(rows, dtype=np.uint64)


def sha(words):
    return hashlib.sha256(np.asarray(words, dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "levy": [], "cases": {}}
    for seed, run, event, slot in DRAWS:
        g["draws"].append([str(seed), run, str(event), slot, str(CO.draw(seed, run, event, slot))])
    rng = np.random.default_rng(20)
    words = np.concatenate([edge_words(), rng.integers(0, 2 ** 64, size=(24, CO.WORDS), dtype=np.uint64)])
    steps, tries = CO.levy_spec(words)
    for w, v, t in zip(words, steps, tries):
        g["levy"].append([[str(int(x)) for x in w], str(CO.f64_bits(v)), int(t), [CO.flight_length(abs(float(v)), n) for n in (2, 3, 52, 280, 1002)]])
    for name, (xy, packed, n, init, o) in CC.golden_cases().items():
        res = CO.solve(xy, packed, n, init, **o)
        CC.check_conditions(name, n, res, o)
        g["cases"][name] = {"tour": [int(v) for v in res["tour"]], "cost_bits": CO.bits(res["cost"]), "counters": {k: int(v) for k, v in res["counters"].items()},
                            "log": CO.log_words(res).tolist(), "routes_sha256": sha(CO.route_words(res, n)), "epochs_sha256": sha(CO.epoch_words(res)),
                            "epochs_head": CO.epoch_words(res)[:1].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
