"""Writes goldens_ga.json from tests/_ga_oracle.py: draw values, and best tours, costs (as f32 bit patterns), counters and a hash of
the per-generation trace of the cases in tests/_ga_cases.py.  Run from the repository root: python tests/golden/make_goldens_ga.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ga_cases as GC  # noqa: E402
import _ga_oracle as GA  # noqa: E402

OUT = os.path.join(HERE, "goldens_ga.json")

# (seed, run, event, slot)
DRAWS = [(0, 0, 0, 0), (1, 0, GA.pair_event(0, 52, 0, 0), 22), (1, 0, GA.pair_event(49, 52, 22, 2), 21), (1, 3, GA.init_event(52, 51, 51), 26),
         (2 ** 64 - 1, 2 ** 32 - 1, GA.pair_event(2 ** 32 - 1, 11000, 5496, 2), 25), (0x0123456789ABCDEF, 17, GA.init_event(1002, 7, 0), 27)]


def bits(f):
    return int(np.array([f], dtype=np.float32).view(np.uint32)[0])


def trace_words(trace):
    """the trace as the library writes it: 4 u32 per generation"""
    return np.array([[b, bits(f), bits(c), ln] for b, f, c, ln in trace], dtype=np.uint32).reshape(-1, 4)


def trace_hash(trace):
    return hashlib.sha256(trace_words(trace).astype("<u4").tobytes()).hexdigest()


def main():
    g = {"draws": [], "cases": {}}
    for seed, run, event, slot in DRAWS:
        g["draws"].append([str(seed), run, str(event), slot, str(GA.draw(seed, run, event, slot))])
    for name, (xy, packed, n, init, epochs, p, e, seed, run) in GC.golden_cases().items():
        tour, cost, trace, cnt = GA.solve(xy, packed, n, init, epochs=epochs, mutation_probability=p, n_elite=e, seed=seed, run=run)
        GC.check_conditions(name, n, epochs, trace, cnt)
        g["cases"][name] = {"tour": [int(v) for v in tour], "cost_bits": bits(cost), "counters": {k: int(v) for k, v in cnt.items()},
                            "trace_sha256": trace_hash(trace), "trace_head": trace_words(trace)[:8].tolist()}
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
