#!/usr/bin/env python3
"""Regenerates tests/golden/goldens_christofides.json: Christofides construction (christofides.rs:12-241) on the synthetic
instances n = 10 000 and n = 13 509 (_oracle.synth_xy(n), the inputs of the greedy-edge and savings goldens) and n = 30 000
(beyond the size whose tree state fits one workgroup's LDS), from the numpy
restatement tests/_christofides_oracle.py: the cost (f32 bits and 5 decimals), the SHA-256 of the route (u32 little-endian
positions), the number of odd-degree vertices of the tree, and how many pairs of the sorted list the matching examines before its
last pair (reference_examined: the literal walk's count).  The packed matrix of n = 30 000 needs 1.8 GB and the whole run about a minute.

Usage: python tests/golden/make_goldens_christofides.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import _christofides_oracle as X  # noqa: E402
import _oracle as O  # noqa: E402


def main():
    out = {}
    for n in (10000, 13509, 30000):
        t0 = time.time()
        xy = O.synth_xy(n)
        route, cost, st = X.christofides(xy, with_stats=True)
        out[f"synthetic{n}"] = {"n": n, "seed": 0, "cost": f"{float(cost):.5f}", "cost_bits": int(np.float32(cost).view(np.uint32)),
                                "route_sha256": X.route_sha256(route), "odd_vertices": int(st["k"]),
                                "reference_examined": int(st["examined"])}
        print(f"n={n}: cost {float(cost):.5f}, k {st['k']}, examined {st['examined']}, {time.time() - t0:.1f} s", flush=True)
    with open(os.path.join(HERE, "goldens_christofides.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
