#!/usr/bin/env python3
"""Regenerates tests/golden/goldens_bhk.json: the Bellman-Held-Karp exact solver (bellman_karp.rs:24-165) on the instances whose
table is too slow to recompute inside a test, from the numpy restatement tests/_bhk_oracle.py:
  ulysses22   TSPLIB ulysses22 with its GEO matrix (k = 21);
  berlin23    the first 23 cities of berlin52, EUC_2D (k = 22; pass --no-berlin23 to leave it out).
Per instance: n, the optimum (f32 bits and 5 decimals) and, for the reference's tolerance walk and for the exact walk of
TL_FLAG_BHK_EXACT_WALK, the route (positions), its tour_length (bits and decimals) and whether it is a permutation.
The run prints its wall time per instance.

Usage: python tests/golden/make_goldens_bhk.py [--no-berlin23]
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import _bhk_oracle as B  # noqa: E402
import _oracle as O  # noqa: E402
import _tsplib as T  # noqa: E402


def walk_entry(w):
    route, cost, _, ok = w
    return {"route": [int(v) for v in route], "cost": f"{float(cost):.5f}", "cost_bits": int(np.float32(cost).view(np.uint32)), "is_tour": int(ok)}


def entry(xy, packed, n):
    ref, ex = B.both(xy, packed, n)
    return {"n": n, "optimal": f"{float(ref[2]):.5f}", "optimal_bits": int(np.float32(ref[2]).view(np.uint32)),
            "reference_walk": walk_entry(ref), "exact_walk": walk_entry(ex)}


def main():
    out = {}
    t0 = time.time()
    e = T.parse_tsplib(os.path.join(HERE, "tsplib", "ulysses22.tsp"))
    pk = e["packed"] if e["packed"] is not None else O.dm_build_packed(e["xy"], geo=True)
    out["ulysses22"] = entry(e["xy"], np.ascontiguousarray(pk, dtype=np.float32), e["n"])
    print(f"ulysses22: optimal {out['ulysses22']['optimal']}, {time.time() - t0:.1f} s", flush=True)
    if "--no-berlin23" not in sys.argv:
        t0 = time.time()
        xy = T.parse_tsplib(os.path.join(HERE, "tsplib", "berlin52.tsp"))["xy"][:23]
        out["berlin23"] = entry(xy, None, 23)
        print(f"berlin23: optimal {out['berlin23']['optimal']} / {out['berlin23']['reference_walk']['cost']}, {time.time() - t0:.1f} s", flush=True)
    with open(os.path.join(HERE, "goldens_bhk.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
