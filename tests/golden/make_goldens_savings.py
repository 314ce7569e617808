#!/usr/bin/env python3
"""Regenerates tests/golden/goldens_savings.json: savings construction (savings.rs:34-163) on the synthetic instances
n = 10 000 and n = 13 509 (_oracle.synth_xy(n)), from the numpy restatement tests/_savings_oracle.py: the hub, the cost (f32 bits
and 5 decimals), the SHA-256 of the route (u32 little-endian positions) and how many edges of the sorted list the selection
examines before its n-th edge (reference_examined: the literal walk's count — nearly all of them, hub pairs sort last).
The sorted list of all n(n-1)/2 edges needs a few GB of RAM and minutes.

Usage: python tests/golden/make_goldens_savings.py
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import _oracle as O  # noqa: E402
import _savings_oracle as S  # noqa: E402


def main():
    out = {}
    for n in (10000, 13509):
        t0 = time.time()
        xy = O.synth_xy(n)
        route, cost, hub, st = S.savings(xy, chunk=1 << 16, with_stats=True)
        out[f"synthetic{n}"] = {"n": n, "seed": 0, "hub": int(hub), "cost": f"{float(cost):.5f}",
                                "cost_bits": int(np.float32(cost).view(np.uint32)), "route_sha256": S.route_sha256(route),
                                "reference_examined": int(st["examined"])}
        print(f"n={n}: hub {hub}, cost {float(cost):.5f}, examined {st['examined']}, {time.time() - t0:.1f} s", flush=True)
    with open(os.path.join(HERE, "goldens_savings.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
