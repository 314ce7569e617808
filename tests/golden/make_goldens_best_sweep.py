#!/usr/bin/env python3
"""Regenerates tests/golden/goldens_best_sweep.json: the oracle's result of the one TL_MODE_BEST_SWEEP case whose oracle run is too slow
for the suite.

  snake65535_best_sweep   the 255 x 257 unit-lattice snake (n = 65 535, the largest size the packed (i, j) key takes; shuffled city ids)
                          with four ranges reversed (tests/_best_sweep_cases.py GOLDEN_CASE), best-improvement 2-opt: cost bits, CRC-32
                          of the final tour (u32 little-endian positions) and of the initial tour, sweeps / candidates / moves / reversed
                          — the fields of lattice257_two_opt in goldens_limits.json — and the winning moves, in order.

The moves come from model_best_sweep (the kernel's scheme restated in numpy), whose tour, cost and counters must equal the oracle's
here.  The script then checks what the case is for: a winning move with i >= 32768, one with i < 32768 <= j, one with j = n-2 and one
with i = n-4, and that a decode of the packed key that masks i or j with 0x7FFF (model defects i and j) gives another move.

tests/test_gpu_best_sweep.py builds the same start (checked against init_crc32) and compares the HIP result with these values.
Usage: python tests/golden/make_goldens_best_sweep.py      (measured: 197 s of one core for the oracle, 7 s for one run of the model, 3 min 47 s in all)
"""
import json
import os
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402

import _best_sweep_cases as B  # noqa: E402


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a, dtype="<u4").tobytes()))


def main():
    case = B.GOLDEN_CASE
    xy, init = case.build()
    n = len(init)
    assert n == 65535 == B.MAX_N
    t = time.time()
    o = B.oracle_best_sweep(xy, init)  # O.two_opt(best=True), once
    t_oracle = time.time() - t
    t = time.time()
    m = B.model_best_sweep(xy, init)
    t_model = time.time() - t
    assert B.same_result(m, o), "the model disagrees with the oracle: the model is wrong"
    moves = [[int(i), int(j)] for i, j in m["move_list"]]
    assert any(i >= 32768 for i, j in moves) and any(i < 32768 <= j for i, j in moves)
    assert any(j == n - 2 for i, j in moves) and any(i == n - 4 for i, j in moves)
    assert any((i & 0x7FFF) != i for i, j in moves) and any((j & 0x7FFF) != j for i, j in moves)
    for d in ("i", "j"):  # the masked decode, applied at the first move it changes: another tour, or no candidate at all
        assert not B.same_result(B.model_best_sweep(xy, init, defect=d, max_sweeps=o["sweeps"] + 1), o), d
    out = {"snake65535_best_sweep": {"n": n, "init_crc32": crc(init), "route_crc32": crc(o["tour"]), "cost_bits": o["cost_bits"],
                                     "cost": f"{float(np.uint32(o['cost_bits']).view(np.float32)):.5f}",
                                     "stats": {k: o[k] for k in ("sweeps", "candidates", "moves", "reversed")}, "moves": moves}}
    with open(os.path.join(HERE, "goldens_best_sweep.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(out, f"oracle {t_oracle:.0f} s, model {t_model:.0f} s")


if __name__ == "__main__":
    main()
