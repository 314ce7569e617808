"""Writes tests/golden/goldens_one_tree.json from the oracle (tests/_one_tree_oracle.py): per instance the ascent's figures with
every f64 as its hexadecimal text, so the file compares bit for bit.  upper is the nearest-neighbour tour's f64 length from
position 0 (tests/_one_tree_cases.py nn_upper); berlin52 runs to the tour it proves, the others 60 iterations."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, "goldens_one_tree.json")
CASES = {"berlin52": dict(iterations=1000), "burma14": dict(iterations=60), "gr17": dict(iterations=60), "a280": dict(iterations=60)}


def record(res, upper):
    """What the file keeps of a result (the oracle's dict or the C ABI's, tests/_one_tree_cases.py)."""
    return {
        "upper": float(upper), "bound": float(res["bound"]).hex(), "best_iter": int(res["best_iter"]), "iterations_run": int(res["iterations_run"]),
        "stop": int(res["stop"]), "is_tour": int(res["is_tour"]), "tour": res["tour"], "root_nb": [int(v) for v in res["root_nb"]],
        "pi": [float(v).hex() for v in res["pi"]], "parent_crc32": int(zlib.crc32(np.asarray(res["parent"], dtype="<u4").tobytes())),
        "log": [[float(v).hex() for v in row] for row in res["log"]],
    }


def main():
    import _one_tree_cases as K
    import _one_tree_oracle as H
    rows = {}
    for name, kw in CASES.items():
        xy, pk, n = K.tsp(name)
        upper = K.nn_upper(xy, pk, n)
        rows[name] = record(H.ascent(xy, pk, n, upper=upper, **kw), upper)
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(rows)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
