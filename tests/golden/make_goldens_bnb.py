"""Writes tests/golden/goldens_bnb.json from the sequential restatement on the CPU (tl_branch_and_bound_host): per larger case of
tests/_bnb_cases.py the expected route, the bits of its length, whether the seed was improved, and the restatement's node and leaf
counts (every case must be proved within 300 000 nodes — gr17, a CPU-only case, within 1 000 000)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _bnb_cases as K  # noqa: E402
import _bnb_oracle as B  # noqa: E402

OUT = os.path.join(HERE, "goldens_bnb.json")


def main():
    rows = {}
    for name, (xy, pk, n, k, start, seeded) in K.large_cases().items():
        init = K.seed_tour(xy, pk, n, start) if seeded else None
        rc, route, cost, proved, improved, st = K.call(None, xy, pk, n, init=init, start=start, K=k)
        assert rc == 0 and proved == 1 and st["nodes"] <= (1_000_000 if name == "gr17" else 300_000), (name, rc, proved, st)
        rows[name] = {"n": n, "K": k, "start": start, "seeded": seeded, "route": route, "bits": B.bits(cost), "improved": improved,
                      "nodes": st["nodes"], "leaves": st["leaves"]}
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(rows)} cases")


if __name__ == "__main__":
    main()
