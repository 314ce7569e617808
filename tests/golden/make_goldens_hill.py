"""Writes tests/golden/goldens_hill.json from the oracle (tests/_hill_oracle.py) and the cases (tests/_hill_cases.py): draw values,
best tours, cost bits, counters, the event log's sha256 and its head.  Run from the repository root:
    python tests/golden/make_goldens_hill.py
Every case's conditions are asserted first, so no golden is frozen of a chain that misses what it is there for."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _hill_cases as HC  # noqa: E402
import _hill_oracle as HO  # noqa: E402


def main():
    cases = HC.cases()
    out = {"draws": [[str(s), c, str(ev), sl, str(HO.draw(s, c, ev, sl))] for s, c, ev, sl in HC.golden_draws()], "cases": {}}
    for name in sorted(cases):
        HC.check_conditions(name, cases[name])
        out["cases"][name] = HC.case_record(HC.run(name, cases[name]))
    with open(os.path.join(HERE, "goldens_hill.json"), "w") as fh:
        json.dump(out, fh, sort_keys=True, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
