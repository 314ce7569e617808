"""Writes goldens_fourier.json from tests/_fourier_oracle.py: basis tables, start coefficients, and the tour, cost, final coefficients,
final sample indices and hashes of the logged sample indices and stage-end coefficients of the cases named in tests/_fourier_cases.py
(GOLDEN).  The goldens are this project's oracle output: the reference itself was never run (no Rust toolchain where this was made).
Run from the repository root: python tests/golden/make_goldens_fourier.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _fourier_cases as FC  # noqa: E402
import _fourier_oracle as FO  # noqa: E402

OUT = os.path.join(HERE, "goldens_fourier.json")
BASIS = [2, 3, 7, 50]
INIT = [("n2", 1), ("circle5", 2), ("berlin52", 4)]


def main():
    g = {"basis": [], "init": [], "cases": {}}
    cases = FC.cases()
    for m in BASIS:
        g["basis"].append([m, [str(int(v)) for v in FO.f64_words(FO.basis_table(m))]])
    for name, k_max in INIT:
        g["init"].append([name, k_max, [str(int(v)) for v in FO.f64_words(FO.init_coefficients(cases[name][0], k_max))]])
    for name in FC.GOLDEN:
        g["cases"][name] = FC.case_record(FC.oracle(name))
    with open(OUT, "w") as fh:
        json.dump(g, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
