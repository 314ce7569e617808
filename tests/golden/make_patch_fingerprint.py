#!/usr/bin/env python3
"""Regenerates tests/golden/reference_patch_targets.json: what integration/patches/0001-gpu-feature.patch needs of the reference
tree it was cut against, as SHA-256 digests (no source text).  Per file the patch changes: the digest of the whole file, its line
count, and per hunk [first line, line count, digest of those lines] at the line numbers the hunk names; null for a file the patch
creates.  tests/test_abi.py::test_reference_patch_applies_cleanly checks the patch against these digests, so it needs no checkout.

Usage: python tests/golden/make_patch_fingerprint.py PATH-TO-A-TEELINE-CHECKOUT     (after the patch was cut anew)
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATCH = os.path.join(ROOT, "integration", "patches", "0001-gpu-feature.patch")
OUT = os.path.join(HERE, "reference_patch_targets.json")


def sha(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()


def parse(text):
    """{path (-p1): [(old first line, old line count, old lines with their newlines)]} of a unified diff."""
    files, lines, k = {}, text.splitlines(keepends=True), 0
    while k < len(lines):
        ln = lines[k]
        if ln.startswith("+++ "):
            hunks = files.setdefault(ln[4:].split("\t")[0].strip().split("/", 1)[1], [])
        elif ln.startswith("@@ "):
            m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,(\d+))? @@", ln)
            start, left_old, left_new = int(m[1]), int(m[2] or 1), int(m[3] or 1)
            old = []
            while left_old or left_new:
                k += 1
                b = " \n" if lines[k] == "\n" else lines[k]
                if b.startswith("\\"):  # "\ No newline at end of file"
                    continue
                if b[0] in " -":
                    old.append(b[1:])
                    left_old -= 1
                if b[0] in " +":
                    left_new -= 1
            hunks.append((start, len(old), old))
        k += 1
    return files


def fingerprint(ref):
    out = {}
    for path, hunks in parse(open(PATCH).read()).items():
        f = os.path.join(ref, path)
        if all(s == 0 and n == 0 for s, n, _ in hunks):
            assert not os.path.exists(f), f"{f}: the patch creates this file, but the checkout has it"
            out[path] = None
            continue
        src = open(f, newline="").read().splitlines(keepends=True)
        out[path] = {"sha256": sha(src), "lines": len(src), "hunks": [[s, n, sha(src[s - 1:s - 1 + n])] for s, n, _ in hunks]}
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src", "tsp")):
        raise SystemExit(__doc__)
    with open(OUT, "w") as fh:
        json.dump(fingerprint(sys.argv[1]), fh, indent=1)
        fh.write("\n")
    print(f"wrote {OUT}")
