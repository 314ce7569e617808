#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 device code of two built libraries (or objects).

For each file: the gfx950 code objects are extracted (llvm-objdump --offloading, as build.verify_ds_min_waits does) and
disassembled; addresses and encodings are stripped; then every kernel's instruction sequence is compared.  Prints, per kernel,
"identical" or the first differing instruction and the count of differing lines, and the kernel descriptors' resource notes
(VGPRs, SGPRs, spills, scratch, static LDS) where they differ.  Exit status 1 if anything differs.

usage: python scripts/isa_diff.py OLD.so NEW.so
"""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
NOTE_KEYS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size", ".agpr_count")


def kernels_of(lib):
    """{kernel symbol: [instruction text]}, {kernel symbol: {note key: value}} over every gfx950 code object of `lib`."""
    code, notes = {}, {}
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        local = os.path.join(tmp, "lib")
        shutil.copy(lib, local)
        subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=tmp)
        for name in sorted(os.listdir(tmp)):
            if "gfx950" not in name:
                continue
            co = os.path.join(tmp, name)
            cur = None
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True).splitlines():
                m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
                if m:
                    if m.group(1) in code:
                        raise RuntimeError(f"{lib}: symbol {m.group(1)} in more than one gfx950 code object")
                    cur = code[m.group(1)] = []
                elif cur is not None and line.startswith(("\t", " ")) and line.strip():
                    cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())  # the text in front of "// address: encoding"
            # the metadata note is YAML: a kernel is one item of the `amdhsa.kernels` list ("  - .key: value", then "    .key: value");
            # its `.name` comes in the middle of the item, and deeper-indented lines (`.args` entries) are not the kernel's own
            entry, in_kernels = None, False
            entries = []
            for line in subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True).splitlines():
                if re.match(r"^\S", line):
                    in_kernels = line.startswith("amdhsa.kernels:")
                    continue
                if not in_kernels:
                    continue
                m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)
                if not m:
                    continue
                if m.group(1) == "- ":
                    entry = {}
                    entries.append(entry)
                if entry is not None:
                    entry[m.group(2)] = m.group(3).strip()
            for entry in entries:
                name = entry.get(".name")
                if name in notes:
                    raise RuntimeError(f"{lib}: kernel {name} in more than one gfx950 code object")
                notes[name] = {k: entry.get(k) for k in NOTE_KEYS}
    return code, notes


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (ca, na), (cb, nb) = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    differs = 0
    for k in sorted(set(ca) | set(cb)):
        if k not in ca or k not in cb:
            print(f"{k}: only in {'the first' if k in ca else 'the second'}")
            differs += 1
            continue
        a, b = ca[k], cb[k]
        if a == b:
            print(f"{k}: identical ({len(a)} instructions)")
            continue
        differs += 1
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        n = sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
        print(f"{k}: DIFFERS in {n} lines ({len(a)} -> {len(b)} instructions); first at #{first}: {a[first] if first < len(a) else '<end>'}  |  {b[first] if first < len(b) else '<end>'}")
    for k in sorted(set(ca) & set(cb)):  # (a kernel on one side only is reported above)
        if k not in na and k not in nb:
            continue  # a device function, not a kernel: no descriptor
        if na.get(k) != nb.get(k):
            differs += 1
            print(f"{k}: descriptor {na.get(k, 'missing')} -> {nb.get(k, 'missing')}")
    print("all kernels identical" if not differs else f"{differs} differences")
    sys.exit(1 if differs else 0)


if __name__ == "__main__":
    main()
