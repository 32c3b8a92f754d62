#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc ... --cuda-device-only -S) kernel by kernel.

    python tools/isa_diff.py before.s after.s

Each file is split per kernel symbol; comments, .loc / .file / .cfi lines and the function numbers inside local labels are dropped, and
what is left is compared as text.  Prints how many kernels are identical and, for each of the others, both instruction counts and the
VGPR, scratch and static LDS figures of the code object's metadata (a kernel's dynamic LDS is a launch argument: it is not in the assembly, its
size comes from the kernel's geometry struct).  Exit status 1 if any kernel differs or exists on one side only."""

import re
import sys

FIELDS = ((".vgpr_count", "VGPRs"), (".private_segment_fixed_size", "scratch"), (".group_segment_fixed_size", "static LDS"))


def kernels(path):
    """{symbol: (cleaned body lines, {metadata field: value})} of the kernels the metadata lists."""
    with open(path) as f:
        text = f.read()
    meta = {}
    for entry in re.split(r"^  - ", text[text.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if name:
            meta[name.group(1)] = {k: int(m.group(1)) if (m := re.search(r"^\s*%s:\s*(\d+)" % re.escape(k), entry, re.M)) else -1 for k, _ in FIELDS}
    out = {}
    for sym, figures in meta.items():
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(sym), text, re.M | re.S)
        if not body:
            sys.exit("%s: no code found for %s" % (path, sym))
        lines = []
        for line in body.group(1).splitlines():
            line = re.sub(r"\.L(BB|tmp|func_begin)\d+", r".L\1", line.split(";")[0]).strip()
            if line and not re.match(r"\.(loc|file|cfi_)", line):
                lines.append(line)
        out[sym] = (lines, figures)
    return out


def main(before, after):
    a, b = kernels(before), kernels(after)
    same = [s for s in a if s in b and a[s][0] == b[s][0]]
    print("%d kernels before, %d after, %d identical" % (len(a), len(b), len(same)))
    for s in sorted(set(a) | set(b)):
        if s in same:
            continue
        if s not in a or s not in b:
            print("%s: only %s" % (s, "before" if s in a else "after"))
            continue
        count = lambda lines: sum(1 for x in lines if not x.endswith(":") and not x.startswith("."))
        figures = ", ".join("%s %d -> %d" % (label, a[s][1][k], b[s][1][k]) for k, label in FIELDS)
        print("%s: instructions %d -> %d, %s" % (s, count(a[s][0]), count(b[s][0]), figures))
    return 0 if len(same) == len(a) == len(b) else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
