#!/usr/bin/env python3
"""Which kernels of two device-code listings differ (tools/isa_stats.sh writes two such listings, one per
translation unit: ISA_OUT=dir tools/isa_stats.sh -> dir/pt_kernel.s, dir/image_ops.s; compare them one at a time).
Kernel bodies are compared line by line with block labels renumbered and comments dropped; the .amdhsa metadata is not part of a
body.  Used to show that a change left the members of the family as they were (adaptive sampling).
usage: python tools/isa_diff.py before.s after.s   -> one line per kernel that differs or exists on one side only; exit 1 if any
       kernel present on both sides differs"""
import difflib
import re
import sys


def bodies(path):
    text, out = open(path).read(), {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        if ".amdhsa_kernel %s\n" % m.group(1) not in text:
            continue
        body = re.sub(r"\s*;.*", "", m.group(2))
        labels = {}
        body = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), "L%d" % len(labels)), body)
        out[m.group(1)] = [l for l in body.split("\n") if l.strip() and not l.strip().startswith(".")]   # no directives (.amdhsa_*, .p2align)
    return out


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    differ = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k:40s} only in {'after' if k in b else 'before'}")
            continue
        if a[k] != b[k]:
            n = sum(1 for l in difflib.unified_diff(a[k], b[k], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print(f"{k:40s} differs: {len(a[k])} -> {len(b[k])} lines, {n} changed lines")
            differ += 1
    print(f"{len(set(a) & set(b))} kernels on both sides, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
