#!/usr/bin/env python3
"""Compares the kernels of two device assembly files (hipcc ... -fuse-cuid=none --cuda-device-only -S) symbol by symbol,
whatever their order in the file: everything from a function's .type line to its .size line (the body and the
.amdhsa_kernel descriptor), with comments and trailing blanks removed and the function index in .LBB<n>_ / .Ltmp<n> /
.Lfunc_end<n> labels normalised.
usage: tools/asm_kernels_cmp.py old.s new.s  -> exit status 0 when the symbol sets and every body are the same"""
import re
import sys

LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def kernels(path):
    out, name, body = {}, None, []
    for raw in open(path):
        line = LABEL.sub(r".\1", raw.split(";", 1)[0].rstrip())
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        if name and line:
            body.append(line)
        if name and re.match(r"\s*\.size\s", line):
            out[name], name = body, None
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
print(f"{len(old)} / {len(new)} functions, {len(old.keys() ^ new.keys())} in one file only, "
      f"{len(differ)} differ")
for k in sorted(old.keys() ^ new.keys()) + differ:
    print(" ", k)
sys.exit(1 if differ or old.keys() != new.keys() else 0)
