#!/usr/bin/env python3
"""Compare two builds' device assembly kernel by kernel, instructions only.

usage: compare_kernel_asm.py PARENT_DIR NEW_DIR FILE.s [FILE.s ...]
Each directory holds, per FILE, the output of
    hipcc <the Makefile's CXXFLAGS> --offload-arch=gfx950 --cuda-device-only -S FILE.hip -o FILE.s
A function's text is what stands between its label and its .Lfunc_end label, comments and directives dropped; metadata (the
kernel descriptors, the argument lists and their sizes) is not compared: appending a field to a struct passed by value grows the
kernarg segment and moves nothing the instructions read.  Prints one line per function and ends with the number that differ."""
import os
import re
import subprocess
import sys


def functions(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and cur is None and not line.startswith(".L"):
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
                continue
            t = line.split(";")[0].rstrip()
            if t.strip() and not t.strip().startswith("."):
                cur.append(t.strip())
            elif re.match(r"^\.LBB\w+:", t.strip()):
                cur.append(t.strip())
    return out


def main():
    parent, new, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    differ = 0
    for f in files:
        a, b = functions(os.path.join(parent, f)), functions(os.path.join(new, f))
        names = sorted(set(a) | set(b))
        dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        print(f"== {f}: {len(names)} functions")
        for n, d in zip(names, dem):
            d = re.sub(r"\(.*", "", d)
            if n not in a or n not in b:
                verdict = "only in " + ("the new build" if n in b else "the parent")
            else:
                verdict = f"identical ({len(a[n])} lines)" if a[n] == b[n] else f"DIFFERS ({len(a[n])} -> {len(b[n])} lines)"
            differ += not verdict.startswith("identical")
            print(f"{d:<110} {verdict}")
    print(f"functions that differ: {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
