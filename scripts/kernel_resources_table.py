#!/usr/bin/env python3
"""Tabulate the compiler's per-kernel resource report of two builds side by side.

usage: kernel_resources_table.py PARENT_DIR NEW_DIR FILE.hip [FILE.hip ...]
Each directory holds, per FILE.hip, FILE.txt: the stderr of
    hipcc <the Makefile's CXXFLAGS> --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c FILE.hip -o /dev/null
(csrc/Makefile, the resource-usage-* recipes).  A kernel of the new build is matched with the parent's kernel of the same
demangled name, and failing that with the parent's kernel whose name is the new one's less its trailing `, false` template
arguments (a new, defaulted parameter).  A cell reads parent->new where the two differ; a kernel without a parent is `new`."""
import os
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sgpr-spill"), ("VGPRs Spill", "vgpr-spill"), ("LDS Size [bytes/block]", "lds")]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    names = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True, check=True).stdout.split("\n")
    def short(n):
        n = re.sub(r"^void ", "", n).replace("(anonymous namespace)::", "")
        return n[:n.index("(")] if "(" in n else n
    return {short(n): v for n, v in zip(names, out.values())}


def main():
    parent_dir, new_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    differ = 0
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        old, new = parse(os.path.join(parent_dir, stem + ".txt")), parse(os.path.join(new_dir, stem + ".txt"))
        print(f"== csrc/{stem}.hip")
        print(f"{'kernel':<62}" + "".join(f"{h:>13}" for _, h in FIELDS))
        for name, v in new.items():
            base, p = name, old.get(name)
            while p is None and base.endswith(", false>"):
                base = base[:-len(", false>")] + ">"
                p = old.get(base)
            cells = []
            for key, _ in FIELDS:
                if p is None:
                    cells.append(f"new {v[key]}")
                elif p[key] != v[key]:
                    cells.append(f"{p[key]}->{v[key]}")
                    differ += 1
                else:
                    cells.append(str(v[key]))
            print(f"{name:<62}" + "".join(f"{c:>13}" for c in cells))
        print()
    print(f"cells of kernels that have a parent and differ from it: {differ}")


if __name__ == "__main__":
    main()
