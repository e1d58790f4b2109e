#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two output directories of tools/device_asm_sums.sh, for a file whose sum moved because kernels were ADDED to it: inserting a
kernel renumbers the labels of the ones behind it (.LBB<n>_<m>, .Lfunc_end<n>, "Header=BB<n>_<m>" comments), which changes every line that names one. With
those numbers and the comment column's padding normalised, a kernel present in both trees either has the instruction stream it had or is listed as changed.

    tools/device_asm_sums.sh HEAD~1 /tmp/parent && tools/device_asm_sums.sh . /tmp/branch
    python tools/device_asm_kernels.py /tmp/parent /tmp/branch kernels_graph [more file stems ...]"""
import re
import sys
from pathlib import Path


def kernels(path: Path) -> dict[str, list[str]]:
    out, cur, name = {}, None, None
    for line in path.read_text().splitlines():
        m = re.match(r"^(_Z[\w$.]+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name] = cur
                cur = None
                continue
            line = re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+", r".L\1", line)
            cur.append(re.sub(r"\s+", " ", re.sub(r"\bBB\d+_", "BB_", line)))
    return out


def main():
    parent, branch, *stems = sys.argv[1:]
    bad = 0
    for stem in stems:
        a, b = kernels(Path(parent) / f"{stem}.s"), kernels(Path(branch) / f"{stem}.s")
        changed = sorted(k for k in a if a[k] != b.get(k))
        print(f"{stem}: {len(a)} kernels before, {len(a) - len(changed)} of them with the instruction stream they had; changed or gone: {changed}; new on the branch: {len(set(b) - set(a))}")
        bad += len(changed)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
