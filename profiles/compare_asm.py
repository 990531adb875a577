#!/usr/bin/env python3
"""Compare two gfx950 assembly files kernel by kernel (no GPU): was a refactor of the source a refactor of the code?

    python profiles/compare_asm.py OLD.s NEW.s

Both files come from `hipcc --cuda-device-only -S` with the flags the Makefile gives the unit
(csrc/check_ring_isa.compile_to_asm does exactly that).  Kernels are matched by their unchanged symbol names.  For each
kernel the body (from its label to `.end_amdhsa_kernel`, i.e. the instructions AND the `.amdhsa_*` resource block) is
normalised - comment-only lines and trailing comments dropped, local labels (`.LBB<n>_<m>`, `.Ltmp<n>`, `.Lfunc_end<n>`,
...) renumbered by order of first appearance - and compared as text.  Output: one line per kernel, `identical`, or the
resource delta (VGPRs, AGPRs, SGPRs, scratch, LDS, occupancy: old -> new) and the instruction-count delta; a summary line;
exit status 1 when any kernel differs or is missing on one side."""
from __future__ import annotations

import re
import sys

_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")
_FACTS = {                     # the compiler's own per-kernel summary comments
    "vgpr": r"; NumVgprs: (\d+)",
    "agpr": r"; NumAgprs: (\d+)",
    "sgpr": r"; NumSgprs: (\d+)",
    "scratch": r"; ScratchSize: (\d+)",
    "lds": r"; LDSByteSize: (\d+)",
    "occupancy": r"; Occupancy: (\d+)",
}


def kernels(asm: str) -> dict:
    """name -> (normalised body lines, resource facts, instruction count) for every kernel of the file"""
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", asm, flags=re.M)
    out = {}
    for name in names:
        start = re.search(rf"^{re.escape(name)}:", asm, flags=re.M).end()
        end = asm.index(".end_amdhsa_kernel", start)
        nxt = asm.find("-- Begin function", end)          # the "; Kernel info:" comments follow the resource block
        tail = asm[end:nxt if nxt > 0 else len(asm)]
        facts = {k: int(m.group(1)) for k, pat in _FACTS.items() if (m := re.search(pat, tail))}
        seen, lines, ninstr = {}, [], 0
        for raw in asm[start:end].split("\n"):
            line = raw.split(";", 1)[0].rstrip()
            if not line.strip():
                continue
            line = _LABEL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), line)
            lines.append(line)
            word = line.split()[0]
            ninstr += not (word.startswith(".") or word.endswith(":"))
        out[name] = (lines, facts, ninstr)
    return out


def main(old_path: str, new_path: str) -> int:
    with open(old_path) as fh:
        old = kernels(fh.read())
    with open(new_path) as fh:
        new = kernels(fh.read())
    same = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only in {'NEW' if name in new else 'OLD'}")
            continue
        (lo, fo, no), (ln, fn, nn) = old[name], new[name]
        if lo == ln:
            same += 1
            print(f"{name}: identical")
            continue
        delta = ", ".join(f"{k} {fo.get(k)} -> {fn.get(k)}" for k in _FACTS if fo.get(k) != fn.get(k)) or "resources equal"
        print(f"{name}: DIFFERENT: {delta}; instructions {no} -> {nn} ({nn - no:+d})")
    total = len(set(old) | set(new))
    print(f"{same} of {total} kernels identical")
    return 0 if same == total else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
