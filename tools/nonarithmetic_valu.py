#!/usr/bin/env python3
"""Compares, selects and moves of a render kernel by stage, from the device assembly of a -DTRT_MARKS=2 build.

usage: tools/nonarithmetic_valu.py build/isa_profile/dev.s [decoupled|plain] > table.md

A stage boundary of such a build is `s_mov_b32 m0, <slot> ; MARK` (csrc/trt_common.hpp).  The instructions are attributed to
the mark that precedes them in the TEXT of the kernel: static counts, every path of a stage included (the wave-uniform fall-backs
-- sweep, full divisions, FP64 sky look-up -- sit in the text of the stage that can take them).  The EXECUTED counts per wave and
round are tools/isa_profile.py's; this table says which instructions they are.
"""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KERNELS = {
    "plain": "render_rounds_kernelILb0ELb0ELb0ELb0ELb0ELb0ELb0EJEEE",
    "decoupled": "render_rounds_kernelILb0ELb0ELb1ELb0ELb0ELb0ELb0EJEEE",
}
from isa_profile import NAMES as STAGES  # an interval starts at its boundary (TRT_MARK_AT in csrc/trt_rounds.hpp)


def kernel_body(lines, mangled):
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN3trt") and mangled in l and l.split(":")[0].endswith("_"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def main():
    path, which = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "decoupled")
    body = kernel_body(open(path).read().split("\n"), KERNELS[which])
    slot, order = 63, [63]
    per = collections.defaultdict(collections.Counter)
    for line in body:
        mark = re.match(r"\s+s_mov_b32 m0, (\d+)\s*;\s*MARK", line)
        if mark:
            slot = int(mark.group(1))
            if slot not in order:
                order.append(slot)
            continue
        m = re.match(r"\s+(v_\w+)", line)
        if not m:
            continue
        op = re.sub(r"_e(32|64)$", "", m.group(1))
        c = per[slot]
        c["valu"] += 1
        if op.startswith("v_cmp"):
            c["cmp"] += 1
            c["cmp f64" if op.endswith("_f64") else "cmp f32" if op.endswith("_f32") else "cmp int"] += 1
            c["op " + op[6:]] += 1
        elif op.startswith("v_cndmask"):
            c["cnd"] += 1
        elif op.startswith("v_mov") or op.startswith("v_accvgpr"):
            c["mov"] += 1
            if re.search(r"v_mov_b(32|64)(_e32)? v\[?\d+(:\d+\])?, (0x|-?\d|s|v_)", line) or re.search(r", (0x[0-9a-f]+|-?[\d.]+)\s*(;.*)?$", line):
                c["mov const"] += 1
    print(f"# compares, selects and moves by stage: the {which} instantiation, static (text of the kernel)\n")
    print("| stage | VALU | cmp | of which f64 / f32 / int | cndmask | mov | of which constants | the compares |")
    print("|---|---|---|---|---|---|---|---|")
    total = collections.Counter()
    for s in order:
        c = per[s]
        total.update(c)
        ops = ", ".join(f"{k[3:]} x{v}" for k, v in sorted(c.items()) if k.startswith("op "))
        print(f"| {STAGES.get(s, 'slot %d' % s)} | {c['valu']} | {c['cmp']} | {c['cmp f64']} / {c['cmp f32']} / {c['cmp int']} | {c['cnd']} | {c['mov']} | {c['mov const']} | {ops} |")
    print(f"| **kernel** | {total['valu']} | {total['cmp']} | {total['cmp f64']} / {total['cmp f32']} / {total['cmp int']} | {total['cnd']} | {total['mov']} | {total['mov const']} | |")


if __name__ == "__main__":
    main()
