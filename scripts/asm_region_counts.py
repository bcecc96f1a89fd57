#!/usr/bin/env python3
"""Static instruction counts of one kernel in a `hipcc -S` listing, per basic block and per loop depth.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S gsn_amd/csrc/layer_rp.hip -o layer_rp.s
    python scripts/asm_region_counts.py layer_rp.s ILi4ELi2ELb0ELb1EE [--blocks]

The second argument is a substring of the kernel's mangled name.  Classes: MFMA, other VALU (v_*), LDS (ds_*), VMEM (buffer_* / global_*
/ flat_* / scratch_*), every s_* instruction (scalar ALU and memory, branches, waits, s_nop: column `s_*(all)`).  A few mnemonics are tallied on their own (register copies, single
and packed multiplies, scalar offset set-up, waits for every load) -- what profiles/layer_rp_instruction_diet.txt follows."""
import collections
import re
import sys

WATCH = ["v_mov_b64", "v_mov_b32", "v_accvgpr", "v_mul_f32", "v_pk_mul_f32", "s_movk_i32", "s_mov_b32", "s_nop", "s_waitcnt"]


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("s_"):
        return "SALU"
    return None


def main():
    path, name = sys.argv[1], sys.argv[2]
    show_blocks = "--blocks" in sys.argv
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*" + re.escape(name) + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks = []          # (label, depth, first line, counters)
    cur = ("entry", 0, start + 1, collections.Counter())
    for i in range(start + 1, end):
        l = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", l)
        if m:
            blocks.append(cur)
            d = re.search(r"Depth=(\d+)", m.group(2))
            cur = (m.group(1), int(d.group(1)) if d else 0, i + 1, collections.Counter())
            continue
        m = re.match(r"^\t([a-z_0-9]+)", l)
        if not m:
            continue
        op = m.group(1)
        c = classify(op)
        if c is None:
            continue
        cur[3][c] += 1
        for w in WATCH:
            if op.startswith(w):
                cur[3][w] += 1
        if op == "s_waitcnt" and re.search(r"vmcnt\(0\)", l):
            cur[3]["vmcnt(0)"] += 1
    blocks.append(cur)
    cols = ["MFMA", "VALU", "LDS", "VMEM", "SALU"] + WATCH + ["vmcnt(0)"]
    head = {"SALU": "s_*(all)"}          # (scalar ALU and memory, branches, waits, s_nop)
    print("%-12s %5s %7s  " % ("block", "depth", "line") + " ".join("%12s" % head.get(c, c) for c in cols))
    by_depth = collections.defaultdict(collections.Counter)
    for label, depth, line, cnt in blocks:
        by_depth[depth].update(cnt)
        if show_blocks and sum(cnt[c] for c in cols[:5]) >= 8:
            print("%-12s %5d %7d  " % (label, depth, line) + " ".join("%12d" % cnt[c] for c in cols))
    for depth in sorted(by_depth):
        print("%-12s %5d %7s  " % ("all", depth, "") + " ".join("%12d" % by_depth[depth][c] for c in cols))


if __name__ == "__main__":
    main()
