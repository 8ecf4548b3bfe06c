#!/usr/bin/env python3
"""Instruction counts per basic block of one kernel in an AMDGPU assembly listing (hipcc --cuda-device-only -S): for every label the
number of vector (v_*) and other instructions, and whether the block ends in a backward branch to itself (a loop body).
  python3 tools/asm_blocks.py listing.s _Z6k_permPmj"""
import re
import sys


def main():
    path, kernel = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    blocks, cur = [], [kernel, 0, 0, False, {}]
    for l in lines[start + 1:]:
        t = l.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            blocks.append(cur)
            cur = [m.group(1), 0, 0, False, {}]
            continue
        if not t or t.startswith("."):
            continue
        op = t.split()[0]
        if op.startswith("v_"):
            cur[1] += 1
            cur[4][op] = cur[4].get(op, 0) + 1
        else:
            cur[2] += 1
        if op.startswith("s_cbranch") or op == "s_branch":  # what follows a branch is a block of its own
            cur[3] = t.split()[-1] == cur[0]
            blocks.append(cur)
            cur = ["  (after " + cur[0].strip() + ")", 0, 0, False, {}]
    blocks.append(cur)
    for name, nv, ns, loop, ops in blocks:
        print(f"{name:16s} valu {nv:5d} other {ns:4d}{'  loop' if loop else ''}")
        if loop and len(sys.argv) > 3:
            print("   ", ", ".join(f"{k} {v}" for k, v in sorted(ops.items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()
