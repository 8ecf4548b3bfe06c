#!/usr/bin/env python3
"""The tree top alone on an idle GPU: HIP-event milliseconds per vx_merkle_build of trees whose leaves are their own digests
(leaf_len 4: the leaf kernel only copies), so the time is the levels above them -- the shapes a proof's tops have: 2^15 digests to a
cap of 16 (eleven levels), 2^15 to the root (fifteen), 2^8 to a cap of 16 (a FRI layer tree).  One JSON line.  VX_LIB_PATH selects
the build (VX_TOP_THREADS / VX_TOP_LANE_MIN variants of vx_poseidon.hip, or the library before k_merkle_top)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vx_import  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
reps, out = 50, {"lib": os.path.basename(vx.lib.LIB_PATH)}
for n, cap_h in ((1 << 15, 4), (1 << 15, 0), (1 << 8, 4)):
    data = ctx.alloc(4 * n)
    ctx.fill_random(data, 4 * n, 5)
    for _ in range(3):
        ctx.merkle(data, n, 4, vx.lib.VX_LEAVES_ROW_MAJOR, cap_h).free()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        ctx.merkle(data, n, 4, vx.lib.VX_LEAVES_ROW_MAJOR, cap_h).free()
    out[f"2^{n.bit_length() - 1}_to_cap_{1 << cap_h}_us"] = round(1e3 * ctx.timer_stop() / reps, 1)
    data.free()
ctx.close()
print(json.dumps(out))
