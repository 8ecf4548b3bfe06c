#!/usr/bin/env python3
"""What the balance check of a generic bus group costs (vx_bus_group_check: the records kernels, the sort, the match) beside the
auxiliary round of the same tables (vx_stark_aux_trace of each): MerkleOpenAir + LeafSpongeAir for n openings of 9-word leaves of
a 2^12-leaf tree with the verifier's 9 n row words outside, at n = 64, 1024 and 4096 (2^15 / 2^19 / 2^21 and 2^12 / 2^16 / 2^18 rows),
once with the compiled MerkleOpenAir (k_bus_records<Air>) and once with its restatement with declared messages (k_bus_records_prog, the
interpreter).  The two alternate, five runs each; a run is the HIP-event time of 10 calls after a warm-up call, in milliseconds per
call.  One JSON line: per size the records, the runs, their means and spreads (max - min), and the check over the auxiliary round.
The call is timed as a whole -- it includes its two host waits and the upload of the outside records; the split into records, sort
and match is read from a kernel trace of this tool (k_bus_records*, rocPRIM's kernels, k_bus_match).  profiles/r13_bus_group_rate.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vx_import  # noqa: E402
import bus_programs as BP  # noqa: E402
import leaf_sponge_ref as R  # noqa: E402
import merkle_open_ref as M  # noqa: E402

vx = vx_import.load()
L = vx.lib
ctx = vx.Context(0)
P = 2**64 - 2**32 + 1
CHAL = M.CHAL
REPS, RUNS = 10, 5
D, LEAF = 12, 9
rng = np.random.default_rng(84)
out = {}


def timed(call):
    call()  # warm-up
    ctx.sync()
    ctx.timer_start()
    for _ in range(REPS):
        call()
    return round(ctx.timer_stop() / REPS, 4)


leaves = rng.integers(0, P, size=(1 << D, LEAF), dtype=np.uint64)
data = ctx.from_host(leaves)
tree = ctx.merkle(data, 1 << D, LEAF, L.VX_LEAVES_ROW_MAJOR, 4)
restated = BP.merkle_open().register()
for n in (64, 1024, 4096):
    idx = [int(v) for v in rng.integers(0, 1 << D, size=n)]
    lo, ls = M.log_rows(n, D), R.log_rows(n, LEAF)
    ob, opub = ctx.merkle_open_air_trace(tree, idx, lo)
    sb, spub = ctx.leaf_sponge_air_trace(data, 1 << D, LEAF, L.VX_LEAVES_ROW_MAJOR, idx, ls)
    outside = np.array([[i, j, int(v), 0, 9, P - 1] for i in idx for j, v in enumerate(leaves[i])], dtype=np.uint64)
    res = {"rows": [1 << lo, 1 << ls], "records": 2 * n + (LEAF + 2) * n + LEAF * n, "runs_ms": {}}
    calls = {}
    for name, first in (("compiled", L.VX_AIR_MERKLE_OPEN), ("interpreted", restated)):
        tables = [(first, ob, lo, opub), (L.VX_AIR_LEAF_SPONGE, sb, ls, spub)]
        assert ctx.bus_group_check(tables, outside) is None, name  # a bus that closes, or the times mean nothing
        assert ctx.bus_group_check(tables, outside[1:]) is not None, name
        calls["check_" + name] = lambda tables=tables: ctx.bus_group_check(tables, outside)
        calls["aux_" + name] = lambda first=first: (ctx.stark_aux_trace(first, ob, lo, CHAL, L.VX_MERKLE_OPEN_AIR_AUX_COLS, opub)[0].free(),
                                                    ctx.stark_aux_trace(L.VX_AIR_LEAF_SPONGE, sb, ls, CHAL, L.VX_LEAF_SPONGE_AIR_AUX_COLS, spub)[0].free())
    for k in calls:
        res["runs_ms"][k] = []
    for _ in range(RUNS):
        for k, call in calls.items():
            res["runs_ms"][k].append(timed(call))
    for k, v in res["runs_ms"].items():
        res[k + "_mean_ms"], res[k + "_spread_ms"] = round(float(np.mean(v)), 4), round(max(v) - min(v), 4)
    for name in ("compiled", "interpreted"):
        res["check_over_aux_" + name] = round(res["check_%s_mean_ms" % name] / res["aux_%s_mean_ms" % name], 3)
    out["openings_%d" % n] = res
    ob.free(), sb.free()
L.air_unregister(restated)
tree.free(), data.free()
print(json.dumps(out))
