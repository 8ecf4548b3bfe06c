#!/usr/bin/env python3
"""MerkleOpenAir + LeafSpongeAir end to end on one GPU at the shape of one STARK proof's query phase into its trace tree: 84
openings of a tree of 2^17 leaves x 1018 words as vx_lde leaves them (VX_LEAVES_COLS_BITREV, cap height 4) = 10,752 sponge
blocks in a 2^19-row table beside 1,428 path blocks in a 2^16-row table.  One JSON line: HIP-event milliseconds (vx_timer_start /
vx_timer_stop on the context's stream, averaged over `reps` calls after a warm-up call) of the sponge witness alone
(vx_leaf_sponge_air_trace: k_leaf_sponge_states + k_leaf_sponge_trace + the claims back to the host and their digest) and of
vx_merkle_rows_prove, and wall milliseconds of vx_merkle_rows_verify on the host.  The two witness kernels are told apart by a
kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/merkle_rows_rate.py)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vx_import  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
D, n_leaves, L, reps = 17, 1 << 17, 1018, 5
layout = vx.lib.VX_LEAVES_COLS_BITREV
data = ctx.alloc(L * n_leaves)
ctx.fill_random(data, L * n_leaves, 2025)
tree = ctx.merkle(data, n_leaves, L, layout, 4)
idx = [int(v) for v in np.random.default_rng(84).integers(0, n_leaves, size=84)]
cap, rows = tree.cap(), ctx.lde_rows(data, D, L, idx)
tb, _ = ctx.leaf_sponge_air_trace(data, n_leaves, L, layout, idx, 19)  # warm-up (pool, tables)
blob = ctx.merkle_rows_prove(tree, data, L, layout, idx)
vx.lib.merkle_rows_verify(blob, cap, D, idx, rows)
ctx.sync()


def timed_events(fn):
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return round(ctx.timer_stop() / reps, 3)


def timed_wall(fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3)


out = {"openings": 84, "log_leaves": D, "leaf_len": L, "rows_log2_open": int(blob[6 + 2]), "rows_log2_sponge": int(blob[6 + int(blob[4]) + 2]),
       "blob_KB": round(blob.size * 8 / 1024, 1)}
out["sponge_witness_ms"] = timed_events(lambda: ctx.leaf_sponge_air_trace(data, n_leaves, L, layout, idx, 19, out=tb))
out["open_witness_ms"] = timed_events(lambda: ctx.merkle_open_air_trace(tree, idx, 16)[0].free())
out["rows_prove_ms"] = timed_events(lambda: ctx.merkle_rows_prove(tree, data, L, layout, idx))
out["rows_prove_wall_ms"] = timed_wall(lambda: ctx.merkle_rows_prove(tree, data, L, layout, idx))
out["openings_prove_ms"] = timed_events(lambda: ctx.merkle_openings_prove(tree, idx))
out["rows_verify_host_ms"] = timed_wall(lambda: vx.lib.merkle_rows_verify(blob, cap, D, idx, rows))
print(json.dumps(out))
