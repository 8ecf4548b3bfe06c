#!/usr/bin/env python3
"""The FRI query phase on one bus, end to end on one GPU at the shape of one STARK proof: 84 queries of a 2^21 LDE, four fold layers
built on the GPU (vx_fri_fold / vx_fri_layer_tree) from GPU-made layer-0 values, the final polynomial interpolated from the 32 values
of the last layer.  Three tables: MerkleOpenSetAir (84 x 44 levels), LeafSpongeSetAir (84 x 4 leaves of four blocks), FriFoldAir.
One JSON line, milliseconds averaged over `reps` calls after a warm-up call: vx_fri_queries_prove as a whole (the gathers, the host
fold check, three witnesses, three STARKs under shared challenges), the two set witnesses alone, vx_fri_queries_verify on the host
(no leaves, no paths, no folds), and the three tables' log2 of rows."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vx_import  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.build()

vx = vx_import.load()
ctx = vx.Context(0)
P = 2**64 - 2**32 + 1
LN, NL, cap_h, reps, HDR = 21, 4, 4, 10, 7
rng = np.random.default_rng(84)
betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
evals = [ctx.alloc(2 << (LN - 4 * l)) for l in range(NL + 1)]
ctx.fill_random(evals[0], 2 << LN, 2184)
shift = 7
for l in range(NL):
    ctx.fri_fold(evals[l], LN - 4 * l, 4, betas[l], shift, evals[l + 1])
    shift = pow(shift, 16, P)
trees = [ctx.fri_layer_tree(evals[l], LN - 4 * l, 4, cap_h) for l in range(NL)]
fpoly = O.ext_coset_ntt(evals[NL].download(), shift, inverse=True).reshape(-1, 2)
index = [int(v) for v in rng.integers(0, 1 << LN, size=84)]
lv0 = ctx.fri_leaves(evals[0], LN, 4, [i >> 4 for i in index]).reshape(84, 16, 2)
ev0 = np.array([lv0[k, i & 15] for k, i in enumerate(index)], dtype=np.uint64)
caps = np.array([t.cap() for t in trees], dtype=np.uint64)
tree_of = [l for _ in index for l in range(NL)]
leaf_idx = [i >> (4 * (l + 1)) for i in index for l in range(NL)]
log_leaves = [LN - 4 * (l + 1) for l in range(NL)]

blob = ctx.fri_queries_prove(LN, betas, fpoly, trees, evals[:NL], index)  # warm-up (pools, side contexts, tables)
vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps, index, ev0)
sizes = [int(v) for v in blob[4:7]]
logs = [int(blob[HDR + 2]), int(blob[HDR + sizes[0] + 2]), int(blob[HDR + sizes[0] + sizes[1] + 2])]
ob, _ = ctx.merkle_open_set_air_trace(trees, tree_of, leaf_idx, logs[0])
sb, _ = ctx.leaf_sponge_set_air_trace(evals[:NL], log_leaves, tree_of, leaf_idx, logs[1])
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
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3)


out = {"queries": 84, "log_lde": LN, "layers": NL, "rows_log2_open_sponge_fold": logs, "blob_KB": round(blob.size * 8 / 1024, 1)}
out["open_set_witness_wall_ms"] = timed_wall(lambda: ctx.merkle_open_set_air_trace(trees, tree_of, leaf_idx, logs[0], out=ob))
out["sponge_set_witness_wall_ms"] = timed_wall(lambda: ctx.leaf_sponge_set_air_trace(evals[:NL], log_leaves, tree_of, leaf_idx, logs[1], out=sb))
out["prove_wall_ms"] = timed_wall(lambda: ctx.fri_queries_prove(LN, betas, fpoly, trees, evals[:NL], index))
out["prove_wall_ms_second_run"] = timed_wall(lambda: ctx.fri_queries_prove(LN, betas, fpoly, trees, evals[:NL], index))
out["verify_host_ms"] = timed_wall(lambda: vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps, index, ev0))
print(json.dumps(out))
