#!/usr/bin/env python3
"""MerkleOpenAir end to end on one GPU at the shape of one STARK proof's query phase: 84 openings of a tree of 2^20 leaves x 8 words
(cap height 4) = 1,680 permutations in one 2^16-row table.  One JSON line: wall milliseconds of the witness kernel alone
(vx_merkle_open_air_trace), of vx_merkle_openings_prove, of vx_merkle_openings_verify on the host, and -- the work the table
replaces -- of a host verifier walking the same 84 Merkle paths (the C oracle's verify_merkle_proof_to_cap)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vx_import  # noqa: E402
from oracle import oracle as O  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
D, n_leaves, reps = 20, 1 << 20, 5
data = ctx.alloc(8 * n_leaves)
ctx.fill_random(data, 8 * n_leaves, 2024)
tree = ctx.merkle(data, n_leaves, 8, vx.lib.VX_LEAVES_ROW_MAJOR, 4)
idx = [int(v) for v in np.random.default_rng(84).integers(0, n_leaves, size=84)]
cap, digs = tree.cap(), tree.leaf_digests()[idx]
tb, _ = ctx.merkle_open_air_trace(tree, idx, 16)  # warm-up (pool, tables)
blob = ctx.merkle_openings_prove(tree, idx)
vx.lib.merkle_openings_verify(blob, cap, D, idx, digs)
ctx.sync()


def timed(fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3)


out = {"openings": 84, "log_leaves": D, "rows_log2": int(blob[6]), "blob_KB": round(blob.size * 8 / 1024, 1)}
out["witness_ms"] = timed(lambda: ctx.merkle_open_air_trace(tree, idx, 16, tb))
out["prove_ms"] = timed(lambda: ctx.merkle_openings_prove(tree, idx))
out["openings_verify_host_ms"] = timed(lambda: vx.lib.merkle_openings_verify(blob, cap, D, idx, digs))
sib = tree.open(idx)
rows = data.download().reshape(n_leaves, 8)[idx]
assert all(O.merkle_verify(rows[k], idx[k], sib[k], cap) for k in range(84))
out["host_walk_of_the_84_paths_ms"] = timed(lambda: [O.merkle_verify(rows[k], idx[k], sib[k], cap) for k in range(84)])
print(json.dumps(out))
