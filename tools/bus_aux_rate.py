#!/usr/bin/env python3
"""The auxiliary round alone -- vx_stark_aux_trace, HIP-event timed, milliseconds averaged over 20 calls after a warm-up call -- for
the twelve tables whose auxiliary columns come from bus_aux.cuh, each at the shape of its rate tool; the witnesses are random claims
of the right ranges (the auxiliary round reads flags and cells, it checks no statement).  One JSON line.  VX_LIB_PATH selects another
libvxprove build (profiles/r11_bus_aux_refactor.json, r14_bus_lists_older.json, r16_bus_lists_sha.json: the parent commit's and this
one alternating)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vx_import  # noqa: E402
import fri_combine_ref as K  # noqa: E402
import fri_fold_ref as F  # noqa: E402
import transcript_ref as T  # noqa: E402

vx = vx_import.load()
L = vx.lib
ctx = vx.Context(0)
P = 2**64 - 2**32 + 1
CHAL = F.CHAL
reps = 20
rng = np.random.default_rng(84)
out = {}


def timed(air, tb, log_n, cols, pub):
    ctx.stark_aux_trace(air, tb, log_n, CHAL, cols, pub)[0].free()  # warm-up
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        ctx.stark_aux_trace(air, tb, log_n, CHAL, cols, pub)[0].free()
    return round(ctx.timer_stop() / reps, 4)


# MerkleOpenAir: 84 openings of a 2^20-leaf tree, 2^16 rows (tools/merkle_open_rate.py)
n_leaves = 1 << 20
data = ctx.alloc(8 * n_leaves)
ctx.fill_random(data, 8 * n_leaves, 2024)
tree = ctx.merkle(data, n_leaves, 8, L.VX_LEAVES_ROW_MAJOR, 4)
idx = [int(v) for v in rng.integers(0, n_leaves, size=84)]
tb, pub = ctx.merkle_open_air_trace(tree, idx, 16)
out["merkle_open_2^16"] = timed(L.VX_AIR_MERKLE_OPEN, tb, 16, L.VX_MERKLE_OPEN_AIR_AUX_COLS, pub)
tb.free(), tree.free(), data.free()

# LeafSpongeAir: 84 rows of 1018 words, 2^19 rows (tools/merkle_rows_rate.py)
n_leaves, LL = 1 << 17, 1018
data = ctx.alloc(LL * n_leaves)
ctx.fill_random(data, LL * n_leaves, 2025)
idx = [int(v) for v in rng.integers(0, n_leaves, size=84)]
tb, pub = ctx.leaf_sponge_air_trace(data, n_leaves, LL, L.VX_LEAVES_COLS_BITREV, idx, 19)
out["leaf_sponge_2^19"] = timed(L.VX_AIR_LEAF_SPONGE, tb, 19, L.VX_LEAF_SPONGE_AIR_AUX_COLS, pub)
tb.free(), data.free()

# FriFoldAir: 84 queries, LN 21, four layers, 2^10 rows, TREE0 3 (tools/fri_fold_rate.py; the witness checks ranges only)
LN, NL = 21, 4
index = [int(v) for v in rng.integers(0, 1 << LN, size=84)]
betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
leaves = rng.integers(0, P, size=(84, NL, 16, 2), dtype=np.uint64)
ev0 = rng.integers(0, P, size=(84, 2), dtype=np.uint64)
tb, pub = ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, 10, 3)
out["fri_fold_2^10"] = timed(L.VX_AIR_FRI_FOLD, tb, 10, L.VX_FRI_FOLD_AIR_AUX_COLS, pub)
tb.free()

# FriCombineAir: 84 queries of 745 + 276 + 4 words, 2^17 rows (tools/fri_combine_rate.py)
cm, ca, nq = 745, 276, 4
st = K.rand_statement(LN, cm, ca, nq, seed=84)
rows = rng.integers(0, P, size=(84, cm + ca + nq), dtype=np.uint64)
tb, pub = ctx.fri_combine_air_trace(LN, st["r"], cm, ca, nq, st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"], index, rows, ev0, 17, K.TREE0)
out["fri_combine_2^17"] = timed(L.VX_AIR_FRI_COMBINE, tb, 17, L.VX_FRI_COMBINE_AIR_AUX_COLS, pub)
tb.free()

# MerkleOpenSetAir / LeafSpongeSetAir: the layer trees of 84 queries, 2^17 and 2^16 rows (tools/fri_queries_rate.py)
evals = [ctx.alloc(2 << (LN - 4 * l)) for l in range(NL)]
for l in range(NL):
    ctx.fill_random(evals[l], 2 << (LN - 4 * l), 2184 + l)
trees = [ctx.fri_layer_tree(evals[l], LN - 4 * l, 4, 4) for l in range(NL)]
tree_of = [l for _ in index for l in range(NL)]
leaf_idx = [i >> (4 * (l + 1)) for i in index for l in range(NL)]
log_leaves = [LN - 4 * (l + 1) for l in range(NL)]
tb, pub = ctx.merkle_open_set_air_trace(trees, tree_of, leaf_idx, 17)
out["merkle_open_set_2^17"] = timed(L.VX_AIR_MERKLE_OPEN_SET, tb, 17, L.VX_MERKLE_OPEN_SET_AIR_AUX_COLS, pub)
tb.free()
tb, pub = ctx.leaf_sponge_set_air_trace(evals, log_leaves, tree_of, leaf_idx, 16)
out["leaf_sponge_set_2^16"] = timed(L.VX_AIR_LEAF_SPONGE_SET, tb, 16, L.VX_LEAF_SPONGE_SET_AIR_AUX_COLS, pub)
tb.free()

# LeafNoopAir: the 84 quotient-tree openings of one proof, 2^7 rows (tools/stark_queries_rate.py)
nrows = [[int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64)] for _ in range(84)]
tb, pub = ctx.leaf_noop_air_trace([10] * 84, [i >> 0 for i in index], nrows, 7)
out["leaf_noop_2^7"] = timed(L.VX_AIR_LEAF_NOOP, tb, 7, L.VX_LEAF_NOOP_AIR_AUX_COLS, pub)
tb.free()

# TranscriptAir: one chain of 650 duplexes (a hash-chain proof's transcript), 2^15 rows (tools/stark_transcripts_rate.py)
chains = [T.filler(650, seed=50)]
tb, pub, _ = ctx.transcript_air_trace([ops for ops, _ in chains], [w for _, w in chains], 15)
out["transcript_2^15"] = timed(L.VX_AIR_TRANSCRIPT, tb, 15, L.VX_TRANSCRIPT_AIR_AUX_COLS, pub)
tb.free()

# ShaTreeAir of 256 leaves, 2^16 rows: random cells (every message row of a bottom-level node receives, as in a full range)
tb = ctx.alloc(L.VX_SHA_TREE_AIR_COLS << 16)
ctx.fill_random(tb, L.VX_SHA_TREE_AIR_COLS << 16, 2026)
out["sha_tree_2^16"] = timed(L.VX_AIR_SHA_TREE[256], tb, 16, 16, [0] * 17)
tb.free()

# EpochEndAir: 300 new authorities, 2^9 rows (the table of vx_rotate_prove)
e = vx.synth.EpochEndHeader(140000, 300)
hb = ctx.from_host(e.padded)
tb, pub, _ = ctx.epoch_end_trace(hb, e.start_position, 300, bus_on=1)
out["epoch_end_2^9"] = timed(L.VX_AIR_EPOCH_END, tb, 9, L.VX_EPOCH_END_AIR_AUX_COLS, pub)
tb.free(), hb.free()

# ShaChainAir: 300 keys, all flagged and sent (mode 1), 2^16 rows (the commitment table of a header_range proof with a justification)
keys = [hashlib.sha256(b"authority %d" % i).digest() for i in range(300)]
tb, pub, _ = ctx.sha_chain_trace(keys, 16, signed=[1] * 300, bus_on=1)
out["sha_chain_2^16"] = timed(L.VX_AIR_SHA_CHAIN, tb, 16, L.VX_SHA_AIR_AUX_COLS, pub)
tb.free()

# Sha512Air15: 201 of the 300 flagged, 2^15 rows (the table hashes R || A || message: the signatures need not verify)
sigs = [hashlib.sha512(b"signature %d" % i).digest() for i in range(300)]
tb, pub = ctx.sha512_trace(keys, sigs, bytes(range(53)), [1] * 201 + [0] * 99, 15, bus_on=1)
out["sha512_2^15"] = timed(L.VX_AIR_SHA512[15], tb, 15, L.VX_SHA512_AIR_AUX_COLS, pub)
tb.free()
print(json.dumps(out))
