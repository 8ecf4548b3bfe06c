#!/usr/bin/env python3
"""Verifying on the GPU, measured: ONE full-size header_range_256 blob (P15k, 300 authorities, proven once) verified by
vx_header_range_verify (host) and vx_header_range_verify_dev (the Merkle openings in one launch of k_merkle_check), alternating,
ROUNDS rounds each, wall-clock milliseconds per call.  The yardstick is the host verifier on the same blob in the same run.  Beside
it the batch of the blob's openings on its own: claims and permutations, and vx_timer_start / vx_timer_stop around vx_merkle_check on
arrays made beforehand -- the call's own argument checks on the host, the staging copies and the kernel -- and around an upload of
the same words alone: the difference bounds the kernel's time from above (the bracket cannot leave the call's host part out; a
kernel trace of this script gives k_merkle_check alone).  One JSON line; with a path as argument it is written there too.
usage: python3 tools/verify_rate.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vx_import  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.build()
from oracle import stark_ref as S  # noqa: E402

ROUNDS, N = 5, 256
vx = vx_import.load()
ctx = vx.Context(0)
ch = vx.synth.Chain(N, profile="P15k")
cfg = ctx.stark_config()
just = vx.lib.PackedJustification(vx.synth.Justification(ch.target_block, ch.target_hash, n_auth=300), 300)
out96, blob = ctx.header_range_prove(ctx.from_host(ch.headers), ch.stride, ch.sizes, N, ch.trusted_block, ch.trusted_hash, ch.target_block, cfg, just=just)
blob = blob.copy()
args = (blob, N, ch.trusted_block, ch.trusted_hash, ch.target_block, out96, cfg)
kw = dict(authority_set_hash=just.sh.tobytes(), authority_set_id=just.struct.authority_set_id)


def wall_ms(fn):
    t0 = time.perf_counter()
    fn(*args, **kw)
    return 1e3 * (time.perf_counter() - t0)


vx.lib.header_range_verify(*args, **kw), ctx.header_range_verify(*args, **kw)  # warm-up: the pool block of the staging area
host, dev = [], []
for _ in range(ROUNDS):
    host.append(wall_ms(vx.lib.header_range_verify))
    dev.append(wall_ms(ctx.header_range_verify))

# the batch on its own: the claims of every table in the verifier's order (segments, Merkle, commitment, Ed25519, SHA-512)
segs, p_sha, p_tree, p_ed, p_h = vx.lib.split_blob_segments(blob)
tables = [np.array(p, dtype=np.uint64) for p in list(segs) + [p_tree, p_sha, p_ed, p_h]]
chal = S.shared_challenges_n([S.proof_peek(p, cfg.cap_height) for p in tables], 4)
caps, log_leaves, tree_of, leaf_idx, leaves, sibs, perms = [], [], [], [], [], [], 0
t0 = time.perf_counter()
claims = [vx.lib.stark_merkle_claims(p, cfg, chal) for p in tables]
replay_ms = 1e3 * (time.perf_counter() - t0)
for cl in claims:
    LN, _, _, a, _, cap_h, _ = cl["shape"]
    slot = {t: len(log_leaves) + k for k, t in enumerate(cl["trees"])}
    log_leaves += [LN if t >= vx.lib.SOPEN_TREE0 else LN - a * (t + 1) for t in cl["trees"]]
    caps.append(cl["caps"].reshape(-1))
    tree_of += [slot[int(t)] for t in cl["tree"]]
    leaf_idx += [int(i) for i in cl["index"]]
    leaves += cl["leaves"]
    sibs += cl["siblings"]
    perms += sum((-(-row.size // 8) if row.size > 4 else 0) + sb.shape[0] for row, sb in zip(cl["leaves"], cl["siblings"]))
cp, ll = np.ascontiguousarray(np.concatenate(caps)), np.array(log_leaves, dtype=np.int32)
tr, ix = np.array(tree_of, dtype=np.uint64), np.array(leaf_idx, dtype=np.uint64)
ln = np.array([r.size for r in leaves], dtype=np.uint64)
lv, sb = np.ascontiguousarray(np.concatenate(leaves)), np.ascontiguousarray(np.concatenate([s.reshape(-1) for s in sibs]))
ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
bad = C.c_size_t(0)


def check():
    rc = ctx.L.vx_merkle_check(ctx.h, ptr(cp), cfg.cap_height, ptr(ll), ll.size, ptr(tr), ptr(ix), ptr(ln), ptr(lv), lv.size, ptr(sb), sb.size, tr.size, C.byref(bad))
    assert rc == 0, rc


staged = np.concatenate([cp, lv, sb, np.zeros(6 * tr.size, dtype=np.uint64)])  # what vx_merkle_check uploads: caps, leaves, siblings, 48 bytes per claim
buf = ctx.alloc(staged.size)
check(), buf.upload(staged)
check_ms, copy_ms = [], []
for _ in range(ROUNDS):
    ctx.timer_start()
    check()
    check_ms.append(ctx.timer_stop())
    ctx.timer_start()
    buf.upload(staged)
    copy_ms.append(ctx.timer_stop())

mean = lambda v: round(sum(v) / len(v), 3)  # noqa: E731
res = {"blob_KB": round(blob.size * 8 / 1024, 1), "tables": len(tables), "claims": int(tr.size), "permutations": int(perms), "staged_MB": round(staged.size * 8 / 2**20, 2),
       "host_verify_ms": [round(v, 3) for v in host], "dev_verify_ms": [round(v, 3) for v in dev], "host_mean_ms": mean(host), "dev_mean_ms": mean(dev),
       "host_spread_ms": round(max(host) - min(host), 3), "dev_spread_ms": round(max(dev) - min(dev), 3),
       "delegated_replay_of_all_tables_ms": round(replay_ms, 3),
       "merkle_check_host_checks_copies_kernel_ms": [round(v, 3) for v in check_ms], "same_words_uploaded_alone_ms": [round(v, 3) for v in copy_ms],
       "k_merkle_check_ms_at_most": round(mean(check_ms) - mean(copy_ms), 3),
       "environment": {k: os.environ.get(k) for k in ("VX_TABLE_STREAMS", "GPU_MAX_HW_QUEUES")}}
res["g_permutations_per_s_at_least"] = round(perms / max(res["k_merkle_check_ms_at_most"], 1e-6) / 1e6, 3)
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
