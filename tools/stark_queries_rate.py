#!/usr/bin/env python3
"""vx_stark_queries_prove end to end on one GPU on the inner proof tools/stark_openings_rate.py uses: the one hash-chain segment of a
header_range_256 proof (BlakeChainAir: 745 main and 276 auxiliary columns, 84 queries, a 2^21 LDE, four fold layers), taken out of a
real vx_header_range_prove blob together with the lookup challenges its tables shared.  One JSON line: the shape, the degree bits of
the group's tables, the sizes (inner proof, its head, the blob) and milliseconds averaged over `reps` calls after a warm-up call --
vx_stark_queries_prove as a whole, vx_stark_queries_verify on the head alone, and beside them the two groups this one replaces, on
the same proof: vx_stark_openings_prove and vx_fri_combine_fold_prove (its claims are read out of the proof by
tests/stark_queries_ref.py, outside the timed region)."""
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
from oracle import blake_air as B  # noqa: E402
from oracle import stark_ref as S  # noqa: E402

import stark_queries_ref as Z  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
reps, N = 5, 256
ch = vx.synth.Chain(N, profile="P15k")
cfg = ctx.stark_config()
out96, blob = ctx.header_range_prove(ctx.from_host(ch.headers), ch.stride, ch.sizes, N, ch.trusted_block, ch.trusted_hash, ch.target_block, cfg)
segs, p_sha, p_tree, p_ed, p_h = vx.lib.split_blob_segments(blob)
assert len(segs) == 1 and p_sha.size == 0
proof = np.array(segs[0], dtype=np.uint64)
chal = S.shared_challenges_n([S.proof_peek(p, cfg.cap_height) for p in (proof, p_tree)], 4)  # bus order: segments, Merkle
head = vx.lib.stark_proof_head(proof, cfg)
out = ctx.stark_queries_prove(proof, cfg, ext_chal=chal)  # warm-up (pool, side contexts)
vx.lib.stark_queries_verify(out, proof, cfg, ext_chal=chal)
vx.lib.stark_queries_verify(out, head, cfg, ext_chal=chal)
n_tab = int(out[Z.HDR - 1])
at, logs = Z.HDR + n_tab, []
for k in range(n_tab):
    logs.append(int(out[at + 2]))
    at += int(out[Z.HDR + k])
S.register_air(B.BlakeChainAir)
cl, hd, st, rows, leaves = Z.claims(proof, None, chal)
fold_args = (st["LN"], st["cm"], st["ca"], st["nq"], st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"], np.array(hd["betas"], dtype=np.uint64), hd["fpoly"],
             np.array(cl["index"], dtype=np.uint64), rows, leaves)
o_open = ctx.stark_openings_prove(proof, cfg, ext_chal=chal)
o_fold = ctx.fri_combine_fold_prove(*fold_args, cfg)


def timed_wall(fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 2)


res = {"shape_LN_cm_ca_a_NL_cap_queries": cl["shape"], "tables_log2_rows": logs, "inner_proof_KB": round(proof.size * 8 / 1024, 1), "head_KB": round(head.size * 8 / 1024, 1),
       "blob_KB": round(out.size * 8 / 1024, 1), "openings_blob_KB": round(o_open.size * 8 / 1024, 1), "combine_fold_blob_KB": round(o_fold.size * 8 / 1024, 1)}
res["queries_prove_wall_ms"] = timed_wall(lambda: ctx.stark_queries_prove(proof, cfg, ext_chal=chal, out=out))
res["queries_verify_head_host_ms"] = timed_wall(lambda: vx.lib.stark_queries_verify(out, head, cfg, ext_chal=chal))
res["openings_prove_wall_ms"] = timed_wall(lambda: ctx.stark_openings_prove(proof, cfg, ext_chal=chal, out=o_open))
res["combine_fold_prove_wall_ms"] = timed_wall(lambda: ctx.fri_combine_fold_prove(*fold_args, cfg, out=o_fold))
res["openings_verify_host_ms"] = timed_wall(lambda: vx.lib.stark_openings_verify(o_open, proof, cfg, ext_chal=chal))
print(json.dumps(res))
