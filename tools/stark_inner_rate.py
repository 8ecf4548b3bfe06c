#!/usr/bin/env python3
"""vx_stark_inner_prove end to end on one GPU on the inner proof tools/stark_queries_rate.py uses: the one hash-chain segment of a
header_range_256 proof (BlakeChainAir: 745 main and 276 auxiliary columns, 84 queries, a 2^21 LDE, four fold layers), taken out of a
real vx_header_range_prove blob together with the lookup challenges its tables shared.  One JSON line: the shape, the degree bits of
the group's tables, n_obs and n_chal, the sizes (inner proof, its head, the three blobs), the permutation counts of the verifier --
the one statement digest of the joined group against the replay of the inner transcript plus the query-phase digest -- and
milliseconds averaged over `reps` calls after a warm-up call: vx_stark_inner_prove as a whole; beside it, on the same proof and each
by itself, the two groups it joins (vx_stark_queries_prove, vx_stark_transcripts_prove); vx_stark_inner_verify on the head alone
beside vx_stark_queries_verify on the head alone.  The stream mode of the run is recorded with it."""
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
import transcript_ref as T  # noqa: E402

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
out = ctx.stark_inner_prove(proof, cfg, ext_chal=chal)  # warm-up (pool, side contexts)
vx.lib.stark_inner_verify(out, proof, cfg, ext_chal=chal)
vx.lib.stark_inner_verify(out, head, cfg, ext_chal=chal)
shape, n_obs, claims, tables = vx.lib.split_stark_inner(out)
logs = [int(p[2]) for p in tables]
o_qry = ctx.stark_queries_prove(proof, cfg, ext_chal=chal)
o_trn = ctx.stark_transcripts_prove([proof], cfg, [chal])
vx.lib.stark_queries_verify(o_qry, head, cfg, ext_chal=chal)
# the verifier's permutations: hash_n_to_hash_no_pad absorbs 8 words per permutation; the replay duplexes once per block of the plan
S.register_air(B.BlakeChainAir)
cl, hd, _, _, _ = Z.claims(proof, None, chal)
ops, seen = [], 0
for a, _ in claims:  # the chain's run lengths from the claims (a challenge run ends where the absorbed count moves)
    a = int(a)
    if a != seen or not ops:
        ops += [a - seen, 0]
        seen = a
    ops[-1] += 1
queries_digest_words = 7 + 4 + sum(np.asarray(hd[k]).size for k in ("ol", "on", "oq", "betas", "fpoly")) + 4 * len(cl["trees"]) + len(cl["index"])
perms = {"inner_digest": -(-(9 + n_obs + 2 * len(claims)) // 8), "transcript_replay": len(T.plan(ops)), "queries_digest": -(-queries_digest_words // 8)}


def timed_wall(fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 2)


env = {k: os.environ.get(k) for k in ("VX_TABLE_STREAMS", "GPU_MAX_HW_QUEUES")}
res = {"shape_LN_cm_ca_a_NL_cap_queries": shape, "tables_log2_rows": logs, "n_obs": n_obs, "n_chal": len(claims), "verifier_permutations": perms,
       "stream_mode": vx.lib.table_streams_mode(env["VX_TABLE_STREAMS"], env["GPU_MAX_HW_QUEUES"]), "environment": env,
       "inner_proof_KB": round(proof.size * 8 / 1024, 1), "head_KB": round(head.size * 8 / 1024, 1), "blob_KB": round(out.size * 8 / 1024, 1),
       "queries_blob_KB": round(o_qry.size * 8 / 1024, 1), "transcripts_blob_KB": round(o_trn.size * 8 / 1024, 1)}
res["inner_prove_wall_ms"] = timed_wall(lambda: ctx.stark_inner_prove(proof, cfg, ext_chal=chal, out=out))
res["queries_prove_wall_ms"] = timed_wall(lambda: ctx.stark_queries_prove(proof, cfg, ext_chal=chal, out=o_qry))
res["transcripts_prove_wall_ms"] = timed_wall(lambda: ctx.stark_transcripts_prove([proof], cfg, [chal], out=o_trn))
res["inner_verify_head_host_ms"] = timed_wall(lambda: vx.lib.stark_inner_verify(out, head, cfg, ext_chal=chal))
res["queries_verify_head_host_ms"] = timed_wall(lambda: vx.lib.stark_queries_verify(o_qry, head, cfg, ext_chal=chal))
print(json.dumps(res))
