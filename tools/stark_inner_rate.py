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

import numpy as np
import stark_rate_common as R
from oracle import blake_air as B
from oracle import stark_ref as S

import stark_queries_ref as Z
import transcript_ref as T

r = R.setup()
vx, ctx, cfg, proof, chal, head = r.vx, r.ctx, r.cfg, r.proof, r.chal, r.head
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

env = {k: os.environ.get(k) for k in ("VX_TABLE_STREAMS", "GPU_MAX_HW_QUEUES")}
res = {"shape_LN_cm_ca_a_NL_cap_queries": shape, "tables_log2_rows": logs, "n_obs": n_obs, "n_chal": len(claims), "verifier_permutations": perms,
       "stream_mode": vx.lib.table_streams_mode(env["VX_TABLE_STREAMS"], env["GPU_MAX_HW_QUEUES"]), "environment": env,
       "inner_proof_KB": round(proof.size * 8 / 1024, 1), "head_KB": round(head.size * 8 / 1024, 1), "blob_KB": round(out.size * 8 / 1024, 1),
       "queries_blob_KB": round(o_qry.size * 8 / 1024, 1), "transcripts_blob_KB": round(o_trn.size * 8 / 1024, 1)}
res["inner_prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.stark_inner_prove(proof, cfg, ext_chal=chal, out=out))
res["queries_prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.stark_queries_prove(proof, cfg, ext_chal=chal, out=o_qry))
res["transcripts_prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.stark_transcripts_prove([proof], cfg, [chal], out=o_trn))
res["inner_verify_head_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.stark_inner_verify(out, head, cfg, ext_chal=chal))
res["queries_verify_head_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.stark_queries_verify(o_qry, head, cfg, ext_chal=chal))
print(json.dumps(res))
