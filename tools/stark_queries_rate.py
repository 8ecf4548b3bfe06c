#!/usr/bin/env python3
"""vx_stark_queries_prove end to end on one GPU on the inner proof tools/stark_openings_rate.py uses: the one hash-chain segment of a
header_range_256 proof (BlakeChainAir: 745 main and 276 auxiliary columns, 84 queries, a 2^21 LDE, four fold layers), taken out of a
real vx_header_range_prove blob together with the lookup challenges its tables shared.  One JSON line: the shape, the degree bits of
the group's tables, the sizes (inner proof, its head, the blob) and milliseconds averaged over `reps` calls after a warm-up call --
vx_stark_queries_prove as a whole, vx_stark_queries_verify on the head alone, and beside them the two groups this one replaces, on
the same proof: vx_stark_openings_prove and vx_fri_combine_fold_prove (its claims are read out of the proof by
tests/stark_queries_ref.py, outside the timed region)."""
import json

import numpy as np
import stark_rate_common as R
from oracle import blake_air as B
from oracle import stark_ref as S

import stark_queries_ref as Z

r = R.setup()
vx, ctx, cfg, proof, chal, head = r.vx, r.ctx, r.cfg, r.proof, r.chal, r.head
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

res = {"shape_LN_cm_ca_a_NL_cap_queries": cl["shape"], "tables_log2_rows": logs, "inner_proof_KB": round(proof.size * 8 / 1024, 1), "head_KB": round(head.size * 8 / 1024, 1),
       "blob_KB": round(out.size * 8 / 1024, 1), "openings_blob_KB": round(o_open.size * 8 / 1024, 1), "combine_fold_blob_KB": round(o_fold.size * 8 / 1024, 1)}
res["queries_prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.stark_queries_prove(proof, cfg, ext_chal=chal, out=out))
res["queries_verify_head_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.stark_queries_verify(out, head, cfg, ext_chal=chal))
res["openings_prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.stark_openings_prove(proof, cfg, ext_chal=chal, out=o_open))
res["combine_fold_prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.fri_combine_fold_prove(*fold_args, cfg, out=o_fold))
res["openings_verify_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.stark_openings_verify(o_open, proof, cfg, ext_chal=chal))
print(json.dumps(res))
