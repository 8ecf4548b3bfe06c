#!/usr/bin/env python3
"""vx_stark_openings_prove end to end on one GPU on a hash-chain-shaped inner proof: the one hash-chain segment of a header_range_256
proof (BlakeChainAir: 745 main and 276 auxiliary columns, 84 queries, a 2^21 LDE, four fold layers), taken out of a real
vx_header_range_prove blob together with the lookup challenges its tables shared.  One JSON line: the shape and the degree bits of
the group's tables, and milliseconds averaged over `reps` calls after a warm-up call -- vx_stark_openings_prove as a whole (the
inner proof verified on the host, the sponge chains and the paths walked on the device, the tables proven under shared challenges),
vx_stark_merkle_claims alone (the host share of it), vx_stark_openings_verify and, for scale, vx_stark_verify_ext's work on the
same proof as the header_range verifier does it (every path walked on the host): the inner proof's claims extraction is that
verifier minus the paths."""
import json

import stark_rate_common as R

r = R.setup()
vx, ctx, cfg, ch, out96, blob, proof, chal, N = r.vx, r.ctx, r.cfg, r.ch, r.out96, r.blob, r.proof, r.chal, R.N
out = ctx.stark_openings_prove(proof, cfg, ext_chal=chal)  # warm-up (pool, side contexts)
vx.lib.stark_openings_verify(out, proof, cfg, ext_chal=chal)
mc = vx.lib.stark_merkle_claims(proof, cfg, ext_chal=chal)
n_tab = int(out[vx.lib.SOPEN_HDR - 1])
at, logs = vx.lib.SOPEN_HDR + n_tab, []
for k in range(n_tab):
    logs.append(int(out[at + 2]))
    at += int(out[vx.lib.SOPEN_HDR + k])

res = {"shape_LN_cm_ca_a_NL_cap_queries": mc["shape"], "claims": int(mc["tree"].size), "tables_log2_rows": logs, "inner_proof_KB": round(proof.size * 8 / 1024, 1),
       "sibling_KB": round(sum(s.size for s in mc["siblings"]) * 8 / 1024, 1), "blob_KB": round(out.size * 8 / 1024, 1)}
res["prove_wall_ms"] = R.timed_wall(ctx, lambda: ctx.stark_openings_prove(proof, cfg, ext_chal=chal, out=out))
res["claims_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.stark_merkle_claims(proof, cfg, ext_chal=chal))
res["verify_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.stark_openings_verify(out, proof, cfg, ext_chal=chal))
res["header_range_verify_host_ms"] = R.timed_wall(ctx, lambda: vx.lib.header_range_verify(blob, N, ch.trusted_block, ch.trusted_hash, ch.target_block, out96, cfg))
print(json.dumps(res))
