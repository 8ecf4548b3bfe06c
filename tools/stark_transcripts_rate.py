#!/usr/bin/env python3
"""vx_stark_transcripts_prove end to end on one GPU on the proofs of a real header_range_256 request (256 P15k headers with a
justification: hash chain, authority commitment, Merkle roots, Ed25519, SHA-512 -- five tables under shared lookup challenges), for
the hash-chain proof alone (one chain) and for all five (five chains).  One JSON line per input: the chains' words, challenges and
blocks, the table's degree bits, blob words against head words, and milliseconds averaged over `reps` calls after a warm-up call:
the TranscriptAir witness as a whole by HIP events on the context's stream (upload, k_transcript_states, k_transcript_trace, the
challenges back), vx_stark_transcripts_prove from whole proofs and from heads (wall), vx_stark_transcripts_verify on heads (host,
wall) and, for scale, the host replay alone (vx_stark_transcript_claims on a head).  The duration of k_transcript_states alone is
read from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/stark_transcripts_rate.py)."""
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
from oracle import stark_ref as S  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
reps, N = 5, 256
ch = vx.synth.Chain(N, profile="P15k")
cfg = ctx.stark_config()
just = vx.lib.PackedJustification(vx.synth.Justification(ch.target_block, ch.target_hash, n_auth=6), 8)
out96, blob = ctx.header_range_prove(ctx.from_host(ch.headers), ch.stride, ch.sizes, N, ch.trusted_block, ch.trusted_hash, ch.target_block, cfg, just=just)
p_blake, p_sha, p_tree, p_ed, p_h = (np.array(p, dtype=np.uint64) for p in vx.lib.split_blob(blob))
order = [p_blake, p_tree, p_sha, p_ed, p_h]  # bus order
chal = S.shared_challenges_n([S.proof_peek(p, cfg.cap_height) for p in order], 4)


def timed_wall(fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3)


def timed_events(fn):
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return round(ctx.timer_stop() / reps, 3)


for name, proofs in (("hash_chain", [p_blake]), ("all_five", order)):
    exts = [chal] * len(proofs)
    heads = [vx.lib.stark_proof_head(p, cfg) for p in proofs]
    claims = [vx.lib.stark_transcript_claims(h, cfg, chal) for h in heads]
    out = ctx.stark_transcripts_prove(proofs, cfg, exts)  # warm-up (pool, side contexts)
    vx.lib.stark_transcripts_verify(out, proofs, cfg, exts)
    vx.lib.stark_transcripts_verify(out, heads, cfg, exts)
    assert (ctx.stark_transcripts_prove(heads, cfg, exts) == out).all()
    at = 2
    for _ in proofs:
        at += 2 + 2 * int(out[at + 1])
    log_n = int(out[at + 1 + 2])
    # the witness alone: the chains' run lengths from the claims (a challenge run ends where the absorbed count moves)
    ops, words = [], []
    for w, c in claims:
        o, seen = [], 0
        for a, _ in c:
            a = int(a)
            if a != seen or not o:
                o += [a - seen, 0]
                seen = a
            o[-1] += 1
        ops.append(o), words.append(w)
    tb, _, drawn = ctx.transcript_air_trace(ops, words, log_n)
    assert all((d == c[:, 1]).all() for d, (_, c) in zip(drawn, claims))
    res = {"input": name, "chains": len(proofs), "n_obs": [int(w.size) for w, _ in claims], "n_chal": [int(c.shape[0]) for _, c in claims], "table_log2_rows": log_n,
           "blob_words": int(out.size), "table_proof_words": int(out[at]), "claim_words": at, "head_words": [int(h.size) for h in heads], "proof_words": [int(p.size) for p in proofs]}
    res["witness_events_ms"] = timed_events(lambda: ctx.transcript_air_trace(ops, words, log_n, out=tb))
    res["prove_whole_wall_ms"] = timed_wall(lambda: ctx.stark_transcripts_prove(proofs, cfg, exts, out=out))
    res["prove_heads_wall_ms"] = timed_wall(lambda: ctx.stark_transcripts_prove(heads, cfg, exts, out=out))
    res["verify_heads_host_ms"] = timed_wall(lambda: vx.lib.stark_transcripts_verify(out, heads, cfg, exts))
    res["replay_heads_host_ms"] = timed_wall(lambda: [vx.lib.stark_transcript_claims(h, cfg, chal) for h in heads])
    res["plain_verify_whole_host_ms"] = timed_wall(lambda: vx.lib.header_range_verify(blob, N, ch.trusted_block, ch.trusted_hash, ch.target_block, out96, cfg,
                                                                                      authority_set_hash=just.sh.tobytes(), authority_set_id=just.struct.authority_set_id)) if name == "all_five" else None
    tb.free()
    print(json.dumps(res))
