"""What tools/stark_openings_rate.py, stark_queries_rate.py and stark_inner_rate.py share: the inner proof they measure on -- the one
hash-chain segment of a header_range_256 proof (BlakeChainAir: 745 main and 276 auxiliary columns, 84 queries, a 2^21 LDE, four fold
layers), taken out of a real vx_header_range_prove blob together with the lookup challenges its tables shared, and its head -- and
their wall-clock timer.  Importing it builds the oracle and puts the repository and tests/ on sys.path."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vx_import  # noqa: E402
from oracle import oracle as O  # noqa: E402

O.build()
from oracle import stark_ref as S  # noqa: E402

REPS, N = 5, 256


def setup():
    """-> vx, ctx, cfg, the synthetic chain `ch`, the header_range output `out96` and `blob`, the inner `proof`, the shared
    challenges `chal` it was made under and its `head`"""
    vx = vx_import.load()
    ctx = vx.Context(0)
    ch = vx.synth.Chain(N, profile="P15k")
    cfg = ctx.stark_config()
    out96, blob = ctx.header_range_prove(ctx.from_host(ch.headers), ch.stride, ch.sizes, N, ch.trusted_block, ch.trusted_hash, ch.target_block, cfg)
    segs, p_sha, p_tree, p_ed, p_h = vx.lib.split_blob_segments(blob)
    assert len(segs) == 1 and p_sha.size == 0
    proof = np.array(segs[0], dtype=np.uint64)
    chal = S.shared_challenges_n([S.proof_peek(p, cfg.cap_height) for p in (proof, p_tree)], 4)  # bus order: segments, Merkle
    return SimpleNamespace(vx=vx, ctx=ctx, cfg=cfg, ch=ch, out96=out96, blob=blob, proof=proof, chal=chal, head=vx.lib.stark_proof_head(proof, cfg))


def timed_wall(ctx, fn):
    """milliseconds per call, averaged over REPS calls and one sync"""
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / REPS, 2)
