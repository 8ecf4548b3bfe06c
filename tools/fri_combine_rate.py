#!/usr/bin/env python3
"""FriCombineAir end to end on one GPU at the shape of the hash-chain table's query phase: 84 queries of 745 + 276 + 4 row words over
a 2^21 LDE = 1046 rows per query in one 2^17-row table; random consistent claims (tests/fri_combine_ref.py).  One JSON line,
milliseconds averaged over `reps` calls after a warm-up call: the witness (vx_fri_combine_air_trace: upload, the powers of alpha,
k_fri_combine_trace, the claims digest on the host), the auxiliary columns (k_bus_aux<FriCombineAir> + the scan), the table's STARK with its
auxiliary round from a ready trace (vx_stark_prove), vx_fri_combine_prove as a whole (host combination check included), the claims
digest alone (the C oracle's hash_n_to_hash_no_pad over the same words), vx_fri_combine_verify on the host, and -- the work the table
proves -- the host combination loop of the 84 queries: vx_fri_combine_prove's native check, timed by handing it a wrong ev_0 for the
LAST query, which it refuses after combining all of them and before anything reaches the GPU."""
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
import fri_combine_ref as K  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
LN, cm, ca, nq, reps, LOG_N = 21, 745, 276, 4, 10, 17
st = K.rand_statement(LN, cm, ca, nq, seed=84)
index = [int(v) for v in np.random.default_rng(84).integers(0, 1 << LN, size=84)]
rows, ev0 = K.rand_claims(st, index)
a = (LN, cm, ca, nq, st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"])
tb, pub = ctx.fri_combine_air_trace(LN, st["r"], *a[1:], index, rows, ev0, LOG_N, K.TREE0)  # warm-up (pool, tables)
blob = ctx.fri_combine_prove(*a, index, rows, ev0)
vx.lib.fri_combine_verify(blob, *a, index, rows, ev0)
ctx.stark_prove(vx.lib.VX_AIR_FRI_COMBINE, tb, LOG_N, pub)
ctx.sync()


def timed_events(fn):
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return round(ctx.timer_stop() / reps, 3)


def timed_wall(fn):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return round(1e3 * (time.perf_counter() - t0) / reps, 3)


words = np.array(K.statement_words(st, len(index)) + [int(v) for i, rw, e in zip(index, rows, ev0) for v in [i] + list(rw) + list(e)], dtype=np.uint64)
assert [int(v) for v in O.hash_no_pad(words)] == [int(v) for v in pub[K.PUB_DIGEST:]]
bad_ev0 = ev0.copy()
bad_ev0[-1, 0] ^= np.uint64(1)


def host_loop():
    try:
        ctx.fri_combine_prove(*a, index, rows, bad_ev0, out=blob)
    except vx.VxError as e:
        assert e.code == -5 and "query 83" in str(e)
    else:
        raise AssertionError("a wrong ev_0 was proven")


out = {"queries": 84, "log_lde": LN, "row_words": cm + ca + nq, "rows_log2": int(blob[K.HDR + 2]), "blob_KB": round(blob.size * 8 / 1024, 1), "claim_words": int(words.size)}
out["witness_ms"] = timed_events(lambda: ctx.fri_combine_air_trace(LN, st["r"], *a[1:], index, rows, ev0, LOG_N, K.TREE0, out=tb))
out["witness_wall_ms"] = timed_wall(lambda: ctx.fri_combine_air_trace(LN, st["r"], *a[1:], index, rows, ev0, LOG_N, K.TREE0, out=tb))
out["aux_ms"] = timed_events(lambda: ctx.stark_aux_trace(vx.lib.VX_AIR_FRI_COMBINE, tb, LOG_N, K.CHAL, vx.lib.VX_FRI_COMBINE_AIR_AUX_COLS, pub)[0].free())
out["stark_with_aux_ms"] = timed_events(lambda: ctx.stark_prove(vx.lib.VX_AIR_FRI_COMBINE, tb, LOG_N, pub))
out["prove_ms"] = timed_events(lambda: ctx.fri_combine_prove(*a, index, rows, ev0))
out["prove_wall_ms"] = timed_wall(lambda: ctx.fri_combine_prove(*a, index, rows, ev0))
out["claims_digest_host_ms"] = timed_wall(lambda: O.hash_no_pad(words))
out["verify_host_ms"] = timed_wall(lambda: vx.lib.fri_combine_verify(blob, *a, index, rows, ev0))
out["host_combine_loop_of_the_84_queries_ms"] = timed_wall(host_loop)
print(json.dumps(out))
