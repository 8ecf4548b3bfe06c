#!/usr/bin/env python3
"""FriFoldAir end to end on one GPU at the shape of one STARK proof's query phase: 84 queries of a 2^21 LDE, four fold layers, five
index bits left = 756 rows in one 2^10-row table; the claims are cut from a FRI commit phase the reference runs on a random
polynomial (tests/fri_fold_ref.py).  One JSON line, milliseconds averaged over `reps` calls after a warm-up call: the witness
(vx_fri_fold_air_trace: upload, k_fri_fold_trace, the claims digest on the host), the auxiliary columns (k_bus_aux<FriFoldAir> + the scan),
the table's STARK with its auxiliary round from a ready trace (vx_stark_prove), vx_fri_fold_prove as a whole (host fold check
included), the claims digest alone (the C oracle's hash_n_to_hash_no_pad over the same words), vx_fri_fold_verify on the host, and
-- the work the table proves -- the same 84 x 4 coset interpolations by the C oracle's compute_evaluation, the Lagrange loop of
vx_stark_verify."""
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
import fri_fold_ref as F  # noqa: E402

vx = vx_import.load()
ctx = vx.Context(0)
LN, NL, reps = 21, 4, 10
betas, fpoly, layers = F.commit_phase(LN, NL, seed=84)
index = [int(v) for v in np.random.default_rng(84).integers(0, 1 << LN, size=84)]
ev0, leaves = F.claims_from(layers, index)
tb, pub = ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, 10)  # warm-up (pool, tables)
blob = ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves)
vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, leaves)
ctx.stark_prove(vx.lib.VX_AIR_FRI_FOLD, tb, 10, pub)
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


words = np.concatenate([np.concatenate([np.array([i], dtype=np.uint64), e, lv.reshape(-1)]) for i, e, lv in zip(index, ev0, leaves)])
assert [int(v) for v in O.hash_no_pad(words)] == [int(v) for v in pub[20:]]


calls = []  # (x_l, within_l, leaf_l, beta_l) of every (query, layer): the points are prepared outside the timed loop
for i, lv in zip(index, leaves):
    x = 7 * pow(O.root(LN), F.brev(i, LN), F.P) % F.P
    for l in range(NL):
        calls.append((x, (i >> (4 * l)) & 15, np.ascontiguousarray(lv[l]).reshape(-1), np.array(betas[l], dtype=np.uint64)))
        x = pow(x, 16, F.P)
got = O.fri_compute_evaluation(calls[NL - 1][0], calls[NL - 1][1], 4, calls[NL - 1][2], calls[NL - 1][3])
want = F.final_eval(fpoly, index[0], LN, NL)
assert [int(v) for v in got] == [want.a, want.b]


def host_loop():  # 336 calls through ctypes: an upper bound of the C loop
    for x, w, lf, be in calls:
        O.fri_compute_evaluation(x, w, 4, lf, be)


out = {"queries": 84, "log_lde": LN, "layers": NL, "rows_log2": int(blob[F.HDR + 2]), "blob_KB": round(blob.size * 8 / 1024, 1), "claim_words": int(words.size)}
out["witness_ms"] = timed_events(lambda: ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, 10, out=tb))
out["witness_wall_ms"] = timed_wall(lambda: ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, 10, out=tb))
out["aux_ms"] = timed_events(lambda: ctx.stark_aux_trace(vx.lib.VX_AIR_FRI_FOLD, tb, 10, F.CHAL, vx.lib.VX_FRI_FOLD_AIR_AUX_COLS, pub)[0].free())
out["stark_with_aux_ms"] = timed_events(lambda: ctx.stark_prove(vx.lib.VX_AIR_FRI_FOLD, tb, 10, pub))
out["prove_ms"] = timed_events(lambda: ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves))
out["prove_wall_ms"] = timed_wall(lambda: ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves))
out["claims_digest_host_ms"] = timed_wall(lambda: O.hash_no_pad(words))
out["verify_host_ms"] = timed_wall(lambda: vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, leaves))
out["host_fold_loop_of_the_84_queries_ms"] = timed_wall(host_loop)
print(json.dumps(out))
