#!/usr/bin/env python3
"""What a run-time table's auxiliary round costs: vx_stark_aux_trace of a table restated as a program with DECLARED bus messages
(k_bus_aux_prog, the interpreter: tests/bus_programs.py) against the compiled table's k_bus_aux<Air> on the same trace and
challenges -- LeafNoopAir at 2^16 rows, TranscriptAir at 2^15, FriFoldAir at 2^15.  The two alternate, five runs each; a run is the
HIP-event time of 20 calls after a warm-up call, in milliseconds per call.  One JSON line: per table the runs, their means, spreads
(max - min) and the ratio of the means (profiles/r12_bus_aux_prog.json)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vx_import  # noqa: E402
import bus_programs as BP  # noqa: E402
import fri_fold_ref as F  # noqa: E402
import transcript_ref as T  # noqa: E402

vx = vx_import.load()
L = vx.lib
ctx = vx.Context(0)
P = 2**64 - 2**32 + 1
CHAL = F.CHAL
REPS, RUNS = 20, 5
rng = np.random.default_rng(84)
out = {}


def timed(air, tb, log_n, cols, pub):
    ctx.stark_aux_trace(air, tb, log_n, CHAL, cols, pub)[0].free()  # warm-up
    ctx.sync()
    ctx.timer_start()
    for _ in range(REPS):
        ctx.stark_aux_trace(air, tb, log_n, CHAL, cols, pub)[0].free()
    return round(ctx.timer_stop() / REPS, 4)


def compare(name, compiled, restated, tb, log_n, cols, pub):
    prog = restated.register()
    a, b = ctx.stark_aux_trace(compiled, tb, log_n, CHAL, cols, pub), ctx.stark_aux_trace(prog, tb, log_n, CHAL, cols, pub)
    assert (a[0].download() == b[0].download()).all() and (a[1] == b[1]).all(), name  # the same words, or the times mean nothing
    a[0].free(), b[0].free()
    runs = {"compiled": [], "interpreted": []}
    for _ in range(RUNS):
        runs["compiled"].append(timed(compiled, tb, log_n, cols, pub))
        runs["interpreted"].append(timed(prog, tb, log_n, cols, pub))
    res = {"runs_ms": runs}
    for k, v in runs.items():
        res[k + "_mean_ms"], res[k + "_spread_ms"] = round(float(np.mean(v)), 4), round(max(v) - min(v), 4)
    res["interpreted_over_compiled"] = round(res["interpreted_mean_ms"] / res["compiled_mean_ms"], 3)
    out[name] = res
    L.air_unregister(prog)


# LeafNoopAir: 60000 openings of 1..4 words, 2^16 rows
n = 60000
rows = [[int(v) for v in r[: 1 + i % 4]] for i, r in enumerate(rng.integers(0, P, size=(n, 4), dtype=np.uint64))]
tb, pub = ctx.leaf_noop_air_trace([8 + i % 3 for i in range(n)], [int(v) for v in rng.integers(0, 1 << 24, size=n)], rows, 16)
compare("leaf_noop_2^16", L.VX_AIR_LEAF_NOOP, BP.leaf_noop(), tb, 16, L.VX_LEAF_NOOP_AIR_AUX_COLS, pub)
tb.free()

# TranscriptAir: one chain of 1000 duplexes, 2^15 rows (1024 blocks)
chains = [T.filler(1000, seed=50)]
tb, pub, _ = ctx.transcript_air_trace([ops for ops, _ in chains], [w for _, w in chains], 15)
compare("transcript_2^15", L.VX_AIR_TRANSCRIPT, BP.transcript(), tb, 15, L.VX_TRANSCRIPT_AIR_AUX_COLS, pub)
tb.free()

# FriFoldAir: 3600 queries, LN 21, four layers (9 rows a query), 2^15 rows, TREE0 3 (the witness checks ranges only)
LN, NL, nq = 21, 4, 3600
index = [int(v) for v in rng.integers(0, 1 << LN, size=nq)]
betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
leaves = rng.integers(0, P, size=(nq, NL, 16, 2), dtype=np.uint64)
ev0 = rng.integers(0, P, size=(nq, 2), dtype=np.uint64)
tb, pub = ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, 15, 3)
compare("fri_fold_2^15", L.VX_AIR_FRI_FOLD, BP.fri_fold(), tb, 15, L.VX_FRI_FOLD_AIR_AUX_COLS, pub)
tb.free()
print(json.dumps(out))
