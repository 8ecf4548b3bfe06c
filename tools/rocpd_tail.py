#!/usr/bin/env python3
"""The small kernels at the end of the kernel list (tree tops, query-phase gathers, runtime copies) in a rocprofv3 (rocpd sqlite)
kernel trace of `bench.py --inflight 1`: launches and kernel time per proof, and for every launch how long it WAITED (from the end
of the kernel before it on the same stream, i.e. the moment it could have started, to its own start) against how long it RAN.
usage: rocpd_tail.py <results.db or directory> [n_proofs_in_trace] [kernel,kernel,...  (these instead of the tail kernels)]"""
import glob
import sqlite3
import sys

TAIL = ("k_merkle_top", "k_merkle_level_coop", "k_merkle_level", "k_hash_leaves_coop", "k_gather_siblings", "k_gather_rows", "k_fri_gather_leaves",
        "__amd_rocclr_copyBuffer")

if len(sys.argv) > 3:
    TAIL = tuple(sys.argv[3].split(","))
db = sys.argv[1]
if not db.endswith(".db"):
    db = glob.glob(db + "/**/*.db", recursive=True)[0]
con = sqlite3.connect(db)
cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
lane = next((c for c in ("stream_id", "queue_id", "stream", "queue", "tid") if c in cols), None)  # what orders dependent launches
rows = con.execute(f"select name, start, end, {lane or '0'} from kernels order by start").fetchall()
end_i = next((i for i, r in enumerate(rows) if r[0].startswith("k_fill_random")), len(rows))  # bench.py's micro-benchmarks follow
rows = rows[:end_i]
n_proofs = int(sys.argv[2]) if len(sys.argv) > 2 else max(1, sum(1 for r in rows if r[0].startswith("k_blake2b_256")))
short = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").split("<")[0]
last_end, agg = {}, {}
for nm, s, e, ln in rows:
    k = short(nm)
    if k in TAIL:
        a = agg.setdefault(k, [0, 0.0, 0.0, []])
        a[0] += 1
        a[1] += (e - s) / 1e3
        if ln in last_end:
            a[2] += max(0, s - last_end[ln]) / 1e3
        a[3].append((e - s) / 1e3)
    last_end[ln] = max(e, last_end.get(ln, 0))
print(f"--- {n_proofs} proofs in the trace, dependent launches ordered by `{lane}`; per proof:")
print(f"{'kernel':28s} {'launches':>8s} {'running ms':>11s} {'waiting ms':>11s} {'median us':>10s} {'max us':>9s}")
for k in TAIL:
    if k in agg:
        n, run, wait, ds = agg[k]
        ds.sort()
        print(f"{k:28s} {n / n_proofs:8.1f} {run / n_proofs / 1e3:11.2f} {wait / n_proofs / 1e3:11.2f} {ds[len(ds) // 2]:10.1f} {ds[-1]:9.1f}")
