#!/usr/bin/env python3
"""Which hardware queue every stream of a rocprofv3 (rocpd sqlite) kernel trace ran on: launches, kernel time and host threads per
(stream, queue).  The runtime gives a new stream the least-used queue, and a stream nobody meant to make (the null stream) takes one
too: this is where one sees that two proofs share a queue (profiles/README.md, `r17_*`).
usage: rocpd_lanes.py <results.db or directory>"""
import glob
import sqlite3
import sys

db = sys.argv[1]
if not db.endswith(".db"):
    db = glob.glob(db + "/**/*.db", recursive=True)[0]
con = sqlite3.connect(db)
cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
if "stream_id" not in cols or "queue_id" not in cols:
    sys.exit(f"this trace has no stream_id / queue_id columns (kernels: {cols})")
rows = con.execute("select stream_id, queue_id, count(*), sum(end - start) / 1e6, count(distinct tid) from kernels group by stream_id, queue_id order by stream_id, queue_id").fetchall()
print("--- streams and the hardware queues they ran on (kernels table of the trace: stream_id, queue_id), whole trace:")
for s, q, n, ms, th in rows:
    print(f"stream {s:2d} -> queue {q}: {n:5d} launches, {ms:8.1f} ms of kernels, {th} host threads")
