#!/usr/bin/env python3
"""Per-launch durations of the lookup-multiplicity kernels in a rocprofv3 (rocpd sqlite) kernel trace of `bench.py --inflight 1`:
min / median / max per kernel, and of the sum per proof of {k_blake_trace, k_blake_count, k_blake_mult} and {k_ed_hist, k_ed_mult}.
usage: rocpd_kernel_sums.py <results.db or directory> [launches_to_skip=2]"""
import glob, sqlite3, sys
db = sys.argv[1]
if not db.endswith(".db"):
    db = glob.glob(db + "/**/*.db", recursive=True)[0]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 2
con = sqlite3.connect(db)
rows = con.execute("select name, start, end from kernels order by start").fetchall()
short = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").split("<")[0]
groups = {"blake": ("k_blake_trace", "k_blake_count", "k_blake_mult"), "ed": ("k_ed_hist", "k_ed_mult")}
per = {}
for nm, s, e in rows:
    k = short(nm)
    if any(k in g for g in groups.values()):
        per.setdefault(k, []).append((e - s) / 1e3)
for g, names in groups.items():
    n = min((len(per[k]) for k in names if k in per), default=0)
    sums = [sum(per[k][i] for k in names if k in per) for i in range(skip, n)]
    for k in names:
        if k in per:
            d = sorted(per[k][skip:n])
            print(f"{k:16s} launches {len(d):3d}  min {d[0]:9.1f}  median {d[len(d) // 2]:9.1f}  max {d[-1]:9.1f} us")
    if sums:
        ss = sorted(sums)
        print(f"== {g} sum per proof: min {ss[0]:9.1f}  median {ss[len(ss) // 2]:9.1f}  max {ss[-1]:9.1f} us  over {len(ss)} proofs (first {skip} skipped)")
