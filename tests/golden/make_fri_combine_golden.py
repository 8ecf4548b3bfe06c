#!/usr/bin/env python3
"""Regenerate tests/golden/fri_combine_blobs.npz: the blobs of vx_fri_combine_prove and vx_fri_combine_fold_prove for the smallest
real statement -- a FibAir proof of 2^7 rows with 5 queries (a 2^8 LDE, one fold layer) -- together with the claims both verifiers are
handed.  The proofs come from the reference prover on the restatements (tests/fri_combine_ref.py, tests/fri_fold_ref.py), which the
GPU tier shows to equal the product's blobs word for word, so this script needs no GPU; the claims come from the product's own host
extractors.  The CPU tier runs both host verifiers on the fixture (tests/test_fri_combine.py).

Run from the repo root:  python tests/golden/make_fri_combine_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vx_import  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import stark_ref as S  # noqa: E402

O.build()
import fri_combine_ref as K  # noqa: E402

NUM_QUERIES, LOG_N = 5, 7


def main():
    vx = vx_import.load()
    cfg, pc = dict(S.DEFAULT_CFG, num_queries=NUM_QUERIES), vx.lib.default_stark_config(num_queries=NUM_QUERIES)
    trace, pub = S.FibAir.trace(LOG_N)
    proof = S.prove(S.FibAir, trace, pub, cfg)
    c, f = vx.lib.stark_combine_claims(proof, pc), vx.lib.stark_fri_claims(proof, pc)
    st = dict(LN=c["log_lde"], r=cfg["rate_bits"], cm=c["cm"], ca=c["ca"], nq=c["nq"], alpha=c["alpha"], zeta=c["zeta"], ol=c["open_local"], on=c["open_next"], oq=c["open_quot"])
    index, rows, ev0 = [int(v) for v in c["index"]], c["rows"], c["ev0"]
    tr, cpub = K.ref_trace(st, index, rows)
    blob = K.wrap(K.prove(tr, cpub, cfg), st, len(index))
    ps, _ = K.group_prove(K.group_tables(st, f["betas"], f["final_poly"], index, rows, f["leaves"]), cfg)
    gblob = K.group_wrap(ps, st, len(f["betas"]), len(index))
    a = (st["LN"], st["cm"], st["ca"], st["nq"], st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"])
    vx.lib.fri_combine_verify(blob, *a, index, rows, ev0, pc)
    vx.lib.fri_combine_fold_verify(gblob, *a, f["betas"], f["final_poly"], index, rows, f["leaves"], pc)
    out = os.path.join(HERE, "fri_combine_blobs.npz")
    np.savez_compressed(out, num_queries=np.uint64(NUM_QUERIES), shape=np.array(a[:4], dtype=np.uint64), alpha=st["alpha"], zeta=st["zeta"], open_local=st["ol"], open_next=st["on"],
                        open_quot=st["oq"], index=np.array(index, dtype=np.uint64), rows=rows, ev0=ev0, betas=f["betas"], final_poly=f["final_poly"], leaves=f["leaves"], combine_blob=blob,
                        combine_fold_blob=gblob)
    print("%s: %d bytes (blobs of %d and %d words)" % (out, os.path.getsize(out), blob.size, gblob.size))


if __name__ == "__main__":
    main()
