#!/usr/bin/env python3
"""The two witness generators alone on the GPU (nothing else running): Ed25519 trace of 201 signatures at 2^16 rows, hash-chain trace of 256 P15k headers at 2^19,
six times each, and a digest of the multiplicity columns.  Run under `rocprofv3 --kernel-trace` and read the trace with
tools/rocpd_kernel_sums.py <dir> 1; VX_LIB_PATH selects another libvxprove build."""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vx_import
vx = vx_import.load()
ctx = vx.Context(0)
th = hashlib.blake2b(b"t", digest_size=32).digest()
just = vx.synth.Justification(100256, th, n_signed=201)
ch = vx.synth.Chain(256, profile="P15k")
hb = ctx.from_host(ch.headers)
ebuf = bbuf = None
for _ in range(6):
    ebuf, pub = ctx.ed_trace(just.pubkeys, just.signatures, just.precommit, just.signed, 16, trace_buf=ebuf)
    ctx.sync()
    bbuf, bpub, _ = ctx.blake_chain_trace(hb, ch.stride, ch.sizes, ch.trusted_hash, ch.trusted_block + 1, 19, trace_buf=bbuf, tree_size=256)
    ctx.sync()
import numpy as np
n = 1 << 16
mult = ebuf.download()[837 * n: 838 * n]
print("ed MULT digest", hashlib.sha256(mult.tobytes()).hexdigest()[:16], int(mult.sum()))
n = 1 << 19
m = bbuf.download()[729 * n: 731 * n]
print("blake M1/M2 digest", hashlib.sha256(m.tobytes()).hexdigest()[:16], int(m.sum()))
