#!/usr/bin/env python3
"""bench.py -- header_range_256 hot path on MI355X (contract: see the task brief / DESIGN.md section 7).

  python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run)
  python bench.py ... --dump-outputs DIR               (also write what the last timed step returned, DIR/*.npy)
  python bench.py ... --full                           (also everything beyond the headline, see below)

One "step" = one pass of the implemented hot path over one synthetic header_range_256 input
resident in HBM (a 256-header P15k chain + its STARK trace): see `config.stages` in the JSON
line for exactly which stages are inside the timed region -- `config.complete_proof` says
whether they add up to a full proof yet.  Independent inputs shard one per rank (weak
scaling, no data-path collective); the only collective is the final RCCL gather of the
fixed-size result blobs, outside the per-step work but inside the timed region.  By default four
proofs are in flight per GPU (`--inflight`): K steps are K complete proofs, handed to four worker
contexts from one queue, so one proof's small-kernel tail overlaps another's bulk kernels.

A plain run sets up, warms up, times the K steps and prints the line.  With `--full` it then
also checks the result (the product's verifier on the blob; every gathered blob at N > 1) and
adds `latency_ms`, `gathered_blobs`, `roofline` (NTT kernel: algorithmic bytes 16*n*c per
transform over its HIP-event time on the ctx stream), `roofline_poseidon`, `pmax` and
`cpu_baseline` (the C oracle, kind "port", timed on a bounded sample on this host).  The oracle
is used ONLY for that baseline leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import vx_import  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; ~6.3 TB/s achievable)

# workload: BASELINE.json configs[1] -- header_range_256, single proof, synthetic 256-header chain
N_HEADERS = 256
PROFILE = "P15k"
# NTT roofline microbench: the shape of the dominant transform of this workload (BlakeChainAir trace,
# 30,720 compressions x 16 rows -> 2^19 rows, 731 main + 268 auxiliary columns), measured on a 1024-column slab.
NTT_LOG_N = 19
NTT_COLS = 1024
BLAKE_COLS = 745 + 276  # main + auxiliary (logUp) columns


class Workload:
    """One header_range input of this rank, resident in HBM.  The contexts of a rank (proofs in flight) prove the SAME input:
    the host-side chain and the justification (300 pure-Python Ed25519 signatures) are built once per rank and shared."""
    _shared = {}

    def __init__(self, vx, ctx, seed_offset=0, profile=None):
        self.vx, self.ctx = vx, ctx
        profile = profile or PROFILE
        key = (N_HEADERS, profile, seed_offset)
        if key not in Workload._shared:
            chain = vx.synth.Chain(N_HEADERS, profile=profile, seed=vx.synth.CHAIN_SEED + seed_offset)
            # 300 authorities, all signing the precommit of the target header
            Workload._shared[key] = (chain, vx.lib.PackedJustification(vx.synth.Justification(chain.target_block, chain.target_hash)))
        self.chain, self.just = Workload._shared[key]
        self.d_headers = ctx.from_host(self.chain.headers)  # resident in HBM before the timed region
        self.cfg = ctx.stark_config()
        if os.environ.get("VX_BENCH_NO_JUSTIFICATION"):  # profiling aid: the hash-chain proof alone on one stream (NOT the metric)
            self.just = None
        self.out = None
        ctx.sync()

    def free(self):
        self.d_headers.free()
        self.out = None

    def step(self):
        ch = self.chain
        out96, proof = self.ctx.header_range_prove(self.d_headers, ch.stride, ch.sizes, N_HEADERS, ch.trusted_block, ch.trusted_hash,
                                                   ch.target_block, self.cfg, self.out, self.just)
        self.out = proof.base if proof.base is not None else proof
        return out96, proof

    def blob(self, res):
        return res[1].view(np.uint8)

    def check(self, res):
        assert res[0] == self.chain.expected_outputs(N_HEADERS), "public outputs differ from the native mirror"
        assert int(res[1][0]) == self.vx.lib.HR_MAGIC and res[1][4:16].tobytes() == res[0]
        # (outside the timed region) the product's host verifier accepts the blob: both tables, the bus balance, the commitment
        ch = self.chain
        self.vx.lib.header_range_verify(res[1], N_HEADERS, ch.trusted_block, ch.trusted_hash, ch.target_block, res[0], self.cfg,
                                        authority_set_hash=self.just.sh.tobytes() if self.just is not None else None,
                                        authority_set_id=self.just.struct.authority_set_id if self.just is not None else 0)


class RotateWorkload:
    """BASELINE.json configs[3]: RotateCircuit -- epoch-end header hash STARK, 300-signature justification, epoch-end
    header checks, commitments of the current and the new 300-key authority set (two ShaChainAir STARKs)."""

    def __init__(self, vx, ctx, seed_offset=0):
        self.vx, self.ctx = vx, ctx
        self.e = vx.synth.EpochEndHeader(397859, 300, size=15360, seed=vx.synth.ROTATE_SEED + seed_offset)
        self.sj = vx.synth.Justification(397859, self.e.hash, n_auth=300, n_signed=201, set_id=117)
        self.just = vx.lib.PackedJustification(self.sj, 300)
        self.d_header = ctx.from_host(self.e.padded)
        self.cfg = ctx.stark_config()
        self.out = None
        ctx.sync()

    def step(self):
        e = self.e
        out32, proof = self.ctx.rotate_prove(self.d_header, e.size, e.number, 300, e.start_position, e.new_pubkeys, self.just, self.cfg, self.out)
        self.out = proof.base if proof.base is not None else proof
        return out32, proof

    def blob(self, res):
        return res[1].view(np.uint8)

    def check(self, res):
        assert res[0] == self.e.new_authority_set_hash, "new authority set hash differs from the native mirror"
        self.vx.lib.rotate_verify(res[1], 117, self.sj.authority_set_hash, res[0], self.cfg)


def ntt_roofline(ctx, iters=10):
    """HIP-event time of the NTT kernel (k_ntt_pass) on the ctx stream."""
    n = 1 << NTT_LOG_N
    buf = ctx.alloc(n * NTT_COLS)
    ctx.fill_random(buf, n * NTT_COLS, 7)
    for _ in range(2):
        ctx.ntt(buf, NTT_LOG_N, NTT_COLS, order=1)
    ctx.sync()
    groups = []
    for _ in range(3):  # three groups of `iters` transforms, the best group counts (the proofs before it leave the clocks where they were)
        ctx.timer_start()
        for _ in range(iters):
            ctx.ntt(buf, NTT_LOG_N, NTT_COLS, order=1)
        groups.append(ctx.timer_stop() / iters)
    ms = min(groups)
    buf.free()
    launches = 1 + (NTT_LOG_N > 12) + (NTT_LOG_N > 20)
    alg_bytes = 16.0 * n * NTT_COLS
    achieved = alg_bytes / (ms * 1e-3) / 1e9
    traffic, traffic_src = None, None
    for tag in ("r03", "r02", "r01"):  # PMC counters cannot be read from inside the bench: the committed rocprofv3 --pmc result of this kernel
        tpath = os.path.join(ROOT, "profiles", f"{tag}_ntt_traffic.json")
        if not os.path.exists(tpath):
            continue
        t = json.load(open(tpath))
        if t["shape"].startswith(f"forward NTT 2^{NTT_LOG_N} x {NTT_COLS}"):
            traffic = round(t["hbm_bytes_per_transform"] / 1e9, 3)
            traffic_src = (f"profiles/{tag}_ntt_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, tools/ntt_pmc.py), calibrated on known "
                           "8-B/lane streams; GB per transform")
            break
    # the two launches of this transform, and what the committed profiler runs of the SAME instantiations say (read, not embedded)
    kernels = [f"k_ntt3<0, 0, {NTT_LOG_N - 12}, 0>", "k_ntt3<0, 0, 12, 0>"] if 16 <= NTT_LOG_N <= 20 else ["k_ntt3 / k_ntt_tile"]
    rocprof = None
    spath = os.path.join(ROOT, "profiles", "r03_ntt_kernel_stats.csv")
    if os.path.exists(spath):
        import csv

        rows = [r for r in csv.DictReader(open(spath)) if "k_ntt" in r.get("Name", "")]
        if rows:
            rocprof = {"source": "profiles/r03_ntt_kernel_stats.csv (rocprofv3 --kernel-trace --stats of this shape, tools/r03_ntt_probe.sh)",
                       "avg_ms_per_launch": {r["Name"].replace("void ", "").split("(")[0]: round(float(r["AverageNs"]) / 1e6, 4) for r in rows}}
            rocprof["avg_ms_per_transform"] = round(sum(rocprof["avg_ms_per_launch"].values()), 4)
    issue = None
    ppath = os.path.join(ROOT, "profiles", "r03_ntt_sq_new.json")
    if os.path.exists(ppath):
        sq = json.load(open(ppath))
        issue = {"source": "profiles/r03_ntt_sq_new.json (rocprofv3 --pmc SQ counters of this shape, tools/r03_ntt_pmc.sh)",
                 "by_kernel": {k: {q: v[q] for q in ("valu_insts_per_wave", "valu_issue_util_per_simd", "SQ_ACTIVE_INST_VALU/WAVE_CYCLES", "SQ_WAIT_ANY/WAVE_CYCLES",
                                                       "SQ_WAIT_INST_ANY/WAVE_CYCLES") if q in v} for k, v in sq.items() if "k_ntt" in k}}
    return {
        "bound": "hbm", "kernel": " + ".join(kernels), "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
        "per": f"one forward NTT of 2^{NTT_LOG_N} x {NTT_COLS} columns = {launches} launches, {alg_bytes / 1e9:.3f} GB algorithmic (16*n*c)",
        "ms_per_transform": round(ms, 4), "ms_per_launch": round(ms / launches, 4), "ms_per_transform_groups": [round(g, 4) for g in groups],
        "rocprof_stats": rocprof, "issue_counters": issue,
    }


def poseidon_roofline(ctx, vx, log_leaves, iters=3):
    """The proof's dominant kernel, k_hash_leaves (Poseidon sponge over the rows of the trace LDE), on the shape of the
    main-trace commitment of this workload: 2^(log rows + 1) leaves x 745 columns.  Integer-ALU work: priced against the VALU-issue
    peak of the permutation code (instruction count x issue cycles, see below), and its HBM fraction beside it."""
    cols = 745
    n = 1 << log_leaves
    buf = ctx.alloc(n * cols)
    ctx.fill_random(buf, n * cols, 11)
    t = ctx.merkle(buf, n, cols, vx.lib.VX_LEAVES_COLS_BITREV, 4)
    t.free()
    ctx.sync()
    ctx.timer_start()
    for _ in range(iters):
        ctx.merkle(buf, n, cols, vx.lib.VX_LEAVES_COLS_BITREV, 4).free()
    ms = ctx.timer_stop() / iters
    buf.free()
    perms = n * ((cols + 7) // 8) + (n - 16)
    alg_bytes = 8.0 * n * cols + 32.0 * (2 * n - 16)
    # VALU-issue peak, measured in this run on this clock: the bare permutation kernel (vx_poseidon_permute_batch: one
    # permutation per lane on 2^23 independent states, 96 B in / 96 B out per lane, no sponge, no tree) -- the same
    # instruction stream without the leaf walk.  ISA accounting (profiles/README.md): ~16 k VALU instructions per
    # wave-permutation at ~4.2 issue cycles each.
    n_states = 1 << 23
    st = ctx.alloc(12 * n_states)
    ctx.fill_random(st, 12 * n_states, 13)
    ctx.poseidon(st, n_states)
    ctx.sync()
    ctx.timer_start()
    for _ in range(iters):
        ctx.poseidon(st, n_states)
    peak = n_states / (ctx.timer_stop() / iters * 1e-3) / 1e9
    st.free()
    ach = perms / (ms * 1e-3) / 1e9
    return {"bound": "valu", "kernel": "k_hash_leaves + k_merkle_level (vx_merkle_build)", "achieved": round(ach, 3), "peak": round(peak, 3),
            "unit": "G permutations/s", "frac": round(min(1.0, ach / peak), 4),
            "frac_note": "the leaf kernel runs at the rate of the bare permutation kernel (which also moves 192 B per permutation and can come out 1-2 % slower): "
                         f"measured ratio {ach / peak:.4f}, reported fraction capped at 1 -- this stage is at the VALU instruction-issue limit, only fewer columns make it cheaper",
            "per": f"Merkle tree over 2^{log_leaves} leaves x {cols} columns, cap height 4 = {perms / 1e6:.1f} M Poseidon permutations, {ms:.2f} ms",
            "peak_source": "measured in this run: vx_poseidon_permute_batch on 2^23 independent states (the bare permutation, one per lane: ~16 k VALU "
                           "instructions per wave-permutation at ~4.2 issue cycles, profiles/r01_isa_issue_rates.json); the leaf kernel adds the sponge walk over the row",
            "hbm": {"achieved": round(alg_bytes / (ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                    "algorithmic_GB": round(alg_bytes / 1e9, 3)}}


CPU_SAMPLE_HEADERS = 32  # 32 x 120 compressions x 16 rows = 61,440 rows -> the smallest complete instance (2^16 rows)


def cpu_baseline(vx, ctx):
    """The CPU restatement (oracle/: C + OpenMP kernels driven from numpy) proving a COMPLETE smaller instance of the
    same step -- header_range over 32 of the 256 headers: the full BlakeChainAir STARK (auxiliary logUp columns, LDE,
    Poseidon Merkle caps, quotient, openings, FRI commit / PoW / 84 queries) on its 2^16 x 999 trace -- scaled by the
    row ratio to the 2^19-row workload, plus verify_subchain over all 256 headers."""
    cores = min(len(os.sched_getaffinity(0)), 16)  # the GPU box grants a 16-core share per GPU
    os.environ["OMP_NUM_THREADS"] = str(cores)  # read by libgomp when the oracle library loads
    from oracle import blake_air as B  # checker code, used here ONLY as the reported CPU baseline
    from oracle import oracle as O
    from oracle import stark_ref as S

    S.register_air(B.BlakeChainAir)
    ch = vx.synth.Chain(N_HEADERS, profile=PROFILE)
    t0 = time.perf_counter()
    rc, _ = O.verify_subchain(ch.headers, ch.sizes, N_HEADERS, ch.trusted_block, ch.trusted_hash, ch.target_block)
    t_chain = time.perf_counter() - t0
    assert rc == 0
    small = vx.synth.Chain(CPU_SAMPLE_HEADERS, profile=PROFILE)
    # the witness (main trace) comes from the GPU generator -- equal to the restatement's cell by cell (tests/test_gpu_blake_air.py);
    # the restatement's own generator is pure Python and would only measure the interpreter
    buf, pub, _ = ctx.blake_chain_trace(ctx.from_host(small.headers), small.stride, small.sizes, small.trusted_hash, small.trusted_block + 1, 16)
    trace = buf.download().reshape(B.COLS, 1 << 16)
    buf.free()
    t0 = time.perf_counter()
    proof = S.prove(B.BlakeChainAir, trace, [int(x) for x in pub])
    t_prove = time.perf_counter() - t0
    S.verify(proof, expect_air=B.ID)
    rows_ratio = (1 << (19 if N_HEADERS == 256 else 20)) / float(1 << 16)
    total = t_chain + rows_ratio * t_prove
    # the WHOLE step -- all five tables at their real sizes, nothing scaled -- takes minutes on the CPU: it was run once on a GPU box's
    # host cores and committed (tools/cpu_full_step.py); the live sample above is what fits the bench's time budget
    full = None
    fpath = os.path.join(ROOT, "profiles", "r03_cpu_full_step.json")
    if os.path.exists(fpath) and N_HEADERS == 256:
        rec = json.load(open(fpath))
        full = {"source": "profiles/r03_cpu_full_step.json (tools/cpu_full_step.py, run once offline on a GPU box's host cores)", "cores": rec["cores"],
                "seconds": rec["total_s"], "proofs_per_s": rec["proofs_per_s"], "tables_s": {k: v["prove_s"] for k, v in rec["tables"].items()}, "not_timed": rec["not_timed"]}
    return {
        "value": round(1.0 / total, 6), "unit": "proofs/s", "cores": cores, "kind": "port",
        "sample": f"oracle/ (C + OpenMP kernels under numpy, {cores} threads): COMPLETE BlakeChainAir STARK of header_range over {CPU_SAMPLE_HEADERS} of the "
                  f"{N_HEADERS} headers (2^16 x 1018 trace: logUp columns, LDE, Poseidon caps, quotient, openings, FRI, PoW, 84 queries; proof verified) "
                  f"= {t_prove:.1f} s, scaled x{rows_ratio:.0f} by rows (under-counts the n log n terms), + verify_subchain on all {N_HEADERS} headers {t_chain:.2f} s. "
                  f"Not included in this live sample: witness generation (trace taken from the GPU path) and the other four tables of the step -- full_step_record has the same step with every table at its real size, run once offline",
        "seconds": {"stark_prove_sample": round(t_prove, 2), "verify_subchain": round(t_chain, 3), "scaled_total": round(total, 1)},
        "full_step_record": full,
    }


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, out_bytes, words):
    """--dump-outputs DIR: what the timed path handed its caller in its last step, as float64 .npy files that hold it exactly:
    public_outputs.npy = the output bytes, proof_words.npy = the proof's 64-bit words as (low 32 bits, high 32 bits) rows.  A proof
    over the size limit is written as a fixed sample of its words (seed 0), their positions in proof_word_index.npy."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "public_outputs.npy"), np.frombuffer(out_bytes, dtype=np.uint8).astype(np.float64))
    w = np.ascontiguousarray(words).view(np.uint64).reshape(-1)
    max_words = (DUMP_LIMIT_BYTES - 8 * len(out_bytes)) // 24  # 16 B per word, 8 B per index if sampled
    ipath = os.path.join(path, "proof_word_index.npy")
    if w.size > max_words:
        idx = np.sort(np.random.default_rng(0).choice(w.size, max_words, replace=False))
        np.save(ipath, idx.astype(np.float64))
        w = w[idx]
    elif os.path.exists(ipath):  # left by an earlier run into the same DIR
        os.remove(ipath)
    np.save(os.path.join(path, "proof_words.npy"), np.stack([w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)], axis=1).astype(np.float64))


def sharded_proof_bench(args, vx, ctx, wl, dist, rank, world, local_rank, barrier):
    """--shard-proof S: K steps = K proofs, each proven by ALL ranks together (table t of the proof on rank t mod world); strong scaling."""
    S = args.shard_proof
    ch = wl.chain
    tdev = "cuda" if dist and dist.get_backend() == "nccl" else None

    def step():
        if dist is None:
            return ctx.header_range_prove(wl.d_headers, ch.stride, ch.sizes, N_HEADERS, ch.trusted_block, ch.trusted_hash, ch.target_block, wl.cfg, just=wl.just, n_segments=S)
        return vx.shard.prove_header_range_sharded(ctx, dist, wl.d_headers, ch.stride, ch.sizes, N_HEADERS, ch.trusted_block, ch.trusted_hash, ch.target_block, wl.cfg,
                                                   just=wl.just, n_segments=S, device=tdev, lib=vx.lib)

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out96, blob = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        import torch

        t = torch.tensor([elapsed], device=tdev or "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, out96, blob)
        if args.full:
            assert out96 == ch.expected_outputs(N_HEADERS)
            vx.lib.header_range_verify(blob, N_HEADERS, ch.trusted_block, ch.trusted_hash, ch.target_block, out96, wl.cfg,
                                       authority_set_hash=wl.just.sh.tobytes() if wl.just is not None else None,
                                       authority_set_id=wl.just.struct.authority_set_id if wl.just is not None else 0)
        emit({
            "metric": f"header_range_{N_HEADERS} proofs/sec, ONE proof sharded over the GPUs", "value": round(args.steps / elapsed, 4), "unit": "proofs/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "u64 (Goldilocks) / u8 (hashes)", "data": "synthetic",
            "config": {"workload": f"header_range_{N_HEADERS} ({PROFILE}), 300 authorities: ONE input for all ranks; hash-chain table in {S} map segments; table t of "
                                   f"{S + 4} (segments, Merkle, commitment, Ed25519, SHA-512) proven by rank t mod {world}; one all-reduce of the trace caps per proof, "
                                   "partial blobs gathered and merged on rank 0", "map_segments": S, "blob_bytes": int(blob.size * 8),
                       "exchange": f"torch.distributed all_reduce ({dist.get_backend()})" if dist else "none (1 rank)"},
            "verified": bool(args.full)})
    ctx.close()
    if dist:
        dist.destroy_process_group()


_REAL_STDOUT = None


def quiet_stdout():
    """stdout carries exactly ONE JSON line.  Libraries print there too (the RCCL build PyTorch ships writes a version banner to stdout
    at its first communicator): from here on file descriptor 1 of this process points at stderr and emit() writes to the real stdout."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(line):
    data = (json.dumps(line) + "\n").encode()
    if _REAL_STDOUT is None:
        sys.stdout.write(data.decode())
        sys.stdout.flush()
    else:
        os.write(_REAL_STDOUT, data)


def launch_ranks(n_gpus, argv):
    """`python bench.py --gpus N` without a launcher: start N ranks under torch.distributed.run as a CHILD process (one
    rank per GPU, rendezvous on 127.0.0.1) and exit with its code.  Nothing in this parent has touched the GPU or
    imported torch, and it never execs: rank 0 of the child prints the JSON line on the inherited stdout."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this host driver
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


def dry_launch(args):
    """--dry-launch: the N > 1 control flow without a GPU -- every rank joins a gloo group and reports the launcher
    environment it sees; rank 0 prints one JSON line (tests/test_bench_launch.py)."""
    import torch.distributed as dist

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    seen = {"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "-1")), "world_size": world,
            "master_addr": os.environ.get("MASTER_ADDR"), "headers": args.headers}
    got = [seen]
    if world > 1:
        dist.init_process_group("gloo")
        got = [None] * world
        dist.all_gather_object(got, seen)
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit({"dry_launch": True, "n_gpus": world, "gpus_arg": args.gpus, "ranks": got})


def main():
    # before anything can initialise the HIP runtime (torch.cuda.set_device in the multi-rank path does, ahead of the library's own
    # constructor): more hardware queues than the runtime's default 4, see vx_core.hip
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--headers", type=int, default=256, choices=(256, 512),
                    help="256 = BASELINE.json configs[1] (the headline metric, default); 512 = configs[2]/[5]")
    ap.add_argument("--inflight", type=int, default=0,
                    help="proofs in flight per GPU (contexts + host threads; steps are handed out from one queue). Default: 4")
    ap.add_argument("--profile", default="P15k", choices=("P15k", "Pmax", "Pmix"),
                    help="header sizes (SURVEY.md section 8d): P15k = every header 15,360 B (the headline, default); Pmax = every header MAX_HEADER_SIZE = "
                         "35,840 B, the capacity the reference circuit always pays for (circuits/consts.rs:9-16); Pmix = uniform in [512, 35840]")
    ap.add_argument("--no-pmax", action="store_true", help="skip the extra Pmax measurement of the default line")
    ap.add_argument("--circuit", default="header_range", choices=("header_range", "rotate"),
                    help="header_range = the headline metric (default); rotate = BASELINE.json configs[3]")
    ap.add_argument("--shard-proof", type=int, default=0, metavar="S",
                    help="STRONG scaling: every step is ONE proof whose tables (S map segments of the hash-chain table + the four small tables) are "
                         "spread over the ranks (SURVEY 8 f2); the ranks exchange their trace caps once per proof and rank 0 merges the partial blobs. "
                         "Not the headline metric (that is one proof per rank, weak scaling)")
    ap.add_argument("--dry-launch", action="store_true", help="rehearse the multi-rank launch on CPU (gloo), no GPU work")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also verify the result and measure latency, the NTT and Poseidon rooflines, the Pmax rate and the CPU "
                         "baseline (off by default: a plain run prints the headline alone)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps write what the last one returned (rank 0): DIR/public_outputs.npy, DIR/proof_words.npy (float64, exact)")
    args = ap.parse_args()
    global N_HEADERS, PROFILE
    N_HEADERS, PROFILE = args.headers, args.profile
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:  # the driver's plain `python bench.py --gpus N`: become the launcher (no GPU touched here)
            sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks")
    quiet_stdout()
    if args.dry_launch:
        return dry_launch(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1 or os.environ.get("VX_BENCH_FORCE_DIST"):  # the env override exercises the RCCL path on one GPU
        import torch
        import torch.distributed as dist_mod

        # VX_BENCH_BACKEND=gloo + VX_BENCH_DEVICE=0 rehearse the N > 1 control flow (barrier, gather, max-reduce) with
        # several ranks on ONE GPU, which RCCL cannot do; the driver's runs use nccl (= RCCL), one rank per GPU.
        backend = os.environ.get("VX_BENCH_BACKEND", "nccl")
        if os.environ.get("VX_BENCH_DEVICE"):
            local_rank = int(os.environ["VX_BENCH_DEVICE"])
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist_mod.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist_mod.init_process_group(backend)
        dist = dist_mod
    vx = vx_import.load()
    # measured with GPU_MAX_HW_QUEUES=16 (set by the library): 7.76 / 7.86 / 7.93 / 7.92 proofs/s with 3 / 4 / 5 / 6 in flight (every proof already
    # runs its five tables on five streams); with the runtime's default of 4 hardware queues 7.26 / 7.22 with 3 / 4
    inflight = args.inflight or (4 if PROFILE == "P15k" else 2)  # a Pmax proof holds 4x the memory of a P15k one
    inflight = max(1, min(inflight, args.steps))
    if args.shard_proof:
        inflight = 1  # one proof at a time, spread over the ranks
    # `inflight` proofs are proven concurrently on this GPU: each worker thread owns a context (stream, pool) and an
    # input resident in HBM and takes the next step from a shared counter, so the tail of one proof (FRI layers, host
    # transcript, queries -- small kernels and syncs) overlaps the bulk kernels of another.  K steps are still K proofs.
    import threading

    ctxs = [vx.Context(local_rank) for _ in range(inflight)]
    ctx = ctxs[0]
    # (one proof sharded over the ranks: every rank holds the SAME input)
    wls = [(RotateWorkload if args.circuit == "rotate" else Workload)(vx, c, seed_offset=0 if args.shard_proof else rank) for c in ctxs]
    wl = wls[0]

    def barrier():
        for c in ctxs:
            c.sync()
        if dist:
            import torch

            dist.barrier()
            torch.cuda.synchronize()

    if args.shard_proof:
        return sharded_proof_bench(args, vx, ctx, wls[0], dist, rank, world, local_rank, barrier)

    def run_steps(n_steps):
        lock, nxt, last, errs = threading.Lock(), [0], [None] * inflight, []

        def worker(i):
            try:
                while True:
                    with lock:
                        if nxt[0] >= n_steps:
                            return
                        nxt[0] += 1
                    last[i] = wls[i].step()
            except BaseException as e:  # noqa: BLE001 -- re-raised on the main thread
                errs.append(e)

        ths = [threading.Thread(target=worker, args=(i,)) for i in range(inflight)]
        for t_ in ths:
            t_.start()
        for t_ in ths:
            t_.join()
        if errs:
            raise errs[0]
        return next(r for r in last if r is not None)

    # the one collective goes through the exported C ABI (vx_gather_proofs, RCCL all-gather on the ctx stream) when every
    # rank could make a raw communicator; otherwise through torch.distributed (same RCCL underneath) -- the line says which
    comm, gather_kind = None, "none (1 rank)"
    if dist and dist.get_backend() == "nccl":
        import torch

        try:
            comm = vx.shard.RcclComm(dist, local_rank)
            ok, why = 1, ""
        except Exception as e:  # noqa: BLE001 -- reported in the JSON line
            ok, why = 0, f"{type(e).__name__}: {e}"
        flag = torch.tensor([ok], device="cuda")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 1:
            gather_kind = "vx_gather_proofs (C ABI, RCCL all-gather)"
        else:
            if comm:
                comm.close()
            comm, gather_kind = None, f"torch.distributed.gather (RCCL); raw communicator unavailable on some rank {why}".strip()
    elif dist:
        gather_kind = f"torch.distributed.gather ({dist.get_backend()})"
    for w in wls:  # W warmup steps on every context (pool, tables)
        for _ in range(args.warmup):
            w.step()
    barrier()
    t0 = time.perf_counter()
    res = run_steps(args.steps)
    blob = wl.blob(res)
    # the one collective: fixed-size result blobs to rank 0 over RCCL/xGMI
    tdev = "cuda" if dist and dist.get_backend() == "nccl" else ("cpu" if dist else None)
    gathered = vx.shard.gather_blobs_abi(ctx, comm, blob) if comm else vx.shard.gather_blobs(blob, dist, device=tdev)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        import torch

        t = torch.tensor([elapsed], device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, res[0], res[1])
        LOG_ROWS = None
        if args.circuit == "header_range":
            comps = sum((int(z) + 127) // 128 for z in wl.chain.sizes)
            LOG_ROWS = max(16, (16 * comps - 1).bit_length())  # 16 rows per compression, padded to a power of two
        gathered_ok = roof = latency_ms = pose = pmax = None
        if args.full:  # everything below the headline: checks, latency, rooflines, Pmax (the CPU baseline follows the line)
            if gathered is not None:
                assert len(gathered) == world and all(g.size == blob.size for g in gathered)
                if args.circuit == "header_range":
                    # (outside the timed region) every rank's blob is a proof of THAT rank's input: rank r proved the chain of seed + r
                    import hashlib

                    digests = set()
                    for r, g in enumerate(gathered):
                        ch_r = wl.chain if r == rank else vx.synth.Chain(N_HEADERS, profile=PROFILE, seed=vx.synth.CHAIN_SEED + r)
                        words = np.ascontiguousarray(g).view(np.uint64)
                        out_r = words[4:16].tobytes()
                        assert out_r == ch_r.expected_outputs(N_HEADERS), f"rank {r}: public outputs differ from the native mirror"
                        vx.lib.header_range_verify(words, N_HEADERS, ch_r.trusted_block, ch_r.trusted_hash, ch_r.target_block, out_r, wl.cfg,
                                                   authority_set_hash=wl.just.sh.tobytes() if wl.just is not None else None,
                                                   authority_set_id=wl.just.struct.authority_set_id if wl.just is not None else 0)
                        digests.add(hashlib.sha256(words.tobytes()).hexdigest())
                    assert len(digests) == world, "ranks proved the same input"
                    gathered_ok = {"verified": world, "distinct": len(digests)}
            wl.check(res)
            roof = ntt_roofline(ctx)
            # single-proof latency: a few steps with ONE proof in flight (value above is throughput with `inflight` in flight)
            t1 = time.perf_counter()
            for _ in range(2):
                wl.step()
            ctx.sync()
            latency_ms = 1e3 * (time.perf_counter() - t1) / 2
            pose = poseidon_roofline(ctx, vx, LOG_ROWS + 1) if args.circuit == "header_range" else None
            if args.circuit == "header_range" and PROFILE == "P15k" and N_HEADERS == 256 and not args.no_pmax and world == 1:
                # the reference circuit's fixed capacity: every header padded to MAX_HEADER_SIZE (circuits/consts.rs:9-16, 71,680 compressions):
                # the same step on a Pmax chain, two proofs in flight, after (outside) the timed region.  A Pmax proof holds 4x the
                # memory of a P15k one: the P15k inputs and the pools of the other contexts are given back first
                k = min(2, inflight)
                for w in wls:
                    w.free()
                for c in ctxs[k:]:
                    c.close()
                pw = [Workload(vx, ctxs[i], seed_offset=rank, profile="Pmax") for i in range(k)]
                for w in pw:  # warm-up: pool blocks of the larger shapes
                    w.step()

                def two(w):
                    w.step()
                    w.step()

                for c in ctxs[:k]:
                    c.sync()
                t2 = time.perf_counter()
                ths = [threading.Thread(target=two, args=(w,)) for w in pw]
                for t_ in ths:
                    t_.start()
                for t_ in ths:
                    t_.join()
                for c in ctxs[:k]:
                    c.sync()
                dt = time.perf_counter() - t2
                res_p = pw[0].step()
                assert res_p[0] == pw[0].chain.expected_outputs(N_HEADERS), "Pmax public outputs differ from the native mirror"
                pmax = {"value": round(2 * k / dt, 4), "unit": "proofs/s", "ms_per_step": round(1e3 * dt / (2 * k), 2), "inflight": k, "steps": 2 * k,
                        "workload": f"header_range_{N_HEADERS} with every header MAX_HEADER_SIZE = 35,840 B (Pmax): 71,680 Blake2b compressions, hash-chain table 2^21 rows -- "
                                    "what the reference circuit always pays for (circuits/consts.rs:9-16); the P15k headline is NOT the circuit's worst case"}
                for w in pw:
                    w.free()
        line = {
            "metric": f"header_range_{N_HEADERS} proofs/sec", "value": round(world * args.steps / elapsed, 4), "unit": "proofs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64 (Goldilocks) / u8 (hashes)",
            "data": "synthetic", "inflight_per_gpu": inflight, "gather": gather_kind,
            "proof_scope": "every statement of HeaderRangeCircuit is inside a STARK: all 96 public output bytes (Blake2b header-chain table + SHA-256 Merkle table "
                           "of the state / data roots), the authority-set commitment, and the justification -- floor(2n/3)+1 = 201 Ed25519 signatures over the precommit of "
                           "the target header (curve table + SHA-512 table), bound to the committed keys; five tables on one logUp bus under shared challenges. "
                           "NOT done: the five STARKs are not aggregated into one succinct proof (no recursion / Groth16 wrap). The reference's MapReduce structure exists as "
                           "map segments of the hash-chain table linked by the verifier (vx_header_range_prove_ex, bench --shard-proof); this line uses ONE segment",
            "config": {
                "workload": "" if args.circuit != "header_range" else
                            f"header_range_{N_HEADERS}: {N_HEADERS} x {'15,360-B' if PROFILE == 'P15k' else '35,840-B' if PROFILE == 'Pmax' else '512..35,840-B'} synthetic Avail headers ({PROFILE}), 300 authorities, one input per GPU; "
                            f"{sum((int(z) + 127) // 128 for z in wl.chain.sizes):,} Blake2b compressions -> BlakeChainAir (byte-lookup AIR) trace 2^{LOG_ROWS} rows x (745 main + 276 logUp) columns + ShaTreeAir (SHA-256 Merkle table, 2^{16 if N_HEADERS == 256 else 17} x 428) "
                            "+ ShaChainAir (2^16 x 418) + EdAir (201 signatures, 2^16 x 1527) + Sha512Air (2^15 x 805) on the same logUp bus",
                "complete_proof": False,
                "complete_statement": True,
                "stages": ["verify_subchain: Blake2b header hashes, SCALE decode, link + numbering checks, SHA-256 Merkle roots -> 96-B output (native on GPU)",
                           "verify_simple_justification: authority-set SHA-256 chain, precommit, 300 Ed25519 verifications, 2/3 threshold (native on GPU)",
                           "BlakeChainAir witness: chaining values, byte-cell trace, XOR-table multiplicities and (after the lookup challenges) the logUp helper / running-sum columns, all generated on the GPU",
                           "STARK prove (starky-style + auxiliary lookup round, rate_bits 1, cap 4, 84 queries, 16 PoW bits): LDE + Poseidon Merkle caps, quotient, openings, "
                           "FRI batch/fold/PoW/queries, proof bytes",
                           "ShaTreeAir witness + STARK: both 256-leaf SHA-256 Merkle trees over the state roots / data roots the hash-chain table decodes "
                           "from the header bytes and sends over the bus (shared lookup challenges; the two roots are its public inputs)",
                           "ShaChainAir witness + STARK: the 599-compression authority-set SHA-256 commitment (2^16 x 414 trace); sends the keys of the 201 chosen signers over the bus",
                           "EdAir witness + STARK: [S]B = R + [h]A for 201 signatures -- 253 double-and-add steps of 14 field multiplications each, 16-bit limbs, "
                           "672 logUp range checks per row; h = H mod l in-table",
                           "Sha512Air witness + STARK: H = SHA-512(R || A || precommit) for the same 201 signatures, exchanged with EdAir over the bus"],
                "missing": ["recursive aggregation of the five STARKs into one succinct proof (f4)"],
            },
        }
        if args.full:
            line.update({"latency_ms": round(latency_ms, 2), "gathered_blobs": gathered_ok, "roofline": roof})
            if pmax:
                line["pmax"] = pmax
            if args.circuit == "header_range":
                line["roofline_poseidon"] = pose
        if args.circuit == "header_range":
            # SURVEY 8d "whole proof" figure: compulsory (algorithmic) bytes of every streaming stage of the BlakeChainAir
            # proof over the time of a step -- trace written 8nc, LDE 8nc(1+2^r), leaf hashing 8Nc, quotient 16Nc,
            # openings 8nc, FRI combine 8Nc (N = 2n, r = 1); the small ShaChainAir proof and FRI tail are left out
            n_rows = float(1 << LOG_ROWS)
            alg = 8 * n_rows * BLAKE_COLS * (1 + 3 + 2 + 4 + 1 + 2)
            line["proof_roofline"] = {"bound": "hbm", "algorithmic_GB": round(alg / 1e9, 1), "achieved": round(alg / 1e9 / (elapsed / args.steps), 1),
                                      "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / 1e9 / (elapsed / args.steps) / HBM_PEAK_GBS, 4),
                                      "note": "the proof is bound by VALU issue (Poseidon leaf hashing ~45 % of kernel time, at its instruction-issue peak: roofline_poseidon), not by bytes"}
        if args.circuit == "rotate":
            line["metric"] = "rotate proofs/sec"
            line["config"] = {
                "workload": "rotate: 15,360-B synthetic epoch-end header carrying a 300-validator ScheduledChange log, justified by 201 of 300 "
                            "current authorities; one input per GPU",
                "complete_proof": False,
                "stages": ["BlakeChainAir witness + STARK over the header's 120 compressions (2^16 x 1018: one copy of the XOR lookup tables)",
                           "verify_simple_justification (native on GPU: 201 Ed25519 verifications, precommit, threshold)",
                           "verify_epoch_end_header (native on GPU: prefix, 300 x (pubkey, weight), delay)",
                           "two ShaChainAir witnesses + STARKs: current and new authority-set commitments (2^16 x 418 each)",
                           "the justification by the current set in-proof: EdAir (201 signatures, 2^16 x 1527) + Sha512Air (2^15 x 805) on one logUp bus with the current set's commitment"],
                "missing": ["recursive aggregation of the six STARKs into one proof"],
            }
        elif args.full and not args.no_cpu_baseline and world == 1:  # the CPU baseline is reported at N = 1 only
            line["cpu_baseline"] = cpu_baseline(vx, ctx)
        emit(line)
    if comm:
        comm.close()
    for c in ctxs:
        c.close()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
