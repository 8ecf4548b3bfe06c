"""bench.py --dump-outputs DIR writes what the timed path returned in its last step, exactly, as float .npy files; a plain
run prints the headline line alone and leaves everything else to --full.  CPU part: the file format (round trip of 64-bit words,
the seeded sample over the size limit).  GPU part: a plain run whose dumped proof the product's verifier accepts."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("latency_ms", "gathered_blobs", "roofline", "roofline_poseidon", "pmax", "cpu_baseline")


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("vx_bench_t", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def words_from_dump(d):
    halves = np.load(os.path.join(d, "proof_words.npy"))
    assert halves.dtype == np.float64 and halves.ndim == 2 and halves.shape[1] == 2
    assert (halves >= 0).all() and (halves < 2.0**32).all() and (halves == np.floor(halves)).all()
    h = halves.astype(np.uint64)
    return h[:, 0] | (h[:, 1] << np.uint64(32))


def test_dump_round_trips_64_bit_words(bench, tmp_path):
    rng = np.random.default_rng(3)
    words = rng.integers(0, 2**64 - 1, size=1000, dtype=np.uint64, endpoint=True)
    words[:3] = [0, 2**64 - 1, 2**63 + 1]
    out = bytes(range(96))
    bench.dump_outputs(str(tmp_path), out, words)
    assert (words_from_dump(str(tmp_path)) == words).all()
    pub = np.load(os.path.join(tmp_path, "public_outputs.npy"))
    assert pub.dtype == np.float64 and bytes(pub.astype(np.uint8).tolist()) == out
    assert not os.path.exists(os.path.join(tmp_path, "proof_word_index.npy"))


def test_dump_over_the_limit_is_a_fixed_sample(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 96 * 8 + 24 * 100)  # room for 100 sampled words
    words = np.arange(10000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), bytes(96), words)
    idx = [np.load(os.path.join(d, "proof_word_index.npy")) for d in dirs]
    assert idx[0].shape == (100,) and (idx[0] == idx[1]).all() and (np.diff(idx[0]) > 0).all()
    assert (words_from_dump(str(dirs[0])) == words[idx[0].astype(np.int64)]).all()
    total = sum(os.path.getsize(os.path.join(dirs[0], f)) for f in os.listdir(dirs[0]))
    assert total <= bench.DUMP_LIMIT_BYTES + 3 * 128  # + the .npy headers


def test_flags_are_offered():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_a_valid_proof(tmp_path, vx):
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--inflight", "2", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
    assert line["metric"] == "header_range_256 proofs/sec" and line["steps"] == 3 and line["higher_is_better"] is True
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
    # the dumped arrays are the proof of the bench's input: the product's verifier accepts them as they are
    words = words_from_dump(str(d))
    out96 = bytes(np.load(os.path.join(d, "public_outputs.npy")).astype(np.uint8).tolist())
    ch = vx.synth.Chain(256, profile="P15k")
    just = vx.lib.PackedJustification(vx.synth.Justification(ch.target_block, ch.target_hash))
    assert out96 == ch.expected_outputs(256) and int(words[0]) == vx.lib.HR_MAGIC
    with vx.Context(0) as ctx:
        cfg = ctx.stark_config()
    vx.lib.header_range_verify(words, 256, ch.trusted_block, ch.trusted_hash, ch.target_block, out96, cfg,
                               authority_set_hash=just.sh.tobytes(), authority_set_id=just.struct.authority_set_id)
