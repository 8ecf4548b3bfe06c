"""CPU tier: the one statement of the VXSTARK1 proof layout and transcript (0-kno-vectorx_amd/csrc/stark_proof.h) -- standard C++,
compiled for the host and driven by tests/host/stark_proof_check.cpp over a grid of shapes (degree bits 2..12, every rate, cap heights
up to the whole tree, with and without the auxiliary round, arity bits 1 / 4 / 5, one and three queries): Writer and View agree word for
word with the layout restated there, every strict prefix of a proof is refused, prover and verifier reach the same query indices, and
reduce_openings is Horner's rule -- plain and under the address / undefined-behaviour sanitizers.  The program ends itself after 30 s.
And vx_stark_proof_bound, now Shape::bound_words, still returns the numbers recorded from the library before the layout moved."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stark_proof_check.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_layout_transcript_and_reduced_openings(tmp_path, flags):
    exe = tmp_path / "stark_proof_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 6000 and int(words[2]) > 1000 and "Sanitizer" not in out.stderr


def test_proof_bound_is_the_recorded_one(vx):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "stark_proof_bound.json")))
    assert golden["columns"] == ["air_id", "log_n", "rate_bits", "cap_height", "final_poly_bits", "bound_words"]
    L = vx.lib.load_library()
    assert len(golden["rows"]) == 636 and len({row[0] for row in golden["rows"]}) == 20
    for air_id, log_n, rate_bits, cap_height, final_poly_bits, want in golden["rows"]:
        cfg = vx.lib.default_stark_config(rate_bits=rate_bits, cap_height=cap_height, final_poly_bits=final_poly_bits)
        need = C.c_size_t()
        assert L.vx_stark_proof_bound(air_id, C.byref(cfg), log_n, C.byref(need)) == 0
        assert need.value == want, (air_id, log_n, rate_bits, cap_height, final_poly_bits)
