"""CPU tier: the host challengers (0-kno-vectorx_amd/csrc/glh_poseidon.h: plain, recording, claimed) and the one transcript over them
(stark_proof.h), standard C++ compiled for the host and driven by tests/host/transcript_check.cpp: over random interleavings the
recording challenger yields the plain one's values, its record obeys TranscriptAir's plan rules and replays to the same challenges
block by block, the claimed challenger answers with them and hashes nothing; the whole transcript agrees over all three on random
proofs of 60 shapes -- plain and under the address / undefined-behaviour sanitizers.  The program ends itself after 60 s."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "transcript_check.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_challengers_and_transcript_agree(tmp_path, flags):
    exe = tmp_path / "transcript_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 20000 and int(words[2]) > 500 and "Sanitizer" not in out.stderr
