"""CPU tier: the checks and the lowering of declared bus messages (0-kno-vectorx_amd/csrc/bus_program.h, a host-only header)
compiled alone with g++ and driven by tests/host/bus_program_check.cpp: the LeafNoop, Transcript, FriFold and MerkleOpen message
programs and a made-up one are lowered and the lowered code, run by air_program_eval on random rows, equals a direct evaluation of
h D_a D_b - m_a D_b - m_b D_a and of the running-sum line; every refusal, every truncation and a few thousand seeded random programs
go through validation -- plain and under the address / undefined-behaviour sanitizers.  Nothing is loaded into Python."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bus_program_check.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "bus_programs.txt")


def test_the_fixture_is_what_the_builder_writes(vx):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_bus_programs
    finally:
        sys.path.pop(0)
    assert open(FIXTURE).read() == make_bus_programs.text(), "stale: run python tests/golden/make_bus_programs.py"


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_lowered_programs_equal_the_direct_evaluation(tmp_path, flags):
    exe = tmp_path / "bus_program_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), SRC])
    out = subprocess.run([str(exe), FIXTURE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ") and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
