"""CPU tier: the rendezvous at which the tables of one bus draw their shared challenges and the bookkeeping of such a group
(0-kno-vectorx_amd/csrc/bus_meet.h, bus_meet.cpp) compiled for the host and driven by tests/host/bus_group_check.cpp: all
arrive, one fails (every position, on a thread or on the caller's), two fail, a group abandoned, and the same with two shards
meeting through an in-process exchange -- 200 rounds each, plain and under the thread and the address / undefined-behaviour
sanitizers.  The program ends itself after 30 s, so a table left waiting is a failure and not a stuck suite."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "host", "bus_group_check.cpp"), os.path.join(ROOT, "0-kno-vectorx_amd", "csrc", "bus_meet.cpp")]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "tsan", "asan_ubsan"])
def test_bus_group_releases_joins_and_reports(tmp_path, flags):
    exe = tmp_path / "bus_group_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", *flags, "-o", str(exe), *SRCS])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ok", "200"] and "Sanitizer" not in out.stderr
