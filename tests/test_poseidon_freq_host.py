"""CPU tier: the partial rounds of the Poseidon permutation in the transform domain of the linear layer
(0-kno-vectorx_amd/csrc/poseidon_freq.h) compiled for the host and checked against glh::poseidon -- the 22 partial rounds alone and
the whole permutation, on random states, all-zero, all p - 1, every word 2^32 - 1, 2^52 - 1, 2^52, 2^48 - 1, 2^48, 2^64 - 1 and mixtures
of them, with canonical and non-canonical s-box outputs (tests/host/poseidon_freq_check.cpp).  A tracking hook records the extreme
low and high parts of the components and of the recombined outputs; they must stay inside the bounds the header states."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_poseidon_freq_partial_rounds_match_host_permutation(tmp_path):
    exe = tmp_path / "poseidon_freq_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "host", "poseidon_freq_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    tag, max_l, max_h, max_yl, max_yh = out.stdout.split()
    assert tag == "ok"
    # poseidon_freq.h: components |l| <= 4322 2^48, |h| <= 4322 2^16; outputs before K p is added |y_l| <= 3307 2^48, |y_h| <= 3307 2^16
    # (K = 2^12 makes them positive), far inside the 2^63 / 2^31 of the types
    assert int(max_l) <= 4322 and int(max_h) <= 4322 and int(max_yl) <= 3307 and int(max_yh) <= 3307
