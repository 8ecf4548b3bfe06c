"""GPU parity for the Poseidon permutation on the states and leaf widths at which its partial rounds can go wrong: words at the split
points of the linear layer's representation, non-canonical words, and leaves whose last absorb holds one element."""
import numpy as np
import pytest

from conftest import P, rand_field
from test_gpu_ntt import bitrev_perm

pytestmark = pytest.mark.gpu

EDGE = [0, P - 1, 2**32 - 1, 2**52 - 1, 2**52, 2**48 - 1, 2**48, 2**64 - 1, 1, 2**32, P - 2**32]


def test_poseidon_batch_edge_states(ctx, oracle, rng):
    n = 4096
    s = rand_field(rng, (n, 12))
    k = 0
    for e in EDGE:  # every word the same edge value
        s[k] = e
        k += 1
    for e in EDGE:  # one edge value against another in the patterns the layer's FFTs subtract
        for f in EDGE:
            for pat in (lambda i: i // 3, lambda i: i // 6, lambda i: i, lambda i: i // 3 + 1):
                s[k] = [e if pat(i) & 1 else f for i in range(12)]
                k += 1
    assert k < n
    s[k:k + 256] = np.where(rng.integers(0, 4, size=(256, 12)) == 0, rng.choice(np.array(EDGE, dtype=np.uint64), size=(256, 12)), s[k:k + 256])
    buf = ctx.from_host(s)
    ctx.poseidon(buf, n)
    got = buf.download().reshape(n, 12)
    want = oracle.poseidon(np.where(s >= P, s - np.uint64(P), s))  # 2^64 - 1 is a non-canonical word: the oracle takes its residue
    assert (got < P).all()
    assert (got == want).all()


@pytest.mark.parametrize("log_n,cols", [(8, 9), (8, 135), (8, 745), (16, 17)])
def test_merkle_cols_bitrev_cap_and_digests(ctx, oracle, rng, log_n, cols):
    """Leaves in the column / bit-reversed layout, cap height 4; 745 = 93 * 8 + 1 and 17 = 2 * 8 + 1 end on a one-element absorb.
    2^8 leaves take the cooperative kernels; 2^16 leaves take one lane per leaf (the chain of non-canonical inner permutations)
    and one lane per parent for the widest level."""
    cap_h = 4
    n = 1 << log_n
    data = rand_field(rng, (cols, n))
    data[:, 3] = P - 1
    data[:, 5] = 0
    data[:, 7] = np.array([EDGE[i % len(EDGE)] % P for i in range(cols)], dtype=np.uint64)
    want = oracle.MerkleTree(data[:, bitrev_perm(log_n)].T.copy(), cap_h)
    t = ctx.merkle(ctx.from_host(data), n, cols, 1, cap_h)
    assert (t.cap() == want.cap).all()
    assert (t.leaf_digests() == want.leaf_digests()).all()
    t.free()
