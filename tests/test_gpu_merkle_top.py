"""GPU parity of the Merkle tree tops (k_merkle_top: a block computes up to nine levels above its 2^s digests): the cap and, sibling
for sibling, the opening paths -- the only check that sees a wrong intermediate level -- against the oracle's MerkleTree."""
import numpy as np
import pytest

from conftest import rand_field
from test_gpu_ntt import bitrev_perm

pytestmark = pytest.mark.gpu

# (n, cap_h): no level; one level, s = 1; exactly one block, s = 9; s = 9 then s = 1; two blocks then the cap; s = 9 then s = 1 below
# a cap of 2; the hand-over between k_merkle_level and the top on both sides (2^15: top only, 2^16: one k_merkle_level first);
# the side tables' real tree
SHAPES = [(16, 4), (32, 4), (512, 0), (1024, 0), (1024, 4), (2048, 1), (1 << 15, 4), (1 << 16, 4), (1 << 17, 4)]


def check_tree(t, want, n, rng):
    assert (t.cap() == want.cap).all()
    if n <= 1024:
        idx = np.arange(n, dtype=np.uint64)
    else:
        idx = np.unique(np.concatenate([rng.integers(0, n, size=64, dtype=np.uint64), np.array([0, n - 1], dtype=np.uint64)]))
    sib = t.open(idx)
    for k, i in enumerate(idx):
        assert (sib[k] == want.prove(int(i))).all(), f"siblings of leaf {int(i)}"


@pytest.mark.parametrize("n,cap_h", SHAPES)
def test_merkle_top_hashed_leaves(ctx, oracle, rng, n, cap_h):
    leaves = rand_field(rng, (n, 5))
    t = ctx.merkle(ctx.from_host(leaves), n, 5, 0, cap_h)
    check_tree(t, oracle.MerkleTree(leaves, cap_h), n, rng)
    t.free()


@pytest.mark.parametrize("n,cap_h", SHAPES[:4])
def test_merkle_top_unhashed_leaves(ctx, oracle, rng, n, cap_h):
    leaves = rand_field(rng, (n, 3))
    t = ctx.merkle(ctx.from_host(leaves), n, 3, 0, cap_h)
    check_tree(t, oracle.MerkleTree(leaves, cap_h), n, rng)
    t.free()


def test_fri_layer_tree_top(ctx, oracle, rng):
    """A FRI layer tree (2^12 extension values, arity 16: 256 leaves of 32 words, cap height 4) goes through the same top."""
    log_n, arity_bits, cap_h = 12, 4, 4
    n = 1 << log_n
    vals = rand_field(rng, 2 * n)
    rev = vals.reshape(-1, 2)[bitrev_perm(log_n)]
    want = oracle.MerkleTree(rev.reshape(-1, 2 << arity_bits), cap_h)
    t = ctx.fri_layer_tree(ctx.from_host(vals), log_n, arity_bits, cap_h)
    check_tree(t, want, n >> arity_bits, rng)
    t.free()
