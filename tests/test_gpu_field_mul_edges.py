"""The fused Goldilocks multiply-reduce (csrc/gl.cuh, gl_mul_nc) at its carry and borrow edges, and the two users whose
representation it changes: the Poseidon permutation on any 64-bit representative, and the leaf sponge, which canonicalises
after the last permutation of a leaf only.

`fused_mul_model` is the instruction sequence of gl_mul_nc in Python integers with explicit 32 / 64-bit wrap-around.  It
returns the flags that steer the sequence: k = carry-out of the cross term t2 = a1 b0 + t1 (weight 2^96 = -1, taken as the
borrow-in of the reduction), b = borrow-out of A = lo - hh' - k, c = carry-out of T = hl' eps + A.  A borrows only if
lo < hh' + k <= 2^32 - 1, i.e. lo(t2) = 0 and lo(t0) < hh' + k, which uniform operands meet with probability 2^-32: the pairs of
FLAG_PAIRS were constructed (b1 solved from lo(t2) = 0 mod 2^32).  (1, 1, 0) would also need hl' = 0 (with b = 1, A >= 2^64 - 2^32 + 1, so
any hl' >= 1 carries); no such pair is known and none is required."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 2**64 - 2**32 + 1
EPS = 2**32 - 1
M32, M64 = 2**32 - 1, 2**64 - 1

EDGES = [
    0, 1, 2, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**33, 2**63 - 1, 2**63, 2**63 + 1, P - 1, P - 2, P - EPS,
    0xFFFFFFFEFFFFFFFF, 0xFFFFFFFE00000001, 0x8000000080000000, 0x00000001FFFFFFFF, 0xFFFFFFFEFFFFFFFE, 0xFFFFFFFEFFFF0000,
    0x0000000100000001, 0xFFFFFFFD00000003,
    # the operands of the flag combinations that random canonical pairs do not reach (b = 1 needs lo(t2) = 0)
    0xFFFFFFFE, 0x200000000, 0xFFFFFFFF00000000, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0x8E73CA47D66B829F, 0xEF39B2AEEA90A8F0,
]  # fmt: skip
# (k, b, c) -> a pair that produces it
FLAG_PAIRS = {
    (0, 0, 1): (0xFFFFFFFE, 0x7FFFFFFFFFFFFFFF),
    (0, 1, 0): (0x200000000, 0x8000000000000000),
    (0, 1, 1): (0x200000000, 0xFFFFFFFF00000000),
    (1, 0, 0): (0x7FFFFFFFFFFFFFFF, 0xFFFFFFFEFFFFFFFF),
    (1, 1, 1): (0x8E73CA47D66B829F, 0xEF39B2AEEA90A8F0),
}


def fused_mul_model(x, y):
    """gl_mul_nc(x, y) as the GPU computes it -> (result in [0, 2^64), (k, b, c))."""
    a0, a1, b0, b1 = x & M32, x >> 32, y & M32, y >> 32
    t0 = a0 * b0
    t1 = a0 * b1 + (t0 >> 32)
    assert t1 <= M64
    t2 = a1 * b0 + t1  # v_mad_u64_u32 with carry-out
    k, t2 = t2 >> 64, t2 & M64
    hi = a1 * b1 + (t2 >> 32)  # hi' (without k 2^32)
    assert hi <= M64 and (hi >> 32) + k <= M32
    hh, hl = hi >> 32, hi & M32
    lo_l, lo_h = t0 & M32, t2 & M32
    v = lo_l - hh - k  # v_subb_co_u32_e64 al, vcc, lo_l, hh', s[k]
    al, bw = v & M32, int(v < 0)
    v = lo_h - bw  # v_subbrev_co_u32 ah, vcc, 0, lo_h, vcc
    ah, b = v & M32, int(v < 0)
    mb = (-b) & M32  # v_subb_co_u32 mb, vcc, x, x, vcc
    t = hl * EPS + ((ah << 32) | al)  # v_mad_u64_u32 T, vcc, hl', -1, A
    c, t = t >> 64, t & M64
    d = (mb + c) & M32  # v_addc_co_u32 d, vcc, 0, mb, vcc
    ds = d - 2**32 if d >> 31 else d
    assert ds == c - b
    r = (t - ds) & M64  # v_mad_i64_i32 r, d, -1, T
    r = (r + (d << 32)) & M64  # d into the high word
    assert 0 <= t - ds + (ds << 32) <= M64  # |d| = 1 does not wrap again
    return r, (k, b, c)


@pytest.fixture(scope="module")
def mul_operands():
    rng = np.random.default_rng(20250)
    pairs = list(itertools.product(EDGES, EDGES)) + list(FLAG_PAIRS.values())
    a = np.array([x for x, _ in pairs], dtype=np.uint64)
    b = np.array([y for _, y in pairs], dtype=np.uint64)
    ra, rb = rng.integers(0, P, size=1 << 16, dtype=np.uint64), rng.integers(0, P, size=1 << 16, dtype=np.uint64)
    return np.concatenate([a, ra]), np.concatenate([b, rb])


def test_edge_list_is_canonical_and_model_is_exact(mul_operands):
    assert all(0 <= e < P for e in EDGES)
    for want, (x, y) in FLAG_PAIRS.items():
        assert fused_mul_model(x, y)[1] == want, (want, hex(x), hex(y))
    a, b = mul_operands
    seen = {}
    for x, y in zip(a.tolist(), b.tolist()):
        r, flags = fused_mul_model(x, y)
        assert r % P == x * y % P, (hex(x), hex(y), hex(r), flags)
        seen.setdefault(flags, (x, y))
    print("flag combinations reached:", {f: (hex(x), hex(y)) for f, (x, y) in sorted(seen.items())})
    for flags in [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 1)]:
        assert flags in seen, flags


def test_field_batch_mul_edges(ctx, mul_operands):
    a, b = mul_operands
    n = a.size
    da, db, do = ctx.from_host(a), ctx.from_host(b), ctx.alloc(n)
    ctx.field_op("mul", da, db, do, n)
    got = do.download(n)
    want = np.array([x * y % P for x, y in zip(a.tolist(), b.tolist())], dtype=np.uint64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, hex(int(a[bad[0]])), hex(int(b[bad[0]])), hex(int(got[bad[0]])), hex(int(want[bad[0]])),
                           fused_mul_model(int(a[bad[0]]), int(b[bad[0]])))  # fmt: skip


def test_poseidon_batch_any_representative(ctx, oracle):
    """4096 states whose words come from the edge list and from [p, 2^64): the kernel takes any representative."""
    rng = np.random.default_rng(20251)
    n = 4096
    edges = np.array(EDGES, dtype=np.uint64)
    st = edges[rng.integers(0, edges.size, size=(n, 12))]
    high = rng.integers(P, 2**64, size=(n, 12), dtype=np.uint64)
    high.reshape(-1)[:4] = [P, P + 1, 2**64 - 1, 2**64 - 2]
    pick = rng.integers(0, 3, size=(n, 12))
    st = np.where(pick == 0, high, st)
    st[0], st[1] = high[0], edges[:12]  # one state all non-canonical, one all edges
    assert (st >= np.uint64(P)).any() and (st < np.uint64(P)).any()
    buf = ctx.from_host(st)
    ctx.poseidon(buf, n)
    got = buf.download(12 * n).reshape(n, 12)
    want = oracle.poseidon(st % np.uint64(P))
    assert (got < np.uint64(P)).all()
    assert (got == want).all()


@pytest.mark.parametrize("log_n", [15, 8])  # one lane per leaf (k_hash_leaves) / sixteen lanes per leaf (k_hash_leaves_coop)
@pytest.mark.parametrize("leaf_len", [17, 8])  # two full absorbs and a one-element tail / exactly one absorb
def test_merkle_sponge_lengths(ctx, oracle, leaf_len, log_n):
    """The sponge canonicalises after the LAST permutation of a leaf only: digests and cap against the reference tree."""
    rng = np.random.default_rng(100 * leaf_len + log_n)
    n, cap_h = 1 << log_n, 4
    leaves = rng.integers(0, P, size=(n, leaf_len), dtype=np.uint64)
    leaves[0], leaves[1], leaves[-1] = 0, P - 1, P - 1
    want = oracle.MerkleTree(leaves, cap_h)
    t = ctx.merkle(ctx.from_host(leaves), n, leaf_len, 0, cap_h)  # row-major
    dig = t.leaf_digests()
    assert (dig < np.uint64(P)).all()
    assert (dig == want.leaf_digests()).all()
    assert (t.cap() == want.cap).all()
    t.free()
    t = ctx.merkle(ctx.from_host(leaves.T.copy()), n, leaf_len, 2, cap_h)  # column-major, leaf j = row j
    assert (t.leaf_digests() == want.leaf_digests()).all()
    assert (t.cap() == want.cap).all()
    t.free()
