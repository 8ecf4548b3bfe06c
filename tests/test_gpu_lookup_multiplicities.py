"""Lookup multiplicities counted in block-private LDS histograms (k_blake_count / k_blake_mult, k_ed_hist / k_ed_mult): the
columns are integers, so they must equal the oracle's cell by cell whatever the counting order.  The chains are hand-built so
that their filler bytes stress single bins (all 0x00, all 0xFF), the boundary between two parts of a table (0x7F / 0x80:
bit 7 of the second operand picks the part) and all bins (a fixed pseudo-random pattern); one bin holds more than a 16-bit
counter can, and the idle slot of the Ed25519 table adds a weight > 1 per cell."""
import functools
import hashlib

import numpy as np
import pytest

from oracle import blake_air as B
from oracle import ed_air as E
from oracle import pyref
from oracle import stark_ref as S

pytestmark = pytest.mark.gpu
S.register_air(B.BlakeChainAir)
L0, STRIDE, FIRST = 16, 384, 50000
LENGTHS = (36, 128, 129, 257)
TRUSTED = hashlib.sha256(b"multiplicities").digest()


def filler(pattern, n):
    if pattern == "zeros":
        return bytes(n)
    if pattern == "ones":
        return b"\xff" * n
    if pattern == "boundary":
        return bytes(0x7F + (i & 1) for i in range(n))
    return bytes((i * i * 131 + 89 * i + 7) >> 3 & 0xFF for i in range(n))  # "random": fixed, no generator state


def chain(pattern, lengths=LENGTHS):
    """Messages parent hash || compact(block number) || filler, linked by their BLAKE2b-256 digests."""
    msgs, d = [], TRUSTED
    for k, n in enumerate(lengths):
        m = d + (4 * (FIRST + k) + 2).to_bytes(4, "little") + filler(pattern, n - 36)
        msgs.append(m)
        d = hashlib.blake2b(m, digest_size=32).digest()
    hdr = np.zeros((len(msgs), STRIDE), dtype=np.uint8)
    for i, m in enumerate(msgs):
        hdr[i, : len(m)] = np.frombuffer(m, dtype=np.uint8)
    return msgs, hdr, [len(m) for m in msgs]


@functools.lru_cache(maxsize=None)
def oracle_trace(pattern):
    msgs, _, _ = chain(pattern)
    want, wpub, _ = B.gen_trace(msgs, L0, TRUSTED)
    want.setflags(write=False)
    return want, wpub


@functools.lru_cache(maxsize=None)
def lookup_counts(pattern):
    """(T1, T2) lookups of the oracle trace: every (selector, tag, tuple) of B.lookups counts once per row where its selector is on."""
    loc, nxt, sel = B.int_rows(oracle_trace(pattern)[0])
    n = loc[0].size
    tot = [0, 0]
    for m, tag, _ in B.lookups(loc, nxt, sel):
        tot[0 if tag == B.TAG_T1 else 1] += int(np.count_nonzero(np.broadcast_to(m, (n,))))
    return tuple(tot)


def gpu_trace(ctx, hdr, sizes, log_n, **kw):
    buf, pub, _ = ctx.blake_chain_trace(ctx.from_host(hdr), hdr.shape[1], sizes, TRUSTED, FIRST, log_n, **kw)
    return buf, pub


@pytest.mark.parametrize("pattern", ["zeros", "ones", "boundary", "random"])
def test_blake_trace_and_multiplicities_match_oracle(ctx, vx, oracle, pattern):
    _, hdr, sizes = chain(pattern)
    want, wpub = oracle_trace(pattern)
    buf, pub = gpu_trace(ctx, hdr, sizes, L0)
    got = buf.download().reshape(B.COLS, 1 << L0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first differing cells (col,row): {bad[:5].tolist()}"
    assert [int(x) for x in pub] == wpub
    t1, t2 = lookup_counts(pattern)
    assert (t1, t2) == ((1 << L0) // 16 * 2560, (1 << L0) // 16 * 768)  # per block: 12 x 128 + 14 x 64 + 16 x 8 into T1, 12 x 64 into T2
    assert int(got[B.M1].sum()) == t1 and int(got[B.M2].sum()) == t2
    assert not got[B.M1, 1 << 16:].any() and not got[B.M2, 1 << 16:].any()
    # determinism: a second run counts the same
    buf2, _ = gpu_trace(ctx, hdr, sizes, L0)
    again = buf2.download().reshape(B.COLS, 1 << L0)
    assert (again[B.M1] == got[B.M1]).all() and (again[B.M2] == got[B.M2]).all()


def test_one_bin_exceeds_sixteen_bits(ctx, vx, oracle):
    """The all-zero chain: every padding row range-checks 8 zero message bytes, so table row 0 (a = b = 0) of T1 counts far more than
    65 535 -- a 16-bit counter, or one flushed per tile into 16 bits, is wrong here.  Asserted on the ORACLE's column, then on the GPU's."""
    want, _ = oracle_trace("zeros")
    assert int(want[B.M1, 0]) > 65535
    _, hdr, sizes = chain("zeros")
    buf, _ = gpu_trace(ctx, hdr, sizes, L0)
    got = buf.download().reshape(B.COLS, 1 << L0)
    assert int(got[B.M1, 0]) == int(want[B.M1, 0])


def test_one_header_most_slices_have_no_real_rows(ctx, vx, oracle):
    ch = vx.synth.Chain(1, profile="Ptiny", stride=512)
    buf, pub, _ = ctx.blake_chain_trace(ctx.from_host(ch.headers), 512, ch.sizes, ch.trusted_hash, ch.trusted_block + 1, L0)
    want, wpub, _ = B.gen_trace([ch.headers[0, : ch.sizes[0]].tobytes()], L0, ch.trusted_hash)
    got = buf.download().reshape(B.COLS, 1 << L0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first differing cells (col,row): {bad[:5].tolist()}"
    assert [int(x) for x in pub] == wpub


@pytest.mark.parametrize("pattern", ["zeros", "ones", "boundary", "random"])
def test_more_tiles_than_slices_proves_and_verifies(ctx, vx, oracle, pattern):
    """2^17 rows: a counting workgroup walks more than one tile.  The logUp running sum closes only if every multiplicity is exact, so
    a proof both verifiers accept pins the columns; the sums of the columns are the lookup counts of 2^17 rows."""
    _, hdr, sizes = chain(pattern)
    log_n = L0 + 1
    buf, pub = gpu_trace(ctx, hdr, sizes, log_n)
    n = 1 << log_n
    m = buf.download()[B.M1 * n: (B.M2 + 1) * n].reshape(2, n)
    assert int(m[0].sum()) == n // 16 * 2560 and int(m[1].sum()) == n // 16 * 768 and not m[:, 1 << 16:].any()
    buf2, _ = gpu_trace(ctx, hdr, sizes, log_n)
    assert (buf2.download()[B.M1 * n: (B.M2 + 1) * n].reshape(2, n) == m).all()
    pcfg, cfg = ctx.stark_config(num_queries=4), dict(S.DEFAULT_CFG, num_queries=4)
    proof = ctx.stark_prove(B.ID, buf, log_n, pub, pcfg)
    wpub = [int(x) for x in pub]
    vx.lib.stark_verify(proof, pcfg, expect_air=B.ID, expect_public=wpub)
    S.verify(proof, cfg, expect_air=B.ID, expect_public=wpub)


def test_rotate_header_table_with_a_byte_window(ctx, vx, oracle):
    """Bus mode 2 (rotate's header table): one message, a window of its bytes on the bus; the same counting kernels."""
    msgs, hdr, sizes = chain("random", lengths=(300,))
    window = (100, 150)
    buf, pub = gpu_trace(ctx, hdr, sizes, L0, window=window)
    want, wpub, _ = B.gen_trace(msgs, L0, TRUSTED, first_number=FIRST, window=window)
    got = buf.download().reshape(B.COLS, 1 << L0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first differing cells (col,row): {bad[:5].tolist()}"
    assert [int(x) for x in pub] == wpub
    buf2, _ = gpu_trace(ctx, hdr, sizes, L0, window=window)
    again = buf2.download().reshape(B.COLS, 1 << L0)
    assert (again[B.M1] == got[B.M1]).all() and (again[B.M2] == got[B.M2]).all()


ED_MSG = b"\x01" + bytes(range(32)) + (100000).to_bytes(4, "little") + (7).to_bytes(8, "little") + (3).to_bytes(8, "little")


def ed_signatures(n, unsigned):
    keys, sigs, flags, recs = [], [], [], []
    for i in range(n):
        sec = bytes([i + 1]) * 32
        A, sg = pyref.ed25519_public(sec), pyref.ed25519_sign(sec, ED_MSG)
        on = i not in unsigned
        keys.append(A), sigs.append(sg), flags.append(1 if on else 0)
        if on:
            recs.append(dict(A=A, R=sg[:32], S=int.from_bytes(sg[32:], "little"), H=hashlib.sha512(sg[:32] + A + ED_MSG).digest(), idx=i))
    return keys, sigs, flags, recs


@pytest.mark.parametrize("n_keys,unsigned", [(5, (2,)), (1, ())])
def test_ed_multiplicities_match_oracle(ctx, vx, n_keys, unsigned):
    """2^16 rows = 256 slots, all but a few idle: the staged rows of the ONE idle slot count with weight 256 - k, added in LDS."""
    keys, sigs, flags, recs = ed_signatures(n_keys, unsigned)
    want, wpub = E.gen_trace(recs, 16, bus_on=1)
    assert int(want[E.MULT].max()) > 65535  # the idle slots' zero cells: (256 - k) x 256 rows x hundreds of cells on one bin
    buf, pub = ctx.ed_trace(keys, sigs, ED_MSG, flags, 16, bus_on=1)
    got = buf.download().reshape(E.COLS, 1 << 16)
    bad = np.argwhere(got[E.MULT] != want[E.MULT])
    assert bad.size == 0, f"first differing multiplicities (bin): {bad[:5].tolist()}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"first differing cells (col,row): {bad[:5].tolist()}"
    assert [int(x) for x in pub] == wpub
    assert int(got[E.MULT].sum()) == (1 << 16) * 2 * E.N_RANGE  # every row range-checks its 672 cells
    buf2, _ = ctx.ed_trace(keys, sigs, ED_MSG, flags, 16, bus_on=1)
    assert (buf2.download().reshape(E.COLS, 1 << 16)[E.MULT] == got[E.MULT]).all()
