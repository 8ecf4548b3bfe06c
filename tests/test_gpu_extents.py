"""Every kernel's output EXTENT on the GPU (tests/extents.py): outputs go to buffers filled with position-dependent words that are
not canonical, with a guard zone behind them (and before them where the API takes an offset), inputs sit in such buffers too.
Every case (1) compares the WHOLE extent with the reference the entry point's own test uses, (2) checks that both guards still
hold their poison and that no word of the extent the header promises is left unstored, (3) checks every input the header declares
const / preserved word for word, guards included.  The shapes are the smallest that leave a ragged block, wave, 16-lane group or
tile; nothing here takes a tolerance."""
import hashlib

import numpy as np
import pytest

import extents as X
from conftest import P, rand_field
from test_gpu_ntt import bitrev_perm

pytestmark = pytest.mark.gpu

CHAL = [3, 5, 7, 11]
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def same(got, want, what="extent"):
    """the whole extent against its reference, cell by cell"""
    want = np.asarray(want, dtype=np.uint64)
    got = np.asarray(got, dtype=np.uint64).reshape(want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d cells differ, first at %s: got %d, want %d" % (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))
    return got


def held(ctx, values, name, before=0, after=X.GUARD):
    """an input in a guarded buffer and its snapshot"""
    g = X.Guarded.holding(ctx, values, before=before, after=after, name=name)
    return g, X.snapshot(g)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def test_the_checker_sees_a_kernel_that_runs_five_words_over(ctx):
    """no kernel is modified: vx_fill_random is asked for n + 5 words while the helper is told the extent is n (the stores stay
    inside the test's own buffer)"""
    n = 1000
    g = X.Guarded(ctx, n, before=3, shape=(1, n), name="fill_random told n + 5")
    ctx.fill_random(g.buf, n + 5, 9, off=g.off)
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "stray stores BEHIND the extent" in msg and "5 words" in msg and "first at offset +0" in msg and "last at +4" in msg, msg
    assert "(column 0, row %d) .. (column 0, row %d)" % (n, n + 4) in msg, msg
    g.free()
    g = X.Guarded(ctx, n, before=3, name="fill_random told n - 1")  # ... and a word that is never stored
    ctx.fill_random(g.buf, n - 1, 9, off=g.off)
    with pytest.raises(AssertionError, match=r"never stored .*: 1 words, first at offset -1, last at -1"):
        g.check()
    g.free()


# ----------------------------------------------------------------------------------------------------------------- primitives
def splitmix_canonical(seed, n):
    """vx_fill_random's definition in Python integers: outputs 1..n of SplitMix64 seeded with `seed`, reduced below P"""
    out = []
    for i in range(n):
        z = (seed + GOLD * (i + 1)) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        out.append(z - P if z >= P else z)
    return np.array(out, dtype=np.uint64)


OFF_N = [(3, 1), (5, 255), (0, 257), (7, 0)]


@pytest.mark.parametrize("off,n", OFF_N)
def test_fill_random(ctx, off, n):
    g = X.Guarded(ctx, n, before=off, name="fill_random")
    ctx.fill_random(g.buf, n, 77, off=g.off)
    same(g.check(), splitmix_canonical(77, n))
    g.free()


@pytest.mark.parametrize("off,n", OFF_N)
def test_copy(ctx, rng, off, n):
    v = rand_field(rng, n)
    src, snap = held(ctx, v, "copy src", before=11 - off)
    dst = X.Guarded(ctx, n, before=off, name="copy dst")
    ctx.copy(dst.buf, src.buf, n, dst_off=dst.off, src_off=src.off)
    same(dst.check(), v)
    X.assert_preserved(src, snap)
    src.free(), dst.free()


# 524289: one past 2048 blocks x 256 lanes -- the grid-stride loop takes a second trip
@pytest.mark.parametrize("n", [1, 255, 257, 524289])
def test_field_batches(ctx, oracle, rng, n):
    a, b = rand_field(rng, 2 * n), rand_field(rng, 2 * n)
    a[n // 2] = 0  # inv: 0 maps to 0
    ga, sa = held(ctx, a, "a")
    gb, sb = held(ctx, b, "b")
    for op in ("add", "sub", "mul", "inv"):
        out = X.Guarded(ctx, n, name="field " + op)
        ctx.field_op(op, ga.buf, None if op == "inv" else gb.buf, out.buf, n)
        same(out.check(), oracle.batch_inv(a[:n]) if op == "inv" else oracle.batch_op(op, a[:n], b[:n]), op)
        out.free()
    assert int(oracle.batch_inv(a[:n])[n // 2]) == 0
    out = X.Guarded(ctx, 2 * n, name="ext_mul")
    ctx.ext_mul(ga.buf, gb.buf, out.buf, n)
    same(out.check(), oracle.ext_mul(a, b), "ext_mul")
    out.free()
    X.assert_preserved(ga, sa), X.assert_preserved(gb, sb)
    ga.free(), gb.free()


def ntt_case(ctx, oracle, rng, log_n, cols, inverse, order):
    """cols columns at offset 33 and column stride n + 7: the gaps, the guard before and the guard behind stay poison"""
    n, off = 1 << log_n, 33
    stride = n + 7
    extent = (cols - 1) * stride + n
    x = rand_field(rng, (cols, n))
    perm = bitrev_perm(log_n)
    g = X.Guarded(ctx, extent, before=off, shape=(1, extent), name="ntt 2^%d" % log_n)
    mask = np.zeros(extent, dtype=bool)
    for c in range(cols):
        mask[c * stride: c * stride + n] = True
        g.buf.upload(x[c][perm] if (inverse and order) else x[c], off=off + c * stride)  # an inverse in BITREV order takes its input bit-reversed
    ctx.ntt(g.buf, log_n, cols, inverse=inverse, order=order, off=off, col_stride=stride)
    ext = g.check(written=mask)
    got = np.stack([ext[c * stride: c * stride + n] for c in range(cols)])
    if order and not inverse:
        got = got[:, perm]  # a forward result in BITREV order is left bit-reversed
    same(got, oracle.ntt(x, inverse=inverse), "ntt")
    g.free()


@pytest.mark.parametrize("log_n", [1, 9, 12, 13, 16])
def test_ntt_strided(ctx, oracle, rng, log_n):
    ntt_case(ctx, oracle, rng, log_n, 3, False, 0)


@pytest.mark.parametrize("inverse,order", [(False, 1), (True, 0), (True, 1)])
def test_ntt_strided_two_passes_every_direction(ctx, oracle, rng, inverse, order):
    ntt_case(ctx, oracle, rng, 13, 3, inverse, order)


def test_ntt_strided_three_passes(ctx, oracle, rng):
    ntt_case(ctx, oracle, rng, 21, 2, False, 0)


@pytest.mark.parametrize("log_n,rate_bits,cols", [(0, 1, 1), (0, 3, 2), (3, 3, 4), (12, 1, 3), (13, 3, 2)])
def test_lde(ctx, oracle, rng, log_n, rate_bits, cols):
    n, N = 1 << log_n, 1 << (log_n + rate_bits)
    vals = rand_field(rng, (cols, n))
    leaves, coeffs = oracle.lde_from_values(vals, rate_bits, 7)
    want = leaves[bitrev_perm(log_n + rate_bits)].T  # plonky2 leaf j = natural row bitrev(j)
    for kind, data in ((0, vals), (1, coeffs)):
        src, snap = held(ctx, data, "lde src (kind %d)" % kind)
        dst = X.Guarded(ctx, N * cols, shape=(cols, N), name="lde dst (kind %d)" % kind)
        co = X.Guarded(ctx, n * cols, shape=(cols, n), name="lde coeffs_out (kind %d)" % kind)
        ctx.lde(src.buf, log_n, cols, rate_bits, dst.buf, shift=7, src_kind=kind, coeffs_out=co.buf)
        same(dst.check(), want, "dst")
        same(co.check(), coeffs, "coeffs_out")
        X.assert_preserved(src, snap)
        src.free(), dst.free(), co.free()


@pytest.mark.parametrize("n", [1, 255, 257])
def test_poseidon(ctx, oracle, rng, n):
    s = rand_field(rng, (n, 12))
    g = X.Guarded.holding(ctx, s, name="poseidon states")
    ctx.poseidon(g.buf, n)
    same(g.check(), oracle.poseidon(s))
    g.free()


_poseidon_ref = {}


def poseidon_air_ref(n_perm):
    """PoseidonAir's witness of the first n_perm of 512 seeded permutations (the reference generator runs once)"""
    import air_programs as AP

    if not _poseidon_ref:
        trace, _, pairs = AP.poseidon_trace(14)
        _poseidon_ref["trace"], _poseidon_ref["inputs"] = trace, np.array([p[0] for p in pairs], dtype=np.uint64)
    return _poseidon_ref["trace"][:, : 32 * n_perm], _poseidon_ref["inputs"][:n_perm]


@pytest.mark.parametrize("n_perm", [1, 2, 256, 512])
def test_poseidon_air_trace(ctx, n_perm):
    want, inputs = poseidon_air_ref(n_perm)
    states, snap = held(ctx, inputs, "poseidon air states")
    out = X.Guarded(ctx, 48 * 32 * n_perm, shape=(48, 32 * n_perm), name="poseidon air trace")
    ctx.poseidon_air_trace(states.buf, n_perm, out=out.buf)
    same(out.check(), want)
    X.assert_preserved(states, snap)
    states.free(), out.free()


@pytest.mark.parametrize("log_n,arity_bits", [(1, 1), (3, 1), (5, 5), (9, 4), (12, 3)])
def test_fri_fold(ctx, oracle, rng, log_n, arity_bits):
    n, shift = 1 << log_n, 7
    coeffs, beta = rand_field(rng, 2 * n), rand_field(rng, 2)
    evals, snap = held(ctx, oracle.ext_coset_ntt(coeffs, shift), "fri_fold evals")
    out = X.Guarded(ctx, 2 * (n >> arity_bits), name="fri_fold out")
    ctx.fri_fold(evals.buf, log_n, arity_bits, beta, shift, out.buf)
    same(out.check(), oracle.ext_coset_ntt(oracle.fri_fold_coeffs(coeffs, arity_bits, beta), pow(shift, 1 << arity_bits, P)))
    X.assert_preserved(evals, snap)
    evals.free(), out.free()


@pytest.mark.parametrize("R,log_n,chunk", [(1, 0, 1), (5, 3, 2), (13, 9, 8), (7, 13, 3)])
def test_partial_products(ctx, rng, R, log_n, chunk):
    from oracle import pyref

    n, m = 1 << log_n, (R + chunk - 1) // chunk
    wires, sigmas = rand_field(rng, (R, n)), rand_field(rng, (R, n))
    k_is = [pow(7, j, P) for j in range(R)]
    beta, gamma = int(rand_field(rng, 1)[0]), int(rand_field(rng, 1)[0])
    gw, sw = held(ctx, wires, "wires")
    gs, ss = held(ctx, sigmas, "sigmas")
    out = X.Guarded(ctx, m * n, shape=(m, n), name="partial products")
    ctx.partial_products(gw.buf, gs.buf, log_n, R, k_is, beta, gamma, chunk, out=out.buf)
    want, _ = pyref.partial_products([[int(v) for v in r] for r in wires], [[int(v) for v in r] for r in sigmas], k_is, beta, gamma, chunk)
    same(out.check(), np.array(want, dtype=np.uint64))
    X.assert_preserved(gw, sw), X.assert_preserved(gs, ss)
    gw.free(), gs.free(), out.free()


QUOTIENT = [("VX_AIR_MIX", 4, 1), ("VX_AIR_MIX", 4, 3), ("VX_AIR_MIX", 8, 1), ("VX_AIR_MIX", 8, 3), ("VX_AIR_LOOKUP", 8, 1), ("VX_AIR_LOOKUP", 8, 3)]


@pytest.mark.parametrize("name,log_n,r", QUOTIENT, ids=["%s-L%d-r%d" % c for c in QUOTIENT])
def test_quotient_eval(ctx, vx, oracle, name, log_n, r):
    import quotient_arbitrary as QA

    air, lde, pub, chal, apub, pairs = QA.arbitrary(name, log_n, r)
    N = 1 << (log_n + r)
    alphas = pairs[0][1]
    buf, snap = held(ctx, lde, "quotient lde")
    out = X.Guarded(ctx, 2 * N, shape=(2, N), name="quotient values")
    got = ctx.quotient_eval(QA.air_id(vx.lib, name), r, buf.buf, log_n, alphas, pub, challenges=chal, aux_public=apub, out=out.buf)
    want = QA.reference(air, lde, pub, chal, apub, alphas, log_n, r)
    same(out.check(), want)
    assert (got == want).all()  # what the wrapper hands back is the extent
    X.assert_preserved(buf, snap)
    buf.free(), out.free()


def test_quotient_eval_without_an_auxiliary_round(ctx, vx, oracle):
    """vx_quotient_eval (the entry point of the AIRs without an auxiliary round) into a caller's buffer"""
    import quotient_arbitrary as QA

    air, lde, pub, _, _, pairs = QA.arbitrary("VX_AIR_MIX", 8, 1)
    buf, snap = held(ctx, lde, "quotient lde")
    out = X.Guarded(ctx, 2 << 9, shape=(2, 1 << 9), name="quotient values")
    ctx.quotient_eval(vx.lib.VX_AIR_MIX, 1, buf.buf, 8, pairs[0][1], pub, out=out.buf)
    same(out.check(), QA.reference(air, lde, pub, [], [], pairs[0][1], 8, 1))
    X.assert_preserved(buf, snap)
    buf.free(), out.free()


def aux_case(ctx, air_id, trace, log_n, n_aux, pub, want_aux, name):
    tb, snap = held(ctx, trace, name + " trace")
    out = X.Guarded(ctx, n_aux << log_n, shape=(n_aux, 1 << log_n), name=name + " aux")
    _, apub = ctx.stark_aux_trace(air_id, tb.buf, log_n, CHAL, n_aux, public_inputs=pub, out=out.buf)
    same(out.check(), want_aux, name + " aux")
    X.assert_preserved(tb, snap)
    tb.free(), out.free()
    return apub


def test_stark_aux_trace_lookup(ctx, oracle):
    from oracle import stark_ref as S

    trace, pub = S.LookupAir.trace(8)
    aux_case(ctx, S.LookupAir.ID, trace, 8, S.LookupAir.AUX, pub, S.LookupAir.gen_aux(trace, CHAL)[0], "LookupAir")


# ------------------------------------------------------------------------------------------------ Merkle trees: guarded inputs
# n_leaves < 16: the surplus groups of the cooperative leaf kernel redo the last leaf; 32768 x 17 in layout 1 is the one-lane kernel
# in the production layout
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("leaf_len", [5, 17])
@pytest.mark.parametrize("n_leaves", [1, 2, 8, 32768])
def test_merkle_keeps_its_input(ctx, vx, oracle, rng, n_leaves, leaf_len, layout):
    from test_gpu_leaf_sponge import in_layout

    leaves = rand_field(rng, (n_leaves, leaf_len))
    cap_h = min(2, n_leaves.bit_length() - 1)
    data, snap = held(ctx, in_layout(vx, leaves, layout), "merkle data", before=13)
    t = ctx.merkle(data.buf, n_leaves, leaf_len, layout, cap_h, off=data.off)
    want = oracle.MerkleTree(leaves, cap_h)
    same(t.cap(), want.cap, "cap")
    same(t.leaf_digests(), want.leaf_digests(), "leaf digests")
    X.assert_preserved(data, snap)
    t.free(), data.free()


@pytest.mark.parametrize("arity_bits", [3, 4])
@pytest.mark.parametrize("n_leaves", [1, 2, 8, 32768])
def test_fri_layer_tree_keeps_its_input(ctx, oracle, rng, n_leaves, arity_bits):
    log_n = n_leaves.bit_length() - 1 + arity_bits
    vals = rand_field(rng, (1 << log_n, 2))
    cap_h = min(2, n_leaves.bit_length() - 1)
    evals, snap = held(ctx, vals, "fri layer")
    t = ctx.fri_layer_tree(evals.buf, log_n, arity_bits, cap_h)
    want = oracle.MerkleTree(vals[bitrev_perm(log_n)].reshape(-1, 2 << arity_bits), cap_h)
    same(t.cap(), want.cap, "cap")
    same(t.leaf_digests(), want.leaf_digests(), "leaf digests")
    X.assert_preserved(evals, snap)
    t.free(), evals.free()


# ----------------------------------------------------------------------------------------- trace generators of the statements
def trace_out(ctx, cols, log_n, name):
    return X.Guarded(ctx, cols << log_n, shape=(cols, 1 << log_n), name=name + " trace")


def edge_chain(sizes, first=50000):
    """a chain of headers of the given byte lengths (the chunk boundaries of the Blake2b table)"""
    trusted = hashlib.sha256(b"edge").digest()
    msgs, d = [], trusted
    for k, n in enumerate(sizes):
        m = d + (4 * (first + k) + 2).to_bytes(4, "little") + bytes((7 * i + n) & 0xFF for i in range(n - 36))
        msgs.append(m)
        d = hashlib.blake2b(m, digest_size=32).digest()
    hdr = np.zeros((len(msgs), 384), dtype=np.uint8)
    for i, m in enumerate(msgs):
        hdr[i, : len(m)] = np.frombuffer(m, dtype=np.uint8)
    return hdr, 384, [len(m) for m in msgs], msgs, trusted, first


@pytest.mark.parametrize("case", ["one_header", "sizes_36_128_129_257"])
def test_blake_chain_trace(ctx, vx, oracle, case):
    from oracle import blake_air as B

    if case == "one_header":
        ch = vx.synth.Chain(1, profile="Ptiny", stride=512)
        hdr, stride, sizes, trusted, first = ch.headers, 512, ch.sizes, ch.trusted_hash, ch.trusted_block + 1
        msgs = [ch.headers[i, : ch.sizes[i]].tobytes() for i in range(ch.n)]
    else:
        hdr, stride, sizes, msgs, trusted, first = edge_chain((36, 128, 129, 257))
    hb, snap = held(ctx, hdr, "headers")
    out = trace_out(ctx, B.COLS, 16, "BlakeChainAir")
    _, pub, dig = ctx.blake_chain_trace(hb.buf, stride, sizes, trusted, first, 16, trace_buf=out.buf)
    want, wpub, _ = B.gen_trace(msgs, 16, trusted)
    same(out.check(), want)
    assert [int(x) for x in pub] == wpub and [d.tobytes() for d in dig] == [hashlib.blake2b(m, digest_size=32).digest() for m in msgs]
    X.assert_preserved(hb, snap)
    hb.free(), out.free()


@pytest.mark.parametrize("n_keys,log_n", [(1, 6), (5, 10)])
def test_sha_chain_trace(ctx, oracle, n_keys, log_n):
    from oracle import sha_air as A

    pks = [hashlib.sha256(bytes([i, 9])).digest() for i in range(n_keys)]
    signed = [(i % 3) != 1 for i in range(n_keys)]
    out = trace_out(ctx, A.CHAIN_COLS, log_n, "ShaChainAir")
    _, pub, _ = ctx.sha_chain_trace(pks, log_n, trace_buf=out.buf, signed=signed, bus_on=1)
    want, wpub, _ = A.gen_trace(pks, log_n, signed=signed, bus_on=1)
    same(out.check(), want)
    assert [int(x) for x in pub] == wpub
    out.free()


def test_ed_trace_and_its_auxiliary_columns(ctx, vx, oracle):
    """one key at 2^16 rows: 255 of the 256 slots are idle and must be stored all the same.  The one large download of this file;
    the trace stays on the device as the input of vx_stark_aux_trace (ED25519[16]), which must leave it alone"""
    from oracle import ed_air as E
    from test_gpu_ed_air import MSG, signatures

    keys, sigs, flags, recs = signatures(1, unsigned=())
    want, wpub = E.gen_trace(recs, 16, bus_on=1)
    tb = trace_out(ctx, E.COLS, 16, "EdAir")
    assert E.COLS == vx.lib.VX_ED_AIR_COLS
    _, pub = ctx.ed_trace(keys, sigs, MSG, flags, 16, bus_on=1, trace_buf=tb.buf)
    same(tb.check(), want)
    assert [int(x) for x in pub] == wpub
    snap = tb.last
    aux = X.Guarded(ctx, E.AUX << 16, shape=(E.AUX, 1 << 16), name="EdAir aux")
    _, apub = ctx.stark_aux_trace(E.IDS[16], tb.buf, 16, CHAL, E.AUX, public_inputs=pub, out=aux.buf)
    waux, wapub = E.gen_aux(want, CHAL, wpub)
    same(aux.check(), waux, "EdAir aux")
    assert [int(x) for x in apub[:2]] == wapub
    X.assert_preserved(tb, snap)
    tb.free(), aux.free()


def test_sha512_trace_and_its_auxiliary_columns(ctx, vx, oracle):
    from oracle import sha512_air as H
    from test_gpu_ed_air import MSG, signatures

    keys, sigs, flags, _ = signatures(5)
    slots = [(sg[:32], k) for k, sg, f in zip(keys, sigs, flags) if f]
    want, wpub, _ = H.gen_trace(slots, MSG, 10, bus_on=1)
    tb = trace_out(ctx, H.COLS, 10, "Sha512Air")
    _, pub = ctx.sha512_trace(keys, sigs, MSG, flags, 10, bus_on=1, trace_buf=tb.buf)
    same(tb.check(), want)
    assert [int(x) for x in pub] == wpub
    tb.free()
    apub = aux_case(ctx, H.IDS[10], want, 10, H.AUX, wpub, H.gen_aux(want, CHAL, wpub)[0], "Sha512Air")
    assert [int(x) for x in apub[:2]] == H.gen_aux(want, CHAL, wpub)[1]


def test_epoch_end_trace(ctx, vx, oracle):
    from oracle import epoch_air as EP

    e = vx.synth.EpochEndHeader(140000, 1)
    hb, snap = held(ctx, e.padded, "epoch-end header")
    assert EP.COLS == vx.lib.VX_EPOCH_END_AIR_COLS
    out = trace_out(ctx, EP.COLS, EP.LOG_N, "EpochEndAir")
    _, pub, wlen = ctx.epoch_end_trace(hb.buf, e.start_position, 1, bus_on=1, trace_buf=out.buf)
    want, wpub, _, plen = EP.gen_trace(e.bytes, e.start_position, 1)
    same(out.check(), want)
    assert [int(x) for x in pub] == wpub and wlen == plen + 40 + 4
    X.assert_preserved(hb, snap)
    hb.free(), out.free()


# ------------------------------------------------------------------------------------------- the tables of the aggregation buses
# each at the smallest shape of its own GPU test, once full and once with at least half of the rows idle
FILL = {"full": 0, "half_idle": 1}  # the extra log2 of rows


@pytest.mark.parametrize("fill", list(FILL))
def test_merkle_open_air_trace(ctx, vx, oracle, fill):
    import merkle_open_ref as M
    from test_gpu_merkle_open import trees

    D, cap_h, idx = 1, 0, [1]
    gtree, rtree = trees(ctx, vx, oracle, D, cap_h)
    log_n = M.log_rows(len(idx), D) + FILL[fill]
    want, wpub, _ = M.ref_trace(rtree, idx, log_n)
    assert int(want[M.ACT].sum()) == want.shape[1] >> FILL[fill]
    out = trace_out(ctx, M.COLS, log_n, "MerkleOpenAir")
    _, pub = ctx.merkle_open_air_trace(gtree, idx, log_n, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    gtree.free(), out.free()


@pytest.mark.parametrize("fill", list(FILL))
def test_leaf_sponge_air_trace(ctx, vx, oracle, fill):
    import leaf_sponge_ref as R

    D, L, idx = 3, 5, [5]
    leaves = np.random.default_rng(7 + 10 * D + 1000 * L).integers(0, P, size=(1 << D, L), dtype=np.uint64)
    data, snap = held(ctx, leaves, "leaves", before=9)
    log_n = R.log_rows(len(idx), L) + FILL[fill]
    want, wpub, _ = R.ref_trace(idx, leaves[idx], log_n)
    out = trace_out(ctx, R.COLS, log_n, "LeafSpongeAir")
    _, pub = ctx.leaf_sponge_air_trace(data.buf, 1 << D, L, vx.lib.VX_LEAVES_ROW_MAJOR, idx, log_n, off=data.off, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    X.assert_preserved(data, snap)
    data.free(), out.free()


@pytest.mark.parametrize("fill", list(FILL))
def test_fri_query_set_tables(ctx, vx, oracle, fill):
    """MerkleOpenSetAir and LeafSpongeSetAir over the layer of the smallest commit phase (LN 5, one layer, one query)"""
    import fri_queries_ref as Q
    from test_gpu_fri_queries import case_of, phase, ref_trees

    LN, NL = 5, 1
    index, cap_h, _ = case_of(LN, NL, "single")
    layers, values = phase(LN, NL)[2], phase(LN, NL)[3]
    rtrees = ref_trees(LN, NL, cap_h)
    tree_of, leaf_idx = Q.openings_of(index, NL)
    rows = [Q.layer_rows(layers)[t][i] for t, i in zip(tree_of, leaf_idx)]
    evals = [held(ctx, v, "layer %d" % l) for l, v in enumerate(values)]
    gtrees = [ctx.fri_layer_tree(evals[l][0].buf, LN - 4 * l, 4, cap_h) for l in range(NL)]
    want, wpub = Q.open_ref_trace(rtrees, tree_of, leaf_idx)
    log_n = want.shape[1].bit_length() - 1 + FILL[fill]
    want, wpub = Q.open_ref_trace(rtrees, tree_of, leaf_idx, log_n)
    out = trace_out(ctx, Q.O_COLS, log_n, "MerkleOpenSetAir")
    _, pub = ctx.merkle_open_set_air_trace(gtrees, tree_of, leaf_idx, log_n, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()
    want, wpub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows)
    log_n = want.shape[1].bit_length() - 1 + FILL[fill]
    want, wpub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows, log_n)
    out = trace_out(ctx, Q.S_COLS, log_n, "LeafSpongeSetAir")
    _, pub = ctx.leaf_sponge_set_air_trace([g.buf for g, _ in evals], [LN - 4 * (l + 1) for l in range(NL)], tree_of, leaf_idx, log_n, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()
    for g, snap in evals:
        X.assert_preserved(g, snap)
        g.free()
    for t in gtrees:
        t.free()


@pytest.mark.parametrize("fill", list(FILL))
def test_merkle_paths_air_trace(ctx, vx, oracle, fill):
    import fri_queries_ref as Q
    import stark_openings_ref as SO
    from test_gpu_stark_openings import PATH_CASES, forest

    name = "one_path_depth_1"
    depths, cap_h, openings = PATH_CASES[name]
    trees, digests, sibs = forest(oracle, name)
    tree_of, leaf_idx = [t for t, _ in openings], [i for _, i in openings]
    caps = [t.cap for t in trees]
    want, wpub, _ = SO.paths_ref_trace(caps, depths, tree_of, leaf_idx, digests, sibs)
    log_n = want.shape[1].bit_length() - 1 + FILL[fill]
    want, wpub, _ = SO.paths_ref_trace(caps, depths, tree_of, leaf_idx, digests, sibs, log_n)
    out = trace_out(ctx, Q.O_COLS, log_n, "MerkleOpenSetAir from paths")
    _, pub = ctx.merkle_paths_air_trace(caps, depths, tree_of, leaf_idx, digests, sibs, log_n, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()


@pytest.mark.parametrize("fill", list(FILL))
def test_leaf_sponge_rows_air_trace(ctx, vx, oracle, fill):
    import fri_queries_ref as Q

    L, n_leaves = 5, 1
    rng = np.random.default_rng(100 * L + n_leaves)
    rows = rng.integers(0, P, size=(n_leaves, L), dtype=np.uint64)
    rows[0, 0], rows[-1, -1] = 0, P - 1
    tree_of, leaf_idx = [9], [0]
    want, wpub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows)
    log_n = want.shape[1].bit_length() - 1 + FILL[fill]
    want, wpub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows, log_n)
    out = trace_out(ctx, Q.S_COLS, log_n, "LeafSpongeSetAir from rows")
    _, pub = ctx.leaf_sponge_rows_air_trace(tree_of, leaf_idx, rows, log_n, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()


@pytest.mark.parametrize("n_idx", [32, 16], ids=["full", "half_idle"])
def test_leaf_noop_air_trace(ctx, vx, n_idx):
    import leaf_noop_ref as N
    from test_gpu_leaf_noop import openings

    trees, index, rows = openings(n_idx)
    want, wpub = N.ref_trace(trees, index, rows, 5)
    assert int(want[N.ACT].sum()) == n_idx
    out = trace_out(ctx, N.COLS, 5, "LeafNoopAir")
    _, pub = ctx.leaf_noop_air_trace(trees, index, rows, 5, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()


@pytest.mark.parametrize("fill", list(FILL))
def test_fri_fold_air_trace(ctx, vx, oracle, fill):
    import fri_fold_ref as F
    from test_gpu_fri_fold import SHAPES, case_queries, rand_claims

    LN, NL = SHAPES["NL1_FB1"]
    index, log_n = case_queries(LN, NL, fill)
    betas, leaves = rand_claims(LN, NL, index)
    ev0 = F.ev0_of(index, leaves)
    want, wpub = F.ref_trace(index, leaves, betas, LN, log_n, 0)
    out = trace_out(ctx, F.COLS, log_n, "FriFoldAir")
    _, pub = ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, log_n, 0, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()


@pytest.mark.parametrize("fill", list(FILL))
@pytest.mark.parametrize("absn", [2, 257])
def test_fri_combine_air_trace(ctx, vx, oracle, absn, fill):
    import fri_combine_ref as K
    from test_gpu_fri_combine import SHAPES, case_queries

    LN, cm, ca, nq = SHAPES[absn]
    index, log_n = case_queries(absn + LN, LN, fill)
    st = K.rand_statement(LN, cm, ca, nq, seed=absn)
    rows, ev0 = K.rand_claims(st, index, seed=absn + 1)
    want, wpub = K.ref_trace(st, index, rows, log_n, K.TREE0)
    out = trace_out(ctx, K.COLS, log_n, "FriCombineAir")
    _, pub = ctx.fri_combine_air_trace(LN, st["r"], cm, ca, nq, st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"], index, rows, ev0, log_n, K.TREE0, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub
    out.free()


@pytest.mark.parametrize("fill", list(FILL))
def test_transcript_air_trace(ctx, vx, oracle, fill):
    import transcript_ref as T

    chains = T.synth_chains(["one_block"])
    log_n = 5 + FILL[fill]
    want, wpub, claims = T.ref_table(chains, log_n)
    assert int(want[T.ACT].sum()) == want.shape[1] >> FILL[fill]
    out = trace_out(ctx, T.COLS, log_n, "TranscriptAir")
    _, pub, chal = ctx.transcript_air_trace([ops for ops, _ in chains], [w for _, w in chains], log_n, out=out.buf)
    same(out.check(), want)
    assert [int(v) for v in pub] == wpub and [[int(v) for v in c] for c in chal] == [[v for _, v in chals] for _, chals in claims]
    out.free()


# ------------------------------------------------------------------------------------------------- provers keep their inputs
@pytest.mark.parametrize("air_name,log_n", [("FibAir", 5), ("LookupAir", 8)])
def test_stark_prove_keeps_its_trace(ctx, oracle, air_name, log_n):
    from oracle import stark_ref as S

    air = getattr(S, air_name)
    trace, pub = air.trace(log_n)
    tb, snap = held(ctx, trace, air_name + " trace")
    got = ctx.stark_prove(air.ID, tb.buf, log_n, pub)
    same(got, S.prove(air, trace, pub), "proof")
    X.assert_preserved(tb, snap)
    tb.free()


def test_bus_group_prove_keeps_its_traces(ctx, vx):
    """the smallest two-table group: a run-time sender [3][2^5] and receiver [3][2^7].  A vx_bus_table's trace must be a buffer of
    EXACTLY cols << log_n words (include/vx.h), so these two inputs cannot carry a guard: their words are compared, nothing around them"""
    from test_gpu_bus_group import air_id, closed_pair

    snd, rcv = closed_pair()
    sid, rid = air_id(vx, "sender"), air_id(vx, "receiver")
    (sb, ssnap), (rb, rsnap) = held(ctx, snd, "sender trace", after=0), held(ctx, rcv, "receiver trace", after=0)
    cfg = ctx.stark_config(num_queries=8)
    tables = [(sid, sb.buf, 5, []), (rid, rb.buf, 7, [])]
    blob = ctx.bus_group_prove(tables, cfg)
    vx.lib.bus_group_verify(blob, [(sid, []), (rid, [])], cfg)
    X.assert_preserved(sb, ssnap), X.assert_preserved(rb, rsnap)
    longer = X.Guarded.holding(ctx, snd)
    with pytest.raises(vx.VxError, match="not cols << log_n words"):  # ... and a guarded trace is refused, as the header says
        ctx.bus_group_prove([(sid, longer.buf, 5, []), tables[1]], cfg)
    sb.free(), rb.free(), longer.free()


def test_header_range_prove_keeps_its_headers(ctx, vx, oracle):
    from oracle import stark_ref as S
    from test_gpu_blake_air import oracle_verify_blob

    ch = vx.synth.Chain(16, profile="Ptiny", stride=512)
    cfg, ocfg = ctx.stark_config(num_queries=6), dict(S.DEFAULT_CFG, num_queries=6)
    hb, snap = held(ctx, ch.headers, "headers")
    out96, blob = ctx.header_range_prove(hb.buf, 512, ch.sizes, 16, ch.trusted_block, ch.trusted_hash, ch.target_block, cfg)
    assert out96 == ch.expected_outputs(16)
    oracle_verify_blob(vx, blob, ocfg, 16)
    vx.lib.header_range_verify(blob, 16, ch.trusted_block, ch.trusted_hash, ch.target_block, out96, cfg)
    X.assert_preserved(hb, snap)
    hb.free()
