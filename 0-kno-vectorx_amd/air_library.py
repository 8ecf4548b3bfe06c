"""Constraint programs that ship with the library (written with air_program.AirBuilder, registered with vx_air_register):
the two tables a recursive STARK verifier is mostly made of (plonky2 v0.2.0 hash/poseidon.rs, hash/merkle_proofs.rs).

  poseidon_builder()        PoseidonAir   -- the Poseidon-Goldilocks permutation (width 12, x^7, 4 + 22 + 4 rounds), one round per row
  merkle_path_builder(d)    MerklePathAir -- verify_merkle_proof_to_cap for a cap of height 0: d levels, one PoseidonAir block each
  sponge_builder(k)         SpongeAir     -- hash_n_to_hash_no_pad of 8 k words (the leaf hash of a Merkle tree): k blocks, overwrite mode
  fri_exit_builder()        FriExitAir    -- an inner proof's query indices, proof of work and FRI exits; on a bus, with declared messages

Each returns an AirBuilder (`.register()` gives the AIR id; `.assemble()` the code).  The witness (trace) of these tables is the
host's to fill: tests/air_programs.py has reference generators; tests/test_gpu_air_program.py proves a path of a GPU-built tree.
FriExitAir's witness is the library's (Context.fri_exit_air_trace)."""
import importlib.util
import os

from . import air_program as ap

P = 2**64 - 2**32 + 1

MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8] + [0] * 11


def poseidon_round_constants():
    """the 360 round constants of plonky2's Poseidon as tools/gen_poseidon_constants.py derives them (ChaCha8Rng, seed 0) -- the same
    generator that writes csrc/poseidon_constants.h"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_poseidon_constants.py")
    spec = importlib.util.spec_from_file_location("_vx_gen_rc_lib", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.round_constants()


def poseidon_builder():
    """columns s[12] (state entering the round), a = x^2, b = a^2, t = x a b = x^7 with x = s + round constant (periodic);
    y_i = t_i in full rounds and for i = 0, x_i otherwise; next s = MDS y on the 30 round rows, next s = s on the output row (32 rows per
    permutation); public inputs: the first permutation's input (12) and the last one's output (12)."""
    rc = poseidon_round_constants()
    per = [[rc[12 * r + i] if r < 30 else 0 for r in range(32)] for i in range(12)]
    per.append([1 if (r < 4 or 26 <= r < 30) else 0 for r in range(32)])  # full
    per.append([1 if r < 30 else 0 for r in range(32)])                   # a round row
    per.append([1 if r == 30 else 0 for r in range(32)])                  # the output row: the state is carried to the spare row
    b = ap.AirBuilder(48, 24, periodic=per)
    full, act, out = b.per(12), b.per(13), b.per(14)
    x = [b.loc(i) + b.per(i) for i in range(12)]
    a, bb, t = [b.loc(12 + i) for i in range(12)], [b.loc(24 + i) for i in range(12)], [b.loc(36 + i) for i in range(12)]
    for i in range(12):
        b.assert_zero(a[i] - x[i] * x[i])
    for i in range(12):
        b.assert_zero(bb[i] - a[i] * a[i])
    for i in range(12):
        b.assert_zero(t[i] - x[i] * a[i] * bb[i])
    y = [t[0]] + [full * t[i] + (1 - full) * x[i] for i in range(1, 12)]
    for row in range(12):
        acc = y[row] * (MDS_CIRC[0] + MDS_DIAG[row])
        for i in range(1, 12):
            acc = acc + y[(i + row) % 12] * MDS_CIRC[i]
        b.assert_zero(act * (b.nxt(row) - acc))
    for i in range(12):
        b.assert_zero(out * (b.nxt(i) - b.loc(i)))
    for i in range(12):
        b.assert_first(b.loc(i) - b.pub(i))
    for i in range(12):
        b.assert_last(b.loc(i) - b.pub(12 + i))
    return b


M_BIT, M_SIB, M_IDX, M_COLS = 48, 49, 53, 54


def merkle_path_builder(depth):
    """The leaf digest is hashed upwards with its siblings, one PoseidonAir block (32 rows) per level: next input = (cur, sib) or
    (sib, cur) by the level's index bit, zero capacity; columns 48 = bit, 49..52 = sibling, 53 = index so far; public inputs: leaf
    digest (4), root (4), leaf index."""
    n = 32 * depth
    assert n & (n - 1) == 0, "32 * depth rows must be a power of two"
    rc = poseidon_round_constants()
    per = [[rc[12 * r + i] if r < 30 else 0 for r in range(32)] for i in range(12)]
    per.append([1 if (r < 4 or 26 <= r < 30) else 0 for r in range(32)])  # 12 full
    per.append([1 if r < 30 else 0 for r in range(32)])                   # 13 a round row
    per.append([1 if r == 30 else 0 for r in range(32)])                  # 14 the output row
    per.append([1 if r == 31 else 0 for r in range(32)])                  # 15 the spare row (holds the level's output)
    per.append([1 if (r % 32 == 31 and r != n - 1) else 0 for r in range(n)])        # 16 link: spare rows but the last (period = the trace)
    per.append([(1 << (r // 32 + 1)) if (r % 32 == 31 and r != n - 1) else 0 for r in range(n)])  # 17 weight of the NEXT level's index bit
    b = ap.AirBuilder(M_COLS, 9, periodic=per)
    full, act, out, spare, link, pown = (b.per(q) for q in range(12, 18))
    x = [b.loc(i) + b.per(i) for i in range(12)]
    a, bb, t = [b.loc(12 + i) for i in range(12)], [b.loc(24 + i) for i in range(12)], [b.loc(36 + i) for i in range(12)]
    for i in range(12):
        b.assert_zero(a[i] - x[i] * x[i])
    for i in range(12):
        b.assert_zero(bb[i] - a[i] * a[i])
    for i in range(12):
        b.assert_zero(t[i] - x[i] * a[i] * bb[i])
    y = [t[0]] + [full * t[i] + (1 - full) * x[i] for i in range(1, 12)]
    for row in range(12):
        acc = y[row] * (MDS_CIRC[0] + MDS_DIAG[row])
        for i in range(1, 12):
            acc = acc + y[(i + row) % 12] * MDS_CIRC[i]
        b.assert_zero(act * (b.nxt(row) - acc))
    for i in range(12):
        b.assert_zero(out * (b.nxt(i) - b.loc(i)))
    bit, bit_n = b.loc(M_BIT), b.nxt(M_BIT)
    b.assert_zero(bit * (bit - 1))
    # the next level's input from this level's output (on the spare row) and the next row's (bit, sibling)
    for i in range(4):
        cur, sib_n = b.loc(i), b.nxt(M_SIB + i)
        d = bit_n * (sib_n - cur)
        b.assert_zero(link * (b.nxt(i) - cur - d))              # left  = bit ? sib : cur
        b.assert_zero(link * (b.nxt(4 + i) - sib_n + d))        # right = bit ? cur : sib
    for i in range(8, 12):
        b.assert_zero(link * b.nxt(i))
    b.assert_zero(link * (b.nxt(M_IDX) - b.loc(M_IDX) - bit_n * pown))
    b.assert_zero((1 - spare) * (b.nxt(M_IDX) - b.loc(M_IDX)))
    # first row: the leaf digest enters level 0; last row: the root and the index
    for i in range(4):
        leaf, sib = b.pub(i), b.loc(M_SIB + i)
        d = bit * (sib - leaf)
        b.assert_first(b.loc(i) - leaf - d)
        b.assert_first(b.loc(4 + i) - sib + d)
    for i in range(8, 12):
        b.assert_first(b.loc(i))
    b.assert_first(b.loc(M_IDX) - bit)
    for i in range(4):
        b.assert_last(b.loc(i) - b.pub(4 + i))
    b.assert_last(b.loc(M_IDX) - b.pub(8))
    return b




def sponge_builder(blocks):
    """SpongeAir: plonky2's hash_n_to_hash_no_pad (hash/hashing.rs: the sponge absorbs 8 words per permutation by OVERWRITING the
    rate part of the state, capacity carried; the digest is the first 4 words of the last output) for a message of 8 * blocks words
    -- what hashes an opened row into the leaf digest MerklePathAir starts from.  `blocks` PoseidonAir blocks (a power of two);
    public inputs: the message (8 * blocks words) then the digest (4)."""
    n = 32 * blocks
    assert blocks >= 1 and n & (n - 1) == 0 and 8 * blocks + 4 <= 64
    rc = poseidon_round_constants()
    per = [[rc[12 * r + i] if r < 30 else 0 for r in range(32)] for i in range(12)]
    per.append([1 if (r < 4 or 26 <= r < 30) else 0 for r in range(32)])  # 12 full
    per.append([1 if r < 30 else 0 for r in range(32)])                   # 13 a round row
    per.append([1 if r == 30 else 0 for r in range(32)])                  # 14 the output row
    for blk in range(1, blocks):                                           # 15.. : the spare row before block blk (period = the trace)
        per.append([1 if r == 32 * blk - 1 else 0 for r in range(n)])
    b = ap.AirBuilder(48, 8 * blocks + 4, periodic=per)
    full, act, out = b.per(12), b.per(13), b.per(14)
    x = [b.loc(i) + b.per(i) for i in range(12)]
    a, bb, t = [b.loc(12 + i) for i in range(12)], [b.loc(24 + i) for i in range(12)], [b.loc(36 + i) for i in range(12)]
    for i in range(12):
        b.assert_zero(a[i] - x[i] * x[i])
    for i in range(12):
        b.assert_zero(bb[i] - a[i] * a[i])
    for i in range(12):
        b.assert_zero(t[i] - x[i] * a[i] * bb[i])
    y = [t[0]] + [full * t[i] + (1 - full) * x[i] for i in range(1, 12)]
    for row in range(12):
        acc = y[row] * (MDS_CIRC[0] + MDS_DIAG[row])
        for i in range(1, 12):
            acc = acc + y[(i + row) % 12] * MDS_CIRC[i]
        b.assert_zero(act * (b.nxt(row) - acc))
    for i in range(12):
        b.assert_zero(out * (b.nxt(i) - b.loc(i)))
    # absorbing block blk: the rate part is overwritten with the next 8 message words, the capacity is carried
    for blk in range(1, blocks):
        sel = b.per(14 + blk)
        for i in range(8):
            b.assert_zero(sel * (b.nxt(i) - b.pub(8 * blk + i)))
        for i in range(8, 12):
            b.assert_zero(sel * (b.nxt(i) - b.loc(i)))
    for i in range(8):
        b.assert_first(b.loc(i) - b.pub(i))
    for i in range(8, 12):
        b.assert_first(b.loc(i))
    for i in range(4):
        b.assert_last(b.loc(i) - b.pub(8 * blocks + i))
    return b


# ---- FriExitAir.  The numbers below are csrc/fri_exit_layout.h's (tests/test_fri_exit.py compares the two).
FRI_EXIT_BLOCK, FRI_EXIT_HORNER_ROW, FRI_EXIT_MAX_FINAL_LEN = 128, 63, 64
(FRI_EXIT_BIT, FRI_EXIT_V, FRI_EXIT_F, FRI_EXIT_C, FRI_EXIT_EF, FRI_EXIT_C2, FRI_EXIT_G, FRI_EXIT_EB, FRI_EXIT_W, FRI_EXIT_X, FRI_EXIT_IDX, FRI_EXIT_T, FRI_EXIT_HF, FRI_EXIT_K,
 FRI_EXIT_CA, FRI_EXIT_CB, FRI_EXIT_ACC) = range(17)
FRI_EXIT_ACT, FRI_EXIT_ISPOW, FRI_EXIT_ORD, FRI_EXIT_COLS = 18, 19, 20, 21
(FRI_EXIT_P_FIRST, FRI_EXIT_P_LAST, FRI_EXIT_P_BIT, FRI_EXIT_P_WEIGHT, FRI_EXIT_P_HIGH, FRI_EXIT_P_HOLD, FRI_EXIT_P_LOW, FRI_EXIT_P_PRE, FRI_EXIT_P_R62,
 FRI_EXIT_PERIODIC) = range(10)
(FRI_EXIT_PUB_ORD_POW, FRI_EXIT_PUB_ABSORBED, FRI_EXIT_PUB_POW_BITS, FRI_EXIT_PUB_SKIP, FRI_EXIT_PUB_FB, FRI_EXIT_PUB_W, FRI_EXIT_PUB_G, FRI_EXIT_PUB_FINAL_LEN,
 FRI_EXIT_PUB_DIGEST) = range(9)
FRI_EXIT_PUB, FRI_EXIT_N_HELP, FRI_EXIT_AUX_COLS = 12, 2, 6
TAG_FRI, TAG_CHAL, TAG_FIN = 10, 13, 14  # csrc/air_bus.cuh


def fri_exit_periodic():
    """the nine position columns of a 128-row block, in the order of the FRI_EXIT_P_* indices"""
    rows = range(FRI_EXIT_BLOCK)
    return [[int(r == 0) for r in rows], [int(r == 127) for r in rows], [int(r < 64) for r in rows], [1 << (63 - r) if r < 64 else 0 for r in rows],
            [int(1 <= r < 32) for r in rows], [int(32 <= r < 63) for r in rows], [int(32 <= r < 64) for r in rows], [int(r < 63) for r in rows], [int(r == 62) for r in rows]]


def fri_exit_builder():
    """FriExitAir: what a verifier does with the challenges an inner proof's transcript yields behind the final polynomial.  One block
    of 128 rows per challenge value v of chain 0, received as chal(0, ordinal, absorbed, v) on the block's last row: block 0 the
    proof-of-work response (ordinal ORD_POW), block 1 + q the index challenge of query q.  Rows 0 .. 63 hold the bits of v, MSB first,
    boolean, their weighted sum v, and the integer they spell is below p (T: if the top 32 are all ones the low 32 are zero).  F is a
    prefix flag of a length the counter C forces exactly: the top pow_bits bits of the PoW response, which are zero, or the top 64 - LN
    bits of an index challenge, which the index (the weighted sum of the other bits) leaves out.  The FB rows behind F (EF, counter
    C2) are the exponent bits of the query's point behind the folds, x_NL = 7^(16^NL) w_FB^brev(index >> 4 NL, FB): the step of weight
    2^s comes s-th, so W is squared on every row and X takes it where the bit is set.  Rows 63 .. 62 + final_len (HF, counter K) are
    the Horner steps ACC' = ACC x + c_k of the final polynomial, every coefficient received as fin(k, c_k); the last row receives the
    exit fri(index, ACC, 1) of the query's fold chain.  Positional: nine periodic columns of period 128 (csrc/fri_exit_layout.h).
    Public inputs: ORD_POW, ABSORBED, pow_bits, 64 - LN, FB, w_FB, 7^(16^NL), final_len, four statement-digest words."""
    b = ap.AirBuilder(FRI_EXIT_COLS, FRI_EXIT_PUB, periodic=fri_exit_periodic())
    loc, nxt, pub = b.loc, b.nxt, b.pub
    first, last, pbit, weight, high, hold, low, pre, r62 = (b.per(q) for q in range(FRI_EXIT_PERIODIC))
    bit, v, f, c, ef, c2, g, eb, w, x, idx, t, hf, k, ca, cb = (loc(j) for j in range(16))
    acc, act, ispow, ordinal = [loc(FRI_EXIT_ACC), loc(FRI_EXIT_ACC + 1)], loc(FRI_EXIT_ACT), loc(FRI_EXIT_ISPOW), loc(FRI_EXIT_ORD)
    idxb, h, h_n = act - ispow, f + ef, nxt(FRI_EXIT_F) + nxt(FRI_EXIT_EF)
    inside = 1 - last
    # 1. boolean cells; no bit behind row 63
    for e in (bit, f, ef, h, hf, act, ispow):
        b.assert_zero(e * (e - 1))
    b.assert_zero(ispow * (1 - act))
    b.assert_zero((1 - pbit) * bit)
    # 2. the blocks: flags constant over a block, ordinals by position from ORD_POW, block 0 alone is the PoW block
    b.assert_zero(inside * (nxt(FRI_EXIT_ACT) - act))
    b.assert_zero(inside * (nxt(FRI_EXIT_ISPOW) - ispow))
    b.assert_transition(nxt(FRI_EXIT_ORD) - ordinal - last)
    b.assert_first(ordinal - pub(FRI_EXIT_PUB_ORD_POW))
    b.assert_first(ispow - act)
    b.assert_transition(last * nxt(FRI_EXIT_ISPOW))
    # 3. the value, and that its bits spell an integer below p
    b.assert_zero(nxt(FRI_EXIT_V) - inside * v - bit * weight)
    b.assert_zero(nxt(FRI_EXIT_T) - first * bit - t * (high * bit + hold))
    b.assert_zero(low * t * bit)
    # 4. the prefix flag of a public length
    b.assert_zero(last * f)
    b.assert_zero(nxt(FRI_EXIT_F) * (1 - f - last))
    b.assert_zero(first * (c - ispow * pub(FRI_EXIT_PUB_POW_BITS) - idxb * pub(FRI_EXIT_PUB_SKIP)))
    b.assert_zero(inside * (nxt(FRI_EXIT_C) - c + f))
    b.assert_zero(last * c)
    # 5. the exponent flag: FB rows behind it
    b.assert_zero(last * ef)
    b.assert_zero(h_n * (1 - h - last))
    b.assert_zero(first * (c2 - idxb * pub(FRI_EXIT_PUB_FB)))
    b.assert_zero(inside * (nxt(FRI_EXIT_C2) - c2 + ef))
    b.assert_zero(last * c2)
    # 6. the products flag x bit; the PoW response has no bit under its flag
    b.assert_zero(g - bit + f * bit)
    b.assert_zero(eb - ef * bit)
    b.assert_zero(ispow * (bit - g))
    # 7. the index: the bits the flag leaves
    b.assert_zero(nxt(FRI_EXIT_IDX) - inside * idx - g * weight)
    # 8. the point
    b.assert_zero(nxt(FRI_EXIT_W) - f * pub(FRI_EXIT_PUB_W) - ef * w * w)
    b.assert_zero(nxt(FRI_EXIT_X) - f * pub(FRI_EXIT_PUB_G) - (1 - f - last) * x - x * eb * (w - 1))
    # 9. the Horner steps
    b.assert_zero(pre * hf)
    b.assert_zero(last * hf)
    b.assert_zero(nxt(FRI_EXIT_HF) * (1 - hf - r62))
    b.assert_zero(first * (k - idxb * pub(FRI_EXIT_PUB_FINAL_LEN)))
    b.assert_zero(inside * (nxt(FRI_EXIT_K) - k + hf))
    b.assert_zero(last * k)
    for j, cj in enumerate((ca, cb)):
        b.assert_zero(nxt(FRI_EXIT_ACC + j) - inside * acc[j] - hf * (acc[j] * (x - 1) + cj))
    # the bus: the challenge (TranscriptAir sends it), the step's coefficient (the holder of the proof head), the exit (FriFoldAir)
    b.receive(TAG_CHAL, [None, ordinal, pub(FRI_EXIT_PUB_ABSORBED), v], last * act)
    b.receive(TAG_FIN, [k - 1, ca, cb], hf)
    b.receive(TAG_FRI, [idx, acc[0], acc[1], b.const(1)], last * idxb)
    return b
