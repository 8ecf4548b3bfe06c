"""The witness tables of a request at their capacity edges: empty, exactly full, one over.

csrc/vx_table_shapes.h picks every table's size from the request; these are the shapes at which that choice switches or a table
has no idle row left: 4096 Blake2b compressions in 2^16 rows (no padding block: the target digest is captured on the last block
and the running sum wraps straight to row 0) and 4097 (2^17 rows); 6 / 7 and 204 / 205 SHA-512 slots (2^10 -> 2^15 -> 2^16 rows);
0, 1, 255 and 256 Ed25519 slots of 2^16 rows (one must stay idle, and counts m - k times in the range table's multiplicities);
authority sets of 1, 2, 3, 8 and 9 through the product.  Every comparison is exact.  Where the oracle's generator is too slow
for the shape, the GPU's own columns are put through the oracle's constraints (S.check_trace) and compared with independent
references: hashlib, numpy, big integers.  Every refusal is an argument check that returns before a kernel is launched."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import blake_air as B
from oracle import ed_air as E
from oracle import pyref
from oracle import sha512_air as H
from oracle import sha_air as A
from oracle import sha_tree_air as T
from oracle import stark_ref as S
from test_gpu_blake_air import limbs, oracle_verify_blob
from test_gpu_ed_air import MSG, signatures

pytestmark = pytest.mark.gpu
AIR_ED = {16: E.make_air(16), 17: E.make_air(17)}
AIR_H = {10: H.make_air(10), 15: H.make_air(15)}
for _air in (B.BlakeChainAir, T.make_air(16), A.ShaChainAir, *AIR_ED.values(), *AIR_H.values()):
    S.register_air(_air)
CHAL = [0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x1111111122222222, 0x3333333344444444]
STRIDE, BIG = 35840, 32768  # MAX_HEADER_SIZE; 256 chunks of 128 bytes


def check_windows(air, trace, aux, pub, apub, windows):
    """S.check_trace on row windows of the GPU's main and auxiliary columns (joined once, not once per window)."""
    both = np.concatenate([trace, aux])
    for lo, hi in windows:
        assert S.check_trace(air, both, pub, CHAL, None, apub, rows=(lo, hi)) is None, f"rows {lo}..{hi}"


def ints(a):
    return [int(x) for x in a]


# ----------------------------------------------------------------------------- 1. BlakeChainAir, 4096 blocks in 2^16 rows
class SizedChain:
    """16 chained headers of the given sizes (vx.synth.Chain has fixed size profiles only): block numbers 100001.. in compact
    mode 2, hashes by hashlib."""

    def __init__(self, vx, sizes):
        syn = vx.synth
        self.trusted_block, self.sizes, self.n = syn.TRUSTED_BLOCK, np.array(sizes, dtype=np.uint32), len(sizes)
        self.trusted_hash = hashlib.blake2b(b"capacity", digest_size=32).digest()
        self.headers = np.zeros((self.n, STRIDE), dtype=np.uint8)
        self.msgs, self.hashes, self.state_roots, self.data_roots = [], [], [], []
        parent = self.trusted_hash
        for i, sz in enumerate(sizes):
            num = self.trusted_block + 1 + i
            assert len(syn.compact_u32(num)) == 4
            hb = syn.encode_header(parent, num, sz, syn.CHAIN_SEED)
            self.headers[i, :sz] = np.frombuffer(hb, dtype=np.uint8)
            self.msgs.append(hb), self.state_roots.append(hb[36:68]), self.data_roots.append(hb[-32:])
            parent = hashlib.blake2b(hb, digest_size=32).digest()
            self.hashes.append(parent)
        self.target_block, self.target_hash = self.trusted_block + self.n, parent
        self.chunks = int(sum((s + 127) // 128 for s in sizes))

    def expected_outputs(self, tree_size):
        """The 96 output bytes, as synth.Chain.expected_outputs computes them."""
        def root(leaves):
            nodes = list(leaves) + [bytes(32)] * (tree_size - len(leaves))
            while len(nodes) > 1:
                nodes = [hashlib.sha256(nodes[i] + nodes[i + 1]).digest() for i in range(0, len(nodes), 2)]
            return nodes[0]

        return self.target_hash + root(self.state_roots) + root(self.data_roots)


SHAPES = {"full": [BIG] * 16, "full_ragged": [BIG] * 15 + [BIG - 127], "one_short": [BIG] * 15 + [BIG - 128], "one_over": [BIG] * 7 + [BIG + 128] + [BIG] * 8}
CHUNKS = {"full": 4096, "full_ragged": 4096, "one_short": 4095, "one_over": 4097}
_chains = {}


@pytest.fixture
def chain(vx):
    def get(shape):
        if shape not in _chains:
            _chains[shape] = SizedChain(vx, SHAPES[shape])
            assert _chains[shape].chunks == CHUNKS[shape]
        return _chains[shape]
    return get


def blake_trace(ctx, ch, log_n, tree):
    """-> (trace buffer, trace [COLS][n], public inputs) after the digest and public-input checks every shape shares."""
    buf, pub, dig = ctx.blake_chain_trace(ctx.from_host(ch.headers), STRIDE, ch.sizes, ch.trusted_hash, ch.trusted_block + 1, log_n, tree_size=tree)
    assert [d.tobytes() for d in dig] == ch.hashes == [hashlib.blake2b(m, digest_size=32).digest() for m in ch.msgs]
    pub = ints(pub)
    assert pub[0:8] == limbs(ch.trusted_hash) and pub[8:16] == limbs(ch.hashes[-1])
    assert pub[16:] == [ch.trusted_block + 1, ch.target_block, ch.trusted_block + 1 if tree else 0, 1 if tree else 0]
    return buf, buf.download().reshape(B.COLS, 1 << log_n), pub


def blake_aux(ctx, buf, log_n, pub):
    abuf, apub = ctx.stark_aux_trace(B.ID, buf, log_n, CHAL, B.AUX, pub)
    aux = abuf.download().reshape(B.AUX, 1 << log_n)
    abuf.free()
    return aux, ints(apub[:2])


@pytest.mark.parametrize("shape", ["full", "full_ragged", "one_short"])
def test_blake_table_without_a_padding_block(ctx, vx, oracle, chain, shape):
    """Every constraint on every row of the GPU's columns, the wrap from the last block's row 15 to row 0 included."""
    ch = chain(shape)
    buf, got, pub = blake_trace(ctx, ch, 16, 16)
    act = got[B.ACT]
    n_real = 16 * ch.chunks
    assert (act[:n_real] == 1).all() and (act[n_real:] == 0).all() and (1 << 16) - n_real == (16 if shape == "one_short" else 0)
    aux, apub = blake_aux(ctx, buf, 16, pub)
    buf.free()
    assert any(apub)  # the roots are on the bus
    assert S.check_trace(B.BlakeChainAir, got, pub, CHAL, aux, apub) is None


def test_blake_full_table_stand_alone_proof(ctx, vx, oracle, chain):
    """Nothing on the bus: a wrong multiplicity in a table without idle rows would leave the published total non-zero."""
    ch = chain("full")
    buf, got, pub = blake_trace(ctx, ch, 16, 0)
    assert (got[B.ACT] == 1).all()
    _, apub = blake_aux(ctx, buf, 16, pub)
    assert apub == [0, 0]
    pcfg, cfg = ctx.stark_config(num_queries=8), dict(S.DEFAULT_CFG, num_queries=8)
    proof = ctx.stark_prove(B.ID, buf, 16, pub, pcfg)
    buf.free()
    vx.lib.stark_verify(proof, pcfg, expect_air=B.ID, expect_public=pub)
    S.verify(proof, cfg, expect_air=B.ID, expect_public=pub)
    bad = proof.copy()
    bad[len(bad) // 2] ^= np.uint64(1)
    with pytest.raises(vx.VxError):
        vx.lib.stark_verify(bad, pcfg)
    with pytest.raises(S.VerifyError):
        S.verify(bad, cfg)


def test_blake_one_compression_over(ctx, vx, oracle, chain):
    """4097 compressions: refused at 2^16 rows, 2^17 rows hold them with 4095 padding blocks."""
    ch = chain("one_over")
    with pytest.raises(vx.VxError) as e:
        ctx.blake_chain_trace(ctx.from_host(ch.headers), STRIDE, ch.sizes, ch.trusted_hash, ch.trusted_block + 1, 16, tree_size=16)
    assert e.value.code == -1 and "do not fit" in str(e.value)
    buf, got, pub = blake_trace(ctx, ch, 17, 16)
    n, n_real = 1 << 17, 16 * 4097
    assert (got[B.ACT, :n_real] == 1).all() and (got[B.ACT, n_real:] == 0).all()
    aux, apub = blake_aux(ctx, buf, 17, pub)
    buf.free()
    # the last real block, the first padding block (and the one after it), the last rows and the wrap
    check_windows(B.BlakeChainAir, got, aux, pub, apub, [(n_real - 20, n_real + 36), (n - 20, n)])


@pytest.mark.parametrize("shape,log_n", [("full", 16), ("one_over", 17)])
def test_header_range_at_the_hash_chain_capacity(ctx, vx, chain, shape, log_n):
    ch = chain(shape)
    cfg = ctx.stark_config(num_queries=8)
    args = (16, ch.trusted_block, ch.trusted_hash, ch.target_block)
    out96, blob = ctx.header_range_prove(ctx.from_host(ch.headers), STRIDE, ch.sizes, *args, cfg)
    assert out96 == ch.expected_outputs(16)
    vx.lib.header_range_verify(blob, *args, out96, cfg)
    p_blake = vx.lib.split_blob(blob)[0]
    assert int(p_blake[1]) == B.ID and int(p_blake[2]) == log_n
    bad = blob.copy()
    bad[vx.lib.HR_HDR + p_blake.size // 2] ^= np.uint64(1)
    with pytest.raises(vx.VxError):
        vx.lib.header_range_verify(bad, *args, out96, cfg)
    if hasattr(ctx.L, "vx_header_range_proof_bound"):
        need = ctypes.c_size_t(0)
        assert ctx.L.vx_header_range_proof_bound(ctypes.byref(cfg), ch.chunks, 0, ctypes.byref(need)) == 0
        assert len(blob) <= need.value


# ----------------------------------------------------------------------------- 2. Sha512Air
@pytest.fixture(scope="module")
def just300(vx):
    """300 authorities, all signed (the justification test_gpu_ed_air.py uses): any subset of the flags is a valid input."""
    return vx.synth.Justification(100256, hashlib.blake2b(b"t", digest_size=32).digest())


def spread(k, n=300):
    """k of n flags, spread as synth.Justification spreads its signers."""
    return [((i + 1) * k) // n != (i * k) // n for i in range(n)]


def small(k):
    keys, sigs, flags, recs = signatures(max(k, 6), unsigned=range(k, 6))
    assert sum(flags) == k and len(recs) == k
    return keys, sigs, flags, recs


@pytest.mark.parametrize("k", [6, 0])
def test_sha512_small_table_full_and_empty(ctx, vx, oracle, k):
    """2^10 rows hold exactly 6 slots: with 6 signatures no slot is idle, with none every flag is zero."""
    keys, sigs, flags, _ = small(k)
    slots = [(sg[:32], ky) for ky, sg, f in zip(keys, sigs, flags) if f]
    for bus_on in (1, 0):
        buf, pub = ctx.sha512_trace(keys, sigs, MSG, flags, 10, bus_on=bus_on)
        want, wpub, _ = H.gen_trace(slots, MSG, 10, bus_on=bus_on)
        got = buf.download().reshape(H.COLS, 1 << 10)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"first differing cells (col,row): {bad[:5].tolist()}"
        assert ints(pub) == wpub and int(got[H.SGF].sum()) == 160 * k
        aux, apub = ctx.stark_aux_trace(H.IDS[10], buf, 10, CHAL, H.AUX, public_inputs=pub)
        waux, wapub = H.gen_aux(want, CHAL, wpub)
        assert (aux.download().reshape(H.AUX, 1 << 10) == waux).all() and ints(apub[:2]) == wapub
        assert (wapub != [0, 0]) == bool(k and bus_on)
        if k == 0 and bus_on:  # nothing is sent: the table is acceptable on its own with the bus on
            proof = ctx.stark_prove(H.IDS[10], buf, 10, pub, ctx.stark_config(num_queries=6))
            vx.lib.stark_verify(proof, ctx.stark_config(num_queries=6), expect_air=H.IDS[10], expect_public=wpub)
            S.verify(proof, dict(S.DEFAULT_CFG, num_queries=6), expect_air=H.IDS[10], expect_public=wpub)
    cfg = dict(S.DEFAULT_CFG, num_queries=6)
    proof = ctx.stark_prove(H.IDS[10], buf, 10, pub, ctx.stark_config(num_queries=6))
    assert (proof == S.prove(AIR_H[10], want, wpub, cfg)).all()
    S.verify(proof, cfg, expect_air=H.IDS[10], expect_public=wpub)
    vx.lib.stark_verify(proof, ctx.stark_config(num_queries=6), expect_air=H.IDS[10], expect_public=wpub)


def test_sha512_one_slot_over_is_refused(ctx, vx, just300):
    keys, sigs, flags, _ = signatures(7, unsigned=())
    with pytest.raises(vx.VxError) as e:
        ctx.sha512_trace(keys, sigs, MSG, flags, 10)
    assert e.value.code == -1
    with pytest.raises(vx.VxError) as e:
        ctx.sha512_trace(just300.pubkeys, just300.signatures, just300.precommit, spread(205), 15)
    assert e.value.code == -1
    buf, pub = ctx.sha512_trace(keys, sigs, MSG, flags, 15)  # the seventh signature switches the request to 2^15 rows
    assert int(buf.download().reshape(H.COLS, 1 << 15)[H.SGF].sum()) == 160 * 7
    buf.free()


def test_sha512_204_slots_of_204(ctx, vx, just300):
    j, flags, n = just300, spread(204), 1 << 15
    buf, pub = ctx.sha512_trace(j.pubkeys, j.signatures, j.precommit, flags, 15, bus_on=1)
    got = buf.download().reshape(H.COLS, n)
    # every slot's digest, on each of its six send rows
    want = [hashlib.sha512(sg[:32] + pk + j.precommit).digest() for pk, sg, f in zip(j.pubkeys, j.signatures, flags) if f]
    assert len(want) == 204
    for r in range(6):
        rows = 160 * np.arange(204) + H.SEND0 + r
        words = (got[H.FFV0 + 1:H.FFV0 + 16:2, rows] << np.uint64(32)) | got[H.FFV0:H.FFV0 + 16:2, rows]  # [8 words][204 slots]
        assert (got[H.FFV0:H.FFV0 + 16, rows] < (1 << 32)).all()
        assert [w.astype(">u8").tobytes() for w in words.T] == want, f"send row {r}"
    assert (got[H.SGF, :204 * 160] == 1).all() and not got[:, 204 * 160:].any()
    assert ints(pub) == H.public_inputs(j.precommit, 1)
    abuf, apub = ctx.stark_aux_trace(H.IDS[15], buf, 15, CHAL, H.AUX, public_inputs=pub)
    aux = abuf.download().reshape(H.AUX, n)
    assert any(ints(apub[:2]))
    check_windows(AIR_H[15], got, aux, ints(pub), ints(apub[:2]), [(203 * 160 - 4, 204 * 160 + 8), (n - 8, n)])
    buf.free(), abuf.free()
    buf, pub = ctx.sha512_trace(j.pubkeys, j.signatures, j.precommit, flags, 15, bus_on=0)
    vx.lib.stark_verify(ctx.stark_prove(H.IDS[15], buf, 15, pub), expect_air=H.IDS[15], expect_public=pub)
    buf.free()


def bus_balance(ctx, keys, sigs, msg, flags, h_log):
    """Sha512Air and EdAir (2^16 rows) under the same challenges: what one sends the other receives; the key receives of EdAir
    (the authority-set table's side, recomputed here from the keys) close the bus."""
    hb, hpub = ctx.sha512_trace(keys, sigs, msg, flags, h_log, bus_on=1)
    ab, apub_h = ctx.stark_aux_trace(H.IDS[h_log], hb, h_log, CHAL, H.AUX, public_inputs=hpub)
    hb.free(), ab.free()
    eb, epub = ctx.ed_trace(keys, sigs, msg, flags, 16, bus_on=1)
    ab, apub_e = ctx.stark_aux_trace(E.IDS[16], eb, 16, CHAL, E.AUX, public_inputs=epub)
    eb.free(), ab.free()
    ExtS = S.ExtS
    beta, gamma = ExtS(CHAL[0], CHAL[1]), ExtS(CHAL[2], CHAL[3])
    g2 = gamma * gamma
    g4 = g2 * g2
    keys_total = ExtS(0)
    for s, (pk, f) in enumerate(zip(keys, flags)):
        if f:
            l = [int.from_bytes(pk[2 * k: 2 * k + 2], "little") for k in range(16)]
            for b in range(4):
                d = beta + (4 * s + b) + gamma * (l[4 * b] + (l[4 * b + 1] << 16)) + g2 * (l[4 * b + 2] + (l[4 * b + 3] << 16)) + g4 * E.TAG_KEY
                keys_total = keys_total + d.inv()
    tot_e = ExtS(int(apub_e[0]), int(apub_e[1])) * (1 << 16)
    tot_h = ExtS(int(apub_h[0]), int(apub_h[1])) * (1 << h_log)
    assert (tot_e.a, tot_e.b) != (0, 0) and (tot_h.a, tot_h.b) != (0, 0)
    rest = tot_e + tot_h + keys_total  # EdAir's total holds the key receives with a minus sign
    assert (rest.a, rest.b) == (0, 0)


def test_sha512_full_tables_balance_the_curve_table(ctx, vx, just300):
    keys, sigs, flags, _ = small(6)
    bus_balance(ctx, keys, sigs, MSG, flags, 10)
    bus_balance(ctx, just300.pubkeys, just300.signatures, just300.precommit, spread(204), 15)


# ----------------------------------------------------------------------------- 3. EdAir, 256 slots in 2^16 rows
def ed_windows(k):
    n = 1 << 16
    w = [(0, 4), (254, 259), (n - 4, n)]
    return w + [(255 * 256 - 3, 255 * 256 + 4)] if k == 255 else w


@pytest.mark.parametrize("k", [0, 1, 255])
def test_ed_table_at_its_slot_limit(ctx, vx, oracle, just300, k):
    j, flags, n = just300, spread(k), 1 << 16
    buf, pub = ctx.ed_trace(j.pubkeys, j.signatures, j.precommit, flags, 16, bus_on=1)
    assert ints(pub) == [k, 1]
    got = buf.download().reshape(E.COLS, n)
    abuf, apub = ctx.stark_aux_trace(E.IDS[16], buf, 16, CHAL, E.AUX, public_inputs=pub)
    aux = abuf.download().reshape(E.AUX, n)
    buf.free(), abuf.free()
    # the range table's multiplicities: an idle slot's lookups count once for each of the m - k idle slots
    cells = got[:E.CELLS]
    assert int(cells.max()) < 65536
    assert (got[E.MULT] == np.bincount(cells.astype(np.int64).ravel(), minlength=65536).astype(np.uint64)).all()
    slots = got.reshape(E.COLS, 256, 256)  # [column][slot][row of the slot]
    idx = [i for i, f in enumerate(flags) if f]
    assert (slots[E.SG, :k] == 1).all() and not slots[E.SG, k:].any()
    assert (slots[E.CNT] == np.minimum(np.arange(1, 257), k).astype(np.uint64)[:, None]).all() and int(got[E.CNT, n - 1]) == k
    assert (slots[E.AIDX, :k] == np.array(idx, dtype=np.uint64)[:, None]).all() and not slots[E.AIDX, k:].any()
    idle = np.delete(slots[:, k:], E.MULT, axis=0)
    assert (idle == idle[:, :1]).all()  # every idle slot is the same slot (k = 0: period 256 in every column but MULT)
    check_windows(AIR_ED[16], got, aux, ints(pub), ints(apub[:2]), ed_windows(k))
    # the signature equation of the first and the last active slot: row 254 holds [S]B - [h]A = R projectively
    for s in sorted({0, k - 1} if k else ()):
        X, Y, Z = (sum(int(got[E.C(g, q), 256 * s + 254]) << (16 * q) for q in range(16)) % E.Q for g in (11, 12, 13))
        zi = pow(Z, E.Q - 2, E.Q)
        R = pyref._decompress(j.signatures[idx[s]][:32])
        assert (X * zi % E.Q, Y * zi % E.Q) == (R[0], R[1])


@pytest.mark.parametrize("k", [0, 255])
def test_ed_proofs_at_the_slot_limit(ctx, vx, oracle, just300, k):
    j = just300
    buf, pub = ctx.ed_trace(j.pubkeys, j.signatures, j.precommit, spread(k), 16)
    pcfg, cfg = ctx.stark_config(num_queries=6), dict(S.DEFAULT_CFG, num_queries=6)
    proof = ctx.stark_prove(E.IDS[16], buf, 16, pub, pcfg)
    buf.free()
    vx.lib.stark_verify(proof, pcfg, expect_air=E.IDS[16], expect_public=[k, 0])
    S.verify(proof, cfg, expect_air=E.IDS[16], expect_public=[k, 0])


def test_ed_256_signatures_need_the_larger_table(ctx, vx, just300):
    j = just300
    with pytest.raises(vx.VxError) as e:
        ctx.ed_trace(j.pubkeys, j.signatures, j.precommit, spread(256), 16)
    assert e.value.code == -1
    buf, pub = ctx.ed_trace(j.pubkeys, j.signatures, j.precommit, spread(256), 17)
    assert ints(pub) == [256, 0]
    buf.free()


# ----------------------------------------------------------------------------- 4. small authority sets through the product
_tiny = {}


@pytest.fixture
def tiny(vx):
    if not _tiny:
        _tiny["ch"] = vx.synth.Chain(16, profile="Ptiny", stride=512)
    return _tiny["ch"]


@pytest.mark.parametrize("n_auth,n_signed", [(1, 1), (2, 2), (3, 3), (8, 6), (9, 7), (8, 8)])
def test_header_range_with_a_small_authority_set(ctx, vx, oracle, tiny, n_auth, n_signed):
    ch, quorum = tiny, 2 * n_auth // 3 + 1
    cfg, ocfg = ctx.stark_config(num_queries=8), dict(S.DEFAULT_CFG, num_queries=8)
    sj = vx.synth.Justification(ch.target_block, ch.target_hash, n_auth=n_auth, n_signed=n_signed)
    just = vx.lib.PackedJustification(sj, 12)
    hb = ctx.from_host(ch.headers)
    args = (16, ch.trusted_block, ch.trusted_hash, ch.target_block)
    out96, blob = ctx.header_range_prove(hb, 512, ch.sizes, *args, cfg, just=just)
    assert out96 == ch.expected_outputs(16)
    ver = dict(authority_set_hash=sj.authority_set_hash, authority_set_id=sj.set_id)
    vx.lib.header_range_verify(blob, *args, out96, cfg, **ver)
    with pytest.raises(vx.VxError):
        vx.lib.header_range_verify(blob, *args, out96, cfg, authority_set_hash=bytes(32), authority_set_id=sj.set_id)
    p_blake, p_sha, p_tree, p_ed, p_h = vx.lib.split_blob(blob)
    h_log = 10 if n_auth <= 8 else 15
    assert (int(p_h[1]), int(p_h[2])) == (H.IDS[h_log], h_log) and (int(p_ed[1]), int(p_ed[2])) == (E.IDS[16], 16)
    assert int(p_sha[2]) == {1: 6, 2: 8, 3: 9, 8: 10, 9: 11}[n_auth]
    # the prover takes the first `quorum` signers, however many signed
    assert S.proof_peek(p_sha, 4)[0][8:] == [n_auth, 1] and S.proof_peek(p_ed, 4)[0] == [quorum, 1]
    if n_signed == n_auth:  # the reference verifier on the smallest set and on the set with more signers than the proof takes
        oracle_verify_blob(vx, blob, ocfg, 16)
    off_ed = vx.lib.HR_HDR + p_blake.size + p_sha.size + p_tree.size
    for w in (off_ed + p_ed.size // 2, off_ed + p_ed.size + p_h.size // 2):
        bad = blob.copy()
        bad[w] ^= np.uint64(1)
        with pytest.raises(vx.VxError):
            vx.lib.header_range_verify(bad, *args, out96, cfg, **ver)
    weak = vx.synth.Justification(ch.target_block, ch.target_hash, n_auth=n_auth, n_signed=quorum - 1)
    with pytest.raises(vx.VxError) as e:
        ctx.header_range_prove(hb, 512, ch.sizes, *args, cfg, just=vx.lib.PackedJustification(weak, 12))
    assert e.value.code == -5
    hb.free()


@pytest.mark.parametrize("n_auth", [1, 8])
def test_rotate_with_a_small_current_set(ctx, vx, n_auth):
    cfg = ctx.stark_config(num_queries=8)
    e = vx.synth.EpochEndHeader(150000 + n_auth, 3)
    sj = vx.synth.Justification(e.number, e.hash, n_auth=n_auth, n_signed=2 * n_auth // 3 + 1, set_id=9)
    hb = ctx.from_host(e.padded)
    out32, blob = ctx.rotate_prove(hb, e.size, e.number, 3, e.start_position, e.new_pubkeys, vx.lib.PackedJustification(sj, 8), cfg)
    hb.free()
    assert out32 == e.new_authority_set_hash
    vx.lib.rotate_verify(blob, 9, sj.authority_set_hash, out32, cfg)
    with pytest.raises(vx.VxError):
        vx.lib.rotate_verify(blob, 9, bytes(32), out32, cfg)


# ----------------------------------------------------------------------------- 5.
def test_sha_chain_refuses_a_table_one_size_too_small(ctx, vx):
    keys = [hashlib.sha256(bytes([i, 9])).digest() for i in range(2)]  # 3 compressions of 64 rows: 2^8 rows
    with pytest.raises(vx.VxError) as e:
        ctx.sha_chain_trace(keys, 7)
    assert e.value.code == -1
    ctx.sha_chain_trace(keys, 8)[0].free()
