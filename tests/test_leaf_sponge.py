"""LeafSpongeAir (AIR id 17) without a GPU: the reference trace satisfies the independently restated AIR at every leaf-length class,
its digests are oracle.MerkleTree's leaf digests, forged witnesses violate a constraint or unbalance the bus, a two-table
reference-prover proof (MerkleOpenAir + LeafSpongeAir under shared challenges) passes the product's vx_merkle_rows_verify -- the
verifier being the other party of the ROW bus -- and every way of changing the verifier's claims is refused.  Everything is exact."""
import numpy as np
import pytest

import leaf_sponge_ref as R
import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CFG = dict(S.DEFAULT_CFG, num_queries=8)
CHAL = R.CHAL
D = 3  # the trees of this file have 8 leaves


def leaves_of(L, seed=5):
    return np.random.default_rng(seed + 100 * L).integers(0, P, size=(1 << D, L), dtype=np.uint64)


def pcfg(vx):
    return vx.lib.default_stark_config(num_queries=CFG["num_queries"])


def test_every_constraint_has_degree_at_most_3():
    b = R.builder()
    worst = max(R.degree(e) for _, e in b.constraints)
    assert worst == 3


@pytest.mark.parametrize("L", R.LENGTHS)
def test_reference_trace_satisfies_the_restated_air(oracle, L):
    leaves = leaves_of(L)
    tree = oracle.MerkleTree(leaves, 0)
    idx = [5, 0, 5]  # one duplicate
    rows = leaves[idx]
    trace, pub, digs = R.ref_trace(idx, rows)
    B = R.n_blocks(L)
    assert trace.shape == (R.COLS, 1 << R.log_rows(3, L)) and pub[:2] == [L, B] and pub[2:10] == R.tail_flags(L)
    assert sum(pub[2:10]) == (L % 8 or 8) and pub[10:] == R.claims_digest(idx, rows)
    assert (digs == tree.leaf_digests()[idx]).all()  # the sponge of the table is the tree's leaf hash
    assert int(trace[R.ACT].sum()) == 32 * 3 * B and int(trace[R.LASTB].sum()) == 32 * 3
    aux, apub = R.gen_aux(trace, CHAL, pub)
    assert S.check_trace(R.air(), trace, pub, CHAL, aux, apub) is None
    # what the table sends is every word of every row once, and it receives the digests: total = sum 1 / D_row - sum 1 / D_open
    tot = S.ExtS(0)
    for i, r, d in zip(idx, rows, digs):
        for j, v in enumerate(r):
            tot = tot + R.d_row(CHAL, i, j, v).inv()
        dlo, dhi = M._denoms(CHAL, i, d)
        tot = tot - dlo.inv() - dhi.inv()
    assert S.ExtS(*apub) * trace.shape[1] == tot


def test_a_leaf_ends_on_the_wrap_around_pair(oracle):
    leaves = leaves_of(16)
    idx = [1, 2]  # 2 leaves x 2 blocks = 128 rows: no idle block
    trace, pub, _ = R.ref_trace(idx, leaves[idx])
    assert trace.shape[1] == 128 and int(trace[R.LASTB, -1]) == 1
    aux, apub = R.gen_aux(trace, CHAL, pub)
    assert S.check_trace(R.air(), trace, pub, CHAL, aux, apub) is None


FORGERIES = ["message_word", "tail_word_sent", "short_leaf", "idx_changed_midway", "capacity_not_carried", "digests_swapped", "started_with_capacity"]


def forged(kind, leaves):
    """two leaves of 21 words (three blocks each: two full ones and a five-word tail); the first one is tampered with
    -> (trace, public inputs, aux, aux public, the rows the forger claims)"""
    idx = [5, 6]
    rows = [[int(v) for v in leaves[i]] for i in idx]
    first, _ = R.leaf_blocks(idx[0], rows[0])
    honest, _ = R.leaf_blocks(idx[1], rows[1])
    tail_sent = False
    if kind == "message_word":  # the word on the bus is not the word absorbed
        first[1]["msg"][3] ^= 1
        rows[0][11] ^= 1
    elif kind == "tail_word_sent":  # the last block also sends the words it only keeps (as if the row had 24 words)
        tail_sent = True
        rows[0] = rows[0] + first[2]["msg"][5:]
    elif kind == "short_leaf":  # a leaf of B - 1 blocks: 16 words hashed, the last block marked as such
        first, _ = R.leaf_blocks(idx[0], rows[0][:16])
        rows[0] = rows[0][:16]
    elif kind == "idx_changed_midway":  # absorbs under one index, delivers the digest under another
        first[2]["idx"] = 2
    elif kind == "capacity_not_carried":
        first[1]["state"][9] ^= 1
    elif kind == "digests_swapped":
        first[2]["dig"], honest[2]["dig"] = honest[2]["dig"], first[2]["dig"]
    elif kind == "started_with_capacity":
        first[0]["state"][8] = 1
    trace = R.assemble(first + honest, 8)
    pub = [21, 3] + R.tail_flags(21) + R.claims_digest(idx, rows)
    aux, apub = R.gen_aux(trace, CHAL, pub, tail_sent=tail_sent)
    return trace, pub, aux, apub


@pytest.mark.parametrize("kind", FORGERIES)
def test_forged_witnesses_violate_a_constraint(oracle, kind):
    trace, pub, aux, apub = forged(kind, leaves_of(21))
    bad = S.check_trace(R.air(), trace, pub, CHAL, aux, apub)
    assert bad is not None and bad[0] >= 60  # never the permutation itself: the shape rules catch it


def test_a_consistently_changed_word_unbalances_the_bus(oracle):
    """a forger who changes a word AND rehashes satisfies every constraint -- of another row: the digest no longer is the tree's, so
    what the sponge table receives is not what the openings table sends"""
    leaves = leaves_of(9)
    tree = oracle.MerkleTree(leaves, 0)
    idx = [3]
    row = [int(v) for v in leaves[3]]
    row[8] ^= 1
    trace, pub, digs = R.ref_trace(idx, [row])
    aux, apub = R.gen_aux(trace, CHAL, pub)
    assert S.check_trace(R.air(), trace, pub, CHAL, aux, apub) is None
    otrace, _, odigs = M.ref_trace(tree, idx)
    _, oapub = M.gen_aux(otrace, CHAL)
    claim = S.ExtS(0)
    for j, v in enumerate(row):
        claim = claim + R.d_row(CHAL, 3, j, v).inv()
    assert not (digs == odigs).all()
    assert not (S.ExtS(*apub) * trace.shape[1] + S.ExtS(*oapub) * otrace.shape[1] == claim)


@pytest.fixture(scope="module")
def round_trip(oracle):
    """ONE two-table reference-prover proof (8 leaves of 9 words, cap height 1, three openings), shared by the tests below"""
    leaves = leaves_of(9)
    tree = oracle.MerkleTree(leaves, 1)
    idx = [1, 6, 3]
    rows = leaves[idx]
    p_open, p_sponge = R.prove_rows(tree, idx, rows, CFG)
    return tree, idx, rows, p_open, p_sponge


def test_round_trip_through_the_product_verifier(vx, round_trip):
    tree, idx, rows, p_open, p_sponge = round_trip
    cfg = pcfg(vx)
    blob = R.wrap(p_open, p_sponge, D, 9, len(idx))
    vx.lib.merkle_rows_verify(blob, tree.cap, D, idx, rows, cfg)
    ok, chal = R.bus_check(p_open, p_sponge, CFG["cap_height"], idx, rows)
    assert ok
    for p, ref_id in ((p_open, M.REF_ID), (p_sponge, R.REF_ID)):
        info = S.verify(p, CFG, expect_air=ref_id, ext_chal=chal)
        assert any(info["aux_public"])

    def refused(blob_=blob, cap=tree.cap, log_leaves=D, idx_=idx, rows_=rows, match=None):
        b = np.array(blob_, dtype=np.uint64)
        b[2], b[3] = np.asarray(rows_).shape[1], len(idx_)  # the blob's own request words follow the forger
        with pytest.raises(vx.VxError, match=match):
            vx.lib.merkle_rows_verify(b, cap, log_leaves, idx_, rows_, cfg)

    r2 = rows.copy()
    r2[1, 8] ^= 1
    refused(rows_=r2)                                               # one row word
    refused(idx_=[1, 6, 2])                                         # one index
    refused(idx_=[6, 1, 3], rows_=rows[[1, 0, 2]])                  # two claims swapped
    refused(idx_=idx[:2], rows_=rows[:2])                           # a claim dropped
    refused(idx_=idx + [0], rows_=np.concatenate([rows, tree.leaves[:1]]))  # a claim added
    refused(rows_=rows[:, :8])                                      # leaf_len wrong
    refused(rows_=np.concatenate([rows, np.zeros((3, 1), dtype=np.uint64)], axis=1))
    c2 = tree.cap.copy()
    c2[1, 0] ^= 1
    refused(cap=c2)                                                 # one cap word
    refused(blob_=R.wrap(p_sponge, p_open, D, 9, 3))                # the two proofs swapped in the blob
    swapped = blob.copy()
    swapped[R.HDR: R.HDR + p_sponge.size], swapped[R.HDR + p_sponge.size:] = blob[R.HDR + p_open.size:], blob[R.HDR: R.HDR + p_open.size]
    swapped[4], swapped[5] = p_sponge.size, p_open.size
    refused(blob_=swapped)                                          # ... with their own id words
    refused(idx_=[1, 6, 8], match="outside the tree")               # an index outside the tree
    r3 = rows.copy()
    r3[0, 0] = P
    refused(rows_=r3, match="non-canonical")                        # a non-canonical word
    with pytest.raises(vx.VxError, match="different request"):      # a blob for another request
        vx.lib.merkle_rows_verify(blob, tree.cap, D + 1, idx, rows, cfg)
    with pytest.raises(vx.VxError, match="different request"):
        vx.lib.merkle_rows_verify(blob, tree.cap, D, idx[:2], rows[:2], cfg)
    # the first proof on its own is no one-table statement: its challenges are shared with the sponge table
    digs = tree.leaf_digests()[idx]
    with pytest.raises(vx.VxError):
        vx.lib.merkle_openings_verify(M.wrap(p_open, D, len(idx)), tree.cap, D, idx, digs, cfg)


def test_truncated_and_damaged_blobs_are_refused(vx, round_trip):
    tree, idx, rows, p_open, p_sponge = round_trip
    cfg = pcfg(vx)
    blob = R.wrap(p_open, p_sponge, D, 9, len(idx))
    for w in range(R.HDR):
        for bit in (0, 1, 7, 31, 63):
            bad = blob.copy()
            bad[w] ^= np.uint64(1 << bit)
            with pytest.raises(vx.VxError):
                vx.lib.merkle_rows_verify(bad, tree.cap, D, idx, rows, cfg)
    cuts = list(range(0, 24)) + list(range(24, blob.size, max(1, blob.size // 40))) + [R.HDR + p_open.size, blob.size - 1]
    for cut in cuts:
        with pytest.raises(vx.VxError):
            vx.lib.merkle_rows_verify(blob[:cut], tree.cap, D, idx, rows, cfg)
        if cut > R.HDR + p_open.size:  # a consistent header over a truncated second proof
            short = blob[:cut].copy()
            short[5] = cut - R.HDR - p_open.size
            with pytest.raises(vx.VxError):
                vx.lib.merkle_rows_verify(short, tree.cap, D, idx, rows, cfg)
    # MerkleOpenAir's claims digest is taken from the proof: changing it there changes the transcript
    pos = R.HDR + 10 + int(p_open[9]) + 2 + 5
    bad = blob.copy()
    bad[pos] ^= 1
    with pytest.raises(vx.VxError):
        vx.lib.merkle_rows_verify(bad, tree.cap, D, idx, rows, cfg)
