"""MerkleOpenAir (AIR id 16) on the GPU: the witness and the auxiliary columns equal the reference generator cell by cell on trees
built by vx_merkle_build, the proof inside the blob of vx_merkle_openings_prove equals the reference prover's word for word, and
the full shape (84 openings of a 2^20-leaf tree in one 2^16-row table) is proven and checked by vx_merkle_openings_verify."""
import numpy as np
import pytest

import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CASES, CHAL = M.CASES, M.CHAL

pytestmark = pytest.mark.gpu


def trees(ctx, vx, oracle, D, cap_height, seed=3):
    """the same leaves as a tree of the GPU and as a reference tree"""
    rng = np.random.default_rng(seed + 10 * D)
    leaves = rng.integers(0, P, size=(1 << D, 8), dtype=np.uint64)
    return ctx.merkle(ctx.from_host(leaves), 1 << D, 8, vx.lib.VX_LEAVES_ROW_MAJOR, cap_height), oracle.MerkleTree(leaves, cap_height)


# ... and the ends of the auxiliary kernel's grid (one lane per block, 64 lanes): one block; 70 blocks of 128, idle ones behind them
WITNESS = dict(CASES, D1_Q1_one_block=(1, 0, [1]), D5_Q14_two_workgroups=(5, 2, [0, 31, 31, 17, 5, 9, 22, 1, 16, 30, 2, 13, 8, 27]))


@pytest.mark.parametrize("name", list(WITNESS))
def test_witness_equals_the_reference(ctx, vx, oracle, name):
    D, cap_height, idx = WITNESS[name]
    gtree, rtree = trees(ctx, vx, oracle, D, cap_height)
    want, want_pub, digs = M.ref_trace(rtree, idx)
    log_n = M.log_rows(len(idx), D)
    assert log_n == {"D1_Q1_one_block": 5, "D5_Q14_two_workgroups": 12}.get(name, log_n)
    tb, pub = ctx.merkle_open_air_trace(gtree, idx, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(M.COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_MERKLE_OPEN, tb, log_n, CHAL, vx.lib.VX_MERKLE_OPEN_AIR_AUX_COLS, pub)
    want_aux, want_apub = M.gen_aux(want, CHAL)
    got_aux = ab.download().reshape(4, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    tb.free(), ab.free(), gtree.free()


# depth 5 at cap heights 0, 2 and 5 (no level is read below the cap): both ends and a duplicate, 20 active blocks and 12 idle ones;
# depth 4: eight paths fill the 32 blocks of 2^10 rows exactly
ONE_TREE = {"D5_cap0": (5, 0, [0, 31, 31, 17]), "D5_cap2": (5, 2, [0, 31, 31, 17]), "D5_cap5": (5, 5, [0, 31, 31, 17]), "D4_full": (4, 1, [0, 15, 7, 8, 3, 3, 12, 1])}


@pytest.mark.parametrize("name", list(ONE_TREE))
def test_the_set_of_one_tree_is_the_single_table(ctx, vx, oracle, name):
    """MerkleOpenSetAir over one tree is MerkleOpenAir with trailing columns: columns 0..65 agree over the whole table, idle blocks included"""
    D, cap_height, idx = ONE_TREE[name]
    gtree, _ = trees(ctx, vx, oracle, D, cap_height)
    single, _ = ctx.merkle_open_air_trace(gtree, idx, 10)
    as_set, _ = ctx.merkle_open_set_air_trace([gtree], [0] * len(idx), idx, 10)
    want = single.download().reshape(M.COLS, -1)
    got = as_set.download().reshape(vx.lib.VX_MERKLE_OPEN_SET_AIR_COLS, -1)
    assert want.shape[1] == got.shape[1] == 1 << 10 and len(idx) * D <= 32
    bad = np.argwhere(got[:M.COLS] != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    single.free(), as_set.free(), gtree.free()


@pytest.mark.parametrize("D,Q,over", [(3, 3, {}), (5, 7, {}), (3, 3, dict(rate_bits=3, num_queries=28))], ids=["D3_Q3", "D5_Q7", "D3_Q3_rate3"])
def test_proof_equals_the_reference_prover(ctx, vx, oracle, D, Q, over):
    gtree, rtree = trees(ctx, vx, oracle, D, 1)
    rng = np.random.default_rng(D * Q)
    idx = [int(v) for v in rng.integers(0, 1 << D, size=Q)]
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    blob = ctx.merkle_openings_prove(gtree, idx, cfg)
    assert [int(v) for v in blob[:3]] == [M.MAGIC, D, Q] and int(blob[3]) == blob.size - M.HDR and int(blob[M.HDR + 1]) == M.AIR_ID
    trace, pub, digs = M.ref_trace(rtree, idx)
    want = M.prove(trace, pub, ocfg)
    got = M.unwrap(blob)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing proof word: %d" % bad[0]
    ok, chal = M.bus_check(got, ocfg["cap_height"], idx, digs)
    assert ok
    S.verify(got, ocfg, expect_air=M.REF_ID, expect_public=pub, ext_chal=chal)
    vx.lib.merkle_openings_verify(blob, gtree.cap(), D, idx, digs, cfg)
    gtree.free()


def test_full_shape(ctx, vx):
    """84 openings (the queries of one STARK proof) of a tree of 2^20 leaves, cap height 4: 1,680 permutations in a 2^16-row table"""
    D, n_leaves = 20, 1 << 20
    data = ctx.alloc(8 * n_leaves)
    ctx.fill_random(data, 8 * n_leaves, 2024)
    tree = ctx.merkle(data, n_leaves, 8, vx.lib.VX_LEAVES_ROW_MAJOR, 4)
    rng = np.random.default_rng(84)
    idx = [0, n_leaves - 1] + [int(v) for v in rng.integers(0, n_leaves, size=81)]
    idx.append(idx[7])  # one duplicate
    assert len(idx) == 84
    blob = ctx.merkle_openings_prove(tree, idx)
    assert int(blob[M.HDR + 2]) == 16  # degree bits of the table
    cap, digs = tree.cap(), tree.leaf_digests()[idx]
    vx.lib.merkle_openings_verify(blob, cap, D, idx, digs)

    def refused(cap_=cap, log_leaves=D, idx_=idx, digs_=digs, n_hdr=None):
        b = blob.copy()
        b[2] = len(idx_) if n_hdr is None else n_hdr
        with pytest.raises(vx.VxError):
            vx.lib.merkle_openings_verify(b, cap_, log_leaves, idx_, digs_)

    refused(idx_=idx[:5] + [idx[5] ^ 1] + idx[6:])                 # one claim index
    d2 = digs.copy()
    d2[40, 2] ^= 1
    refused(digs_=d2)                                              # one digest word
    perm = list(range(84))
    perm[10], perm[11] = 11, 10
    refused(idx_=[idx[k] for k in perm], digs_=digs[perm])         # the order of two claims
    c2 = cap.copy()
    c2[9, 1] ^= 1
    refused(cap_=c2)                                               # one cap word
    refused(log_leaves=21)                                         # log_leaves
    refused(idx_=idx[:-1], digs_=digs[:-1])                        # one claim dropped
    refused(idx_=idx[:-1], digs_=digs[:-1], n_hdr=84)              # ... with the blob's own count left alone
    refused(idx_=idx + [5], digs_=np.concatenate([digs, tree.leaf_digests()[5:6]]))  # one claim added
    p16 = blob[M.HDR:]
    with pytest.raises(vx.VxError):
        vx.lib.stark_verify(p16, expect_air=M.AIR_ID)              # the table proof on its own
    tree.free(), data.free()


def test_argument_errors(ctx, vx, oracle):
    gtree, _ = trees(ctx, vx, oracle, 3, 0)
    with pytest.raises(vx.VxError):
        ctx.merkle_openings_prove(gtree, [])
    with pytest.raises(vx.VxError):
        ctx.merkle_openings_prove(gtree, [1, 8])
    with pytest.raises(vx.VxError):
        ctx.merkle_open_air_trace(gtree, [], 7)
    with pytest.raises(vx.VxError):
        ctx.merkle_open_air_trace(gtree, [1, 8], 8)
    with pytest.raises(vx.VxError):
        ctx.merkle_open_air_trace(gtree, [1, 2, 3], 7)  # nine blocks do not fit 2^7 rows
    cfg = ctx.stark_config(num_queries=8)
    full = ctx.merkle_openings_prove(gtree, [1, 6], cfg)
    with pytest.raises(vx.VxError) as e:
        ctx.merkle_openings_prove(gtree, [1, 6], cfg, out=np.zeros(full.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == full.size  # VX_ERR_BUFSZ with the length set
    gtree.free()
