"""LeafSpongeAir (AIR id 17) on the GPU: the witness, the auxiliary columns and the public inputs equal the reference generator cell
by cell for all three leaf layouts, both proofs inside the blob of vx_merkle_rows_prove equal the two-table reference prover's word
for word, and the full shape (84 rows of 1018 words of a 2^17-leaf tree: 10,752 sponge blocks in 2^19 rows beside 1,428 path blocks
in 2^16 rows) is proven and checked by vx_merkle_rows_verify."""
import numpy as np
import pytest

import leaf_sponge_ref as R
import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CHAL = R.CHAL

pytestmark = pytest.mark.gpu


def bitrev(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)])


def in_layout(vx, leaves, layout):
    """the leaves [n][L] as vx_merkle_build reads them in `layout`"""
    if layout == vx.lib.VX_LEAVES_ROW_MAJOR:
        return np.ascontiguousarray(leaves)
    cols = np.ascontiguousarray(leaves.T)  # [L][n]
    return cols if layout == vx.lib.VX_LEAVES_COLS else np.ascontiguousarray(cols[:, bitrev(leaves.shape[0])])


def layouts(vx):
    return {"row_major": vx.lib.VX_LEAVES_ROW_MAJOR, "cols_bitrev": vx.lib.VX_LEAVES_COLS_BITREV, "cols": vx.lib.VX_LEAVES_COLS}


def make(ctx, vx, oracle, D, L, layout, cap_height, seed=7):
    """the same leaves as a device buffer in `layout`, a tree of the GPU and a reference tree"""
    leaves = np.random.default_rng(seed + 10 * D + 1000 * L).integers(0, P, size=(1 << D, L), dtype=np.uint64)
    data = ctx.from_host(in_layout(vx, leaves, layout))
    return leaves, data, ctx.merkle(data, 1 << D, L, layout, cap_height), oracle.MerkleTree(leaves, cap_height)


# (D, L, layout, indices, idle blocks behind the leaves: extra log_n)
WITNESS = {
    "D3_L5_row_major": (3, 5, "row_major", [5], 0),
    "D3_L8_cols_bitrev_duplicate": (3, 8, "cols_bitrev", [4, 1, 4], 0),
    "D3_L9_cols_no_idle_block": (3, 9, "cols", [6, 0], 0),
    "D5_L21_cols_bitrev_idle_tail": (5, 21, "cols_bitrev", [0, 31, 13], 0),
    "D5_L9_row_major_idle_half": (5, 9, "row_major", [30, 2], 1),
    "D5_L21_cols": (5, 21, "cols", [17], 0),
    "D5_L5_cols_bitrev": (5, 5, "cols_bitrev", [9, 22, 9, 1, 16], 0),
    # two workgroups of the auxiliary kernel (one lane per block, 64 lanes): 69 blocks of 128, idle ones behind them
    "D5_L21_row_major_two_workgroups": (5, 21, "row_major", [0, 31, 13, 17, 5, 9, 22, 1, 16, 30, 2, 8, 27, 3, 11, 19, 24, 6, 29, 14, 21, 10, 7], 0),
}


@pytest.mark.parametrize("name", list(WITNESS))
def test_witness_equals_the_reference(ctx, vx, oracle, name):
    D, L, lay, idx, extra = WITNESS[name]
    layout = layouts(vx)[lay]
    leaves, data, gtree, rtree = make(ctx, vx, oracle, D, L, layout, 0)
    log_n = R.log_rows(len(idx), L) + extra
    assert log_n == {"D3_L5_row_major": 5, "D5_L21_row_major_two_workgroups": 12}.get(name, log_n)
    want, want_pub, digs = R.ref_trace(idx, leaves[idx], log_n)
    assert (digs == gtree.leaf_digests()[idx]).all()
    tb, pub = ctx.leaf_sponge_air_trace(data, 1 << D, L, layout, idx, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(R.COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_LEAF_SPONGE, tb, log_n, CHAL, vx.lib.VX_LEAF_SPONGE_AIR_AUX_COLS, pub)
    want_aux, want_apub = R.gen_aux(want, CHAL, want_pub)
    got_aux = ab.download().reshape(R.AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    tb.free(), ab.free(), gtree.free(), data.free()


@pytest.mark.parametrize("n", [1, 17])  # 17: a second group of 16 lanes plus one
@pytest.mark.parametrize("L", [5, 8, 9])  # one partial block, exactly one block, a one-word tail
def test_the_rows_table_is_the_single_table(ctx, vx, L, n):
    """LeafSpongeSetAir from rows handed over is LeafSpongeAir on the same rows with a trailing column: columns 0..65 agree"""
    D = 5
    leaves = np.random.default_rng(100 * L + n).integers(0, P, size=(1 << D, L), dtype=np.uint64)
    idx = [int(v) for v in np.random.default_rng(n).permutation(1 << D)[:n]]
    data = ctx.from_host(leaves)
    log_n = R.log_rows(n, L)
    single, _ = ctx.leaf_sponge_air_trace(data, 1 << D, L, vx.lib.VX_LEAVES_ROW_MAJOR, idx, log_n)
    as_rows, _ = ctx.leaf_sponge_rows_air_trace([0] * n, idx, leaves[idx], log_n)
    want = single.download().reshape(R.COLS, -1)
    got = as_rows.download().reshape(vx.lib.VX_LEAF_SPONGE_SET_AIR_COLS, -1)
    assert want.shape[1] == got.shape[1] == 1 << log_n
    bad = np.argwhere(got[:R.COLS] != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    single.free(), as_rows.free(), data.free()


PROOFS = {
    "D3_cap0_L9_row_major": (3, 0, 9, "row_major", [1, 6, 3], {}),
    "D5_cap1_L21_cols_bitrev": (5, 1, 21, "cols_bitrev", [31, 4], {}),
    "D3_cap1_L5_cols_rate3": (3, 1, 5, "cols", [2, 7, 2], dict(rate_bits=3, num_queries=28)),
}


@pytest.mark.parametrize("name", list(PROOFS))
def test_both_proofs_equal_the_reference_prover(ctx, vx, oracle, name):
    D, cap_height, L, lay, idx, over = PROOFS[name]
    layout = layouts(vx)[lay]
    leaves, data, gtree, rtree = make(ctx, vx, oracle, D, L, layout, cap_height)
    rows = leaves[idx]
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    blob = ctx.merkle_rows_prove(gtree, data, L, layout, idx, cfg)
    assert [int(v) for v in blob[:4]] == [R.MAGIC, D, L, len(idx)] and int(blob[4]) + int(blob[5]) == blob.size - R.HDR
    assert int(blob[R.HDR + 1]) == M.AIR_ID and int(blob[R.HDR + int(blob[4]) + 1]) == R.AIR_ID
    want = R.prove_rows(rtree, idx, rows, ocfg)
    got = R.unwrap(blob)
    for g, w, what in zip(got, want, ("MerkleOpenAir", "LeafSpongeAir")):
        assert g.size == w.size, what
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "first differing word of the %s proof: %d" % (what, bad[0])
    ok, _ = R.bus_check(got[0], got[1], ocfg["cap_height"], idx, rows)
    assert ok
    vx.lib.merkle_rows_verify(blob, gtree.cap(), D, idx, rows, cfg)
    # the first proof on its own must not pass as a one-table proof: its challenges are shared with the sponge table
    with pytest.raises(vx.VxError):
        vx.lib.merkle_openings_verify(M.wrap(got[0], D, len(idx)), gtree.cap(), D, idx, gtree.leaf_digests()[idx], cfg)
    gtree.free(), data.free()


def test_full_shape(ctx, vx):
    """84 openings (the queries of one STARK proof) of a tree of 2^17 leaves x 1018 words as vx_lde leaves them, cap height 4"""
    D, n_leaves, L = 17, 1 << 17, 1018
    layout = vx.lib.VX_LEAVES_COLS_BITREV
    data = ctx.alloc(L * n_leaves)
    ctx.fill_random(data, L * n_leaves, 2025)
    tree = ctx.merkle(data, n_leaves, L, layout, 4)
    rng = np.random.default_rng(84)
    idx = [0, n_leaves - 1] + [int(v) for v in rng.integers(0, n_leaves, size=81)]
    idx.append(idx[7])  # one duplicate
    assert len(idx) == 84
    blob = ctx.merkle_rows_prove(tree, data, L, layout, idx)
    p_open, p_sponge = blob[R.HDR: R.HDR + int(blob[4])], blob[R.HDR + int(blob[4]):]
    assert 84 * 17 == 1428 and 84 * R.n_blocks(L) == 10752
    assert int(p_open[2]) == 16 and int(p_sponge[2]) == 19  # degree bits of the two tables
    cap = tree.cap()
    rows = ctx.lde_rows(data, D, L, idx)  # the rows a verifier holds: gathered by another primitive, leaf j = row bitrev(j)
    vx.lib.merkle_rows_verify(blob, cap, D, idx, rows)

    def refused(blob_=blob, cap_=cap, log_leaves=D, idx_=idx, rows_=rows, follow=True):
        b = blob_.copy()
        if follow:
            b[2], b[3] = np.asarray(rows_).shape[1], len(idx_)
        with pytest.raises(vx.VxError):
            vx.lib.merkle_rows_verify(b, cap_, log_leaves, idx_, rows_)

    r2 = rows.copy()
    r2[40, 1017] ^= 1
    refused(rows_=r2)                                               # one row word
    refused(idx_=idx[:5] + [idx[5] ^ 1] + idx[6:])                  # one index
    perm = list(range(84))
    perm[10], perm[11] = 11, 10
    refused(idx_=[idx[k] for k in perm], rows_=rows[perm])          # two claims swapped
    refused(idx_=idx[:-1], rows_=rows[:-1])                         # a claim dropped
    refused(idx_=idx[:-1], rows_=rows[:-1], follow=False)           # ... with the blob's own count left alone
    refused(idx_=idx + [5], rows_=np.concatenate([rows, ctx.lde_rows(data, D, L, [5])]))  # a claim added
    refused(rows_=np.ascontiguousarray(rows[:, :1017]))             # leaf_len wrong
    c2 = cap.copy()
    c2[9, 1] ^= 1
    refused(cap_=c2)                                                # one cap word
    sw = np.concatenate([blob[:4], blob[[5, 4]], p_sponge, p_open])
    refused(blob_=sw)                                               # the two proofs swapped in the blob
    with pytest.raises(vx.VxError):
        vx.lib.merkle_rows_verify(blob[:-1], cap, D, idx, rows)     # a truncated blob
    with pytest.raises(vx.VxError):
        vx.lib.merkle_openings_verify(M.wrap(p_open, D, 84), cap, D, idx, tree.leaf_digests()[idx])  # the first proof on its own
    tree.free(), data.free()


def test_statement_refusal(ctx, vx, oracle):
    """the leaf data is not what the tree was built from: one word of an opened leaf differs -> an ordinary error, nothing proven"""
    layout = vx.lib.VX_LEAVES_COLS_BITREV
    leaves, data, gtree, _ = make(ctx, vx, oracle, 3, 9, layout, 0)
    other = leaves.copy()
    other[6, 8] ^= 1
    data2 = ctx.from_host(in_layout(vx, other, layout))
    cfg = ctx.stark_config(num_queries=8)
    with pytest.raises(vx.VxError, match="leaf digest") as e:
        ctx.merkle_rows_prove(gtree, data2, 9, layout, [1, 6, 3], cfg)
    assert e.value.code == -5  # VX_ERR_STATEMENT
    blob = ctx.merkle_rows_prove(gtree, data2, 9, layout, [1, 3], cfg)  # the changed leaf is not opened: the rows agree
    vx.lib.merkle_rows_verify(blob, gtree.cap(), 3, [1, 3], leaves[[1, 3]], cfg)
    gtree.free(), data.free(), data2.free()


def test_the_first_mismatch_is_the_one_named(ctx, vx, oracle):
    """two opened leaves differ from what the tree was built from: the refusal names the lower opening number"""
    layout = vx.lib.VX_LEAVES_COLS_BITREV
    leaves, data, gtree, _ = make(ctx, vx, oracle, 3, 9, layout, 0)
    other = leaves.copy()
    other[3, 0] ^= 1
    other[6, 8] ^= 1
    data2 = ctx.from_host(in_layout(vx, other, layout))
    with pytest.raises(vx.VxError, match=r"opening 1 \(leaf 6\)") as e:  # openings 1 (leaf 6) and 2 (leaf 3) are wrong
        ctx.merkle_rows_prove(gtree, data2, 9, layout, [1, 6, 3], ctx.stark_config(num_queries=8))
    assert e.value.code == -5  # VX_ERR_STATEMENT
    gtree.free(), data.free(), data2.free()


def test_argument_errors(ctx, vx, oracle):
    row_major = vx.lib.VX_LEAVES_ROW_MAJOR
    _, data, gtree, _ = make(ctx, vx, oracle, 3, 9, row_major, 0)
    _, data4, gtree4, _ = make(ctx, vx, oracle, 3, 4, row_major, 0)
    cfg = ctx.stark_config(num_queries=8)
    for call in (lambda: ctx.merkle_rows_prove(gtree4, data4, 4, row_major, [1], cfg),       # leaf_len 4: hash_or_noop's no-op
                 lambda: ctx.leaf_sponge_air_trace(data4, 8, 4, row_major, [1], 5),
                 lambda: ctx.merkle_rows_prove(gtree, data, 9, row_major, [], cfg),          # an empty index list
                 lambda: ctx.leaf_sponge_air_trace(data, 8, 9, row_major, [], 6),
                 lambda: ctx.merkle_rows_prove(gtree, data, 9, row_major, [1, 8], cfg),      # an index >= n_leaves
                 lambda: ctx.leaf_sponge_air_trace(data, 8, 9, row_major, [1, 8], 7),
                 lambda: ctx.leaf_sponge_air_trace(data, 8, 9, row_major, [1, 2, 3], 7),     # six blocks do not fit 2^7 rows
                 lambda: ctx.leaf_sponge_air_trace(data, 16, 9, row_major, [1], 6),          # more leaves than the buffer holds
                 lambda: ctx.merkle_rows_prove(gtree, data, 10, row_major, [1], cfg)):
        with pytest.raises(vx.VxError) as e:
            call()
        assert e.value.code == -1  # VX_ERR_ARG
    full = ctx.merkle_rows_prove(gtree, data, 9, row_major, [1, 6], cfg)
    with pytest.raises(vx.VxError) as e:
        ctx.merkle_rows_prove(gtree, data, 9, row_major, [1, 6], cfg, out=np.zeros(full.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == full.size  # VX_ERR_BUFSZ with the length set
    gtree.free(), gtree4.free(), data.free(), data4.free()
