"""The FRI query phase on one bus without a GPU: MerkleOpenSetAir (id 19) and LeafSpongeSetAir (id 20) restated independently
(fri_queries_ref), their honest traces, the three-table bus with FriFoldAir -- TAG_OPEN and TAG_ROW close BETWEEN tables in several
trees, the verifier holds caps, betas, the final polynomial and (index, ev_0) only --, forged witnesses refused by a named rule or by
the bus, and reference-prover blobs through the product's vx_fri_queries_verify.  Everything is exact."""
import numpy as np
import pytest

import fri_fold_ref as F
import fri_queries_ref as Q
import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CFG = dict(S.DEFAULT_CFG, num_queries=8)
CHAL = Q.CHAL
# (LN, NL) -> (cap height of the layer trees, the queries): (9, 2) has depths 5 and 1 -- two roots and two depths meet; its queries
# 0x1a3 and 0x0a3 share their layer-1 leaf (index >> 8) but not their layer-0 leaf (index >> 4)
SHAPES = {(5, 1): (0, [19]), (9, 2): (1, [0x1A3, 0x0A3])}


def pcfg(vx):
    return vx.lib.default_stark_config(num_queries=CFG["num_queries"])


_made = {}


def phase(LN, NL):
    """one commit phase per shape, its layer trees and the three honest tables (computed once, never modified)"""
    if (LN, NL) not in _made:
        cap_h, index = SHAPES[(LN, NL)]
        betas, fpoly, layers = F.commit_phase(LN, NL, seed=7)
        trees = Q.layer_trees(layers, cap_h)
        tabs, ev0 = Q.tables(LN, betas, fpoly, layers, trees, index)
        _made[(LN, NL)] = dict(LN=LN, NL=NL, cap_h=cap_h, index=index, betas=betas, fpoly=fpoly, layers=layers, trees=trees, tabs=tabs, ev0=ev0, roots=Q.roots_of(trees))
    return _made[(LN, NL)]


def aux_of(tabs, chal=CHAL):
    return [gen(tr, chal, pub) for gen, (tr, pub) in zip((Q.open_gen_aux, Q.sponge_gen_aux, F.gen_aux), tabs)]


def balances(ph, tabs, roots=None, chal=CHAL):
    auxs = aux_of(tabs, chal)
    return Q.tables_sum([apub for _, apub in auxs], tabs) == Q.outside_sum(chal, ph["LN"], ph["NL"], ph["fpoly"], ph["roots"] if roots is None else roots, ph["index"], ph["ev0"])


def test_every_constraint_has_degree_at_most_3(oracle):
    # ids 16 / 17 have 121 / 136: six / one more block-constant columns, TREE carried, the second helper
    for builder, n in ((Q.open_builder, 121 + 6 + 1 + 2), (Q.sponge_builder, 136 + 1 + 1)):
        b = builder()
        assert len(b.constraints) == n
        assert max(Q.degree(e) for _, e in b.constraints) == 3


@pytest.mark.parametrize("shape", list(SHAPES))
def test_honest_traces_satisfy_the_restated_airs_and_the_bus_balances(oracle, shape):
    ph = phase(*shape)
    (otr, opub), (str_, spub), (ftr, fpub) = ph["tabs"]
    NL, n_q = ph["NL"], len(ph["index"])
    assert otr.shape == (Q.O_COLS, 1 << max(5, (32 * n_q * sum(shape[0] - 4 * (l + 1) for l in range(NL)) - 1).bit_length()))
    assert str_.shape == (Q.S_COLS, 1 << max(5, (32 * n_q * NL * 4 - 1).bit_length()))
    assert opub == spub[10:] == fpub[F.PUB_DIGEST:] and spub[:10] == [32, 4] + [1] * 8
    assert int(otr[M.FIRSTB].sum()) == 32 * n_q * NL == int(otr[M.END].sum()) == int(str_[Q.R.LASTB].sum())
    assert sorted(set(int(v) for v in otr[Q.O_DEPTH][otr[M.ACT] == 1])) == sorted(shape[0] - 4 * (l + 1) for l in range(NL))
    (oaux, oap), (saux, sap), (faux, fap) = aux_of(ph["tabs"])
    assert S.check_trace(Q.open_air(), otr, opub, CHAL, oaux, oap) is None
    assert S.check_trace(Q.sponge_air(), str_, spub, CHAL, saux, sap) is None
    assert S.check_trace(F.air(), ftr, fpub, CHAL, faux, fap) is None
    assert balances(ph, ph["tabs"])
    # no table closes on its own, and no pair does: all three message kinds cross a table boundary
    tot = [S.ExtS(*ap) * tr.shape[1] for ap, (tr, _) in zip((oap, sap, fap), ph["tabs"])]
    out = Q.outside_sum(CHAL, ph["LN"], NL, ph["fpoly"], ph["roots"], ph["index"], ph["ev0"])
    assert not (tot[0] + tot[1] == out) and not (tot[1] + tot[2] == out) and not (tot[0] + tot[2] == out)


def test_the_set_witnesses_alone_carry_their_claims_digests(oracle):
    ph = phase(9, 2)
    tree_of, leaf_idx = Q.openings_of(ph["index"], 2)
    rows = [Q.layer_rows(ph["layers"])[t][i] for t, i in zip(tree_of, leaf_idx)]
    otr, opub = Q.open_ref_trace(ph["trees"], tree_of, leaf_idx)
    str_, spub, digs = Q.sponge_ref_trace(tree_of, leaf_idx, rows)
    assert (otr == ph["tabs"][0][0]).all() and (str_ == ph["tabs"][1][0]).all()
    assert opub == Q.open_claims_digest(tree_of, leaf_idx, digs) and spub[10:] == Q.sponge_claims_digest(tree_of, leaf_idx, rows)
    for t, i, d in zip(tree_of, leaf_idx, digs):  # the sponge of the table is the layer tree's leaf hash
        assert (ph["trees"][t].leaf_digests()[i] == d).all()


def open_forged(ph, edit):
    """the openings table of (9, 2) with the blocks of its first path (tree 0, five levels) edited -> (trace, aux, aux public)"""
    nodes = [M.tree_nodes(t) for t in ph["trees"]]
    tree_of, leaf_idx = Q.openings_of(ph["index"], ph["NL"])
    paths = [Q.open_blocks(nodes, t, i) for t, i in zip(tree_of, leaf_idx)]
    paths[0] = edit(nodes, paths[0], leaf_idx[0])
    tr = Q.open_assemble([blk for p in paths for blk in p], 9)
    return (tr,) + Q.open_gen_aux(tr, CHAL)


def test_tree_switched_in_the_middle_of_a_path(oracle):
    ph = phase(9, 2)

    def edit(nodes, path, idx):
        for blk in path[2:]:
            blk["tree"] = 1
        return path

    tr, aux, apub = open_forged(ph, edit)
    bad = S.check_trace(Q.open_air(), tr, ph["tabs"][0][1], CHAL, aux, apub)
    assert bad is not None and bad[0] == Q.OPEN_RULES["tree_carried"]


def test_a_path_ended_early(oracle):
    """a depth-5 path ended at a level-1 node while DEPTH says 1: with index bits left the END rule names it; with none left (leaf 1)
    the table is satisfied -- it is a depth-1 path to SOME root -- and the bus is not: the verifier knows tree 0 has depth 5"""
    ph = phase(9, 2)

    def early(leaf):
        def edit(nodes, path, idx):
            short = M.path_blocks(nodes[0], leaf, levels=1)
            _, out = M.block_rows((short[0]["sib"] + short[0]["cur"] if short[0]["bit"] else short[0]["cur"] + short[0]["sib"]) + [0] * 4)
            short[0].update(tree=0, root=out[:4], depth=1)
            return short
        return edit

    tr, aux, apub = open_forged(ph, early(ph["index"][0] >> 4))
    bad = S.check_trace(Q.open_air(), tr, ph["tabs"][0][1], CHAL, aux, apub)
    assert bad is not None and bad[0] == Q.OPEN_RULES["no_bit_left"]
    tr, aux, apub = open_forged(ph, early(1))
    assert S.check_trace(Q.open_air(), tr, ph["tabs"][0][1], CHAL, aux, apub) is None
    assert not balances(ph, [(tr, ph["tabs"][0][1])] + ph["tabs"][1:])


def test_root_cells_changed(oracle):
    """ROOT cells that are not the path's output violate the END rule; a path into ANOTHER tree (an unopened leaf changed: the same
    opened digests, another root) satisfies the table, and the outside sum fails: the verifier receives the root of ITS cap"""
    ph = phase(9, 2)

    def edit(nodes, path, idx):
        for blk in path:
            blk["root"] = [blk["root"][0] ^ 1] + blk["root"][1:]
        return path

    tr, aux, apub = open_forged(ph, edit)
    bad = S.check_trace(Q.open_air(), tr, ph["tabs"][0][1], CHAL, aux, apub)
    assert bad is not None and bad[0] == Q.OPEN_RULES["output_is_root"]
    rows = [r.copy() for r in Q.layer_rows(ph["layers"])]
    tree_of, leaf_idx = Q.openings_of(ph["index"], 2)
    other = next(i for i in range(32) if i not in [j for t, j in zip(tree_of, leaf_idx) if t == 0])
    rows[0][other, 0] ^= np.uint64(1)
    trees2 = [oracle.MerkleTree(rows[0], ph["cap_h"]), ph["trees"][1]]
    tr, _ = Q.open_ref_trace(trees2, tree_of, leaf_idx)
    aux, apub = Q.open_gen_aux(tr, CHAL)
    assert S.check_trace(Q.open_air(), tr, ph["tabs"][0][1], CHAL, aux, apub) is None
    assert Q.roots_of(trees2)[0] != ph["roots"][0]
    assert not balances(ph, [(tr, ph["tabs"][0][1])] + ph["tabs"][1:])
    assert balances(ph, [(tr, ph["tabs"][0][1])] + ph["tabs"][1:], roots=Q.roots_of(trees2))  # ... and only that: for the other tree's verifier it closes


def sponge_forged(ph, edit):
    tree_of, leaf_idx = Q.openings_of(ph["index"], ph["NL"])
    rows = [[int(v) for v in Q.layer_rows(ph["layers"])[t][i]] for t, i in zip(tree_of, leaf_idx)]
    tree_of, rows = edit(list(tree_of), rows)
    tr, pub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows)
    return tr, ph["tabs"][1][1]


def test_a_sponge_leaf_labelled_with_the_other_tree(oracle):
    ph = phase(9, 2)

    def edit(tree_of, rows):
        tree_of[0] = 1
        return tree_of, rows

    tr, pub = sponge_forged(ph, edit)
    aux, apub = Q.sponge_gen_aux(tr, CHAL, pub)
    assert S.check_trace(Q.sponge_air(), tr, pub, CHAL, aux, apub) is None  # the table alone is satisfied
    assert not balances(ph, [ph["tabs"][0], (tr, pub), ph["tabs"][2]])      # TAG_OPEN (and TAG_ROW) of tree 0 stay open


def test_a_leaf_word_changed_in_the_sponge_table_only(oracle):
    ph = phase(9, 2)

    def edit(tree_of, rows):
        rows[1][7] ^= 1
        return tree_of, rows

    tr, pub = sponge_forged(ph, edit)
    aux, apub = Q.sponge_gen_aux(tr, CHAL, pub)
    assert S.check_trace(Q.sponge_air(), tr, pub, CHAL, aux, apub) is None
    assert not balances(ph, [ph["tabs"][0], (tr, pub), ph["tabs"][2]])  # FriFoldAir receives the word the chain was folded from
    # a tree id changed in the middle of a leaf is a rule of the table
    tr2 = tr.copy()
    tr2[Q.S_TREE, 64:128] = 1
    aux, apub = Q.sponge_gen_aux(tr2, CHAL, pub)
    bad = S.check_trace(Q.sponge_air(), tr2, pub, CHAL, aux, apub)
    assert bad is not None and bad[0] == Q.SPONGE_RULES["tree_carried"]


def test_two_roots_swapped_on_the_verifier_side(oracle):
    ph = phase(9, 2)
    assert not balances(ph, ph["tabs"], roots=ph["roots"][::-1])


@pytest.fixture(scope="module")
def proven(oracle):
    """ONE three-table reference-prover proof per shape, shared by the tests below"""
    out = {}
    for shape in SHAPES:
        ph = phase(*shape)
        out[shape] = Q.prove(ph["tabs"], CFG)
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_bus_balances_with_the_reference_prover(vx, proven, shape):
    ph, proofs = phase(*shape), proven[shape]
    ok, chal = Q.bus_check(proofs, CFG["cap_height"], ph["LN"], ph["NL"], ph["fpoly"], ph["roots"], ph["index"], ph["ev0"])
    assert ok
    for p, ref_id in zip(proofs, (Q.OPEN_REF_ID, Q.SPONGE_REF_ID, F.REF_ID)):
        assert any(S.verify(p, CFG, expect_air=ref_id, ext_chal=chal)["aux_public"])
    blob = Q.wrap(proofs, ph["LN"], ph["NL"], len(ph["index"]))
    assert all((a == b).all() for a, b in zip(Q.unwrap(blob), proofs))
    caps = np.array([t.cap for t in ph["trees"]], dtype=np.uint64)
    vx.lib.fri_queries_verify(blob, ph["LN"], ph["betas"], ph["fpoly"], caps, ph["index"], ph["ev0"], pcfg(vx))


def test_the_product_verifier_refuses_every_changed_claim(vx, proven):
    ph, proofs = phase(9, 2), proven[(9, 2)]
    cfg = pcfg(vx)
    blob = Q.wrap(proofs, 9, 2, 2)
    caps = np.array([t.cap for t in ph["trees"]], dtype=np.uint64)
    betas, fpoly, index, ev0 = np.array(ph["betas"], dtype=np.uint64), np.array(ph["fpoly"], dtype=np.uint64), list(ph["index"]), np.array(ph["ev0"], dtype=np.uint64)

    def refused(match=None, blob_=blob, LN=9, betas_=betas, fpoly_=fpoly, caps_=caps, index_=index, ev0_=ev0):
        with pytest.raises(vx.VxError, match=match):
            vx.lib.fri_queries_verify(blob_, LN, betas_, fpoly_, caps_, index_, ev0_, cfg)

    e2 = ev0.copy()
    e2[1, 0] ^= np.uint64(1)
    refused(ev0_=e2)                                   # one ev_0 word
    refused(index_=[index[0] ^ 1, index[1]])           # one index
    refused(index_=index[::-1], ev0_=ev0[::-1])        # two queries swapped
    b2 = betas.copy()
    b2[1, 1] ^= np.uint64(1)
    refused(betas_=b2)                                 # one beta word
    f2 = fpoly.copy()
    f2[0, 0] ^= np.uint64(1)
    refused(fpoly_=f2)                                 # one final-polynomial word
    c2 = caps.copy()
    c2[1, 1, 2] ^= np.uint64(1)
    refused(caps_=c2)                                  # one cap word
    refused(caps_=caps[::-1])                          # two caps swapped
    refused(match="different request", LN=10)          # a blob for another request
    refused(match="different request", index_=index[:1], ev0_=ev0[:1])
    refused(match="non-canonical", ev0_=np.array([[P, 0], ev0[1]], dtype=np.uint64))
    refused(match="outside the LDE", index_=[1 << 9, index[1]])
    other = Q.wrap([proofs[1], proofs[0], proofs[2]], 9, 2, 2)
    refused(blob_=other)                               # two proofs swapped in the blob
    for w in range(Q.HDR):
        bad = blob.copy()
        bad[w] ^= np.uint64(1)
        refused(blob_=bad)
    for cut in (0, 3, Q.HDR, Q.HDR + proofs[0].size, blob.size - 1):
        refused(blob_=blob[:cut])
    # none of the three proofs is a statement on its own: their challenges are shared
    with pytest.raises(vx.VxError):
        ev, leaves = F.claims_from(ph["layers"], index)
        vx.lib.fri_fold_verify(F.wrap(proofs[2], 9, 2, 2), 9, betas, fpoly, index, ev, leaves, cfg)
