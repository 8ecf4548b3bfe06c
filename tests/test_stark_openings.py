"""A STARK proof's Merkle openings proven from the paths it carries, without a GPU: the openings table built from authentication
paths equals the one built from trees word for word; the reference group (stark_openings_ref: MerkleOpenSetAir and one
LeafSpongeSetAir table per leaf length above 4, under shared challenges) proves the openings of reference-prover proofs and the
product's vx_stark_openings_verify -- which walks no path, hashes no leaf and reads no sibling -- accepts them and refuses every
change; forged witnesses are refused by a named rule or by the bus.  Everything is exact."""
import numpy as np
import pytest

import fri_queries_ref as Q
import merkle_open_ref as M
import stark_openings_ref as SO
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CFG = dict(S.DEFAULT_CFG, num_queries=5)
CHAL = SO.CHAL


def pcfg(vx):
    return vx.lib.default_stark_config(num_queries=CFG["num_queries"])


@pytest.fixture(scope="module", autouse=True)
def entry_points(vx):
    """everything here restates or drives ONE feature of the library: without its entry points no test of this tier says anything"""
    L = vx.lib.load_library()
    for name in ("vx_stark_merkle_claims", "vx_merkle_paths_air_trace", "vx_leaf_sponge_rows_air_trace", "vx_stark_openings_proof_bound", "vx_stark_openings_prove",
                 "vx_stark_openings_verify"):
        assert hasattr(L, name), name


# ---- from paths equals from trees
# (depth, cap height) of the trees of one table, and the openings (tree, leaf): index 0 and the last index, a duplicate, a tree whose
# paths lie wholly above its cap (none of their siblings is in a proof) and one whose cap is its root (all of them are)
TREES = [(1, 0), (5, 2), (9, 3), (3, 3)]
OPENINGS = [(0, 1), (1, 0), (1, 31), (2, 0x155), (2, 511), (2, 0x155), (3, 5), (0, 0), (3, 0)]


@pytest.fixture(scope="module")
def forest(oracle):
    rng = np.random.default_rng(19)
    return [oracle.MerkleTree(rng.integers(0, P, size=(1 << d, 6), dtype=np.uint64), cap_h) for d, cap_h in TREES]


def paths_of(forest):
    tree_of, leaf_idx = [t for t, _ in OPENINGS], [i for _, i in OPENINGS]
    digests = [[int(v) for v in forest[t].leaf_digests()[i]] for t, i in OPENINGS]
    sibs = [np.array(forest[t].prove(i), dtype=np.uint64).reshape(-1, 4) for t, i in OPENINGS]
    return tree_of, leaf_idx, digests, sibs


def test_the_trace_from_paths_equals_the_trace_from_trees(oracle, forest):
    tree_of, leaf_idx, digests, sibs = paths_of(forest)
    for (d, cap_h), (t, _), s in zip([TREES[t] for t, _ in OPENINGS], OPENINGS, sibs):
        assert s.shape == (d - cap_h, 4)
    want, want_pub = Q.open_ref_trace(forest, tree_of, leaf_idx)
    got, got_pub, ends = SO.paths_ref_trace([t.cap for t in forest], [d for d, _ in TREES], tree_of, leaf_idx, digests, sibs)
    assert got.shape == want.shape == (Q.O_COLS, 1 << 11)  # 32 x (1 + 5 + 5 + 9 + 9 + 9 + 3 + 1 + 3) rows
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    assert got_pub == want_pub
    assert ends == [M.fold_cap(forest[t].cap) for t in tree_of]
    aux, apub = Q.open_gen_aux(got, CHAL)
    assert S.check_trace(Q.open_air(), got, got_pub, CHAL, aux, apub) is None


def forged_open(forest, edit):
    """the table of OPENINGS with the blocks of its fourth path (tree 2, nine levels, six siblings from the proof) replaced"""
    tree_of, leaf_idx, digests, sibs = paths_of(forest)
    caps, depths = [t.cap for t in forest], [d for d, _ in TREES]
    paths = [SO.path_blocks(t, i, d, s, caps[t], depths[t])[0] for t, i, d, s in zip(tree_of, leaf_idx, digests, sibs)]
    paths[3] = edit(caps, depths, digests[3], sibs[3])
    tr = Q.open_assemble([blk for p in paths for blk in p], 11)
    aux, apub = Q.open_gen_aux(tr, CHAL)
    return S.check_trace(Q.open_air(), tr, [0, 0, 0, 0], CHAL, aux, apub)


def test_a_changed_sibling_is_refused_by_the_root_rule_at_end(oracle, forest):
    def edit(caps, depths, digest, sib):
        sib = sib.copy()
        sib[2, 1] ^= np.uint64(1)
        blocks, end = SO.path_blocks(2, 0x155, digest, sib, caps[2], 9)
        assert end != blocks[0]["root"]
        return blocks

    bad = forged_open(forest, edit)
    assert bad is not None and bad[0] == Q.OPEN_RULES["output_is_root"]


def test_a_path_ended_at_another_trees_depth_is_refused(oracle, forest):
    def edit(caps, depths, digest, sib):
        return SO.path_blocks(2, 0x155, digest, sib, caps[2], 9, depth=5)[0]  # DEPTH says 5: the depth of tree 1

    bad = forged_open(forest, edit)
    assert bad is not None and bad[0] == Q.OPEN_RULES["level_is_depth"]


# ---- end to end on reference-prover proofs
def inner(name, other=False):
    if name == "fib":  # 2^5 rows: no FRI layer, every tree a no-op tree -> the openings table is alone
        return (S.FibAir,) + S.FibAir.trace(5, 3 if other else 0, 1)
    return (S.LookupAir,) + S.LookupAir.trace(8, seed=12 if other else 11)  # leaf lengths 7, 6 and 32 -> three sponge tables


@pytest.fixture(scope="module")
def proven(oracle):
    """per inner proof: the proof, its claims, the group's tables, their proofs and the blob (made once, never modified)"""
    out = {}
    for name in ("fib", "lookup"):
        air, tr, pub = inner(name)
        proof = S.prove(air, tr, pub, CFG)
        cl = SO.extract(proof, CFG)
        tabs, lens = SO.tables(cl)
        proofs = SO.prove(tabs, CFG)
        out[name] = dict(air=air, pub=pub, proof=proof, cl=cl, tabs=tabs, lens=lens, proofs=proofs, blob=SO.wrap(proofs, cl["shape"]))
    return out


def test_the_claims_of_the_product_are_the_restated_ones(vx, proven):
    for name, pv in proven.items():
        cl, mc = pv["cl"], vx.lib.stark_merkle_claims(pv["proof"], pcfg(vx))
        assert mc["shape"] == cl["shape"] and mc["trees"] == cl["trees"]
        assert (mc["caps"] == np.array([cl["caps"][t] for t in cl["trees"]], dtype=np.uint64)).all()
        assert len(mc["tree"]) == len(cl["claims"]) == CFG["num_queries"] * len(cl["trees"])
        for i, c in enumerate(cl["claims"]):
            assert (int(mc["tree"][i]), int(mc["index"][i]), int(mc["leaf_len"][i])) == (c["tree"], c["index"], len(c["leaf"]))
            assert [int(v) for v in mc["leaves"][i]] == [int(v) for v in c["leaf"]]
            assert (mc["siblings"][i] == c["sib"]).all()
    assert proven["fib"]["cl"]["shape"] == [6, 2, 0, 4, 0, 4, 5] and proven["fib"]["cl"]["trees"] == [8, 10]
    assert proven["lookup"]["cl"]["shape"] == [9, 7, 6, 4, 1, 4, 5] and proven["lookup"]["cl"]["trees"] == [8, 9, 10, 0]


def test_the_group_proves_the_openings_and_the_product_verifier_accepts(vx, proven):
    assert proven["fib"]["lens"] == [] and proven["lookup"]["lens"] == [6, 7, 32]
    # rows: 32 per level of every path, 32 per 8 words of every leaf
    assert [t.shape[1] for t, _ in proven["fib"]["tabs"]] == [1 << 11]                        # 32 x 5 x (6 + 6)
    assert [t.shape[1] for t, _ in proven["lookup"]["tabs"]] == [1 << 13, 1 << 8, 1 << 8, 1 << 10]  # 32 x 5 x (9 + 9 + 9 + 5); 32 x 5; 32 x 5; 32 x 5 x 4
    for name, pv in proven.items():
        cl, proofs, blob = pv["cl"], pv["proofs"], pv["blob"]
        for (tr, pub), a in zip(pv["tabs"], SO.airs(len(pv["tabs"]))):
            aux, apub = (Q.open_gen_aux if a is Q.open_air() else Q.sponge_gen_aux)(tr, CHAL, pub)
            assert S.check_trace(a, tr, pub, CHAL, aux, apub) is None
        ok, chal = SO.bus_check(proofs, CFG["cap_height"], cl)
        assert ok
        for p, a, (_, pub) in zip(proofs, SO.airs(len(proofs)), pv["tabs"]):
            S.verify(p, CFG, expect_air=a.ID, expect_public=pub, ext_chal=chal)
        assert all((a == b).all() for a, b in zip(SO.unwrap(blob), proofs))
        vx.lib.stark_openings_verify(blob, pv["proof"], pcfg(vx), expect_air=pv["air"].ID, expect_public=pv["pub"])
        vx.lib.stark_openings_verify(blob, pv["proof"], pcfg(vx))


def test_no_sibling_is_read(vx, proven):
    for pv in proven.values():
        zeroed = SO.zero_siblings(pv["proof"], pv["cl"])
        assert (zeroed != pv["proof"]).any()
        vx.lib.stark_openings_verify(pv["blob"], zeroed, pcfg(vx))
        with pytest.raises(vx.VxError, match="Merkle proof invalid"):
            vx.lib.stark_verify(zeroed, pcfg(vx))
        # ... not even for being canonical: only a mode that never looks at them accepts these
        junk = zeroed.copy()
        for c in pv["cl"]["claims"]:
            junk[c["sib_at"]: c["sib_at"] + c["sib"].size] = np.uint64(2**64 - 1)
        vx.lib.stark_openings_verify(pv["blob"], junk, pcfg(vx))


def flipped(proof, at):
    p = np.array(proof, dtype=np.uint64)
    p[at] ^= np.uint64(1)
    return p


def test_the_verifier_refuses_changed_proofs_and_blobs(vx, oracle, proven):
    cfg = pcfg(vx)
    for name, pv in proven.items():
        proof, blob, cl = pv["proof"], pv["blob"], pv["cl"]
        LN, cm, ca, a, NL, cap_h, n_q = cl["shape"]
        q0 = int(min(c["sib_at"] for c in cl["claims"])) - cm  # the first word of the first query record

        def refused(blob_=blob, proof_=proof, match=None, **kw):
            with pytest.raises(vx.VxError, match=match) as e:
                vx.lib.stark_openings_verify(blob_, proof_, cfg, **kw)
            assert e.value.code == -5

        assert [int(v) for v in proof[q0: q0 + cm]] == [int(v) for v in cl["claims"][0]["leaf"]]
        refused(proof_=flipped(proof, q0 + 1))                                   # one row word
        last = cl["claims"][-1]                                                  # (the quotient row of the last query, or its layer leaf)
        if NL:
            assert last["tree"] == 0 and len(last["leaf"]) == 32
            refused(proof_=flipped(proof, last["sib_at"] - 3))                   # one layer-leaf word
        cap_at = 12 + NL + len(pv["pub"])
        assert [int(v) for v in proof[cap_at: cap_at + 4]] == [int(v) for v in cl["caps"][8][0]]
        refused(proof_=flipped(proof, cap_at + 5))                               # one cap word
        air, tr, pub = inner(name, other=True)
        other = S.prove(air, tr, pub, CFG)
        assert other.size == proof.size and SO.extract(other, CFG)["shape"] == cl["shape"]
        refused(proof_=other)                                                    # the blob of another proof of the same shape
        if pv["pub"]:
            refused(match="public input", expect_public=[pv["pub"][0], pv["pub"][1], pv["pub"][2] ^ 1])
        refused(match="unexpected AIR", expect_air=2)
        refused(blob_=blob[:-9], match="inconsistent")                           # truncated by 9 words
        n_tab = int(blob[SO.HDR - 1])
        at, offsets = SO.HDR + n_tab, [0, 1, 4, SO.HDR - 1, SO.HDR]              # magic, shape words, the table count, a length
        for k in range(n_tab):                                                   # ... and inside each table proof: its head, a cap word, its last word
            size = int(blob[SO.HDR + k])
            offsets += [at + 2, at + 12 + int(blob[at + 9]) + 4 + 3, at + size - 1]
            at += size
        for w in offsets:
            refused(blob_=flipped(blob, w))


def test_a_sponge_leaf_labelled_with_the_wrong_tree(oracle, proven):
    """halfway through a leaf the label is a rule of the table (tree_carried); a whole leaf relabelled satisfies the sponge table
    alone and the bus refuses it: TAG_OPEN of its tree stays open, and the verifier receives the row words of ITS tree"""
    pv = proven["lookup"]
    cl, k = pv["cl"], 1 + pv["lens"].index(32)
    tr, pub = pv["tabs"][k]
    mid = tr.copy()
    mid[Q.S_TREE, 64:128] = 3
    aux, apub = Q.sponge_gen_aux(mid, CHAL, pub)
    bad = S.check_trace(Q.sponge_air(), mid, pub, CHAL, aux, apub)
    assert bad is not None and bad[0] == Q.SPONGE_RULES["tree_carried"]
    whole = tr.copy()
    whole[Q.S_TREE, 0:128] = 3
    aux, apub = Q.sponge_gen_aux(whole, CHAL, pub)
    assert S.check_trace(Q.sponge_air(), whole, pub, CHAL, aux, apub) is None

    def total(tabs):
        tot = S.ExtS(0)
        for (t, p), a in zip(tabs, SO.airs(len(tabs))):
            _, ap = (Q.open_gen_aux if a is Q.open_air() else Q.sponge_gen_aux)(t, CHAL, p)
            tot = tot + S.ExtS(*ap) * t.shape[1]
        return tot

    out = SO.outside_sum(CHAL, cl)
    assert total(pv["tabs"]) == out
    assert not (total(pv["tabs"][:k] + [(whole, pub)] + pv["tabs"][k + 1:]) == out)
