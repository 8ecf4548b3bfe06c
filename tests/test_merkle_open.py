"""MerkleOpenAir (AIR id 16) without a GPU: the reference trace satisfies the independently restated AIR, forged witnesses do not
(and proofs made from them are refused by the product's host verifier), a reference-prover proof of the restatement passes the
product's vx_merkle_openings_verify -- the verifier being the other party of the logUp bus -- and every way of changing the
verifier's claims is refused.  Everything is exact."""
import numpy as np
import pytest

import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CFG = dict(S.DEFAULT_CFG, num_queries=8)
CASES, CHAL = M.CASES, M.CHAL


def make_tree(oracle, D, cap_height, seed=3):
    rng = np.random.default_rng(seed + 10 * D)
    return oracle.MerkleTree(rng.integers(0, P, size=(1 << D, 8), dtype=np.uint64), cap_height)


def pcfg(vx):
    return vx.lib.default_stark_config(num_queries=CFG["num_queries"])


def claims_of(trace):
    """the openings a trace sends: (R, LEAF) of every block with FIRSTB set"""
    rows = [r for r in range(0, trace.shape[1], 32) if int(trace[M.FIRSTB, r])]
    return [int(trace[M.R, r]) for r in rows], np.array([[int(trace[M.LEAF + i, r]) for i in range(4)] for r in rows], dtype=np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_trace_satisfies_the_restated_air(oracle, name):
    D, cap_height, idx = CASES[name]
    tree = make_tree(oracle, D, cap_height)
    trace, pub, digs = M.ref_trace(tree, idx)
    assert trace.shape == (M.COLS, 1 << M.log_rows(len(idx), D))
    assert pub[:4] == M.fold_cap(tree.cap) and pub[4] == D and pub[5:] == M.claims_digest(idx, digs)
    if cap_height == 0:
        assert pub[:4] == [int(v) for v in tree.cap[0]]
    assert (digs == tree.leaf_digests()[idx]).all()
    if name == "D2_Q4_no_idle_block":
        assert int(trace[M.END, -1]) == 1  # a path ends on the wrap-around pair
    aux, apub = M.gen_aux(trace, CHAL)
    assert S.check_trace(M.air(), trace, pub, CHAL, aux, apub) is None
    got_idx, got_digs = claims_of(trace)
    assert got_idx == idx and (got_digs == digs).all()


def forged(nodes, kind):
    """a witness that claims something the tree does not hold (D = 3, two paths; the first one is tampered with)"""
    honest = M.path_blocks(nodes, 6)
    first = M.path_blocks(nodes, 5)
    post = None
    if kind == "sibling_word":
        first[1]["sib"][2] ^= 1
    elif kind == "short_path":
        first = M.path_blocks(nodes, 5, start=1)
    elif kind == "top_is_not_the_root":
        first = M.path_blocks(nodes, 5, leaf=[9, 8, 7, 6])
    elif kind == "firstb_on_an_idle_block":
        def post(tr):
            tr[M.FIRSTB, 32 * 6: 32 * 7] = 1
    elif kind == "r_does_not_match_the_bits":
        first[0]["r"] ^= 2
    elif kind == "leaf_changed_midway":
        first[1]["leaf"] = [1, 2, 3, 4]
        first[2]["leaf"] = [1, 2, 3, 4]
    trace = M.assemble(first + honest, 8)
    if post:
        post(trace)
    return trace


@pytest.mark.parametrize("kind", ["sibling_word", "short_path", "top_is_not_the_root", "firstb_on_an_idle_block", "r_does_not_match_the_bits", "leaf_changed_midway"])
def test_forged_witnesses_are_refused(vx, oracle, kind):
    tree = make_tree(oracle, 3, 0)
    nodes = M.tree_nodes(tree)
    trace = forged(nodes, kind)
    idx, digs = claims_of(trace)
    pub = list(nodes[3][0]) + [3] + M.claims_digest(idx, digs)
    aux, apub = M.gen_aux(trace, CHAL)
    assert S.check_trace(M.air(), trace, pub, CHAL, aux, apub) is not None
    proof = M.prove(trace, pub, CFG)  # the prover does not care; the proof claims exactly what the forger wants
    ok, _ = M.bus_check(proof, CFG["cap_height"], idx, digs)
    assert ok  # ... and its bus balances against those claims: only the constraints stand in the way
    with pytest.raises(vx.VxError, match="constraint identity"):
        vx.lib.merkle_openings_verify(M.wrap(proof, 3, len(idx)), tree.cap, 3, idx, digs, pcfg(vx))


@pytest.fixture(scope="module")
def round_trip(oracle):
    """ONE reference-prover proof of the restatement (D = 3, three openings, cap height 1), shared by the tests below"""
    tree = make_tree(oracle, 3, 1)
    idx = [1, 6, 3]
    trace, pub, digs = M.ref_trace(tree, idx)
    proof = M.prove(trace, pub, CFG)
    return tree, idx, digs, pub, proof


def test_round_trip_through_both_verifiers(vx, round_trip):
    tree, idx, digs, pub, proof = round_trip
    blob = M.wrap(proof, 3, len(idx))
    cfg = pcfg(vx)
    vx.lib.merkle_openings_verify(blob, tree.cap, 3, idx, digs, cfg)
    ok, chal = M.bus_check(proof, CFG["cap_height"], idx, digs)
    assert ok
    info = S.verify(proof, CFG, expect_air=M.REF_ID, expect_public=pub, ext_chal=chal)
    assert any(info["aux_public"])

    def refused(cap=tree.cap, log_leaves=3, idx_=idx, digs_=digs, match=None):
        with pytest.raises(vx.VxError, match=match):
            vx.lib.merkle_openings_verify(M.wrap(proof, 3, len(idx_)), cap, log_leaves, idx_, digs_, cfg)

    refused(idx_=[1, 6, 2])                                       # one claim index
    d2 = digs.copy()
    d2[1, 3] ^= 1
    refused(digs_=d2)                                             # one digest word
    refused(idx_=[6, 1, 3], digs_=digs[[1, 0, 2]])                # the order of two claims
    c2 = tree.cap.copy()
    c2[1, 0] ^= 1
    refused(cap=c2)                                               # one cap word
    refused(log_leaves=4, match="different request")              # log_leaves
    refused(idx_=idx[:2], digs_=digs[:2])                         # one claim dropped
    refused(idx_=idx + [0], digs_=np.concatenate([digs, tree.leaf_digests()[:1]]))  # one claim added
    # the right digests attached to the wrong indices
    with pytest.raises(vx.VxError):
        vx.lib.merkle_openings_verify(blob, tree.cap, 3, [1, 6, 3], digs[[0, 2, 1]], cfg)
    # the table proof on its own is no statement: plain vx_stark_verify draws the lookup challenges from the proof's own transcript
    # (the identity at zeta fails under them) and would in any case refuse a stand-alone proof that publishes a non-zero bus total
    p16 = proof.copy()
    p16[1] = M.AIR_ID
    assert p16[10 + int(p16[9]) + 2 + 9 + (4 << CFG["cap_height"]):][:2].any()  # the published total is not zero
    with pytest.raises(vx.VxError, match="constraint identity|non-zero bus total"):
        vx.lib.stark_verify(p16, cfg, expect_air=M.AIR_ID)


def test_parser_robustness(vx, round_trip):
    tree, idx, digs, _, proof = round_trip
    blob = M.wrap(proof, 3, len(idx))
    cfg = pcfg(vx)
    for w in range(M.HDR):
        for b in range(64):
            bad = blob.copy()
            bad[w] ^= np.uint64(1 << b)
            with pytest.raises(vx.VxError):
                vx.lib.merkle_openings_verify(bad, tree.cap, 3, idx, digs, cfg)
    cuts = list(range(0, 40)) + list(range(40, blob.size, max(1, blob.size // 50))) + [blob.size - 1]
    for cut in cuts:
        with pytest.raises(vx.VxError):
            vx.lib.merkle_openings_verify(blob[:cut], tree.cap, 3, idx, digs, cfg)
        short = blob[:cut].copy()
        if cut > 3:
            short[3] = cut - M.HDR  # a consistent header over a truncated proof
            with pytest.raises(vx.VxError):
                vx.lib.merkle_openings_verify(short, tree.cap, 3, idx, digs, cfg)
