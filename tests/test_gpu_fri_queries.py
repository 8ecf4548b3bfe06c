"""The FRI query phase on one bus on the GPU: the witnesses and auxiliary columns of MerkleOpenSetAir (id 19) and LeafSpongeSetAir
(id 20) equal the reference generators cell by cell, public inputs included; the blob of vx_fri_queries_prove equals the reference
three-table prover's word for word and vx_fri_queries_verify -- which holds caps, betas, the final polynomial and (index, ev_0)
only -- accepts it and refuses every changed claim; a layer that is not its tree's, or not the fold of the layer before, is refused
with VX_ERR_STATEMENT before anything is proven; and the workload's shape (84 queries, a 2^21 LDE, four layers) built on the GPU
is proven and verified."""
import numpy as np
import pytest

import fri_fold_ref as F
import fri_queries_ref as Q
from oracle import stark_ref as S

P = F.P
CHAL = Q.CHAL

pytestmark = pytest.mark.gpu

# (LN, NL): one tree of depth 1; depths 5 and 1 (the smallest shape where two roots and two depths meet); depths 10, 6 and 2
SHAPES = [(5, 1), (9, 2), (14, 3)]
_phases, _trees = {}, {}


def phase(LN, NL):
    """one commit phase per shape (computed once, never modified): betas, final polynomial, layers as leaves, layers as values"""
    if (LN, NL) not in _phases:
        betas, fpoly, layers = F.commit_phase(LN, NL, seed=3 * LN + NL)
        _phases[(LN, NL)] = (betas, fpoly, layers, Q.layer_values(layers))
    return _phases[(LN, NL)]


def ref_trees(LN, NL, cap_h):
    if (LN, NL, cap_h) not in _trees:
        _trees[(LN, NL, cap_h)] = Q.layer_trees(phase(LN, NL)[2], cap_h)
    return _trees[(LN, NL, cap_h)]


def gpu_layers(ctx, LN, NL, cap_h, values=None):
    """the layers uploaded in natural order and their trees built by vx_fri_layer_tree"""
    values = phase(LN, NL)[3] if values is None else values
    evals = [ctx.from_host(v) for v in values]
    trees = [ctx.fri_layer_tree(evals[l], LN - 4 * l, 4, cap_h) for l in range(NL)]
    return evals, trees


def free(evals, trees):
    for t in trees:
        t.free()
    for e in evals:
        e.free()


def case_of(LN, NL, case):
    """-> (query indices, cap height of the layer trees, extra log2 of rows)"""
    top, cap_max = (1 << LN) - 1, LN - 4 * NL
    rng = np.random.default_rng(LN * 16 + NL)
    i = int(rng.integers(0, top + 1))
    if case == "single":
        return [i], min(1, cap_max), 0
    if case == "first_and_last_index":
        return [0, top], min(1, cap_max), 0
    if case == "duplicate":
        return [i, top // 3, i], min(1, cap_max), 0
    if case == "shared_layer1_leaf":  # the same index >> 8, another index >> 4
        return [i, i ^ 0x10], min(1, cap_max), 0
    if case == "idle_blocks":
        return [i, top // 5, top // 7], min(1, cap_max), 1
    if case == "fullest":  # fewer idle blocks in the openings table than one query takes
        levels = sum(LN - 4 * (l + 1) for l in range(NL))
        n_q = {1: 4, 6: 5, 18: 7}[levels]
        return [int(v) for v in rng.integers(0, top + 1, size=n_q)], min(1, cap_max), 0
    if case == "cap_height_0":
        return [i, top // 3], 0, 0
    if case == "cap_height_max":  # the last layer's paths lie wholly above the cap
        return [i, top // 3], cap_max, 0
    raise ValueError(case)


CASES = ["single", "first_and_last_index", "duplicate", "shared_layer1_leaf", "idle_blocks", "fullest", "cap_height_0", "cap_height_max"]
WITNESS = [(s, c) for s in SHAPES for c in CASES if not (c == "shared_layer1_leaf" and s[1] < 2)]


@pytest.mark.parametrize("shape,case", WITNESS, ids=["LN%d_NL%d-%s" % (s[0], s[1], c) for s, c in WITNESS])
def test_witnesses_equal_the_reference(ctx, vx, oracle, shape, case):
    LN, NL = shape
    index, cap_h, extra = case_of(LN, NL, case)
    layers = phase(LN, NL)[2]
    rtrees = ref_trees(LN, NL, cap_h)
    tree_of, leaf_idx = Q.openings_of(index, NL)
    rows = [Q.layer_rows(layers)[t][i] for t, i in zip(tree_of, leaf_idx)]
    if case == "shared_layer1_leaf":
        assert leaf_idx[1] == leaf_idx[NL + 1] and leaf_idx[0] != leaf_idx[NL]
    evals, trees = gpu_layers(ctx, LN, NL, cap_h)
    for t, rt in zip(trees, rtrees):
        assert (t.cap() == rt.cap).all()
    # ---- the openings table
    want, want_pub = Q.open_ref_trace(rtrees, tree_of, leaf_idx)
    log_n = want.shape[1].bit_length() - 1 + extra
    if extra:
        want, want_pub = Q.open_ref_trace(rtrees, tree_of, leaf_idx, log_n)
    if case == "fullest":
        assert want.shape[1] // 32 - int(want[Q.M.ACT].sum()) // 32 < sum(LN - 4 * (l + 1) for l in range(NL))
    tb, pub = ctx.merkle_open_set_air_trace(trees, tree_of, leaf_idx, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(Q.O_COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "openings: first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_MERKLE_OPEN_SET, tb, log_n, CHAL, vx.lib.VX_MERKLE_OPEN_SET_AIR_AUX_COLS, pub)
    want_aux, want_apub = Q.open_gen_aux(want, CHAL)
    got_aux = ab.download().reshape(Q.O_AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "openings: first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    assert S.check_trace(Q.open_air(), got, want_pub, CHAL, got_aux, want_apub) is None
    tb.free(), ab.free()
    # ---- the sponge table
    want, want_pub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows)
    log_n = want.shape[1].bit_length() - 1 + extra
    if extra:
        want, want_pub, _ = Q.sponge_ref_trace(tree_of, leaf_idx, rows, log_n)
    tb, pub = ctx.leaf_sponge_set_air_trace(evals, [LN - 4 * (l + 1) for l in range(NL)], tree_of, leaf_idx, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(Q.S_COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "sponge: first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_LEAF_SPONGE_SET, tb, log_n, CHAL, vx.lib.VX_LEAF_SPONGE_SET_AIR_AUX_COLS, pub)
    want_aux, want_apub = Q.sponge_gen_aux(want, CHAL, want_pub)
    got_aux = ab.download().reshape(Q.S_AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "sponge: first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    assert S.check_trace(Q.sponge_air(), got, want_pub, CHAL, got_aux, want_apub) is None
    tb.free(), ab.free()
    free(evals, trees)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=["LN5_NL1", "LN9_NL2"])
def test_blob_equals_the_reference_prover(ctx, vx, oracle, shape):
    LN, NL = shape
    betas, fpoly, layers, _ = phase(LN, NL)
    cap_h = LN - 4 * NL
    rng = np.random.default_rng(LN)
    index = [0, (1 << LN) - 1, int(rng.integers(0, 1 << LN))]
    index.append(index[2])  # one duplicate
    over = dict(num_queries=8)
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    evals, trees = gpu_layers(ctx, LN, NL, cap_h)
    blob = ctx.fri_queries_prove(LN, betas, fpoly, trees, evals, index, cfg)
    caps = np.array([t.cap() for t in trees], dtype=np.uint64)
    free(evals, trees)
    assert [int(v) for v in blob[:4]] == [Q.MAGIC, LN, NL, len(index)] and sum(int(v) for v in blob[4:7]) == blob.size - Q.HDR
    rtrees = ref_trees(LN, NL, cap_h)
    assert (caps == np.array([t.cap for t in rtrees], dtype=np.uint64)).all()
    tabs, ev0 = Q.tables(LN, betas, fpoly, layers, rtrees, index)
    want = Q.prove(tabs, ocfg)
    got = Q.unwrap(blob)
    for name, g, w in zip(("openings", "sponge", "fold"), got, want):
        assert g.size == w.size, name
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s: first differing proof word: %d" % (name, bad[0])
    ok, chal = Q.bus_check(got, ocfg["cap_height"], LN, NL, fpoly, Q.roots_of(rtrees), index, ev0)
    assert ok
    for p, ref_id, (_, pub) in zip(got, (Q.OPEN_REF_ID, Q.SPONGE_REF_ID, F.REF_ID), tabs):
        S.verify(p, ocfg, expect_air=ref_id, expect_public=pub, ext_chal=chal)
    vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps, index, ev0, cfg)


def test_verifier_refuses_changed_claims_and_prover_refuses_false_statements(ctx, vx, oracle):
    LN, NL, cap_h = 14, 3, 2
    betas, fpoly, layers, values = phase(LN, NL)
    index = [5, 0x2A7F, 0x1234]
    cfg = ctx.stark_config(num_queries=8)
    evals, trees = gpu_layers(ctx, LN, NL, cap_h)
    blob = ctx.fri_queries_prove(LN, betas, fpoly, trees, evals, index, cfg)
    caps = np.array([t.cap() for t in trees], dtype=np.uint64)
    ev0, _ = F.claims_from(layers, index)
    assert [int(blob[Q.HDR + 2]), int(blob[Q.HDR + int(blob[4]) + 2])] == [11, 11]  # 32 x 3 x 18 and 32 x 3 x 3 x 4 rows
    vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps, index, ev0, cfg)
    betas_a, fpoly_a = np.array(betas, dtype=np.uint64), np.array(fpoly, dtype=np.uint64)

    def refused(match=None, LN_=LN, betas_=betas_a, fpoly_=fpoly_a, caps_=caps, index_=index, ev0_=ev0):
        with pytest.raises(vx.VxError, match=match):
            vx.lib.fri_queries_verify(blob, LN_, betas_, fpoly_, caps_, index_, ev0_, cfg)

    e2 = ev0.copy()
    e2[2, 1] ^= np.uint64(1)
    refused(ev0_=e2)                                     # one ev_0 word
    refused(index_=[5, 0x2A7F, 0x1235])                  # one index
    b2 = betas_a.copy()
    b2[2, 0] ^= np.uint64(1)
    refused(betas_=b2)                                   # one beta word
    f2 = fpoly_a.copy()
    f2[1, 1] ^= np.uint64(1)
    refused(fpoly_=f2)                                   # one final-polynomial word
    c2 = caps.copy()
    c2[2, 3, 0] ^= np.uint64(1)
    refused(caps_=c2)                                    # one cap word
    refused(caps_=caps[[1, 0, 2]])                       # two caps swapped
    refused(match="different request", LN_=15)           # a blob for another request
    refused(match="different request", index_=index[:2], ev0_=ev0[:2])
    with pytest.raises(vx.VxError):
        vx.lib.stark_verify(blob[Q.HDR: Q.HDR + int(blob[4])], cfg, expect_air=Q.OPEN_ID)  # a table proof on its own
    # ---- trees[1] is not the tree of evals[1]: an OPENED leaf of layer 1 differs in what the tree was built from
    l2 = [lv.copy() for lv in layers]
    l2[1][index[1] >> 8, 3, 0] ^= np.uint64(1)
    assert (index[1] >> 4) & 15 != 3
    ev_b, tr_b = gpu_layers(ctx, LN, NL, cap_h, Q.layer_values(l2))
    with pytest.raises(vx.VxError, match="does not hash") as e:
        ctx.fri_queries_prove(LN, betas, fpoly, [trees[0], tr_b[1], trees[2]], evals, index, cfg)
    assert e.value.code == -5  # VX_ERR_STATEMENT
    # ---- evals[1] is not the fold of evals[0]: the slot query 1 enters layer 1 by (its tree is built from the changed layer)
    l3 = [lv.copy() for lv in layers]
    l3[1][index[1] >> 8, (index[1] >> 4) & 15, 1] ^= np.uint64(1)
    ev_c, tr_c = gpu_layers(ctx, LN, NL, cap_h, Q.layer_values(l3))
    with pytest.raises(vx.VxError, match="query 1, layer 1") as e:
        ctx.fri_queries_prove(LN, betas, fpoly, [trees[0], tr_c[1], trees[2]], [evals[0], ev_c[1], evals[2]], index, cfg)
    assert e.value.code == -5
    # ---- arguments
    with pytest.raises(vx.VxError, match="arity_bits 4") as e:
        ctx.fri_queries_prove(LN, betas, fpoly, trees, evals, index, ctx.stark_config(num_queries=8, arity_bits=3), out=np.zeros(1 << 16, dtype=np.uint64))
    assert e.value.code == -1  # VX_ERR_ARG
    # cap_height > LN - 4 NL: no tree of the last layer has such a cap, so it can only come with trees of mixed heights
    tr_d = [ctx.fri_layer_tree(evals[l], LN - 4 * l, 4, 3) for l in range(2)]
    with pytest.raises(vx.VxError, match="cap height") as e:
        ctx.fri_queries_prove(LN, betas, fpoly, tr_d + [trees[2]], evals, index, cfg)
    assert e.value.code == -1
    with pytest.raises(vx.VxError):
        ctx.fri_queries_prove(LN, betas, fpoly, trees, evals, [5, 1 << LN], cfg)  # an index outside the LDE
    with pytest.raises(vx.VxError) as e:
        ctx.fri_queries_prove(LN, betas, fpoly, trees, evals, index, cfg, out=np.zeros(blob.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == blob.size  # VX_ERR_BUFSZ with the length set
    again = ctx.fri_queries_prove(LN, betas, fpoly, trees, evals, index, cfg)  # the context is usable after every refusal
    assert (again == blob).all()
    for ev, tr in ((evals, trees), (ev_b, tr_b), (ev_c, tr_c), ([], tr_d)):
        free(ev, tr)


def test_workload_shape(ctx, vx, oracle):
    """84 queries (the queries of one STARK proof) of a 2^21 LDE, four layers built on the GPU from GPU-made layer-0 values.  The
    tables prove chains, not low degree: the final polynomial is interpolated from all 32 values of the last layer."""
    LN, NL, cap_h = 21, 4, 4
    rng = np.random.default_rng(84)
    betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
    evals = [ctx.alloc(2 << (LN - 4 * l)) for l in range(NL + 1)]
    ctx.fill_random(evals[0], 2 << LN, 2184)
    shift = 7
    for l in range(NL):
        ctx.fri_fold(evals[l], LN - 4 * l, 4, betas[l], shift, evals[l + 1])
        shift = pow(shift, 16, P)
    trees = [ctx.fri_layer_tree(evals[l], LN - 4 * l, 4, cap_h) for l in range(NL)]
    fpoly = oracle.ext_coset_ntt(evals[NL].download(), shift, inverse=True).reshape(-1, 2)
    index = [0, (1 << LN) - 1] + [int(v) for v in rng.integers(0, 1 << LN, size=81)]
    index.append(index[7])  # one duplicate
    assert len(index) == 84 and fpoly.shape == (32, 2)
    blob = ctx.fri_queries_prove(LN, betas, fpoly, trees[:NL], evals[:NL], index)
    sizes = [int(v) for v in blob[4:7]]
    assert [int(blob[Q.HDR + 2]), int(blob[Q.HDR + sizes[0] + 2]), int(blob[Q.HDR + sizes[0] + sizes[1] + 2])] == [17, 16, 10]  # degree bits of the three tables
    caps = np.array([t.cap() for t in trees], dtype=np.uint64)
    lv0 = ctx.fri_leaves(evals[0], LN, 4, [i >> 4 for i in index]).reshape(84, 16, 2)
    ev0 = np.array([lv0[k, i & 15] for k, i in enumerate(index)], dtype=np.uint64)
    vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps, index, ev0)
    e2 = ev0.copy()
    e2[83, 0] ^= np.uint64(1)
    with pytest.raises(vx.VxError):
        vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps, index, e2)
    with pytest.raises(vx.VxError):
        vx.lib.fri_queries_verify(blob, LN, betas, fpoly, caps[[0, 1, 3, 2]], index, ev0)
    free(evals, trees)
