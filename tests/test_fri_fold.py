"""FriFoldAir (AIR id 18) without a GPU: every constraint of the independently restated AIR has degree <= 3, the reference fold is
the Lagrange interpolation of the verifier's loop (restated here in big integers), the reference trace satisfies the restatement and
forged witnesses do not, a reference-prover proof of the restatement passes the product's vx_fri_fold_verify -- the verifier being
the other party of the bus -- and every way of changing the verifier's claims is refused.  Everything is exact."""
import numpy as np
import pytest

import fri_fold_ref as F
from oracle import stark_ref as S

P = F.P
CFG = dict(S.DEFAULT_CFG, num_queries=8)
CHAL = F.CHAL


def pcfg(vx, **over):
    return vx.lib.default_stark_config(num_queries=CFG["num_queries"], **over)


def rand_claims(LN, NL, index, seed=5):
    """random leaves made chains (the table checks the chain, not low degree) -> (betas, leaves [n][NL][16][2])"""
    rng = np.random.default_rng(seed)
    betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
    leaves = np.array([F.chain_leaves(i, rng.integers(0, P, size=(NL, 16, 2), dtype=np.uint64), betas, LN) for i in index], dtype=np.uint64)
    return betas, leaves


def test_every_constraint_has_degree_at_most_3(oracle):
    b = F.builder()
    degs = [F.degree(e) for _, e in b.constraints]
    assert len(degs) == 147 and max(degs) == 3
    assert all(kind == "assert_zero" for kind, _ in b.constraints)  # no first-row, last-row or transition constraints
    assert not b.periodic


# ---- the verifier's loop (compute_evaluation), restated in big integers
def ext_mul(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def lagrange_fold(leaf, within, beta, x):
    """leaf [16][2] in leaf order, x the point of slot `within`: interpolate the coset {start g^i} and evaluate at beta"""
    g = pow(7, (P - 1) // 16, P)
    evn = [None] * 16
    for t in range(16):
        evn[F.brev(t, 4)] = (int(leaf[t][0]), int(leaf[t][1]))
    start = x * pow(g, 16 - F.brev(within, 4), P) % P
    pts = [start * pow(g, t, P) % P for t in range(16)]
    acc = (0, 0)
    for i in range(16):
        num, den = (1, 0), 1
        for j in range(16):
            if j != i:
                num = ext_mul(num, ((beta[0] - pts[j]) % P, beta[1]))
                den = den * (pts[i] - pts[j]) % P
        term = ext_mul(ext_mul(evn[i], num), (pow(den, P - 2, P), 0))
        acc = ((acc[0] + term[0]) % P, (acc[1] + term[1]) % P)
    return acc


@pytest.mark.parametrize("within", [0, 6, 15])
def test_reference_fold_is_the_lagrange_form(oracle, within):
    assert pow(7, (P - 1) // 16, P) == F.G16
    rng = np.random.default_rng(within)
    LN, index = 13, (0x1A5 << 4) | within
    x = 7 * pow(oracle.root(LN), F.brev(index, LN), P) % P  # x from a real index
    leaf = rng.integers(0, P, size=(16, 2), dtype=np.uint64)
    beta = [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)]
    got, _ = F.fold_leaf([F.ext(v) for v in leaf], within, F.ext(beta), F.x_inv_of(index, LN))
    assert (got.a, got.b) == lagrange_fold(leaf, within, beta, x)
    # ... and of a second layer: x^16, the next digit
    x2, w2 = pow(x, 16, P), (index >> 4) & 15
    got, _ = F.fold_leaf([F.ext(v) for v in leaf], w2, F.ext(beta), pow(F.x_inv_of(index, LN), 16, P))
    assert (got.a, got.b) == lagrange_fold(leaf, w2, beta, x2)


SHAPES = {
    "NL1_FB1": (5, 1, [19, 0, 31, 19]),
    "NL2_FB1": (9, 2, [0x155, 0, 511]),
    "NL1_FB5": (9, 1, [300, 7]),
    "NL3_FB2": (14, 3, [0x2ABC, (1 << 14) - 1]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_trace_satisfies_the_restated_air(oracle, name):
    LN, NL, index = SHAPES[name]
    betas, leaves = rand_claims(LN, NL, index)
    trace, pub = F.ref_trace(index, leaves, betas, LN)
    assert trace.shape == (F.COLS, 1 << F.log_rows(len(index), LN, NL))
    assert pub[:2] == [NL, LN - 3 * NL] and pub[2] * oracle.root(LN) % P == 1 and pub[F.PUB_BETA + 2 * NL: F.PUB_DIGEST] == [0] * (16 - 2 * NL)
    aux, apub = F.gen_aux(trace, CHAL, pub)
    assert S.check_trace(F.air(), trace, pub, CHAL, aux, apub) is None
    # what leaves the table is the fold of the chain
    for k, i in enumerate(index):
        row = k * (LN - 3 * NL) + NL
        want = F.fold_query(i, leaves[k], betas, LN)
        assert int(trace[F.FBIT, row]) == 1 and (int(trace[F.EV, row]), int(trace[F.EV + 1, row])) == (want.a, want.b)


def test_a_table_without_an_idle_row_wraps_around(oracle):
    LN, NL = 5, 1
    index = list(range(3, 19))  # 16 queries of 2 rows: 2^5 rows
    betas, leaves = rand_claims(LN, NL, index)
    trace, pub = F.ref_trace(index, leaves, betas, LN)
    assert trace.shape[1] == 32 and int(trace[F.LAST, -1]) == 1  # a query ends on the wrap-around pair
    aux, apub = F.gen_aux(trace, CHAL, pub)
    assert S.check_trace(F.air(), trace, pub, CHAL, aux, apub) is None


# positions in the constraint order of fri_fold_ref.builder (31 boolean cells, 12 shape constraints, then group 3 ...)
N_BOOL, N_SHAPE = 31, 12
ROWS_RULE, CLOSING = N_BOOL + N_SHAPE + 2, N_BOOL + N_SHAPE + 5   # LAST (CNT + 1 - rows), LAST Q
ONE_HOT = N_BOOL + N_SHAPE + 8 + 1                                # sum t OH[t] = FOLD within
X0_RULE = N_BOOL + N_SHAPE + 8 + 4 + 7 + 6                        # LAST (Y0 - A1 / 7)
LEAF_SLOT = X0_RULE + 1 + 8                                       # sum OH[t] LEAF[t] = FOLD EV (first word)


@pytest.mark.parametrize("kind", ["wrong_digit_hidden_by_division", "one_hot_disagrees_with_the_bits", "leaf_slot_is_not_ev", "x0_from_another_index", "one_row_short"])
def test_forged_witnesses_are_refused(oracle, kind):
    LN, NL, index = 14, 3, 0x2ABC
    betas, leaves = rand_claims(LN, NL, [index, 77])
    honest = F.query_rows(77, leaves[1], betas, LN)
    want_bad = None
    if kind == "wrong_digit_hidden_by_division":
        # the chain is folded as another index (digit 1 differs) while R starts from the claimed one and is continued by field
        # division: every row rule holds, the entry message names the claimed index -- only the closing rule (no bit left) fails
        other = index ^ (5 << 4)
        lv = F.chain_leaves(other, leaves[0], betas, LN)
        first = F.query_rows(other, lv, betas, LN, r_start=index)
        assert int(first[F.IDX, 0]) == index and int(first[F.Q, -1]) != 0
        want_bad = (CLOSING, LN - 3 * NL - 1)
    elif kind == "one_hot_disagrees_with_the_bits":
        first = F.query_rows(index, leaves[0], betas, LN)
        w = (index >> 4) & 15
        first[F.OH + w, 1], first[F.OH + (w ^ 3), 1] = 0, 1
        want_bad = (ONE_HOT, 1)
    elif kind == "leaf_slot_is_not_ev":
        first = F.query_rows(index, leaves[0], betas, LN)
        first[F.LEAF + 2 * ((index >> 4) & 15), 1] ^= np.uint64(1)
        want_bad = (LEAF_SLOT, 1)
    elif kind == "x0_from_another_index":
        first = F.query_rows(index, leaves[0], betas, LN, y_index=index ^ 1)
        want_bad = (X0_RULE, LN - 3 * NL - 1)
    elif kind == "one_row_short":
        first = F.query_rows(index, leaves[0], betas, LN, n_rows=LN - 3 * NL - 1)
        want_bad = (ROWS_RULE, LN - 3 * NL - 2)
    trace = F.assemble([first, honest], 5)
    pub = F.public_inputs([index, 77], F.ev0_of([index, 77], leaves), leaves, betas, LN)
    aux, apub = F.gen_aux(trace, CHAL, pub)
    assert S.check_trace(F.air(), trace, pub, CHAL, aux, apub) == want_bad


@pytest.fixture(scope="module")
def round_trip(oracle):
    """ONE reference-prover proof of the restatement (LN = 9, two layers, three queries cut from a commit phase on a random
    polynomial; one index twice), shared by the tests below"""
    LN, NL = 9, 2
    betas, fpoly, layers = F.commit_phase(LN, NL, seed=4)
    index = [5, 500, 5]
    ev0, leaves = F.claims_from(layers, index)
    for i, lv in zip(index, leaves):
        assert F.fold_query(i, lv, betas, LN) == F.final_eval(fpoly, i, LN, NL)  # the commit phase and the fold agree
    trace, pub = F.ref_trace(index, leaves, betas, LN)
    return LN, betas, fpoly, index, ev0, leaves, pub, F.prove(trace, pub, CFG)


def test_round_trip_through_both_verifiers(vx, round_trip):
    LN, betas, fpoly, index, ev0, leaves, pub, proof = round_trip
    NL = len(betas)
    blob = F.wrap(proof, LN, NL, len(index))
    cfg = pcfg(vx)
    vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, leaves, cfg)
    ok, chal = F.bus_check(proof, CFG["cap_height"], index, ev0, leaves, fpoly, LN, NL)
    assert ok
    info = S.verify(proof, CFG, expect_air=F.REF_ID, expect_public=pub, ext_chal=chal)
    assert any(info["aux_public"])

    def refused(betas_=betas, fpoly_=fpoly, index_=index, ev0_=ev0, leaves_=leaves, log_lde=LN, match=None):
        with pytest.raises(vx.VxError, match=match):
            vx.lib.fri_fold_verify(F.wrap(proof, LN, NL, len(index_)), log_lde, betas_, fpoly_, index_, ev0_, leaves_, cfg)

    within = index[1] & 15
    l2 = leaves.copy()
    l2[1, 0, (within + 1) & 15, 1] ^= np.uint64(1)
    refused(leaves_=l2)                                           # one leaf word outside the `within` slot
    l2 = leaves.copy()
    l2[2, 1, 3, 0] ^= np.uint64(1)
    refused(leaves_=l2)                                           # ... in the second layer
    e2 = ev0.copy()
    e2[0, 1] ^= np.uint64(1)
    refused(ev0_=e2)                                              # one ev_0
    b2 = [list(b) for b in betas]
    b2[1][0] ^= 1
    refused(betas_=b2)                                            # one beta
    f2 = fpoly.copy()
    f2[-1, 0] ^= np.uint64(1)
    refused(fpoly_=f2)                                            # one final-polynomial coefficient
    refused(index_=[5, 501, 5])                                   # one index
    refused(index_=[500, 5, 5], ev0_=ev0[[1, 0, 2]], leaves_=leaves[[1, 0, 2]])  # the order of two claims
    refused(index_=index[:2], ev0_=ev0[:2], leaves_=leaves[:2])   # one claim dropped
    refused(log_lde=10, match="different request")
    with pytest.raises(vx.VxError) as e:
        vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, leaves, pcfg(vx, arity_bits=3))
    assert e.value.code == -1 and "arity_bits 4" in str(e.value)  # VX_ERR_ARG, and says why
    # the table proof on its own is no statement
    p18 = proof.copy()
    p18[1] = F.AIR_ID
    with pytest.raises(vx.VxError, match="constraint identity|non-zero bus total"):
        vx.lib.stark_verify(p18, cfg, expect_air=F.AIR_ID)


def test_a_forged_proof_is_refused_by_the_product(vx, oracle):
    """the prover does not care: a proof made from the wrong-digit witness balances its bus against the forger's claims, and only
    the compiled constraints stand in the way"""
    LN, NL, index = 9, 2, 0x155
    betas, leaves = rand_claims(LN, NL, [index])
    other = index ^ (5 << 4)
    lv = F.chain_leaves(other, leaves[0], betas, LN)
    trace = F.assemble([F.query_rows(other, lv, betas, LN, r_start=index)], 5)
    ev0 = F.ev0_of([other], [lv])
    pub = F.public_inputs([index], ev0, [lv], betas, LN)
    proof = F.prove(trace, pub, CFG)
    fpoly = np.zeros((1, 2), dtype=np.uint64)
    with pytest.raises(vx.VxError, match="constraint identity"):
        vx.lib.fri_fold_verify(F.wrap(proof, LN, NL, 1), LN, betas, fpoly, [index], ev0, [lv], pcfg(vx))


def test_parser_robustness(vx, round_trip):
    LN, betas, fpoly, index, ev0, leaves, _, proof = round_trip
    blob = F.wrap(proof, LN, len(betas), len(index))
    cfg = pcfg(vx)
    for w in range(F.HDR):
        for b in range(64):
            bad = blob.copy()
            bad[w] ^= np.uint64(1 << b)
            with pytest.raises(vx.VxError):
                vx.lib.fri_fold_verify(bad, LN, betas, fpoly, index, ev0, leaves, cfg)
    for cut in list(range(0, 40)) + list(range(40, blob.size, max(1, blob.size // 50))) + [blob.size - 1]:
        with pytest.raises(vx.VxError):
            vx.lib.fri_fold_verify(blob[:cut], LN, betas, fpoly, index, ev0, leaves, cfg)
        short = blob[:cut].copy()
        if cut > 4:
            short[4] = cut - F.HDR  # a consistent header over a truncated proof
            with pytest.raises(vx.VxError):
                vx.lib.fri_fold_verify(short, LN, betas, fpoly, index, ev0, leaves, cfg)
    nc = leaves.copy()
    nc[0, 0, 0, 0] = np.uint64(P)
    with pytest.raises(vx.VxError, match="non-canonical"):
        vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, nc, cfg)
    with pytest.raises(vx.VxError, match="outside the LDE"):
        vx.lib.fri_fold_verify(blob, LN, betas, fpoly, [5, 512, 5], ev0, leaves, cfg)


def test_fri_claims_of_a_reference_proof(vx, oracle):
    """vx_stark_fri_claims on a FibAir proof by the reference prover (2^13 rows: a 2^14 LDE, two layers): the extracted chains
    fold to what the final polynomial gives, slot `within` of every leaf is filled, and the claims' own table accepts them"""
    cfg = dict(S.DEFAULT_CFG, num_queries=5)
    trace, pub = S.FibAir.trace(13)
    proof = S.prove(S.FibAir, trace, pub, cfg)
    pc = vx.lib.default_stark_config(num_queries=5)
    c = vx.lib.stark_fri_claims(proof, pc)
    LN, NL = c["log_lde"], len(c["betas"])
    assert (LN, NL, len(c["index"]), c["final_poly"].shape, c["leaves"].shape) == (14, 2, 5, (32, 2), (5, 2, 32))
    for k, i in enumerate(c["index"]):
        lv = c["leaves"][k].reshape(NL, 16, 2)
        assert [int(v) for v in lv[0, int(i) & 15]] == [int(v) for v in c["ev0"][k]]
        assert (F.chain_leaves(int(i), lv, c["betas"], LN) == lv).all()
        ev = F.fold_query(int(i), lv, c["betas"], LN)
        assert [ev.a, ev.b] == [int(v) for v in c["ev_last"][k]] and ev == F.final_eval(c["final_poly"], int(i), LN, NL)
    tr, fpub = F.ref_trace(c["index"], c["leaves"], c["betas"], LN)
    blob = F.wrap(F.prove(tr, fpub, cfg), LN, NL, 5)
    vx.lib.fri_fold_verify(blob, LN, c["betas"], c["final_poly"], c["index"], c["ev0"], c["leaves"], pc)
    bad = proof.copy()
    bad[-3] ^= np.uint64(1)
    with pytest.raises(vx.VxError):
        vx.lib.stark_fri_claims(bad, pc)  # the proof is verified on the way
    with pytest.raises(vx.VxError) as e:
        vx.lib.stark_fri_claims(proof, vx.lib.default_stark_config(num_queries=5, arity_bits=3))
    assert e.value.code == -1 and "arity_bits 4" in str(e.value)
