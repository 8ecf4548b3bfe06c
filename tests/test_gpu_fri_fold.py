"""FriFoldAir (AIR id 18) on the GPU: the witness, the auxiliary columns and the public inputs equal the reference generator cell by
cell, the proof inside the blob of vx_fri_fold_prove equals the reference prover's word for word, a real vx_stark_prove proof is
turned into claims by vx_stark_fri_claims and its fold chains are proven and checked, and the workload's shape (84 queries of a 2^21
LDE, four layers, one 2^10-row table) is proven and checked by vx_fri_fold_verify."""
import numpy as np
import pytest

import fri_fold_ref as F
from oracle import stark_ref as S

P = F.P
CHAL = F.CHAL

pytestmark = pytest.mark.gpu

# name -> (LN, NL): FB = LN - 4 NL; rows per query NL + FB = 2, 3, 6, 5
SHAPES = {"NL1_FB1": (5, 1), "NL2_FB1": (9, 2), "NL1_FB5": (9, 1), "NL3_FB2": (14, 3)}


def case_queries(LN, NL, case):
    """-> (query indices, log_n).  Only NL + FB = 2 divides a power of two: the other shapes' fullest table has fewer idle rows
    than one query takes"""
    rpq, top = LN - 3 * NL, (1 << LN) - 1
    rng = np.random.default_rng(LN * 16 + NL)
    if case == "single":
        return [int(rng.integers(0, top + 1))], 5
    if case == "duplicates":
        i = int(rng.integers(0, top + 1))
        return [i, top // 3, i, i], 5
    if case == "first_and_last_index":
        return [0, top], 5
    if case == "full":
        n = 64 // rpq
        return [int(v) for v in rng.integers(0, top + 1, size=n)], 6
    if case == "half_idle":
        n = 32 // rpq
        return [int(v) for v in rng.integers(0, top + 1, size=n)], 6
    if case == "two_workgroups":  # of the auxiliary kernel's 64 lanes: the queries end in the second, idle rows behind them
        n = 80 // rpq
        return [int(v) for v in rng.integers(0, top + 1, size=n)], 7
    raise ValueError(case)


def rand_claims(LN, NL, index, seed=5):
    """random leaves made chains (the table checks the chain, not low degree)"""
    rng = np.random.default_rng(seed)
    betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
    leaves = np.array([F.chain_leaves(i, rng.integers(0, P, size=(NL, 16, 2), dtype=np.uint64), betas, LN) for i in index], dtype=np.uint64)
    return betas, leaves


@pytest.mark.parametrize("case", ["single", "duplicates", "first_and_last_index", "full", "half_idle", "two_workgroups"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_witness_equals_the_reference(ctx, vx, oracle, shape, case):
    LN, NL = SHAPES[shape]
    index, log_n = case_queries(LN, NL, case)
    rpq, n = LN - 3 * NL, 1 << log_n
    if case == "full":
        assert n - len(index) * rpq < rpq and (shape != "NL1_FB1" or len(index) * rpq == n)
    if case == "half_idle":
        assert n // 2 - rpq < len(index) * rpq <= n // 2
    if case == "two_workgroups":
        assert 64 < len(index) * rpq < n
    tree0 = 3 if case in ("duplicates", "two_workgroups") else 0
    betas, leaves = rand_claims(LN, NL, index)
    ev0 = F.ev0_of(index, leaves)
    want, want_pub = F.ref_trace(index, leaves, betas, LN, log_n, tree0)
    tb, pub = ctx.fri_fold_air_trace(LN, betas, index, ev0, leaves, log_n, tree0)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(F.COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_FRI_FOLD, tb, log_n, CHAL, vx.lib.VX_FRI_FOLD_AIR_AUX_COLS, pub)
    want_aux, want_apub = F.gen_aux(want, CHAL, want_pub)
    got_aux = ab.download().reshape(F.AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    assert S.check_trace(F.air(), got, want_pub, CHAL, got_aux, want_apub) is None
    tb.free(), ab.free()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_proof_equals_the_reference_prover(ctx, vx, oracle, shape):
    LN, NL = SHAPES[shape]
    betas, fpoly, layers = F.commit_phase(LN, NL, seed=LN + NL)
    rng = np.random.default_rng(LN)
    index = [0, (1 << LN) - 1] + [int(v) for v in rng.integers(0, 1 << LN, size=3)]
    index.append(index[2])  # one duplicate
    ev0, leaves = F.claims_from(layers, index)
    over = dict(num_queries=8)
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    blob = ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves, cfg)
    assert [int(v) for v in blob[:4]] == [F.MAGIC, LN, NL, len(index)] and int(blob[4]) == blob.size - F.HDR and int(blob[F.HDR + 1]) == F.AIR_ID
    assert int(blob[F.HDR + 2]) == F.log_rows(len(index), LN, NL)
    trace, pub = F.ref_trace(index, leaves, betas, LN)
    want = F.prove(trace, pub, ocfg)
    got = F.unwrap(blob)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing proof word: %d" % bad[0]
    ok, chal = F.bus_check(got, ocfg["cap_height"], index, ev0, leaves, fpoly, LN, NL)
    assert ok
    S.verify(got, ocfg, expect_air=F.REF_ID, expect_public=pub, ext_chal=chal)
    vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, leaves, cfg)
    l2 = leaves.copy()
    l2[3, NL - 1, ((index[3] >> (4 * (NL - 1))) + 1) & 15, 0] ^= np.uint64(1)
    with pytest.raises(vx.VxError):  # (the claims digest is a public input: a changed claim is refused there, before the bus)
        vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, l2, cfg)


def test_the_fold_chains_of_a_real_proof(ctx, vx, oracle):
    """a FibAir proof of 2^13 rows at the default arity: a 2^14 LDE, two layers, six index bits left"""
    log_n = 13
    cfg, ocfg = ctx.stark_config(num_queries=5), dict(S.DEFAULT_CFG, num_queries=5)
    trace, pub = S.FibAir.trace(log_n)
    proof = ctx.stark_prove(S.FibAir.ID, ctx.from_host(trace), log_n, pub, cfg)
    vx.lib.stark_verify(proof, cfg, expect_air=S.FibAir.ID, expect_public=pub)
    c = vx.lib.stark_fri_claims(proof, cfg)
    LN, NL = c["log_lde"], len(c["betas"])
    assert (LN, NL, len(c["index"]), c["final_poly"].shape) == (14, 2, 5, (32, 2)) and c["leaves"].shape == (5, 2, 32)
    for k, i in enumerate(c["index"]):
        # slot `within` of the first leaf is ev_0, and the fold of the extracted chain is what the verifier compared with the final polynomial
        assert [int(v) for v in c["leaves"][k, 0].reshape(16, 2)[int(i) & 15]] == [int(v) for v in c["ev0"][k]]
        ev = F.fold_query(int(i), c["leaves"][k].reshape(NL, 16, 2), c["betas"], LN)
        assert [ev.a, ev.b] == [int(v) for v in c["ev_last"][k]]
        assert ev == F.final_eval(c["final_poly"], int(i), LN, NL)
    blob = ctx.fri_fold_prove(LN, c["betas"], c["final_poly"], c["index"], c["ev0"], c["leaves"], cfg)
    vx.lib.fri_fold_verify(blob, LN, c["betas"], c["final_poly"], c["index"], c["ev0"], c["leaves"], cfg)
    ok, _ = F.bus_check(F.unwrap(blob), ocfg["cap_height"], c["index"], c["ev0"], c["leaves"], c["final_poly"], LN, NL)
    assert ok
    e2 = c["ev0"].copy()
    e2[4, 0] ^= np.uint64(1)
    with pytest.raises(vx.VxError):  # (the claims digest is a public input: a changed claim is refused there, before the bus)
        vx.lib.fri_fold_verify(blob, LN, c["betas"], c["final_poly"], c["index"], e2, c["leaves"], cfg)
    bad = proof.copy()
    bad[-3] ^= np.uint64(1)
    with pytest.raises(vx.VxError):
        vx.lib.stark_fri_claims(bad, cfg)  # the proof is verified on the way


def test_workload_shape(ctx, vx, oracle):
    """84 queries (the queries of one STARK proof) of a 2^21 LDE, four layers, five index bits left: 756 rows in a 2^10-row table"""
    LN, NL = 21, 4
    betas, fpoly, layers = F.commit_phase(LN, NL, seed=84)
    rng = np.random.default_rng(84)
    index = [0, (1 << LN) - 1] + [int(v) for v in rng.integers(0, 1 << LN, size=81)]
    index.append(index[7])  # one duplicate
    assert len(index) == 84
    ev0, leaves = F.claims_from(layers, index)
    blob = ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves)
    assert int(blob[F.HDR + 2]) == 10  # degree bits of the table
    vx.lib.fri_fold_verify(blob, LN, betas, fpoly, index, ev0, leaves)

    def refused(betas_=betas, fpoly_=fpoly, index_=index, ev0_=ev0, leaves_=leaves):
        with pytest.raises(vx.VxError):
            vx.lib.fri_fold_verify(blob, LN, betas_, fpoly_, index_, ev0_, leaves_)

    l2 = leaves.copy()
    l2[40, 3, ((index[40] >> 12) + 5) & 15, 1] ^= np.uint64(1)
    refused(leaves_=l2)                                            # one leaf word outside the `within` slot
    e2 = ev0.copy()
    e2[83, 0] ^= np.uint64(1)
    refused(ev0_=e2)                                               # one ev_0
    b2 = [list(b) for b in betas]
    b2[3][1] ^= 1
    refused(betas_=b2)                                             # one beta
    f2 = fpoly.copy()
    f2[9, 1] ^= np.uint64(1)
    refused(fpoly_=f2)                                             # one final-polynomial coefficient
    refused(index_=index[:5] + [index[5] ^ 16] + index[6:])        # one index
    with pytest.raises(vx.VxError):
        vx.lib.stark_verify(blob[F.HDR:], expect_air=F.AIR_ID)     # the table proof on its own


def test_statement_and_argument_errors(ctx, vx, oracle):
    LN, NL = 9, 2
    betas, fpoly, layers = F.commit_phase(LN, NL, seed=2)
    index = [17, 400]
    ev0, leaves = F.claims_from(layers, index)
    cfg = ctx.stark_config(num_queries=8)
    l2 = leaves.copy()
    l2[1, 1, 5, 0] ^= np.uint64(1)  # an inconsistent leaf: not the slot the chain enters by, so the fold no longer ends in the final polynomial
    assert (index[1] >> 4) & 15 != 5
    with pytest.raises(vx.VxError, match="query 1, layer 2") as e:
        ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, l2, cfg)
    assert e.value.code == -5  # VX_ERR_STATEMENT
    l2 = leaves.copy()
    l2[0, 1, (index[0] >> 4) & 15, 1] ^= np.uint64(1)  # the slot the chain enters layer 1 by
    with pytest.raises(vx.VxError, match="query 0, layer 1") as e:
        ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, l2, cfg)
    assert e.value.code == -5
    e2 = ev0.copy()
    e2[0, 0] ^= np.uint64(1)
    with pytest.raises(vx.VxError, match="query 0, layer 0"):
        ctx.fri_fold_prove(LN, betas, fpoly, index, e2, leaves, cfg)
    with pytest.raises(vx.VxError, match="arity_bits 4") as e:
        ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves, ctx.stark_config(num_queries=8, arity_bits=3), out=np.zeros(1 << 16, dtype=np.uint64))
    assert e.value.code == -1  # VX_ERR_ARG
    with pytest.raises(vx.VxError) as e:
        ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves, ctx.stark_config(num_queries=8, arity_bits=3))
    assert e.value.code == -1
    with pytest.raises(vx.VxError):
        ctx.fri_fold_prove(LN, betas, fpoly, [17, 512], ev0, leaves, cfg)  # an index outside the LDE
    with pytest.raises(vx.VxError):
        ctx.fri_fold_prove(8, betas, fpoly, index, ev0, leaves, cfg)  # no index bit left behind two layers
    with pytest.raises(vx.VxError):
        ctx.fri_fold_air_trace(LN, betas, index * 6, np.tile(ev0, (6, 1)), np.tile(leaves, (6, 1, 1, 1)), 5)  # 36 rows do not fit 2^5
    full = ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves, cfg)
    with pytest.raises(vx.VxError) as e:
        ctx.fri_fold_prove(LN, betas, fpoly, index, ev0, leaves, cfg, out=np.zeros(full.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == full.size  # VX_ERR_BUFSZ with the length set
