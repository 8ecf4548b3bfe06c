"""The coefficient-space reference prover and its verifier agree with each other (CPU only)."""
import numpy as np
import pytest

from oracle import stark_ref as S


@pytest.mark.parametrize("air,log_n", [(S.FibAir, 5), (S.MixAir, 6), (S.MixAir, 9), (S.FibAir, 10), (S.LookupAir, 8), (S.LookupAir, 10)])
def test_prove_verify_roundtrip(oracle, air, log_n):
    trace, pub = air.trace(log_n)
    proof = S.prove(air, trace, pub)
    info = S.verify(proof, expect_air=air.ID, expect_public=pub)
    assert info["degree_bits"] == log_n
    for w in (12, 40, len(proof) // 2, len(proof) - 3):
        bad = proof.copy()
        bad[w] ^= np.uint64(1)
        with pytest.raises(S.VerifyError):
            S.verify(bad)
    with pytest.raises(S.VerifyError):
        S.verify(proof[:-1])
    with pytest.raises(S.VerifyError):
        S.verify(proof, expect_public=[p + 1 for p in pub] or [1])


def test_violating_trace_is_rejected_by_the_verifier(oracle):
    trace, pub = S.MixAir.trace(7)
    trace[1, 10] ^= np.uint64(1)
    with pytest.raises(S.VerifyError):
        S.verify(S.prove(S.MixAir, trace, pub))
    trace, pub = S.FibAir.trace(6)
    with pytest.raises(S.VerifyError):
        S.verify(S.prove(S.FibAir, trace, [pub[0], pub[1], pub[2] + 1]))


def test_lookup_air_auxiliary_round(oracle):
    """logUp: the honest trace satisfies every constraint for ANY challenges; a wrong multiplicity or a tuple that is
    not in the table breaks the running sum, and the verifier rejects the resulting proof."""
    A = S.LookupAir
    tr, pub = A.trace(9)
    chal = [3, 5, 7, 11]
    aux, apub = A.gen_aux(tr, chal)
    assert S.check_trace(A, tr, pub, chal, aux, apub) is None
    for col, row in ((6, 3), (2, 100), (0, 511)):
        bad = tr.copy()
        bad[col, row] = (int(bad[col, row]) + 1) % 16 if col != 6 else bad[col, row] + np.uint64(1)
        aux, apub = A.gen_aux(bad, chal)
        assert S.check_trace(A, bad, pub, chal, aux, apub) is not None
        with pytest.raises(S.VerifyError):
            S.verify(S.prove(A, bad, pub, dict(S.DEFAULT_CFG, num_queries=5)), dict(S.DEFAULT_CFG, num_queries=5))
    for air, L in ((S.FibAir, 6), (S.MixAir, 6)):
        t_, p_ = air.trace(L)
        assert S.check_trace(air, t_, p_) is None


# rate_bits 2 and 3: the coset has N = n 2^r points, the quotient 2n coefficients per challenge (the reference's outer
# Plonky2 config runs at rate_bits 3 with 28 queries)
HI_RATE = [(S.FibAir, 6), (S.MixAir, 7), (S.LookupAir, 8)]


def rate_cfg(r):
    return dict(S.DEFAULT_CFG, rate_bits=r, num_queries=28, pow_bits=8)


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("air,log_n", HI_RATE)
def test_prove_verify_roundtrip_high_rate(oracle, air, log_n, r):
    cfg = rate_cfg(r)
    trace, pub = air.trace(log_n)
    proof = S.prove(air, trace, pub, cfg)
    assert int(proof[5]) == r
    info = S.verify(proof, cfg, expect_air=air.ID, expect_public=pub)
    assert info["degree_bits"] == log_n
    for w in (12, 40, len(proof) // 2, len(proof) - 3):
        bad = proof.copy()
        bad[w] ^= np.uint64(1)
        with pytest.raises(S.VerifyError):
            S.verify(bad, cfg)
    with pytest.raises(S.VerifyError):
        S.verify(proof[:-1], cfg)
    with pytest.raises(S.VerifyError):
        S.verify(proof, cfg, expect_public=[p + 1 for p in pub] or [1])
    for other in (dict(cfg, rate_bits=1), dict(cfg, rate_bits=5 - r)):
        with pytest.raises(S.VerifyError, match="config mismatch"):
            S.verify(proof, other)


def quotient_coeffs(air, trace, pub, r, alphas, chal=None):
    """The prover's step 2 on its own: quotient values on the size-n 2^r coset -> coset_ifft coefficients [2][N]."""
    log_n = trace.shape[1].bit_length() - 1
    aux_pub = None
    if chal is not None:
        aux, aux_pub = air.gen_aux(trace, chal)
        trace = np.concatenate([trace, aux])
    leaves, _ = S.O.lde_from_values(trace, r, S.G)
    lde_nat = leaves[S.bitrev_perm(log_n + r)].T.copy()
    qv = S.quotient_values(air, lde_nat, [int(x) % S.P for x in pub], alphas, log_n, r, chal, aux_pub)
    return S.O.ntt(qv, inverse=True, shift=S.G)


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("air,log_n", HI_RATE)
def test_quotient_degree_is_below_2n(oracle, air, log_n, r):
    """For an honest trace every coefficient of the quotient from 2n on is exactly zero: what lets both provers commit only the
    first 2n (two chunks of n) per challenge at any rate.  A violating trace leaves non-zero coefficients up there at r >= 2."""
    n = 1 << log_n
    alphas = [0x0123456789ABCDEF % S.P, 0xFEDCBA9876543210 % S.P]
    chal = [3, 5, 7, 11] if getattr(air, "AUX", 0) else None
    trace, pub = air.trace(log_n)
    qc = quotient_coeffs(air, trace, pub, r, alphas, chal)
    assert qc.shape == (2, n << r)
    assert not qc[:, 2 * n:].any()
    assert qc[:, n:2 * n].any() == (air is not S.FibAir)  # constraints of degree 3 fill the second chunk (FibAir's are of degree 2)
    if r >= 2:
        bad = trace.copy()
        bad[1, n // 3] ^= np.uint64(1)
        assert quotient_coeffs(air, bad, pub, r, alphas, chal)[:, 2 * n:].any()


def test_violating_trace_is_rejected_at_rate_3(oracle):
    cfg = rate_cfg(3)
    trace, pub = S.MixAir.trace(7)
    trace[1, 10] ^= np.uint64(1)
    with pytest.raises(S.VerifyError, match="constraint identity"):
        S.verify(S.prove(S.MixAir, trace, pub, cfg), cfg)
    trace, pub = S.FibAir.trace(6)
    with pytest.raises(S.VerifyError, match="constraint identity"):
        S.verify(S.prove(S.FibAir, trace, [pub[0], pub[1], pub[2] + 1], cfg), cfg)
    tr, pub = S.LookupAir.trace(8)
    tr[6, 3] += np.uint64(1)  # a multiplicity one too high: the running sum does not close
    with pytest.raises(S.VerifyError):
        S.verify(S.prove(S.LookupAir, tr, pub, cfg), cfg)


@pytest.mark.parametrize("name,log_n,r", [("VX_AIR_MIX", 6, 2), ("VX_AIR_LOOKUP", 8, 1), ("VX_AIR_LOOKUP", 9, 3), ("VX_AIR_TRANSCRIPT", 6, 2), ("VX_AIR_FRI_FOLD", 3, 1)])
def test_quotient_values_at_chosen_points(oracle, name, log_n, r):
    """quotient_values(points=...) from the rows at the points and at their successors alone equals the corresponding entries of the
    full computation: the wrap-around (N - 2^r .. N - 1), point 0, repeated and unsorted points, periodic columns shorter than the
    trace (LookupAir at 2^9 rows: its table has period 2^8), an AIR with and without an auxiliary round."""
    import quotient_arbitrary as QA

    air, lde, pub, chal, apub, pairs = QA.arbitrary(name, log_n, r)
    N, step = 1 << (log_n + r), 1 << r
    rng = np.random.default_rng(9)
    pts = np.array([N - 1, 0, N - step, step - 1, N - step - 1, 1, 0, N // 2] + [int(v) for v in rng.integers(0, N, size=40)])
    for _, alphas in pairs:
        full = QA.reference(air, lde, pub, chal, apub, alphas, log_n, r)
        got = QA.reference(air, np.ascontiguousarray(lde[:, pts]), pub, chal, apub, alphas, log_n, r, points=pts, nxt_rows=np.ascontiguousarray(lde[:, (pts + step) % N]))
        assert got.shape == (2, pts.size) and (got == full[:, pts]).all()
    with pytest.raises(AssertionError):  # a point outside the coset
        QA.reference(air, np.ascontiguousarray(lde[:, :1]), pub, chal, apub, alphas, log_n, r, points=np.array([N]), nxt_rows=np.ascontiguousarray(lde[:, :1]))


def test_every_compiled_air_has_an_arbitrary_data_case(vx):
    """every AIR id the binding names is run by test_gpu_quotient_arbitrary.py or named in its docstring as covered through its
    template's smallest instantiation -- an AIR cannot be added without a case -- and the binding names every AIR of air_list.h"""
    import os
    import re

    import quotient_arbitrary as QA
    import test_gpu_quotient_arbitrary as G

    ids = QA.binding_air_ids(vx.lib)
    run = {name for name, _, _ in G.SMALL + G.FIXED + G.DEVICE}
    same_template = set(QA.AIR_NAME.findall(G.__doc__.split("Covered through their template's smallest instantiation")[1]))
    assert run <= set(ids) and same_template <= set(ids)
    assert run | same_template == set(ids), "AIRs without a case: %s" % sorted(set(ids) - run - same_template)
    assert run == set(QA.restatements()), "a restatement that no case uses, or a case without one"
    assert len(set(ids.values())) == len(ids)
    csrc = os.path.join(os.path.dirname(os.path.abspath(vx.lib.__file__)), "csrc")
    listed = re.search(r"using VxAirs = AirList<([^>]*)>", open(os.path.join(csrc, "air_list.h")).read()).group(1)
    assert len([a for a in listed.split(",") if a.strip()]) == len(ids)
