"""GPU STARK prover (evaluation-space) vs the coefficient-space reference prover: identical bytes,
and the reference verifier accepts the GPU's proof."""
import numpy as np
import pytest

from oracle import oracle as O
from oracle import stark_ref as S
from quotient_arbitrary import sample_points

P = 2**64 - 2**32 + 1

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("air,log_n", [(S.FibAir, 5), (S.FibAir, 6), (S.FibAir, 9), (S.FibAir, 13), (S.MixAir, 4), (S.MixAir, 6),
                                        (S.MixAir, 10), (S.MixAir, 14), (S.LookupAir, 8), (S.LookupAir, 9), (S.LookupAir, 13)])
def test_proof_bytes_match_reference_prover(ctx, oracle, air, log_n):
    trace, pub = air.trace(log_n)
    got = ctx.stark_prove(air.ID, ctx.from_host(trace), log_n, pub)
    want = S.prove(air, trace, pub)
    assert got.size == want.size
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"first differing word {diff[:5]} of {got.size}"
    S.verify(got, expect_air=air.ID, expect_public=pub)


# rate_bits 2 and 3 (the reference's outer config is rate_bits 3 with 28 queries).  MixAir's quotient kernel takes two points per
# lane once N = n 2^r >= 512 (launch_q): (4, 3) and (6, 2) stay below that, (7, 2) and (9, 3) are above it.
@pytest.mark.parametrize("air,log_n,r", [(S.FibAir, 5, 2), (S.FibAir, 9, 3), (S.MixAir, 4, 3), (S.MixAir, 6, 2), (S.MixAir, 7, 2), (S.MixAir, 9, 3),
                                          (S.LookupAir, 8, 2), (S.LookupAir, 9, 3)])
def test_proof_bytes_match_reference_prover_high_rate(ctx, vx, oracle, air, log_n, r):
    over = dict(rate_bits=r, num_queries=28, pow_bits=8)
    cfg, pcfg = dict(S.DEFAULT_CFG, **over), ctx.stark_config(**over)
    trace, pub = air.trace(log_n)
    got = ctx.stark_prove(air.ID, ctx.from_host(trace), log_n, pub, pcfg)
    want = S.prove(air, trace, pub, cfg)
    assert got.size == want.size
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"first differing word {diff[:5]} of {got.size}"
    S.verify(got, cfg, expect_air=air.ID, expect_public=pub)
    vx.lib.stark_verify(got, pcfg, expect_air=air.ID, expect_public=pub)


def test_other_configs(ctx, oracle):
    trace, pub = S.MixAir.trace(11)
    for over in (dict(num_queries=10, pow_bits=8), dict(cap_height=0, num_queries=5), dict(arity_bits=3, final_poly_bits=3, num_queries=7),
                 dict(arity_bits=2, final_poly_bits=0, num_queries=3, pow_bits=0), dict(rate_bits=3, num_queries=28)):
        cfg = dict(S.DEFAULT_CFG, **over)
        got = ctx.stark_prove(S.MixAir.ID, ctx.from_host(trace), 11, pub, ctx.stark_config(**over))
        assert (got == S.prove(S.MixAir, trace, pub, cfg)).all(), over
        S.verify(got, cfg)


def test_large_trace_verifies(ctx, oracle):
    """2^18-row trace: too slow for the python prover, but the reference VERIFIER checks the GPU proof."""
    log_n = 18
    trace, pub = S.FibAir.trace(log_n)
    proof = ctx.stark_prove(S.FibAir.ID, ctx.from_host(trace), log_n, pub)
    S.verify(proof, expect_public=pub)
    bad = proof.copy()
    bad[-7] ^= np.uint64(1)
    with pytest.raises(S.VerifyError):
        S.verify(bad)


def test_argument_errors(ctx, vx):
    trace, pub = S.FibAir.trace(6)
    buf = ctx.from_host(trace)
    with pytest.raises(vx.VxError) as e:
        ctx.stark_prove(99, buf, 6, pub)
    assert e.value.code == -1
    with pytest.raises(vx.VxError):
        ctx.stark_prove(S.FibAir.ID, buf, 6, pub[:2])
    with pytest.raises(vx.VxError):
        ctx.stark_prove(S.FibAir.ID, buf, 9, pub)  # trace buffer too small for 2^9 rows


@pytest.mark.parametrize("air_name,log_n", [("mix", 6), ("fib", 5)])
def test_quotient_eval_primitive_matches_reference(ctx, vx, oracle, air_name, log_n):
    """K5 on its own (vx_quotient_eval): every quotient value on the coset, both challenges, equals the reference's
    compute_quotient_polys restatement (oracle/stark_ref.quotient_values)."""
    air = S.MixAir if air_name == "mix" else S.FibAir
    trace, pub = air.trace(log_n)
    r = 1
    leaves, _ = oracle.lde_from_values(trace, r, 7)
    lde_nat = leaves[S.bitrev_perm(log_n + r)].T.copy()
    alphas = [0x123456789ABCDEF % P, 0xFEDCBA987654321 % P]
    want = S.quotient_values(air, lde_nat, [int(x) % P for x in pub], alphas, log_n, r)
    got = ctx.quotient_eval(air.ID, r, ctx.from_host(np.ascontiguousarray(lde_nat)), log_n, alphas, pub)
    assert (got == want).all()


@pytest.mark.parametrize("air_name,log_n,r", [("mix", 6, 2), ("mix", 7, 3), ("fib", 5, 2), ("fib", 6, 3)])
def test_quotient_eval_primitive_high_rate(ctx, vx, oracle, air_name, log_n, r):
    """vx_quotient_eval at rate_bits 2 and 3 (mix (7, 3) takes the two-points-per-lane kernel) against the reference."""
    air = S.MixAir if air_name == "mix" else S.FibAir
    trace, pub = air.trace(log_n)
    leaves, _ = oracle.lde_from_values(trace, r, 7)
    lde_nat = leaves[S.bitrev_perm(log_n + r)].T.copy()
    alphas = [0x123456789ABCDEF % P, 0xFEDCBA987654321 % P]
    want = S.quotient_values(air, lde_nat, [int(x) % P for x in pub], alphas, log_n, r)
    got = ctx.quotient_eval(air.ID, r, ctx.from_host(np.ascontiguousarray(lde_nat)), log_n, alphas, pub)
    assert (got == want).all()


def quotient_at(air, lde, i, log_n, r, pub, alphas):
    """One quotient value pair, straight from the definition in python integers: the AIR's own eval on the row (i, i + 2^r) of the
    size-n 2^r coset g<w_N>, starky's ConstraintConsumer, divided by Z_H(x) = x^n - 1."""
    N, n = 1 << (log_n + r), 1 << log_n
    X = S.ExtS
    x = S.G * pow(O.root(log_n + r), i, P) % P
    last = pow(O.root(log_n), P - 2, P)
    zh = (pow(x, n, P) - 1) % P
    ninv = pow(n, P - 2, P)
    l_first = zh * ninv % P * pow((x - 1) % P, P - 2, P) % P
    l_last = zh * ninv % P * last % P * pow((x - last) % P, P - 2, P) % P
    cons = S.Consumer([X(a) for a in alphas], X(x - last), X(l_first), X(l_last), X(0))
    c = lde.shape[0]
    loc = [X(int(lde[j, i])) for j in range(c)]
    nxt = [X(int(lde[j, (i + (1 << r)) % N])) for j in range(c)]
    per = []
    for vals in air.periodic_values():
        co, y, acc = S.periodic_poly_coeffs(vals), pow(x, n // len(vals), P), 0
        for k in reversed(co):
            acc = (acc * y + k) % P
        per.append(X(acc))
    air.eval(loc, nxt, per, [X(v) for v in pub], cons)
    zinv = pow(zh, P - 2, P)
    assert all(a.b == 0 for a in cons.acc)
    return [a.a * zinv % P for a in cons.acc]


@pytest.mark.parametrize("air", [S.FibAir, S.MixAir])
def test_quotient_eval_at_2_22_points(ctx, vx, oracle, air):
    """log_n 19 at rate_bits 3: a 2^22-point coset, the first shape that uses the third level of the root table (root_pow_f,
    log_s > 21).  The GPU's quotient values are checked at a few thousand points against a per-point big-integer evaluation."""
    log_n, r = 19, 3
    N = 1 << (log_n + r)
    trace, pub = air.trace(log_n)
    src, lde = ctx.from_host(trace), ctx.alloc(N * air.COLS)
    ctx.lde(src, log_n, air.COLS, r, lde)
    alphas = [0x123456789ABCDEF % P, 0xFEDCBA987654321 % P]
    got = ctx.quotient_eval(air.ID, r, lde, log_n, alphas, pub)
    lde_h = lde.download().reshape(air.COLS, N)
    pub = [int(x) % P for x in pub]
    rng = np.random.default_rng(19)
    bad = [(i, k) for i in sample_points(rng, log_n + r, 2500) for k, v in enumerate(quotient_at(air, lde_h, i, log_n, r, pub, alphas)) if int(got[k, i]) != v]
    assert not bad, f"quotient values differ at (point, challenge) {bad[:8]}"


def test_rate_3_proof_of_2_19_rows(ctx, vx, oracle):
    """FibAir over 2^19 rows at the reference's outer config: a 2^22-point LDE, quotient and first FRI layer.  Both verifiers accept
    the proof and refuse it with one word flipped (in the quotient openings, mid-proof, near the end)."""
    log_n = 19
    over = dict(rate_bits=3, num_queries=28)
    cfg, pcfg = dict(S.DEFAULT_CFG, **over), ctx.stark_config(**over)
    trace, pub = S.FibAir.trace(log_n)
    proof = ctx.stark_prove(S.FibAir.ID, ctx.from_host(trace), log_n, pub, pcfg)
    S.verify(proof, cfg, expect_air=S.FibAir.ID, expect_public=pub)
    vx.lib.stark_verify(proof, pcfg, expect_air=S.FibAir.ID, expect_public=pub)
    with pytest.raises(vx.VxError):
        vx.lib.stark_verify(proof, ctx.stark_config(num_queries=28))
    o_quot = 10 + int(proof[9]) + 2 + 3 + 2 * (4 << 4) + 4 * S.FibAir.COLS  # header, plan, publics, two caps, two opening sets
    for w in (o_quot + 3, len(proof) // 2, len(proof) - 7):
        bad = proof.copy()
        bad[w] ^= np.uint64(1)
        with pytest.raises(S.VerifyError):
            S.verify(bad, cfg)
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(bad, pcfg)


def test_lookup_air_broken_multiplicity_is_rejected(ctx, vx, oracle):
    """The auxiliary (logUp) round on the GPU: a wrong multiplicity or a tuple outside the table gives a proof that
    BOTH verifiers reject."""
    A = S.LookupAir
    tr, pub = A.trace(10)
    cfg, pcfg = dict(S.DEFAULT_CFG, num_queries=9), ctx.stark_config(num_queries=9)
    good = ctx.stark_prove(A.ID, ctx.from_host(tr), 10, pub, pcfg)
    S.verify(good, cfg, expect_air=A.ID)
    vx.lib.stark_verify(good, pcfg, expect_air=A.ID)
    for col, row in ((6, 5), (5, 700)):
        bad = tr.copy()
        bad[col, row] = bad[col, row] ^ np.uint64(1)
        pr = ctx.stark_prove(A.ID, ctx.from_host(bad), 10, pub, pcfg)
        with pytest.raises(S.VerifyError):
            S.verify(pr, cfg)
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(pr, pcfg)
    # tampering with the auxiliary cap or an auxiliary opening is caught too
    for w in (14 + 16 * 4 + 3, 14 + 2 * 16 * 4 + 2 * 9):
        bad = good.copy()
        bad[w] ^= np.uint64(1)
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(bad, pcfg)
