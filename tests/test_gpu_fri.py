"""GPU parity for K6: evaluation-space folding equals the reference's coefficient fold + coset FFT."""
import numpy as np
import pytest

from conftest import P, rand_field
from test_gpu_ntt import bitrev_perm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("log_n,arity_bits", [(3, 1), (6, 2), (8, 3), (10, 4), (12, 5), (15, 4), (5, 5)])
def test_fold_matches_coefficient_fold(ctx, oracle, rng, log_n, arity_bits):
    n, shift = 1 << log_n, 7
    coeffs = rand_field(rng, 2 * n)
    beta = rand_field(rng, 2)
    evals = oracle.ext_coset_ntt(coeffs, shift)
    want = oracle.ext_coset_ntt(oracle.fri_fold_coeffs(coeffs, arity_bits, beta), pow(shift, 1 << arity_bits, P))
    out = ctx.alloc(2 * (n >> arity_bits))
    ctx.fri_fold(ctx.from_host(evals), log_n, arity_bits, beta, shift, out)
    assert (out.download() == want).all()


def test_two_layer_reduction_like_the_prover(ctx, oracle, rng):
    """fri_committed_trees with arity bits (4, 3): caps and folded values per layer."""
    log_n, cap_h = 11, 2
    n = 1 << log_n
    coeffs = rand_field(rng, 2 * n)
    coeffs[2 * (n // 8):] = 0  # rate 1/8, as after an LDE
    shift, cur_c, cur_log = 7, coeffs, log_n
    d = ctx.from_host(oracle.ext_coset_ntt(coeffs, shift))
    for arity_bits in (4, 3):
        arity = 1 << arity_bits
        vals = oracle.ext_coset_ntt(cur_c, shift).reshape(-1, 2)
        rev = vals[bitrev_perm(cur_log)]
        want = oracle.MerkleTree(rev.reshape(-1, 2 * arity), cap_h)
        t = ctx.fri_layer_tree(d, cur_log, arity_bits, cap_h)
        assert (t.cap() == want.cap).all()
        q = np.array([0, 3, (1 << (cur_log - arity_bits)) - 1], dtype=np.uint64)
        leaves = ctx.fri_leaves(d, cur_log, arity_bits, q)
        assert (leaves == rev.reshape(-1, 2 * arity)[q.astype(np.int64)]).all()
        for k, i in enumerate(q):
            assert oracle.merkle_verify(leaves[k], int(i), t.open(q)[k], want.cap)
        beta = rand_field(rng, 2)
        nxt = ctx.alloc(2 << (cur_log - arity_bits))
        ctx.fri_fold(d, cur_log, arity_bits, beta, shift, nxt)
        cur_c = oracle.fri_fold_coeffs(cur_c, arity_bits, beta)
        shift = pow(shift, arity, P)
        cur_log -= arity_bits
        assert (nxt.download() == oracle.ext_coset_ntt(cur_c, shift)).all()
        d = nxt
        t.free()
    # final polynomial: degree < n/8/128 -> high coefficients vanish
    assert (cur_c.reshape(-1, 2)[(n // 8) >> 7:] == 0).all()


@pytest.mark.parametrize("bits,pos", [(0, 0), (8, 3), (16, 5)])
def test_pow_smallest_nonce(ctx, oracle, rng, bits, pos):
    st = rand_field(rng, 12)
    nonce = ctx.fri_pow(st, pos, bits)
    assert nonce == oracle.fri_pow(st, pos, bits)


def fold_at(vals, i, log_n, arity_bits, beta, shift):
    """Output i of an arity-2^a fold, from the definition in python integers over F_p[X]/(X^2 - 7): a binary folds
        P'(x^2) = (P(x) + P(-x))/2 + beta (P(x) - P(-x))/(2x)
    with beta, beta^2, beta^4, ...; at step j the points are x = shift^(2^j) w^(i + k M) of the size-2^(log_n - j) domain and -x sits
    half a domain further on."""
    from oracle.stark_ref import ExtS

    M = 1 << (log_n - arity_bits)
    v = [ExtS(int(vals[2 * (i + k * M)]), int(vals[2 * (i + k * M) + 1])) for k in range(1 << arity_bits)]
    b, sh, half = ExtS(int(beta[0]), int(beta[1])), shift, pow(2, P - 2, P)
    for j in range(arity_bits):
        cnt = len(v) // 2
        w = root(log_n - j)
        nv = []
        for k in range(cnt):
            x = sh * pow(w, i + k * M, P) % P
            u, t = v[k], v[k + cnt]
            nv.append((u + t) * half + b * (u - t) * pow(2 * x % P, P - 2, P))
        v, b, sh = nv, b * b, sh * sh % P
    return v[0]


def root(log_n):
    """w_(2^log_n) = 7^((p - 1) / 2^log_n), computed here rather than taken from any table."""
    return pow(7, (P - 1) >> log_n, P)


@pytest.mark.parametrize("log_n", [22, 23])
def test_fold_at_2_22_and_2_23_points(ctx, oracle, rng, log_n):
    """Layers of 2^22 and 2^23 points (a 2^19- / 2^20-row trace at rate_bits 3): the fold's 1/(2x) takes the third level of the
    inverse root table (root_pow_inv, log_s > 21).  Arities 2 to 16, compared with the definition at sampled outputs: 0, the last,
    every index whose low bits are all ones, and random ones."""
    n, shift = 1 << log_n, 7
    vals = rand_field(rng, 2 * n)
    d = ctx.from_host(vals)
    for a in (1, 2, 3, 4):
        M = n >> a
        beta = rand_field(rng, 2)
        out = ctx.alloc(2 * M)
        ctx.fri_fold(d, log_n, a, beta, shift, out)
        got = out.download().reshape(M, 2)
        out.free()
        pts = {0, M - 1} | {(1 << b) - 1 for b in range(1, log_n - a + 1)} | {int(v) for v in rng.integers(0, M, size=2000)}
        bad = []
        for i in sorted(pts):
            e = fold_at(vals, i, log_n, a, beta, shift)
            if (int(got[i, 0]), int(got[i, 1])) != (e.a, e.b):
                bad.append(i)
        assert not bad, f"arity 2^{a}: folded values differ at {bad[:8]}"
