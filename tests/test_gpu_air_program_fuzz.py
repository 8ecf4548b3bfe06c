"""Generated constraint programs on the GPU interpreter (k_quotient_prog), bit-exact against the reference reading
(oracle/air_program.py run by oracle/stark_ref.py): raw programs over the whole 32-register file on arbitrary, edge-valued data
(vx_quotient_eval needs no witness), whole proofs of random satisfiable programs, and hand-assembled aliasing snippets.  The
generators and the case lists are tests/air_program_fuzz.py; tests/test_air_program_fuzz.py asserts what the cases cover."""
import numpy as np
import pytest

import air_program_fuzz as F
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = 2**64 - 2**32 + 1
pytestmark = pytest.mark.gpu


def assert_same_quotients(got, want, r, what):
    bad = np.argwhere(got != want)
    if bad.size:
        k, i = (int(v) for v in bad[0])
        pytest.fail("%s: %d of %d quotient values differ; first at (challenge %d, point %d): got %#018x want %#018x, point mod 2^rate_bits = %d"
                    % (what, len(bad), got.size, k, i, int(got[k, i]), int(want[k, i]), i % (1 << r)))


def compare_program(ctx, vx, variants, cols, n_public, consts, periodic, public, log_n, rates, alphas_list, lde_of, what):
    """Registers every variant (at most two: a program and its relabelling), evaluates each at every rate_bits and challenge
    pair on the same context -- the second rate meets a warm code cache and a new periodic table -- and compares with the
    reference reading of the FIRST variant."""
    ids = [vx.lib.air_register(cols, n_public, code, consts, periodic, n_regs) for code, n_regs in variants]
    assert len(ids) <= 3
    try:
        ref_air = ProgramAir(ids[0], cols, n_public, variants[0][0], consts, periodic)
        for r in rates:
            lde = lde_of(r)
            buf = ctx.from_host(lde)
            for alphas in alphas_list:
                want = S.quotient_values(ref_air, lde, public, alphas, log_n, r)
                assert want.any()
                for air_id, (_, n_regs) in zip(ids, variants):
                    got = ctx.quotient_eval(air_id, r, buf, log_n, alphas, public)
                    assert_same_quotients(got, want, r, "%s, rate_bits %d, n_regs %d, alphas %s" % (what, r, n_regs, [hex(a) for a in alphas]))
            buf.free()
    finally:
        for air_id in ids:
            vx.lib.air_unregister(air_id)


@pytest.mark.parametrize("case", F.RAW_CASES, ids=F.RAW_IDS)
def test_quotient_values_of_raw_programs_on_arbitrary_data(ctx, vx, oracle, case):
    c = F.RawCase(case)
    compare_program(ctx, vx, c.variants, c.cols, c.n_public, c.consts, c.periodic, c.public, c.log_n, (c.rate_bits, F.other_rate(c.rate_bits)),
                    c.alphas, c.lde, "raw program seed %d" % c.seed)


@pytest.mark.parametrize("name,code,consts,n_regs", F.SNIPPETS, ids=[s[0] for s in F.SNIPPETS])
def test_hand_assembled_aliasing_snippets(ctx, vx, oracle, name, code, consts, n_regs):
    rng = np.random.default_rng(len(name))
    alphas = [[P - 1, 2**32], [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)]]
    seed = int(rng.integers(0, 2**31))
    compare_program(ctx, vx, [(np.array(code, dtype=np.uint64), n_regs)], 2, 0, consts, [], [], 4, (1, 3), alphas,
                    lambda r: F.special_lde(np.random.default_rng([seed, r]), 2, 1 << (4 + r)), "snippet " + name)


def proof_cfgs(seed):
    cfgs = [{}]
    if seed in F.RATE_SEEDS:
        cfgs += [dict(rate_bits=2, num_queries=4), dict(rate_bits=3, num_queries=4)]
    return cfgs


@pytest.mark.parametrize("seed,log_n", F.RECURRENCE_CASES)
def test_proofs_of_random_satisfiable_programs(ctx, vx, oracle, seed, log_n):
    c = F.RecurrenceCase(vx.air_program, seed, log_n)
    air_id = vx.lib.air_register(c.cols, c.n_public, c.code, c.consts, c.periodic, 32)
    air = ProgramAir(air_id, c.cols, c.n_public, c.code, c.consts, c.periodic)
    S.register_air(air)
    try:
        assert S.check_trace(air, c.trace, c.public) is None
        buf = ctx.from_host(c.trace)
        for over in proof_cfgs(seed):
            got = ctx.stark_prove(air_id, buf, log_n, c.public, ctx.stark_config(**over))
            want = S.prove(air, c.trace, c.public, dict(S.DEFAULT_CFG, **over))
            assert got.size == want.size, (seed, over)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "seed %d %s: proofs differ from word %d on: got %#x want %#x" % (seed, over, bad[0], int(got[bad[0]]), int(want[bad[0]]))
            vx.lib.stark_verify(got, vx.lib.default_stark_config(**over), expect_air=air_id, expect_public=c.public)
            S.verify(got, dict(S.DEFAULT_CFG, **over), expect_air=air_id, expect_public=c.public)
        # one trace cell changed in the middle row: the prover still emits a proof, nobody accepts it
        n = 1 << log_n
        broken = c.trace.copy()
        broken[seed % c.cols, n // 2] = (int(broken[seed % c.cols, n // 2]) + 1) % P
        assert S.check_trace(air, broken, c.public) is not None
        bad_proof = ctx.stark_prove(air_id, ctx.from_host(broken), log_n, c.public)
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(bad_proof, expect_air=air_id, expect_public=c.public)
        with pytest.raises(S.VerifyError):
            S.verify(bad_proof, expect_air=air_id, expect_public=c.public)
    finally:
        vx.lib.air_unregister(air_id)
        S.AIRS.pop(air_id, None)
