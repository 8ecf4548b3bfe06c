"""Generated constraint programs, CPU tier (no GPU): the generators of tests/air_program_fuzz.py really cover the corners of the
format they were written for -- asserted per seed, so that an edit of a generator cannot quietly thin what the GPU tier runs --
and the product's HOST interpreter (air_program_eval inside vx_stark_verify, at zeta in the extension field) agrees with the
reference reading (oracle/air_program.py) on random satisfiable programs relabelled onto register 31."""
import numpy as np
import pytest

import air_program_fuzz as F
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = 2**64 - 2**32 + 1


@pytest.fixture(scope="module")
def raw_cases():
    return [F.RawCase(c) for c in F.RAW_CASES]


@pytest.mark.parametrize("k", range(len(F.RAW_CASES)), ids=F.RAW_IDS)
def test_raw_programs_register_and_cover_the_format(vx, raw_cases, k):
    case = raw_cases[k]
    assert len(case.code) == case.n_code and case.n_constraints >= 4
    assert len(case.variants) == (2 if case.n_regs < 32 else 1)
    for code, n_regs in case.variants:
        air_id = vx.lib.air_register(case.cols, case.n_public, code, case.consts, case.periodic, n_regs)
        vx.lib.air_unregister(air_id)
        cov = F.coverage(code)
        want = {F.LOC, F.NXT, F.CONST, F.ADD, F.SUB, F.MUL} | set(F.ASSERTS) | ({F.PER} if case.period_logs else set()) | ({F.PUB} if case.n_public else set())
        assert cov["ops"] == want, (case.seed, sorted(want - cov["ops"]))
        assert cov["d_eq_a"] and cov["a_eq_b"] and cov["in_place"] and cov["square"] and cov["asserted_twice"], (case.seed, cov)
        assert max(F.registers_written(code)) == n_regs - 1, case.seed  # the whole register file that is asked for is used
    # the last variant of every case asks for all 32 registers (65,536 bytes of LDS on the GPU) and writes register 31
    code, n_regs = case.variants[-1]
    assert n_regs == 32 and F.coverage(code)["reg31"], case.seed
    # the data: the column loads reach the last column, the public loads the last public input
    loads = {(op, a) for op, _, a, _ in map(F.decode, case.code)}
    assert (F.LOC, case.cols - 1) in loads and (not case.n_public or (F.PUB, case.n_public - 1) in loads), case.seed
    assert {a for op, a in loads if op == F.PER} == set(range(len(case.period_logs))), case.seed
    assert set(F.EDGES) <= {int(c) for c in case.consts}


@pytest.mark.parametrize("k", range(len(F.RAW_CASES)), ids=F.RAW_IDS)
def test_raw_program_quotients_are_not_vacuous(oracle, raw_cases, k):
    """The reference's quotient values of every case (on the data the GPU tier uses) are non-zero somewhere and depend on which
    challenge is which; a relabelled program has the values of the original."""
    case = raw_cases[k]
    r = case.rate_bits
    lde = case.lde(r)
    assert lde.shape == (case.cols, 1 << (case.log_n + r)) and (lde < np.uint64(P)).all()
    assert (lde[:, 0] == np.uint64(P - 1)).all() and (lde[:, 1] == 0).all()
    alphas = case.alphas[1]
    vals = [S.quotient_values(ProgramAir(0, case.cols, case.n_public, code, case.consts, case.periodic), lde, case.public, alphas, case.log_n, r)
            for code, _ in case.variants]
    assert vals[0].any() and (vals[0] < np.uint64(P)).all()
    assert all((v == vals[0]).all() for v in vals[1:])
    swapped = S.quotient_values(ProgramAir(0, case.cols, case.n_public, case.code, case.consts, case.periodic), lde, case.public, alphas[::-1], case.log_n, r)
    assert (swapped[::-1] == vals[0]).all() and (swapped != vals[0]).any()


def test_relabel_is_a_renaming():
    code = np.array([F.insn(F.LOC, 3, 7), F.insn(F.PUB, 4, 2), F.insn(F.SUB, 3, 3, 4), F.insn(F.ASSERT_FIRST, 0, 3)], dtype=np.uint64)
    perm = list(range(32))
    perm[3], perm[4], perm[31], perm[30] = 31, 30, 3, 4
    got = F.relabel(code, perm)
    assert list(got) == [F.insn(F.LOC, 31, 7), F.insn(F.PUB, 30, 2), F.insn(F.SUB, 31, 31, 30), F.insn(F.ASSERT_FIRST, 0, 31)]
    inv = [perm.index(i) for i in range(32)]
    assert (F.relabel(got, inv) == code).all()


def test_recurrence_airs_span_the_shapes(vx):
    """Over the seed list: every column count 1..6, every number of periodic columns 0..3, all three kinds of the
    degree-3 constraint, a period-1 column and a period-n column."""
    cases = [F.RecurrenceCase(vx.air_program, seed, log_n) for seed, log_n in F.RECURRENCE_CASES]
    assert len(cases) == 12 and {c.log_n for c in cases} == {3, 4, 5, 6} and set(F.RATE_SEEDS) <= {c.seed for c in cases}
    assert {c.cols for c in cases} == {1, 2, 3, 4, 5, 6} and {len(c.periodic) for c in cases} == {0, 1, 2, 3}
    assert {c.builder.cubic_kind for c in cases} == {"selector", "fed", "alternate"}
    logs = {(len(col).bit_length() - 1, c.log_n) for c in cases for col in c.periodic}
    assert any(pl == 0 for pl, _ in logs) and any(pl == L for pl, L in logs)
    for c in cases:
        assert 31 in F.registers_written(c.code) and len(c.public) == 2 * c.cols
        assert [int(v) for v in c.trace[:, -1]] == c.public[c.cols:]


def verify_cfgs(seed):
    cfgs = [dict(S.DEFAULT_CFG, num_queries=4)]
    if seed in F.RATE_SEEDS[:2]:
        cfgs.append(dict(S.DEFAULT_CFG, num_queries=4, rate_bits=3))
    return cfgs


@pytest.mark.parametrize("seed,log_n", F.RECURRENCE_CASES)
def test_host_interpreter_on_random_satisfiable_programs(vx, oracle, seed, log_n):
    c = F.RecurrenceCase(vx.air_program, seed, log_n)
    air_id = vx.lib.air_register(c.cols, c.n_public, c.code, c.consts, c.periodic, 32)
    twin_id = vx.lib.air_register(c.cols, c.n_public, c.twin_code, c.twin_consts, c.periodic, 32)
    try:
        air = ProgramAir(air_id, c.cols, c.n_public, c.code, c.consts, c.periodic)
        assert S.check_trace(air, c.trace, c.public) is None
        # the twin's recurrence is another one: the same trace breaks its first transition constraint
        assert S.check_trace(ProgramAir(twin_id, c.cols, c.n_public, c.twin_code, c.twin_consts, c.periodic), c.trace, c.public) is not None
        for cfg in verify_cfgs(seed):
            proof = S.prove(air, c.trace, c.public, cfg)
            pcfg = vx.lib.default_stark_config(**cfg)
            vx.lib.stark_verify(proof, pcfg, expect_air=air_id, expect_public=c.public)
            # one public input changed: as the verifier's expectation, and inside the proof
            j = seed % len(c.public)
            wrong = c.public[:j] + [(c.public[j] + 1) % P] + c.public[j + 1:]
            with pytest.raises(vx.VxError):
                vx.lib.stark_verify(proof, pcfg, expect_air=air_id, expect_public=wrong)
            pub_at = 10 + int(proof[9]) + 2
            assert [int(v) for v in proof[pub_at:pub_at + len(c.public)]] == c.public
            bad = proof.copy()
            bad[pub_at + j] = wrong[j]
            with pytest.raises(vx.VxError):
                vx.lib.stark_verify(bad, pcfg, expect_air=air_id)
            # one word flipped
            for w in (pub_at + len(c.public) + 1, len(proof) // 2, len(proof) - 4):
                bad = proof.copy()
                bad[w] ^= np.uint64(1)
                with pytest.raises(vx.VxError):
                    vx.lib.stark_verify(bad, pcfg, expect_air=air_id)
            # the same bytes under the twin program (E_0 + 1): the openings do not satisfy ITS constraints at zeta
            forged = proof.copy()
            forged[1] = twin_id
            with pytest.raises(vx.VxError, match="constraint identity"):
                vx.lib.stark_verify(forged, pcfg, expect_air=twin_id)
    finally:
        vx.lib.air_unregister(air_id)
        vx.lib.air_unregister(twin_id)
