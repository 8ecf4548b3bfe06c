"""Declared bus messages of a run-time AIR (include/vx.h vx_air_register_bus) without a GPU: what registration refuses, that the
constraints the library derives from a declaration are the ones the hand-written restatements state (the host verifier accepts the
reference prover's proof of the hand-written program under the id of the declared one), and the builder's message programs."""
import numpy as np
import pytest

import bus_programs as BP
import leaf_noop_ref as N
import transcript_ref as T
from oracle import stark_ref as S

P = BP.P
CFG = dict(S.DEFAULT_CFG, num_queries=8)


def I(op, d=0, a=0, b=0):
    return op | (d << 8) | (a << 16) | (b << 32)


LOC, NXT, PER, PUB, CONST, ADD, SUB, MUL, ASSERT, CHAL, APUB, SLOT, MSG = 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 64, 65
OWN = [I(LOC, 0, 0), I(ASSERT, 0, 0)]                                    # the program's own constraint: column 0 is zero
ONE = [I(LOC, 0, 0), I(SLOT, 0, 0), I(LOC, 1, 1), I(MSG, 0, 1, 3)]      # one message (column 0; tag 3) with multiplicity column 1
FIRST32 = [[1] + [0] * 31]


def register(vx, bus_code=ONE, **kw):
    args = dict(cols=2, n_public=1, code=OWN, bus_code=bus_code)
    args.update(kw)
    return vx.lib.air_register_bus(**args)


REFUSALS = {
    "callback_with_a_bus": (dict(gen_aux=lambda *a: [0, 0]), "gen_aux callback given together with a bus"),
    "aux_cols_disagree": (dict(aux_cols=6), "need aux_cols 4"),
    "n_challenges_disagree": (dict(n_challenges=2), "n_challenges 4"),
    "n_aux_public_disagree": (dict(n_aux_public=2), "n_aux_public 1"),
    "nxt": (dict(bus_code=[I(NXT, 0, 0)] + ONE), "NXT is not allowed"),
    "chal": (dict(bus_code=[I(CHAL, 0, 0)] + ONE), "CHAL is not allowed"),
    "apub": (dict(bus_code=[I(APUB, 0, 0)] + ONE), "APUB is not allowed"),
    "assert": (dict(bus_code=ONE + [I(ASSERT, 0, 0)]), "an assert is not allowed"),
    "assert_first": (dict(bus_code=ONE + [I(11, 0, 0)]), "an assert is not allowed"),
    "unknown_op_15": (dict(bus_code=[I(15, 0, 0)] + ONE), "unknown opcode 15"),
    "unknown_op_66": (dict(bus_code=ONE + [I(66, 0, 0)]), "unknown opcode 66"),
    "loc_of_an_auxiliary_column": (dict(bus_code=[I(LOC, 0, 2)] + ONE), "LOC of an auxiliary column"),
    "slot_index_4": (dict(bus_code=[I(LOC, 0, 0), I(SLOT, 4, 0), I(MSG, 0, 0, 3)]), "slot index 4 above 3"),
    "slot_without_msg": (dict(bus_code=ONE + [I(SLOT, 1, 0)], aux_cols=4), "SLOT not followed by a MSG"),
    "no_message": (dict(bus_code=[I(LOC, 0, 0)], aux_cols=4), "no message"),
    "too_many_helpers": (dict(bus_code=ONE * 39), "more than 19 helpers"),
    "non_canonical_constant": (dict(bus_code=[I(CONST, 0, 0)] + ONE, bus_consts=[P]), "non-canonical constant"),
    "read_before_written": (dict(bus_code=[I(ADD, 0, 0, 1)] + ONE), "never written"),
    "msg_reads_unwritten": (dict(bus_code=[I(MSG, 0, 0, 3)]), "never written"),
    "slot_reads_unwritten": (dict(bus_code=[I(SLOT, 0, 5)] + ONE, bus_n_regs=8), "never written"),
    "too_many_registers": (dict(bus_n_regs=13), "13 registers"),
    "reserved_bits": (dict(bus_code=[1 << 48 | I(LOC, 0, 0)] + ONE), "reserved bits"),
    "step_column_without_blocks": (dict(step_periodic=0, periodic=FIRST32), "wrong step column"),
    "step_column_missing": (dict(block_log=5), "wrong step column"),
    "step_column_out_of_range": (dict(block_log=5, step_periodic=1, periodic=FIRST32), "wrong step column"),
    "step_column_of_period_4": (dict(block_log=5, step_periodic=0, periodic=[[1, 0, 0, 0]]), "wrong step column"),
    "step_column_not_first_row": (dict(block_log=5, step_periodic=1, periodic=FIRST32 + [[0, 1] + [0] * 30]), "wrong step column"),
    "step_column_two_ones": (dict(block_log=5, step_periodic=0, periodic=[[1] + [0] * 30 + [1]]), "wrong step column"),
    "block_log_3": (dict(block_log=3, step_periodic=0, periodic=[[1] + [0] * 7]), "block_log 3 is not supported"),
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_registration_refuses(vx, kind):
    kw, why = REFUSALS[kind]
    with pytest.raises(vx.VxError, match=why) as e:
        register(vx, **kw)
    assert e.value.code == -1  # VX_ERR_ARG


def test_a_program_with_messages_registers_and_unregisters(vx):
    ids = [register(vx), register(vx, bus_code=ONE * 3), register(vx, bus_code=ONE * 38),
           register(vx, block_log=5, step_periodic=1, periodic=[[0, 1] + [0] * 30] + FIRST32)]
    assert all(i >= 4096 for i in ids) and len(set(ids)) == 4
    for i in ids:
        vx.lib.air_unregister(i)
    with pytest.raises(vx.VxError):
        vx.lib.air_unregister(ids[0])
    # the opcode space of a CONSTRAINT program is what it was: 15 and the two bus opcodes are refused there
    for op in (15, SLOT, MSG):
        with pytest.raises(vx.VxError, match="unknown opcode"):
            vx.lib.air_register(1, 0, [I(LOC, 0, 0), I(op, 0, 0), I(ASSERT, 0, 0)])
    # a multiplicity of degree 4 makes the derived helper constraint degree 4: the degree check of vx_air_register covers the lowered code
    with pytest.raises(vx.VxError, match="degree"):
        register(vx, bus_code=[I(LOC, 0, 0), I(SLOT, 0, 0), I(LOC, 1, 1), I(MUL, 1, 1, 1), I(MUL, 1, 1, 1), I(MSG, 0, 1, 3)])


def _leaf_noop_case():
    trees, index = [8, 10, 10, 9, 8, 10, 8], [5, 5, 300, 0, 5, (1 << 40) - 1, 77]
    rows = [[3, P - 1], [1, 2, 3, 4], [P - 2, 0, 7, 9], [6], [3, P - 1], [11, 12, 13], [0, 0]]
    trace, pub = N.ref_trace(trees, index, rows)
    return N, BP.leaf_noop, trace, pub


def _transcript_case():
    trace, pub, _ = T.ref_table(T.synth_chains(["one_block"]))
    return T, BP.transcript, trace, pub


@pytest.mark.parametrize("case", [_leaf_noop_case, _transcript_case], ids=["leaf_noop", "transcript"])
def test_the_derived_constraints_accept_a_reference_proof_of_the_hand_written_ones(vx, oracle, case):
    """The reference prover proves the restatement whose bus block is written out by hand; the product's host verifier checks that
    proof against the program whose bus block the LIBRARY derived from the declared messages.  A table alone has nobody to cancel its
    total against, so the last check of a stand-alone verification refuses it -- after the constraint identity, the proof of work and
    the whole query phase have passed (tests/test_leaf_noop.py reads the compiled AIR's verdict the same way); with one helper word
    of the proof changed the identity itself fails."""
    R, declared, trace, pub = case()
    proof = np.array(S.prove(R.air(), trace, pub, CFG), dtype=np.uint64)
    b = declared()
    air_id = b.register()
    try:
        assert (b.aux_cols, b.n_challenges, b.n_aux_public) == (R.AUX, 4, 1)
        proof[1] = air_id
        cfg = vx.lib.default_stark_config(num_queries=CFG["num_queries"])
        with pytest.raises(vx.VxError, match="stand-alone proof publishes a non-zero bus total"):
            vx.lib.stark_verify(proof, cfg, expect_air=air_id, expect_public=pub)
        cap_words = 4 << CFG["cap_height"]
        o_local = 12 + int(proof[9]) + R.PUB + cap_words + 2 + cap_words + cap_words  # header, public inputs, cap, total, two caps
        for col in (R.COLS, R.COLS + 2 * R.N_HELP - 1):  # the first word of the first helper, the last word of the last one
            bad = proof.copy()
            bad[o_local + 2 * col] ^= 1
            with pytest.raises(vx.VxError, match="constraint identity fails at zeta"):
                vx.lib.stark_verify(bad, cfg, expect_air=air_id)
    finally:
        vx.lib.air_unregister(air_id)


def test_an_idle_table_is_accepted_outright(vx, oracle):
    """no message at all: the total is zero and the stand-alone verifier returns success"""
    trace = np.zeros((N.COLS, 32), dtype=np.uint64)
    pub = [1, 2, 3, 4]
    proof = np.array(S.prove(N.air(), trace, pub, CFG), dtype=np.uint64)
    air_id = BP.leaf_noop().register()
    try:
        proof[1] = air_id
        vx.lib.stark_verify(proof, vx.lib.default_stark_config(num_queries=CFG["num_queries"]), expect_air=air_id, expect_public=pub)
    finally:
        vx.lib.air_unregister(air_id)


def interpret(code, consts, row, pub):
    """a message program read independently of the library: -> [(tag, [t0..t3 or None], m)]"""
    r, slots, out = {}, [None] * 4, []
    for w in (int(x) for x in code):
        op, d, a, b = w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFFFF, (w >> 32) & 0xFFFF
        if op == LOC:
            r[d] = int(row[a])
        elif op == PUB:
            r[d] = int(pub[a])
        elif op == CONST:
            r[d] = int(consts[a])
        elif op == ADD:
            r[d] = (r[a] + r[b]) % P
        elif op == SUB:
            r[d] = (r[a] - r[b]) % P
        elif op == MUL:
            r[d] = r[a] * r[b] % P
        elif op == SLOT:
            assert slots[d] is None
            slots[d] = r[a]
        elif op == MSG:
            assert d == 0
            out.append((b, slots, r[a]))
            slots = [None] * 4
        else:
            raise AssertionError("opcode %d in a message program" % op)
    assert slots == [None] * 4
    return out


def test_the_builder_writes_the_declared_messages(vx):
    b = BP.made_up()
    code, consts, n_regs = b.assemble_bus()
    assert 1 <= n_regs <= vx.lib.VX_BUSP_MAX_REGS == vx.air_program.BUS_MAX_REGS
    assert [int(w) & 0xFF for w in code].count(MSG) == 3 and [int(w) & 0xFF for w in code].count(SLOT) == 2 + 2 + 3
    tr, pub = BP.made_up_trace(4), [P - 7]
    for i in range(tr.shape[1]):
        assert interpret(code, consts, tr[:, i], pub) == BP.made_up_messages(tr[:, i], pub), i
    # a receive is a send of 0 - m
    r = vx.air_program.AirBuilder(2, 0)
    r.receive(9, [r.loc(0)], r.loc(1))
    code, consts, _ = r.assemble_bus()
    assert interpret(code, consts, [5, 3], []) == [(9, [5, None, None, None], P - 3)]
    # a builder without messages registers as before; the constraint side of the allocator is unchanged by the declaration
    code0, consts0, regs0 = BP.made_up().assemble()
    plain = vx.air_program.AirBuilder(BP.MADE_UP_COLS, 1)
    plain.assert_zero(plain.const(0) * plain.loc(5))
    code1, consts1, regs1 = plain.assemble()
    assert code0.tolist() == code1.tolist() and consts0.tolist() == consts1.tolist() and regs0 == regs1
    air_id = plain.register()
    assert air_id >= 4096
    vx.lib.air_unregister(air_id)
    with pytest.raises(ValueError, match="registers"):
        big = vx.air_program.AirBuilder(40, 0)
        deep = big.loc(0)
        for j in range(1, 20):  # a right-leaning chain keeps every left operand alive
            deep = big.loc(j) * (big.loc(20 + j) + deep)
        big.send(1, [big.loc(0)], deep)
        big.assemble_bus()
