"""FriExitAir (air_library.fri_exit_builder(), a shipped constraint program with declared bus messages) and the exit group of an inner
proof -- FriFoldAir, TranscriptAir and FriExitAir on one bus -- without a GPU: the degree of the independent restatement
(tests/fri_exit_ref.py), the layout header against the builder, the constraints the library derives from the declaration against the
hand-written ones, edge values, forged witnesses proven by the reference prover and judged by the product verifier, reference groups
through lib.fri_exits_verify with the outside party's sum in Python, refusals through the group, the public inputs.  Everything is
exact."""
import os
import re

import numpy as np
import pytest

import fri_exit_ref as E
import fri_fold_ref as F
import test_bus_group as BG
from oracle import stark_ref as S

P = E.P
CFG = dict(S.DEFAULT_CFG, num_queries=8)
LN, NL, POW_BITS, ORD_POW, ABSORBED = (E.HAND[k] for k in ("LN", "NL", "pow_bits", "ord_pow", "absorbed"))
INDEX_VALUES, GROUP_SHAPES, final_poly = E.INDEX_VALUES, E.GROUP_SHAPES, E.final_poly
ERR_ARG, ERR_STATEMENT = -1, -5
BUS_TOTAL, IDENTITY = "stand-alone proof publishes a non-zero bus total", "constraint identity fails at zeta"


def product_verdict(vx, proof, pub):
    """what the product's stand-alone verifier says of a reference-prover proof under the SHIPPED program (the constraints the
    library derived): a table alone has nobody to cancel its total against, so BUS_TOTAL is the verdict of a proof whose constraint
    identity, proof of work and query phase have all passed"""
    p = np.array(proof, dtype=np.uint64)
    p[1] = vx.lib.fri_exit_air_id()
    with pytest.raises(vx.VxError) as e:
        vx.lib.stark_verify(p, vx.lib.default_stark_config(num_queries=CFG["num_queries"]), expect_air=vx.lib.fri_exit_air_id(), expect_public=pub)
    assert e.value.code == ERR_STATEMENT
    return str(e.value)


def pcfg(vx, cfg):
    cfg = dict(S.DEFAULT_CFG, **cfg)
    return vx.lib.default_stark_config(**{k: cfg[k] for k in ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")})


def test_every_constraint_has_degree_at_most_3(vx):
    b = E.builder()
    degs = [E.degree(e) for _, e in b.constraints]
    assert max(degs) == 3 and len(degs) == 48
    assert all(E.degree(e) <= 2 for kind, e in b.constraints if kind != "assert_zero")  # vx.h: the three other kinds carry degree 2
    d = vx.air_library.fri_exit_builder()
    assert max(E.degree(e) for _, e in d.constraints) == 3 and len(d.constraints) == 48 - 2 * E.N_HELP - 2
    for _, slots, mult in d.messages:  # vx.h: two messages to a helper -- a slot has degree at most 1, a multiplicity at most 2
        assert all(E.degree(s) <= 1 for s in slots if s is not None) and E.degree(mult) <= 2


def test_the_layout_header_and_the_builder_agree(vx):
    """csrc/fri_exit_layout.h states every index for C, air_library.py for the builder, tests/fri_exit_ref.py for the restatement"""
    A = vx.air_library
    text = open(os.path.join(os.path.dirname(os.path.abspath(A.__file__)), "csrc", "fri_exit_layout.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    header = {}
    for name, value in re.findall(r"\b(FRI_EXIT_[A-Z0-9_]+)\s*=\s*([^,\n}]+)", text):
        header[name] = eval(value, {}, dict(header))  # `1 << FRI_EXIT_BLOCK_LOG` names an earlier entry
    mine = {k: v for k, v in vars(A).items() if k.startswith("FRI_EXIT_")}
    assert len(mine) >= 45 and all(header[k] == v for k, v in mine.items())
    assert set(header) - set(mine) == {"FRI_EXIT_BLOCK_LOG", "FRI_EXIT_BITS", "FRI_EXIT_MAX_LAYERS"}
    b = A.fri_exit_builder()
    assert (b.cols, b.n_public, len(b.periodic), len(b.messages)) == (header["FRI_EXIT_COLS"], header["FRI_EXIT_PUB"], header["FRI_EXIT_PERIODIC"], 3)
    assert b.periodic == [[v % P for v in col] for col in E.periodic()] and all(len(col) == header["FRI_EXIT_BLOCK"] for col in b.periodic)
    assert [t for t, _, _ in b.messages] == [E.TAG_CHAL, E.TAG_FIN, E.TAG_FRI] == [A.TAG_CHAL, A.TAG_FIN, A.TAG_FRI] == [13, 14, 10]
    ref = dict(BIT=E.BIT, V=E.V, F=E.FL, C=E.C, EF=E.EF, C2=E.C2, G=E.G, EB=E.EB, W=E.W, X=E.X, IDX=E.IDX, T=E.TT, HF=E.HF, K=E.K, CA=E.CA, CB=E.CB, ACC=E.ACC, ACT=E.ACT, ISPOW=E.ISPOW,
               ORD=E.ORD, COLS=E.COLS, PUB=E.PUB, N_HELP=E.N_HELP, AUX_COLS=E.AUX, BLOCK=E.BLOCK, HORNER_ROW=E.HROW, MAX_FINAL_LEN=E.MAX_FINAL, PUB_DIGEST=E.PUB_DIGEST, PUB_W=E.PUB_W,
               PUB_G=E.PUB_G, PUB_FB=E.PUB_FB, PUB_SKIP=E.PUB_SKIP, PUB_ORD_POW=E.PUB_ORD_POW, PUB_ABSORBED=E.PUB_ABSORBED, PUB_POW_BITS=E.PUB_POW_BITS, PUB_FINAL_LEN=E.PUB_FINAL_LEN)
    assert all(header["FRI_EXIT_" + k] == v for k, v in ref.items())
    assert (vx.lib.FRI_EXIT_AIR_COLS, vx.lib.FRI_EXIT_AIR_AUX_COLS, vx.lib.FRI_EXIT_PUBLIC, vx.lib.FRI_EXIT_BLOCK, vx.lib.FRI_EXIT_MAX_FINAL_LEN) == (E.COLS, E.AUX, E.PUB, E.BLOCK, E.MAX_FINAL)
    assert not [k for k in vars(vx.lib) if k.startswith("VX_AIR") and "EXIT" in k]  # a shipped program, not a compiled AIR


def test_the_derived_constraints_accept_a_reference_proof_of_the_hand_written_ones(vx, oracle):
    """as tests/test_air_bus_program.py reads the other declared tables: alone on its bus the table publishes a total nobody
    cancels, which the stand-alone verifier says AFTER the constraint identity has passed; one helper word changed and it fails"""
    trace, pub = E.ref_trace([5, 0x1A3, P - 1], LN, NL, POW_BITS, ORD_POW, ABSORBED, final_poly(16))
    proof = np.array(S.prove(E.air(), trace, pub, CFG), dtype=np.uint64)
    b = vx.air_library.fri_exit_builder()
    air_id = b.register()
    try:
        assert (b.aux_cols, b.n_challenges, b.n_aux_public) == (E.AUX, 4, 1)
        proof[1] = air_id
        cfg = vx.lib.default_stark_config(num_queries=CFG["num_queries"])
        with pytest.raises(vx.VxError, match=BUS_TOTAL):
            vx.lib.stark_verify(proof, cfg, expect_air=air_id, expect_public=pub)
        cap_words = 4 << CFG["cap_height"]
        o_local = 12 + int(proof[9]) + E.PUB + cap_words + 2 + cap_words + cap_words
        for col in (E.COLS, E.COLS + 2 * E.N_HELP - 1):
            bad = proof.copy()
            bad[o_local + 2 * col] ^= 1
            with pytest.raises(vx.VxError, match=IDENTITY):
                vx.lib.stark_verify(bad, cfg, expect_air=air_id)
    finally:
        vx.lib.air_unregister(air_id)


@pytest.mark.parametrize("case", list(E.EDGES))
def test_edge_values_satisfy_every_constraint(vx, oracle, case):
    """... of the restatement row by row, and of the shipped program: the product verifier passes the constraint identity of a
    reference proof of the trace and stops at the total a table alone cannot cancel"""
    pow_bits, response = E.EDGES[case]
    fp = final_poly(16)
    trace, pub = E.ref_trace([response] + INDEX_VALUES, LN, NL, pow_bits, ORD_POW, ABSORBED, fp)
    assert trace.shape == (E.COLS, 2048) and E.check(trace, pub) is None
    assert BUS_TOTAL in product_verdict(vx, E.prove_alone(trace, pub, CFG), pub)
    for q, v in enumerate(INDEX_VALUES):  # what the block hands to the bus is what the verifier used to compute
        last = E.BLOCK * (q + 2) - 1
        fe = F.final_eval(fp, v % (1 << LN), LN, NL)
        assert int(trace[E.V, last]) == v and int(trace[E.IDX, last]) == v % (1 << LN) and (int(trace[E.ACC, last]), int(trace[E.ACC + 1, last])) == (fe.a, fe.b)
        assert int(trace[E.X, last]) == pow(7 * pow(oracle.root(LN), F.brev(v % (1 << LN), LN), P), 16 ** NL, P)


def _bits(v):
    return [(v >> (63 - r)) & 1 for r in range(64)]


def _non_boolean():
    bits = _bits(0x155)
    bits[63], bits[62] = 3, P - 1  # 3 + 2 (p - 1) = 1: the same value
    return bits


FORGERIES = {
    "a_bits_of_v_plus_p": ([0, 5], {1: dict(bits=_bits(5 + P))}),
    "b_pow_bit_set": ([1 << (63 - (POW_BITS - 1)), 5], {}),
    "c_index_takes_one_bit_more": ([0, 0x3FF], {1: dict(length=64 - LN - 1)}),
    "d_wrong_exponent_bit": ([0, 0x155], {1: dict(eb_flip=2)}),
    "e_horner_skips_a_coefficient": ([0, 0x155], {1: dict(k_jump=3)}),
    "f_pow_block_elsewhere": ([0, 0x155], {0: dict(ispow=False), 1: dict(ispow=True)}),
    "g_non_boolean_bit": ([0, 0x155], {1: dict(bits=_non_boolean())}),
}


def test_the_honest_trace_of_the_forgeries_reaches_the_bus_total(vx, oracle):
    """the positive control of the forgeries below: by the same route the honest witness passes the constraint identity"""
    trace, pub = E.ref_trace([0, 0x155], LN, NL, POW_BITS, ORD_POW, ABSORBED, final_poly(16))
    assert E.check(trace, pub) is None
    assert BUS_TOTAL in product_verdict(vx, E.prove_alone(trace, pub, CFG), pub)


@pytest.mark.parametrize("kind", list(FORGERIES))
def test_forged_witnesses_are_refused_by_the_constraints(vx, oracle, kind):
    """the reference prover proves what it is handed, as a stand-alone table (drawn lookup challenges, the transcript the product's
    stand-alone verifier runs); the product verifier, under the program the library derived, finds the constraint identity broken"""
    values, forge = FORGERIES[kind]
    trace, pub = E.ref_trace(values, LN, NL, POW_BITS, ORD_POW, ABSORBED, final_poly(16), forge=forge)
    assert E.check(trace, pub) is not None
    assert IDENTITY in product_verdict(vx, E.prove_alone(trace, pub, CFG), pub)


# ---- the group
def ids(vx):
    return [vx.lib.VX_AIR_FRI_FOLD, vx.lib.VX_AIR_TRANSCRIPT, vx.lib.fri_exit_air_id()]


@pytest.mark.parametrize("name", list(GROUP_SHAPES))
def test_the_reference_group_passes_the_product_verifier(vx, oracle, name):
    g = E.group(name)
    c, cfg = g["c"], pcfg(vx, g["cfg"])
    assert (c["LN"], c["NL"], len(c["fpoly"])) == GROUP_SHAPES[name] and c["pow_bits"] == (0 if name == "fib8_pow0" else 16)
    if name == "fib8_40_queries":
        assert len(set(c["index"])) < len(c["index"])  # an index drawn twice: two equal exit messages
    blob = BG.wrap(g["proofs"], ids(vx))
    vx.lib.fri_exits_verify(blob, g["proof"], cfg)
    tot, chal = E.totals(g["proofs"], g["cfg"]["cap_height"])
    assert tot == E.outside_sum(chal, c["ord_pow"], c["words"], c["chals"], c["fpoly"], c["index"], c["ev0"], c["leaves"])
    # the binding's outside words say the same, message by message
    out = vx.lib.fri_exits_outside(c["LN"], c["ord_pow"], c["words"], [list(x) for x in c["chals"]], c["fpoly"], c["index"], c["ev0"], c["leaves"])
    n_q = len(c["index"])
    assert out.shape == (n_q * (32 * c["NL"] + 1) + len(c["words"]) + c["ord_pow"] + len(c["fpoly"]), 6)
    assert [int(v) for v in g["tabs"][2][1][:8]] == [int(v) for v in vx.lib.fri_exit_public(c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), c["fpoly"])[:8]]


def test_public_inputs_and_their_refusals(vx, oracle):
    for name in GROUP_SHAPES:
        c = E.claims_of(name)
        want = E.public_inputs(c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), c["fpoly"])
        assert [int(v) for v in vx.lib.fri_exit_public(c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), c["fpoly"])] == want
    assert vx.lib.fri_exit_log_n(1) == 8 and vx.lib.fri_exit_log_n(3) == 9 and vx.lib.fri_exit_log_n(4) == 10 and vx.lib.fri_exit_log_n(84) == 14 == E.log_rows(84)
    for kw, text in ((dict(n=0), "a final polynomial of 0 coefficients \\(1..64\\)"), (dict(n=65), "a final polynomial of 65 coefficients \\(1..64\\): more do not fit"),
                     (dict(n_layers=0), "0 fold layers \\(1..8\\)"), (dict(n_layers=9, log_lde=32), "9 fold layers \\(1..8\\)"),
                     (dict(log_lde=8, n_layers=2), "0 index bits behind the fold layers \\(FB, at least 1\\)")):
        a = dict(log_lde=9, n_layers=1, n=16)
        a.update(kw)
        with pytest.raises(vx.VxError, match=text) as e:
            vx.lib.fri_exit_public(a["log_lde"], a["n_layers"], POW_BITS, ORD_POW, ABSORBED, final_poly(a["n"]))
        assert e.value.code == ERR_ARG
    vx.lib.fri_exit_public(9, 1, POW_BITS, ORD_POW, ABSORBED, final_poly(64))


def test_refusals_through_the_group(vx, oracle):
    g, other = E.group("fib8"), E.group("fib8_pow0")
    c, cfg = g["c"], pcfg(vx, g["cfg"])
    blob = BG.wrap(g["proofs"], ids(vx))
    L = vx.lib
    stmt = g["stmt"]
    expect = [(i, pub) for i, (_, pub) in zip(ids(vx), g["tabs"])]

    def outside(**kw):
        a = dict(index=c["index"], ev0=c["ev0"], leaves=c["leaves"], fpoly=c["fpoly"], words=c["words"], chals=[list(x) for x in c["chals"]])
        a.update(kw)
        return L.fri_exits_outside(c["LN"], c["ord_pow"], a["words"], a["chals"], a["fpoly"], a["index"], a["ev0"], a["leaves"])

    def refused(outside_, expect_=expect, blob_=blob, match="does not (balance|close)"):
        with pytest.raises(vx.VxError, match=match) as e:
            L.bus_group_verify(blob_, expect_, cfg, outside_)
        assert e.value.code == ERR_STATEMENT

    L.bus_group_verify(blob, expect, cfg, outside())  # what fri_exits_verify composes
    # a) one fold claim's index replaced by another valid index of the same proof, its own ev_0 and leaves kept
    q = next(k for k in range(1, len(c["index"])) if c["index"][k] != c["index"][0])
    swapped = list(c["index"])
    swapped[0] = c["index"][q]
    refused(outside(index=swapped))
    # b) one final-polynomial word of the head, c) the head's nonce: as the verifier of a changed head would state them
    fp = np.array(c["fpoly"], dtype=np.uint64).copy()
    fp[3, 1] ^= np.uint64(1)
    refused(outside(fpoly=fp))
    words = list(c["words"])
    at = len(words) - 1 - 2 * len(c["fpoly"]) + 2 * 3 + 1
    assert words[-1 - 2 * len(c["fpoly"]):-1] == [int(v) for v in c["fpoly"].reshape(-1)]  # the final polynomial, then the nonce, are the last observed words
    words[at] ^= 1
    refused(outside(words=words, fpoly=fp))
    words = list(c["words"])
    words[-1] ^= 1
    refused(outside(words=words))
    for bad in (fp, None):  # ... and through fri_exits_verify itself, on the changed proof
        pr = g["proof"].copy()
        hd = E.Z.head(pr, g["cfg"])
        o_nonce = hd["o_queries"] - 1
        assert int(pr[o_nonce]) == c["words"][-1]
        pr[o_nonce - 2 * len(c["fpoly"]) + 7 if bad is not None else o_nonce] ^= np.uint64(1)
        with pytest.raises(vx.VxError, match="proof of work invalid") as e:  # the claims are cut from a proof the inner verifier refuses:
            L.fri_exits_verify(blob, pr, cfg)                                # both words are absorbed before the response is drawn
        assert e.value.code == ERR_STATEMENT
    # d) a chal message for an ordinal at or above ORD_POW added
    for j in (c["ord_pow"], c["ord_pow"] + 1, len(c["chals"]) - 1):
        a, v = c["chals"][j]
        refused(np.concatenate([outside(), np.array([[0, j, a, v, E.TAG_CHAL, P - 1]], dtype=np.uint64)]))
    # e) the exit table's proof swapped for one made for a different inner proof
    swapped = BG.wrap([g["proofs"][0], g["proofs"][1], other["proofs"][2]], ids(vx))
    refused(outside(), blob_=swapped, match=IDENTITY)  # other public inputs and another trace cap: other shared challenges for all three
    refused(outside(), [expect[0], expect[1], (expect[2][0], other["tabs"][2][1])], swapped, match=IDENTITY)
    # f) fin sent with multiplicity n_queries - 1
    o = outside()
    fin = o[:, 4] == E.TAG_FIN
    assert int(fin.sum()) == len(c["fpoly"]) and set(o[fin, 5].tolist()) == {len(c["index"])}
    o[fin, 5] -= np.uint64(1)
    refused(o)
    one = outside()
    one[np.flatnonzero(fin)[5], 5] -= np.uint64(1)
    refused(one)
    # the digest is every table's: a verifier that states another one is refused on the public inputs
    pub2 = [list(p) for _, p in expect]
    pub2[2][-1] ^= 1
    refused(outside(), [expect[0], expect[1], (expect[2][0], pub2[2])], match="public input 11 differs")
    assert all(list(p[-4:]) == list(stmt) for _, p in expect)
