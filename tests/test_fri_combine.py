"""FriCombineAir (AIR id 21) without a GPU: every constraint of the independently restated AIR has degree <= 3, the closing formula
is the verifier's expression (restated here in big integers), the reference trace satisfies the restatement and forged witnesses do
not -- each refused with the broken rule named --, the claims of reference-prover proofs (with and without an auxiliary tree)
combine to the value their first FRI leaf holds, and reference-prover proofs of the restatement pass the product's
vx_fri_combine_verify and, with FriFoldAir on the same bus and NO ev_0 handed over, vx_fri_combine_fold_verify.  Everything is exact."""
import numpy as np
import pytest

import fri_combine_ref as K
import fri_fold_ref as F
from oracle import oracle as O
from oracle import stark_ref as S

P = K.P
CFG = dict(S.DEFAULT_CFG, num_queries=8)
CHAL = K.CHAL


def pcfg(vx, **over):
    return vx.lib.default_stark_config(**dict(dict(num_queries=CFG["num_queries"]), **over))


def test_every_constraint_has_degree_at_most_3(oracle):
    b = K.builder()
    degs = [K.degree(e) for _, e in b.constraints]
    assert len(degs) == 60 and max(degs) == 3
    assert all(kind == "assert_zero" for kind, _ in b.constraints)  # no first-row, last-row or transition constraints
    assert not b.periodic and (b.cols, b.n_public, b.aux_cols) == (K.COLS, K.PUB, K.AUX)


# ---- the verifier's expression (vx_stark_verify_ext's query loop), restated in big integers
def ext_mul(x, y):
    return ((x[0] * y[0] + 7 * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def ext_inv(x):
    ni = pow((x[0] * x[0] - 7 * x[1] * x[1]) % P, P - 2, P)
    return (x[0] * ni % P, -x[1] * ni % P)


def ext_add(x, y, sign=1):
    return ((x[0] + sign * y[0]) % P, (x[1] + sign * y[1]) % P)


def verifier_ev0(st, index, row):
    alpha, zeta = tuple(int(v) for v in st["alpha"]), tuple(int(v) for v in st["zeta"])
    c, nq = st["cm"] + st["ca"], st["nq"]
    tup = lambda v: (int(v[0]), int(v[1]))  # noqa: E731
    apow, y0, y1 = (1, 0), (0, 0), (0, 0)
    for j in range(c + nq):
        if j < c:
            y0, y1 = ext_add(y0, ext_mul(apow, tup(st["ol"][j]))), ext_add(y1, ext_mul(apow, tup(st["on"][j])))
        else:
            y0 = ext_add(y0, ext_mul(apow, tup(st["oq"][j - c])))
        apow = ext_mul(apow, alpha)
    alpha_c = (1, 0)
    for _ in range(c):
        alpha_c = ext_mul(alpha_c, alpha)
    zeta_next = ext_mul(zeta, (O.root(st["LN"] - st["r"]), 0))
    x = 7 * pow(O.root(st["LN"]), K.brev(index, st["LN"]), P) % P
    s1, ap = (0, 0), (1, 0)
    for j in range(c):
        s1, ap = ext_add(s1, ext_mul(ap, (int(row[j]), 0))), ext_mul(ap, alpha)
    s0 = s1
    for j in range(nq):
        s0, ap = ext_add(s0, ext_mul(ap, (int(row[c + j]), 0))), ext_mul(ap, alpha)
    return ext_add(ext_mul(ext_mul(alpha_c, ext_add(s0, y0, -1)), ext_inv(ext_add((x, 0), zeta, -1))), ext_mul(ext_add(s1, y1, -1), ext_inv(ext_add((x, 0), zeta_next, -1))))


SHAPES = {  # name -> (LN, cm, ca, nq, indices)
    "no_aux": (5, 3, 0, 2, [19, 0, 31]),
    "aux": (9, 3, 2, 2, [0x155, 511]),
    "one_main_one_quot": (6, 1, 3, 1, [33, 33, 7]),
    "four_quot": (14, 5, 1, 4, [0x2ABC]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_trace_satisfies_the_restated_air(oracle, name):
    LN, cm, ca, nq, index = SHAPES[name]
    st = K.rand_statement(LN, cm, ca, nq)
    rows, ev0 = K.rand_claims(st, index)
    trace, pub = K.ref_trace(st, index, rows)
    rpq = cm + ca + nq + LN
    assert trace.shape == (K.COLS, 1 << K.log_rows(len(index), st)) and pub[:6] == [rpq, cm, ca, nq, K.TREE0, oracle.root(LN)]
    aux, apub = K.gen_aux(trace, CHAL, pub)
    assert S.check_trace(K.air(), trace, pub, CHAL, aux, apub) is None
    # what leaves the table is the verifier's expression
    for k, i in enumerate(index):
        last = (k + 1) * rpq - 1
        want = verifier_ev0(st, i, rows[k])
        assert int(trace[K.LAST, last]) == 1 and (int(trace[K.EV, last]), int(trace[K.EV + 1, last])) == want == (int(ev0[k, 0]), int(ev0[k, 1]))


def test_a_table_without_an_idle_row_wraps_around(oracle):
    st = K.rand_statement(5, 1, 0, 2)  # 8 rows per query
    index = [3, 30, 0, 31]
    rows, _ = K.rand_claims(st, index)
    trace, pub = K.ref_trace(st, index, rows)
    assert trace.shape[1] == 32 and int(trace[K.LAST, -1]) == 1
    aux, apub = K.gen_aux(trace, CHAL, pub)
    assert S.check_trace(K.air(), trace, pub, CHAL, aux, apub) is None


# positions in the constraint order of fri_combine_ref.builder: 7 boolean cells, 14 shape rules, 5 tree-length / POS rules, 3 counter
# rules, 13 word / power / sum rules, 5 index rules, 3 accumulator rules, 6 closing rules, 4 bus rules
AUX_SKIPPED, TM_END, POS_STEP, AP_STEP, S_STEP, S1_BIND, CLOSING, A_START, D0_RULE, EV_RULE = 20, 21, 24, 32, 36, 40, 44, 47, 50, 54
FORGERIES = ["word_changed_s_recomputed", "pos_skipped", "tree_one_row_early", "tree_one_row_late", "aux_skipped", "ap_not_advanced", "s1_one_row_off",
             "bit_flipped_hidden_by_division", "a_started_off_1", "d0_not_the_inverse", "ev_changed"]


@pytest.mark.parametrize("kind", FORGERIES)
def test_forged_witnesses_are_refused(oracle, kind):
    LN, cm, ca, nq, index = 5, 3, 2, 2, 0b10110
    st = K.rand_statement(LN, cm, ca, nq)
    rows, ev0 = K.rand_claims(st, [index, 9])
    absn, last = cm + ca + nq, cm + ca + nq + LN - 1
    honest = K.query_rows(st, 9, rows[1])
    first = K.query_rows(st, index, rows[0])
    if kind == "word_changed_s_recomputed":
        # the word of row 1 is another one and S of that row follows it; the next row's sum does not
        first[K.W, 1] ^= np.uint64(1)
        s = K.ext(first[K.SS: K.SS + 2, 0]) + K.ext(first[K.AP: K.AP + 2, 1]) * int(first[K.W, 1])
        first[K.SS, 1], first[K.SS + 1, 1] = s.a, s.b
        want_bad = (S_STEP, 1)
    elif kind == "pos_skipped":
        first = K.query_rows(st, index, rows[0], pos=[0, 2, 2, 0, 1, 0, 1])
        want_bad = (POS_STEP, 0)
    elif kind == "tree_one_row_early":
        first = K.query_rows(st, index, rows[0], trees=[0, 0, 1, 1, 1, 2, 2])
        want_bad = (TM_END, 1)
    elif kind == "tree_one_row_late":
        first = K.query_rows(st, index, rows[0], trees=[0, 0, 0, 0, 1, 2, 2])
        want_bad = (TM_END, 3)
    elif kind == "aux_skipped":
        first = K.query_rows(st, index, rows[0], trees=[0, 0, 0, 2, 2, 2, 2])
        want_bad = (AUX_SKIPPED, 2)
    elif kind == "ap_not_advanced":
        first = K.query_rows(st, index, rows[0], ap_stall=2)
        want_bad = (AP_STEP, 1)
    elif kind == "s1_one_row_off":
        first = K.query_rows(st, index, rows[0], s1_row=cm + ca - 2)
        want_bad = (S1_BIND, cm + ca - 1)
    elif kind == "bit_flipped_hidden_by_division":
        # x comes from another index while R starts from the claimed one and is continued by field division: every row rule
        # holds, the message names the claimed index -- only the closing rule (no bit left) fails
        first = K.query_rows(st, index, rows[0], flip_bit=1)
        assert int(first[K.IDX, 0]) == index and int(first[K.RR, absn]) == index and int(first[K.Q, -1]) != 0
        want_bad = (CLOSING, last)
    elif kind == "a_started_off_1":
        first = K.query_rows(st, index, rows[0], a_start=2)
        want_bad = (A_START, absn)
    elif kind == "d0_not_the_inverse":
        first[K.D0, last] ^= np.uint64(1)
        want_bad = (D0_RULE, last)
    elif kind == "ev_changed":
        first[K.EV, last] ^= np.uint64(1)
        want_bad = (EV_RULE, last)
    trace = K.assemble([first, honest], 5)
    pub = K.public_inputs(st, [index, 9], rows, ev0)
    aux, apub = K.gen_aux(trace, CHAL, pub)
    assert S.check_trace(K.air(), trace, pub, CHAL, aux, apub) == want_bad


@pytest.fixture(scope="module")
def real(vx, oracle):
    """reference-prover proofs of FibAir (no auxiliary tree) and LookupAir (auxiliary tree), 2^10 rows and 5 queries: a 2^11 LDE,
    one fold layer; shared by the tests below"""
    cfg = dict(S.DEFAULT_CFG, num_queries=5)
    out = {}
    for name, a in (("fib", S.FibAir), ("lookup", S.LookupAir)):
        trace, pub = a.trace(10)
        out[name] = S.prove(a, trace, pub, cfg)
    return cfg, vx.lib.default_stark_config(num_queries=5), out


@pytest.mark.parametrize("name", ["fib", "lookup"])
def test_claims_of_a_reference_proof_combine_to_the_first_fri_leaf(vx, real, name):
    cfg, pc, proofs = real
    proof = proofs[name]
    st, index, rows, first, cap = K.claims_of(proof, cfg)
    assert (st["ca"] > 0) == (name == "lookup") and st["LN"] == 11 and len(index) == 5
    fc = vx.lib.stark_fri_claims(proof, pc)
    c = vx.lib.stark_combine_claims(proof, pc)
    assert (c["log_lde"], c["cm"], c["ca"], c["nq"]) == (st["LN"], st["cm"], st["ca"], st["nq"])
    for k in ("alpha", "zeta"):
        assert [int(v) for v in c[k]] == [int(v) for v in st[k]]
    for k, m in (("open_local", "ol"), ("open_next", "on"), ("open_quot", "oq")):
        assert (c[k] == st[m]).all()
    assert [int(v) for v in c["index"]] == index and (c["rows"] == rows).all() and (c["ev0"] == fc["ev0"]).all()
    for k, i in enumerate(index):
        ev = K.combine(st, i, rows[k])
        assert [ev.a, ev.b] == [int(v) for v in c["ev0"][k]]
        # ... and it is the `within` slot of the query's first FRI leaf: with it in place the leaf lies under the layer's cap
        others, sib = first[k]
        within = i & 15
        leaf = np.array(others[: 2 * within] + [ev.a, ev.b] + others[2 * within:], dtype=np.uint64)
        assert O.merkle_verify(leaf, i >> 4, sib, cap)
        assert (leaf == fc["leaves"][k, 0]).all()
    with pytest.raises(vx.VxError):
        vx.lib.stark_combine_claims(proof[:-7], pc)  # a truncated proof: it is verified on the way
    bad = proof.copy()
    bad[-3] ^= np.uint64(1)
    with pytest.raises(vx.VxError):
        vx.lib.stark_combine_claims(bad, pc)


@pytest.fixture(scope="module")
def round_trip(oracle):
    """ONE reference-prover proof of the restatement (LN = 9, three queries, one index twice), shared by the tests below"""
    st = K.rand_statement(9, 3, 2, 2, seed=4)
    index = [5, 500, 5]
    rows, ev0 = K.rand_claims(st, index)
    trace, pub = K.ref_trace(st, index, rows)
    return st, index, rows, ev0, pub, K.prove(trace, pub, CFG)


def verify(vx, blob, st, index, rows, ev0, cfg, **over):
    a = dict(st, **over)
    vx.lib.fri_combine_verify(blob, a["LN"], a["cm"], a["ca"], a["nq"], a["alpha"], a["zeta"], a["ol"], a["on"], a["oq"], index, rows, ev0, cfg)


def flip(a, *at):
    a = np.array(a, dtype=np.uint64)
    a[at] ^= np.uint64(1)
    return a


def test_round_trip_through_both_verifiers(vx, round_trip):
    st, index, rows, ev0, pub, proof = round_trip
    blob, cfg = K.wrap(proof, st, len(index)), pcfg(vx)
    verify(vx, blob, st, index, rows, ev0, cfg)
    ok, chal = K.bus_check(proof, CFG["cap_height"], st, index, rows, ev0)
    assert ok
    info = S.verify(proof, CFG, expect_air=K.REF_ID, expect_public=pub, ext_chal=chal)
    assert any(info["aux_public"])

    def refused(index_=index, rows_=rows, ev0_=ev0, match=None, **over):
        with pytest.raises(vx.VxError, match=match):
            verify(vx, K.wrap(proof, st, len(index_)), st, index_, rows_, ev0_, cfg, **over)

    refused(rows_=flip(rows, 1, 4))                      # one row word
    refused(ev0_=flip(ev0, 2, 1))                        # one ev_0
    refused(ol=flip(st["ol"], 3, 0))                     # one opening
    refused(on=flip(st["on"], 0, 1))
    refused(oq=flip(st["oq"], 1, 0))
    refused(alpha=flip(st["alpha"], 0))
    refused(zeta=flip(st["zeta"], 1))
    refused(index_=[5, 501, 5])                          # one index
    refused(index_=[500, 5, 5], rows_=rows[[1, 0, 2]], ev0_=ev0[[1, 0, 2]])  # the order of two claims
    refused(index_=index[:2], rows_=rows[:2], ev0_=ev0[:2])                  # one claim dropped
    with pytest.raises(vx.VxError, match="different request"):
        verify(vx, blob, st, index, rows, ev0, cfg, LN=10)
    with pytest.raises(vx.VxError, match="outside the LDE"):
        verify(vx, blob, st, [5, 512, 5], rows, ev0, cfg)
    nc = rows.copy()
    nc[0, 0] = np.uint64(P)
    with pytest.raises(vx.VxError, match="non-canonical"):
        verify(vx, blob, st, index, nc, ev0, cfg)
    for cut in list(range(0, 24)) + list(range(24, blob.size, max(1, blob.size // 40))) + [blob.size - 1]:
        with pytest.raises(vx.VxError):
            verify(vx, blob[:cut], st, index, rows, ev0, cfg)
    # the table proof on its own is no statement
    p21 = proof.copy()
    p21[1] = K.AIR_ID
    with pytest.raises(vx.VxError, match="constraint identity|non-zero bus total"):
        vx.lib.stark_verify(p21, cfg, expect_air=K.AIR_ID)


def test_a_forged_proof_is_refused_by_the_product(vx, oracle):
    """the prover does not care: a proof made from the flipped-bit witness balances its bus against the forger's claims, and only
    the compiled constraints stand in the way"""
    st = K.rand_statement(5, 2, 0, 1, seed=8)
    index = 0b01101
    rows, _ = K.rand_claims(st, [index])
    q = K.query_rows(st, index, rows[0], flip_bit=2)
    trace = K.assemble([q], 5)
    ev0 = np.array([[q[K.EV, -1], q[K.EV + 1, -1]]], dtype=np.uint64)
    pub = K.public_inputs(st, [index], rows, ev0)
    proof = K.prove(trace, pub, CFG)
    with pytest.raises(vx.VxError, match="constraint identity"):
        verify(vx, K.wrap(proof, st, 1), st, [index], rows, ev0, pcfg(vx))


def test_combine_and_fold_on_one_bus_without_ev0(vx, real):
    """the query-phase arithmetic of a reference-prover FibAir proof: FriCombineAir + FriFoldAir proven by the reference prover on
    the restatements under shared challenges; the product's group verifier is handed rows and leaves, never ev_0"""
    cfg, pc, proofs = real
    proof = proofs["fib"]
    c, f = vx.lib.stark_combine_claims(proof, pc), vx.lib.stark_fri_claims(proof, pc)
    st = dict(LN=c["log_lde"], r=cfg["rate_bits"], cm=c["cm"], ca=c["ca"], nq=c["nq"], alpha=c["alpha"], zeta=c["zeta"], ol=c["open_local"], on=c["open_next"], oq=c["open_quot"])
    index, rows, leaves, betas, fpoly = [int(v) for v in c["index"]], c["rows"], f["leaves"], f["betas"], f["final_poly"]
    NL = len(betas)
    tabs = K.group_tables(st, betas, fpoly, index, rows, leaves)
    ps, chal = K.group_prove(tabs, cfg)
    assert K.group_sum(ps, cfg["cap_height"], chal, st, betas, fpoly, index, rows, leaves)
    blob = K.group_wrap(ps, st, NL, len(index))

    def gverify(blob_=blob, index_=index, rows_=rows, leaves_=leaves, betas_=betas, fpoly_=fpoly, **over):
        a = dict(st, **over)
        vx.lib.fri_combine_fold_verify(blob_, a["LN"], a["cm"], a["ca"], a["nq"], a["alpha"], a["zeta"], a["ol"], a["on"], a["oq"], betas_, fpoly_, index_, rows_, leaves_, pc)

    gverify()
    for bad in (dict(rows_=flip(rows, 2, 1)), dict(leaves_=flip(leaves, 3, 0, 5)), dict(ol=flip(st["ol"], 0, 0)), dict(alpha=flip(st["alpha"], 1)), dict(zeta=flip(st["zeta"], 0)),
                dict(index_=index[:1] + [index[1] ^ 1] + index[2:]), dict(betas_=flip(betas, 0, 0)), dict(fpoly_=flip(fpoly, 1, 1)), dict(blob_=blob[:-5]), dict(blob_=blob[: K.GHDR + 3])):
        with pytest.raises(vx.VxError):
            gverify(**bad)
    # the two proofs under challenges of their own do not make a group
    alone = K.group_wrap([K.prove(*tabs[0], cfg), ps[1]], st, NL, len(index))
    with pytest.raises(vx.VxError):
        gverify(blob_=alone)


def test_golden_blobs_pass_both_host_verifiers(vx):
    """tests/golden/fri_combine_blobs.npz (tests/golden/make_fri_combine_golden.py): the stand-alone blob and the combine + fold blob of
    a FibAir proof's five queries, with the claims each verifier is handed; one flipped word anywhere is refused"""
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fri_combine_blobs.npz"), allow_pickle=False)
    pc = vx.lib.default_stark_config(num_queries=int(g["num_queries"]))
    a = [int(v) for v in g["shape"]] + [g["alpha"], g["zeta"], g["open_local"], g["open_next"], g["open_quot"]]
    blob, gblob = g["combine_blob"], g["combine_fold_blob"]
    assert int(blob[0]) == K.MAGIC and int(gblob[0]) == K.GMAGIC
    vx.lib.fri_combine_verify(blob, *a, g["index"], g["rows"], g["ev0"], pc)
    vx.lib.fri_combine_fold_verify(gblob, *a, g["betas"], g["final_poly"], g["index"], g["rows"], g["leaves"], pc)
    for w in (3, K.HDR + 40, blob.size // 2, blob.size - 1):
        with pytest.raises(vx.VxError):
            vx.lib.fri_combine_verify(flip(blob, w), *a, g["index"], g["rows"], g["ev0"], pc)
    for w in (5, K.GHDR + 40, gblob.size // 2, gblob.size - 1):
        with pytest.raises(vx.VxError):
            vx.lib.fri_combine_fold_verify(flip(gblob, w), *a, g["betas"], g["final_poly"], g["index"], g["rows"], g["leaves"], pc)
    with pytest.raises(vx.VxError):
        vx.lib.fri_combine_verify(blob, *a, g["index"], flip(g["rows"], 0, 0), g["ev0"], pc)
    with pytest.raises(vx.VxError):
        vx.lib.fri_combine_fold_verify(gblob, *a, g["betas"], g["final_poly"], g["index"], g["rows"], flip(g["leaves"], 0, 0, 0), pc)
