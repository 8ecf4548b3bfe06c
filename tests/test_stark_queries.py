"""The whole query phase of a STARK proof on one bus, without a GPU: the reference prover makes the inner proof and the group's blob
(tests/stark_queries_ref.py), the product's host verifier judges them.  vx_stark_queries_verify accepts the blob with the whole
proof, with the proof's head alone and with every word of the query section replaced by junk -- vx_stark_verify refuses the last two
--, refuses every change to the head, to the blob and to the proof's length, and forged groups -- one table holding something else
than the others -- miss the balance or fail a table.  Everything is exact."""
import numpy as np
import pytest

import stark_queries_ref as Z
from oracle import stark_ref as S

P = Z.P
ERR_ARG, ERR_STATEMENT = -1, -5


def pcfg(vx, cfg):
    keys = ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")
    return vx.lib.default_stark_config(**{k: cfg[k] for k in keys if k in cfg})


@pytest.mark.parametrize("name", list(Z.SHAPES))
def test_reference_blobs_pass_the_product_verifier_in_all_three_forms(vx, oracle, name):
    g = Z.group(name)
    cl, hd, cfg = g["cl"], g["hd"], pcfg(vx, g["cfg"])
    assert cl["shape"] == Z.SHAPES[name][3]
    n_sponge = len(Z.X.sponge_lengths(cl))
    assert len(g["tabs"]) == 4 + n_sponge and int(g["blob"][Z.HDR - 1]) == 4 + n_sponge
    if name == "fib8":
        assert n_sponge == 1 and sorted(len(c["leaf"]) for c in cl["claims"][:3]) == [2, 4, 32]  # main and quotient through the noop table
    if name == "lookup8":
        assert Z.X.sponge_lengths(cl) == [6, 7, 32]
    if name == "fib8_40_queries":
        assert cl["index"].count(284) == 2  # a duplicate index: both copies are proven
    ok, chal = Z.bus_check(g["proofs"], g["cfg"]["cap_height"], cl, hd)
    assert ok
    head = g["proof"][:hd["o_queries"]]
    assert (vx.lib.stark_proof_head(g["proof"], cfg) == head).all() and head.size < g["proof"].size
    junk = Z.garbled(g["proof"], hd)
    vx.lib.stark_queries_verify(g["blob"], g["proof"], cfg)
    vx.lib.stark_queries_verify(g["blob"], head, cfg)
    vx.lib.stark_queries_verify(g["blob"], junk, cfg)
    vx.lib.stark_verify(g["proof"], cfg)
    for p in (head, junk):
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(p, cfg)


@pytest.mark.parametrize("name", ["fib8", "lookup8"])
def test_every_claim_extractor_reads_what_the_reference_reads(vx, oracle, name):
    """vx_stark_fri_claims, vx_stark_combine_claims and vx_stark_merkle_claims fill from ONE sink of the verifier's query phase: each
    must hand out, word for word, what the reference reads from the same proof, and they must agree on index and ev_0."""
    g = Z.group(name)
    cl, hd, rows, leaves, cfg = g["cl"], g["hd"], g["rows"], g["leaves"], pcfg(vx, g["cfg"])
    LN, cm, ca, a, NL, cap_h, n_q = cl["shape"]
    index = np.array(cl["index"], dtype=np.uint64)
    ev0 = np.array([leaves[q, 0, 2 * (int(i) & 15): 2 * (int(i) & 15) + 2] for q, i in enumerate(index)], dtype=np.uint64)  # the slot the chain enters layer 0 with
    ev_last = np.array([[e.a, e.b] for e in (Z.F.final_eval(hd["fpoly"], int(i), LN, NL) for i in index)], dtype=np.uint64)
    f, c, m = vx.lib.stark_fri_claims(g["proof"], cfg), vx.lib.stark_combine_claims(g["proof"], cfg), vx.lib.stark_merkle_claims(g["proof"], cfg)
    same = lambda got, want: np.array_equal(np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64))  # noqa: E731
    # the fold side
    assert f["log_lde"] == LN and f["leaves"].shape == (n_q, NL, 32)
    assert same(f["betas"], hd["betas"]) and same(f["final_poly"], hd["fpoly"]) and same(f["index"], index) and same(f["ev0"], ev0)
    assert same(f["leaves"], leaves) and same(f["ev_last"], ev_last)
    # the combination side
    assert (c["log_lde"], c["cm"], c["ca"], c["nq"]) == (LN, cm, ca, Z.NQ) and c["rows"].shape == (n_q, cm + ca + Z.NQ)
    assert same(c["alpha"], hd["alpha"]) and same(c["zeta"], hd["zeta"])
    assert same(c["open_local"], hd["ol"]) and same(c["open_next"], hd["on"]) and same(c["open_quot"], hd["oq"])
    assert same(c["index"], index) and same(c["ev0"], ev0) and same(c["rows"], rows)
    # the Merkle side: one claim per (query, tree), in record order
    assert m["shape"] == list(cl["shape"]) and m["trees"] == list(cl["trees"]) and len(cl["claims"]) == n_q * len(cl["trees"]) == m["tree"].size
    for k, t in enumerate(cl["trees"]):
        assert same(m["caps"][k], cl["caps"][t])
    for i, want in enumerate(cl["claims"]):
        assert (int(m["tree"][i]), int(m["index"][i]), int(m["leaf_len"][i])) == (want["tree"], want["index"], len(want["leaf"]))
        assert same(m["leaves"][i], want["leaf"]) and same(m["siblings"][i], want["sib"])
    # ... and with each other
    assert same(f["index"], c["index"]) and same(f["ev0"], c["ev0"]) and same(m["index"][::len(cl["trees"])], f["index"])


def test_the_statement_digest_holds_no_row_and_no_leaf_word(oracle):
    g = Z.group("fib8")
    words = len(g["cl"]["shape"]) + 4 + 2 * (2 * 2 + 4) + 2 * 1 + 2 * len(g["hd"]["fpoly"]) + 4 * len(g["cl"]["trees"]) + 5
    assert words < 100  # the shape, alpha, zeta, the openings, beta, the final polynomial, three roots, five indices
    for tr, pub in g["tabs"]:
        assert pub[-4:] == Z.statement_digest(g["cl"], g["hd"])


def test_changes_to_the_head_are_refused(vx, oracle):
    g = Z.group("fib8")
    cfg, proof, hd, blob = pcfg(vx, g["cfg"]), g["proof"], g["hd"], g["blob"]
    o_pub = 12 + int(proof[9])
    cw = 4 << g["cfg"]["cap_height"]
    o_cap, o_quot_cap = o_pub + int(proof[o_pub - 1]), o_pub + int(proof[o_pub - 1]) + cw
    o_local = o_quot_cap + cw
    o_final = hd["o_queries"] - 1 - 2 * len(hd["fpoly"])
    for what, at in (("trace cap", o_cap + 5), ("quotient cap", o_quot_cap + 1), ("opening", o_local + 3), ("layer cap", o_local + 2 * (4 + 4 + 4) + 2), ("final polynomial", o_final + 1)):
        for form in (proof, proof[:hd["o_queries"]]):
            bad = form.copy()
            bad[at] ^= 1
            with pytest.raises(vx.VxError) as e:
                vx.lib.stark_queries_verify(blob, bad, cfg)
            assert e.value.code == ERR_STATEMENT, what
    # another proof of the same shape: the blob is not its query phase
    air, trace, pub, rcfg = Z.inner("fib8")
    other_trace, other_pub = air.trace(8, 3, 5)
    other = np.array(S.prove(air, other_trace, other_pub, rcfg), dtype=np.uint64)
    vx.lib.stark_verify(other, cfg)
    with pytest.raises(vx.VxError) as e:
        vx.lib.stark_queries_verify(blob, other, cfg)
    assert e.value.code == ERR_STATEMENT
    other = Z.group("fib8_rate2")  # ... and a proof of another shape
    with pytest.raises(vx.VxError):
        vx.lib.stark_queries_verify(blob, other["proof"], pcfg(vx, other["cfg"]))
    # expected public inputs and AIR are checked on the head
    vx.lib.stark_queries_verify(blob, proof[:hd["o_queries"]], cfg, expect_air=vx.lib.VX_AIR_FIBONACCI, expect_public=pub)
    with pytest.raises(vx.VxError, match="public input"):
        vx.lib.stark_queries_verify(blob, proof[:hd["o_queries"]], cfg, expect_air=vx.lib.VX_AIR_FIBONACCI, expect_public=[int(pub[0]) ^ 1] + [int(v) for v in pub[1:]])
    with pytest.raises(vx.VxError, match="unexpected AIR"):
        vx.lib.stark_queries_verify(blob, proof, cfg, expect_air=vx.lib.VX_AIR_MIX)


def test_only_the_head_or_the_whole_proof_is_a_proof(vx, oracle):
    g = Z.group("fib8")
    cfg, proof, hd, blob = pcfg(vx, g["cfg"]), g["proof"], g["hd"], g["blob"]
    for n in (hd["o_queries"] + 1, hd["o_queries"] + hd["q_words"], proof.size - 1, hd["o_queries"] - 1, 40):
        with pytest.raises(vx.VxError, match="truncated") as e:
            vx.lib.stark_queries_verify(blob, proof[:n], cfg)
        assert e.value.code == ERR_STATEMENT
    with pytest.raises(vx.VxError, match="trailing"):
        vx.lib.stark_queries_verify(blob, np.concatenate([proof, proof[:1]]), cfg)
    bad = proof[:hd["o_queries"]].copy()  # the head is checked for canonical words; the query section is not read
    bad[hd["o_queries"] - 3] = P
    with pytest.raises(vx.VxError, match="non-canonical"):
        vx.lib.stark_queries_verify(blob, bad, cfg)
    with pytest.raises(vx.VxError) as e:  # FriFoldAir is compiled for arity 4
        vx.lib.stark_queries_verify(blob, proof, vx.lib.default_stark_config(num_queries=5, arity_bits=3))
    assert e.value.code == ERR_ARG


def test_truncated_and_damaged_blobs_are_refused(vx, oracle):
    g = Z.group("fib8")
    cfg, proof, blob = pcfg(vx, g["cfg"]), g["proof"], g["blob"]
    n = int(blob[Z.HDR - 1])
    with pytest.raises(vx.VxError):
        vx.lib.stark_queries_verify(blob[:-9], proof, cfg)
    for w in range(Z.HDR + n):  # every header word: magic, shape, table count, lengths
        for bit in (0, 3, 40):
            bad = blob.copy()
            bad[w] ^= np.uint64(1 << bit)
            with pytest.raises(vx.VxError):
                vx.lib.stark_queries_verify(bad, proof, cfg)
    at = Z.HDR + n
    for k in range(n):  # one word in each table proof: a public input (the statement digest) and a word deep inside
        ln = int(blob[Z.HDR + k])
        for off in (12 + int(blob[at + 9]) + 1, ln // 2, ln - 1):
            bad = blob.copy()
            bad[at + off] ^= 1
            with pytest.raises(vx.VxError):
                vx.lib.stark_queries_verify(bad, proof, cfg)
        at += ln
    # two tables swapped, with their lengths
    ps = Z.unwrap(blob)
    swapped = Z.wrap([ps[0], ps[1], ps[3], ps[2], ps[4]], g["cl"]["shape"])
    with pytest.raises(vx.VxError):
        vx.lib.stark_queries_verify(swapped, proof, cfg)


# ---- forged groups: ONE table holds something else than the others.  Every table is then still a valid table of its AIR (unless
# the row check says otherwise), so the reference prover proves it; what fails is the balance of the bus.
def _flip(leaf, at):
    leaf = list(leaf)
    leaf[at] ^= 1
    return leaf


FORGED = {
    "row_word_in_the_sponge_table_only": ("lookup8", dict(sponge=lambda t, i, leaf: _flip(leaf, 3) if t == 8 and len(leaf) == 7 else leaf)),
    "quotient_word_in_the_noop_table_only": ("fib8", dict(noop=lambda t, i, leaf: (t, _flip(leaf, 2) if t == 10 else leaf))),
    "noop_row_labelled_with_the_wrong_tree": ("fib8", dict(noop=lambda t, i, leaf: (8 if t == 10 else t, leaf))),
    "layer_leaf_in_the_sponge_table_only": ("fib8", dict(sponge=lambda t, i, leaf: _flip(leaf, 17) if t == 0 else leaf)),
    "rows_of_two_queries_swapped_in_the_combine_table": ("fib8", dict(rows=lambda rows: rows[[1, 0] + list(range(2, len(rows)))])),
}


@pytest.mark.parametrize("kind", list(FORGED))
def test_forged_groups_miss_the_balance_or_fail_a_table(vx, oracle, kind):
    name, forge = FORGED[kind]
    g = Z.group(name)
    cl, hd, cfg = g["cl"], g["hd"], pcfg(vx, g["cfg"])
    if kind.startswith("rows_of_two"):
        assert cl["index"][0] != cl["index"][1]
    tabs, airs, _ = Z.tables(cl, hd, g["st"], g["rows"], g["leaves"], forge, g["cfg"])
    assert any((a[0] != b[0]).any() for a, b in zip(tabs, g["tabs"]))  # the forgery changed a table
    tot, bad = Z.tables_sum(tabs, airs, Z.CHAL)
    assert bad is not None or not (tot == Z.outside_sum(Z.CHAL, cl, hd))
    if bad is None:  # every table satisfies its AIR: proven by the reference prover, refused by the product's verifier at the balance
        blob = Z.wrap(Z.prove(tabs, airs, g["cfg"]), cl["shape"])
        with pytest.raises(vx.VxError, match="does not balance") as e:
            vx.lib.stark_queries_verify(blob, g["proof"], cfg)
        assert e.value.code == ERR_STATEMENT
