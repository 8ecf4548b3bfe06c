"""An inner proof's query phase AND transcript on one bus, without a GPU: the reference prover makes the inner proof and the group's
blob (tests/stark_inner_ref.py composes stark_queries_ref and transcript_ref), the product's host verifier judges them.
vx_stark_inner_verify accepts the blob with the whole proof, with its head alone and with the query section garbled; the ONE statement
digest is the public-input digest of every table and holds nothing of the query phase twice; every change to the blob's header and
claims, to the table proofs, to the head and to the proof's length is refused; forged groups -- proven by the reference prover -- are
refused at the balance of the bus or by the verifier's own check on the claimed values, whichever the forgery meets first.  Everything
is exact."""
import ctypes as C

import numpy as np
import pytest

import stark_inner_ref as I
from oracle import stark_ref as S

Z, T, P = I.Z, I.T, I.P
ERR_ARG, ERR_STATEMENT = -1, -5


def pcfg(vx, cfg):
    keys = ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")
    return vx.lib.default_stark_config(**{k: cfg[k] for k in keys if k in cfg})


def verify(vx, g, blob=None, proof=None, cfg=None, **kw):
    vx.lib.stark_inner_verify(g["blob"] if blob is None else blob, g["proof"] if proof is None else proof, cfg or pcfg(vx, g["cfg"]), ext_chal=g["ext"], **kw)


def refused(vx, g, blob=None, proof=None, match=None, code=None, **kw):
    with pytest.raises(vx.VxError, match=match) as e:
        verify(vx, g, blob, proof, **kw)
    if code is not None:
        assert e.value.code == code, e.value
    return e.value


@pytest.mark.parametrize("name", list(I.INNER))
def test_reference_blobs_pass_the_product_verifier_in_all_three_forms(vx, oracle, name):
    g = I.group(name)
    cl, hd, cfg = g["cl"], g["hd"], pcfg(vx, g["cfg"])
    ops, words = g["chain"]
    shape, ext, facts = I.INNER[name]
    assert cl["shape"] == Z.SHAPES[shape][3]
    if facts:
        assert (len(words), len(g["chals"]), len(T.plan(ops)), g["tabs"][-1][0].shape[1].bit_length() - 1, len(g["tabs"])) == facts
    if name == "fib8":  # a full transcript table: every block is a duplex of the chain
        assert int(g["tabs"][-1][0][T.ACT].sum()) == g["tabs"][-1][0].shape[1]
    if ext:  # the external challenges are absorbed, not drawn: four challenges fewer, four words more than the drawn form
        o = I.group("lookup8")
        assert len(words) == len(o["chain"][1]) + 4 and len(g["chals"]) == len(o["chals"]) - 4
    blob = g["blob"]
    assert [int(v) for v in blob[:I.HDR]] == [I.MAGIC] + cl["shape"] + [len(g["tabs"]), len(words), len(g["chals"])] and I.blob_claims(blob) == g["chals"]
    assert I.bus_check(g["proofs"], g["cfg"]["cap_height"], cl, hd, words, g["chals"])
    # the product's own replay hands out the same claims
    got_w, got_c = vx.lib.stark_transcript_claims(g["proof"], cfg, ext)
    assert [int(v) for v in got_w] == words and [(int(a), int(v)) for a, v in got_c] == g["chals"]
    head = g["proof"][:hd["o_queries"]]
    assert (vx.lib.stark_proof_head(g["proof"], cfg) == head).all() and head.size < g["proof"].size
    junk = Z.garbled(g["proof"], hd)
    for p in (g["proof"], head, junk):
        verify(vx, g, proof=p)
    for p in (head, junk):
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(p, cfg)
    # the header split of the binding
    sw, n_obs, claims, proofs = vx.lib.split_stark_inner(blob)
    assert sw == cl["shape"] and n_obs == len(words) and [(int(a), int(v)) for a, v in claims] == g["chals"]
    assert len(proofs) == len(g["proofs"]) and all(p.size == len(q) for p, q in zip(proofs, g["proofs"]))


@pytest.mark.parametrize("name", ["fib8", "lookup8"])
def test_one_digest_for_every_table_and_nothing_hashed_twice(oracle, name):
    g = I.group(name)
    cl, hd = g["cl"], g["hd"]
    ops, words = g["chain"]
    hashed = [int(v) for v in cl["shape"]] + [len(words), len(g["chals"])] + [int(v) for v in words] + [int(x) for c in g["chals"] for x in c]
    assert len(hashed) == 9 + len(words) + 2 * len(g["chals"])
    stmt = [int(v) for v in I.O.hash_no_pad(np.array(hashed, dtype=np.uint64))]
    assert stmt == g["stmt"] and stmt != Z.statement_digest(cl, hd)
    for p in I.unwrap(g["blob"])[0]:  # the public inputs inside every table proof of the blob end on it
        pub, _ = S.proof_peek(p, g["cfg"]["cap_height"])
        assert [int(v) for v in pub[-4:]] == stmt
    # no row word and no leaf word (field elements of full size: a small one could meet a count by chance)
    big = lambda ws: {int(v) for v in np.asarray(ws, dtype=np.uint64).reshape(-1) if int(v) >> 32}  # noqa: E731
    opened = big(g["rows"]) | big(g["leaves"])
    assert 2 * len(opened) > g["rows"].size + g["leaves"].size  # (the check is not vacuous: most opened words are of full size)
    assert not opened & set(hashed)
    # of the words of the query-phase digest: alpha and zeta are there ONCE, as claimed values; the folded roots and the indices
    # (value mod N) are not there at all -- the caps and the values are
    for v in list(hd["alpha"]) + list(hd["zeta"]) + [int(b) for be in hd["betas"] for b in be]:
        assert hashed.count(int(v)) == 1
    for r in Z.X.roots_of(cl):
        assert not set(int(v) for v in r) & set(hashed)
    N = 1 << cl["shape"][0]
    tail = [v for _, v in g["chals"][-len(cl["index"]):]]
    assert [v % N for v in tail] == [int(i) for i in cl["index"]] and all(v >= N for v in tail)


def test_every_change_to_the_blob_is_refused(vx, oracle):
    g = I.group("fib8")
    blob = g["blob"]
    proofs, o_len = I.unwrap(blob)
    n = len(proofs)
    verify(vx, g)
    for w in range(o_len + n):  # magic, shape, table count, n_obs, n_chal, every claim word, every length
        for bit in (0, 3, 40):
            bad = blob.copy()
            bad[w] ^= np.uint64(1 << bit)
            refused(vx, g, bad)
    at = o_len + n
    for k in range(n):  # one word in each table proof: a public input (the statement digest), a middle word, the last word
        ln = int(blob[o_len + k])
        for off in (12 + int(blob[at + 9]) + 1, ln // 2, ln - 1):
            bad = blob.copy()
            bad[at + off] ^= 1
            refused(vx, g, bad)
        at += ln
    for bad in (blob[:-1], np.concatenate([blob, blob[:1]]), blob[:o_len + n], blob[:I.HDR], blob[:5]):
        refused(vx, g, bad)
    # two tables swapped, with their lengths
    segs = list(vx.lib.split_stark_inner(blob)[3])
    for a, b in ((2, 3), (n - 2, n - 1)):
        ps = list(segs)
        ps[a], ps[b] = ps[b], ps[a]
        swapped = np.concatenate([blob[:o_len], np.array([p.size for p in ps], dtype=np.uint64)] + ps)
        assert swapped.size == blob.size and sorted(swapped.tolist()) == sorted(blob.tolist())
        refused(vx, g, swapped)


def test_blobs_of_the_other_groups_are_not_this_one(vx, oracle):
    g = I.group("fib8")
    cfg, n = pcfg(vx, g["cfg"]), len(g["proofs"])
    words, chals = g["chain"][1], g["chals"]
    queries = Z.wrap(g["proofs"][:n - 1], g["cl"]["shape"])      # the same table proofs in the two older layouts
    transcripts = T.wrap(g["proofs"][-1], [(words, chals)])
    for other in (queries, transcripts):
        refused(vx, g, other, match="bad stark-inner blob", code=ERR_STATEMENT)
    with pytest.raises(vx.VxError, match="bad stark-queries blob"):
        vx.lib.stark_queries_verify(g["blob"], g["proof"], cfg)
    with pytest.raises(vx.VxError, match="bad stark-transcripts blob"):
        vx.lib.stark_transcripts_verify(g["blob"], [g["proof"]], cfg)
    # ... and the halves of this group are no groups of the older kinds: their digest is another one
    with pytest.raises(vx.VxError, match="public input"):
        vx.lib.stark_queries_verify(queries, g["proof"], cfg)
    with pytest.raises(vx.VxError, match="public input"):
        vx.lib.stark_transcripts_verify(transcripts, [g["proof"]], cfg)


def test_every_change_to_the_head_and_every_other_length_is_refused(vx, oracle):
    g = I.group("fib8")
    proof, hd = g["proof"], g["hd"]
    head = proof[:hd["o_queries"]]
    for at in range(head.size):
        bad = head.copy()
        bad[at] ^= 1
        refused(vx, g, proof=bad)
    for at in (3, 20, head.size - 2):  # ... and in the whole proof
        bad = proof.copy()
        bad[at] ^= 1
        refused(vx, g, proof=bad)
    for n in (hd["o_queries"] + 1, hd["o_queries"] + hd["q_words"], proof.size - 1, hd["o_queries"] - 1, 40):
        refused(vx, g, proof=proof[:n], match="truncated", code=ERR_STATEMENT)
    refused(vx, g, proof=np.concatenate([proof, proof[:1]]), match="trailing")
    bad = head.copy()
    bad[head.size - 3] = P
    refused(vx, g, proof=bad, match="non-canonical")
    # expected AIR and public inputs are checked on the head; arity 3 has no group
    verify(vx, g, proof=head, expect_air=vx.lib.VX_AIR_FIBONACCI, expect_public=g["pub"])
    refused(vx, g, proof=head, match="public input", expect_air=vx.lib.VX_AIR_FIBONACCI, expect_public=[int(g["pub"][0]) ^ 1] + [int(v) for v in g["pub"][1:]])
    refused(vx, g, match="unexpected AIR", expect_air=vx.lib.VX_AIR_MIX)
    refused(vx, g, cfg=vx.lib.default_stark_config(num_queries=5, arity_bits=3), code=ERR_ARG)
    # another proof of the same shape: the blob is neither its query phase nor its transcript
    trace, pub = g["air"].trace(8, 3, 5)
    other = np.array(S.prove(g["air"], trace, pub, g["cfg"]), dtype=np.uint64)
    vx.lib.stark_verify(other, pcfg(vx, g["cfg"]))
    refused(vx, g, proof=other, code=ERR_STATEMENT)
    # a claim that is no field element, and more claims than the blob holds
    bad = g["blob"].copy()
    bad[I.HDR + 1] = P
    refused(vx, g, bad, match="not canonical")
    bad = g["blob"].copy()
    bad[10] = bad.size
    refused(vx, g, bad, match="truncated")


def test_both_verifiers_of_a_claimed_transcript_refuse_bad_claims_in_the_same_words(vx, oracle):
    """the claimed-transcript check is ONE check with two callers: vx_stark_inner_verify (the one chain, bare messages) and
    vx_stark_transcripts_verify (per chain, `chain c: ` in front).  Both refuse before they read a table, so the same table proofs serve."""
    g = I.group("fib8_two_layers_cap0")
    cfg, words, chals = pcfg(vx, g["cfg"]), g["chain"][1], list(g["chals"])
    cases = [([(chals[0][0], P)] + chals[1:], "claimed challenge 0 is not canonical"),
             (chals[:-1], f"the blob claims {len(chals) - 1} challenges, the proof's shape draws more")]
    for forged, text in cases:
        inner = refused(vx, g, I.wrap(g["proofs"], g["cl"]["shape"], len(words), forged), code=ERR_STATEMENT)
        with pytest.raises(vx.VxError) as e:
            vx.lib.stark_transcripts_verify(T.wrap(g["proofs"][-1], [(words, forged)]), [g["proof"]], cfg, [g["ext"]])
        assert e.value.code == ERR_STATEMENT
        assert str(inner).endswith(": " + text) and "chain 0: " in str(e.value) and str(e.value).replace("chain 0: ", "", 1) == str(inner)


# ---- forged groups on fib8: the reference prover proves them, the product verifier must refuse them
def _forged_blob(g, chals=None, hd=None, forge=None):
    """-> (blob, the first (table, constraint, row) a row check refuses or None, whether the tables balance against the outside party)"""
    hd = hd or g["hd"]
    chals = g["chals"] if chals is None else chals
    ops, words = g["chain"]
    tabs, airs, _ = I.tables(g["cl"], hd, g["st"], g["rows"], g["leaves"], g["chain"], chals, forge, g["cfg"])
    tot, bad = Z.tables_sum(tabs, airs, I.CHAL)
    balanced = tot == I.outside_sum(I.CHAL, g["cl"], hd, words, chals)
    blob = None if bad is not None else I.wrap(I.prove(tabs, airs, g["cfg"]), g["cl"]["shape"], len(words), chals)
    return blob, bad, balanced


def _both_forms(vx, g, blob, match):
    head = g["proof"][:g["hd"]["o_queries"]]
    for p in (g["proof"], head):
        refused(vx, g, blob, proof=p, match=match, code=ERR_STATEMENT)


def test_forged_an_observed_word_changed_in_the_transcript_table_only(vx, oracle):
    """the digest is unchanged; the chain hashes other words than the head has, and draws other challenges"""
    g = I.group("fib8")

    def other_word(ops, words):
        words[100] = (words[100] + 1) % P
        return ops, words

    blob, bad, balanced = _forged_blob(g, forge=dict(transcript=other_word))
    assert bad is None and not balanced
    assert (I.unwrap(blob)[0][0][:40] == I.unwrap(g["blob"])[0][0][:40]).all()  # (the same public inputs: the same digest)
    _both_forms(vx, g, blob, "does not balance")


def test_forged_an_index_claim_raised_by_the_domain_size(vx, oracle):
    """v -> v + N in the blob, digest and public inputs rebuilt from it, the transcript table honest: the index, hence every message of
    the query phase, is unchanged -- only the chal message differs"""
    g = I.group("fib8")
    N, n_q = 1 << g["cl"]["shape"][0], len(g["cl"]["index"])
    first = len(g["chals"]) - n_q
    assert all(v + N < P for _, v in g["chals"][first:])  # canonical for every index challenge of this proof
    for j in (first, len(g["chals"]) - 1):
        chals = list(g["chals"])
        chals[j] = (chals[j][0], chals[j][1] + N)
        blob, bad, balanced = _forged_blob(g, chals=chals)
        assert bad is None and not balanced
        _both_forms(vx, g, blob, "does not balance")


def test_forged_a_claim_drawn_one_word_early(vx, oracle):
    """`absorbed` lowered by one, everything rebuilt from it: the verifier's own run notes where the shape draws the challenge"""
    g = I.group("fib8")
    chals = list(g["chals"])
    chals[4] = (chals[4][0] - 1, chals[4][1])
    blob, bad, balanced = _forged_blob(g, chals=chals)
    assert bad is None and not balanced
    _both_forms(vx, g, blob, r"challenge 4 is claimed after \d+ absorbed words, the proof's shape draws it after")


def test_forged_a_beta_claim_with_the_fold_table_rebuilt_from_it(vx, oracle):
    """query-free the verifier's own checks never use beta: the fold table's constraints or the balance must object"""
    g = I.group("fib8")
    j = 6  # two alphas, zeta, alpha; then beta_0
    assert [g["chals"][j][1], g["chals"][j + 1][1]] == [int(v) for v in g["hd"]["betas"][0]]
    chals = list(g["chals"])
    chals[j] = (chals[j][0], (chals[j][1] + 1) % P)
    hd = dict(g["hd"], betas=[[chals[j][1], chals[j + 1][1]]] + [list(b) for b in g["hd"]["betas"][1:]])
    blob, bad, balanced = _forged_blob(g, chals=chals, hd=hd)
    assert not balanced
    if bad is not None:  # the fold table itself breaks a rule under the other beta: it has no proof
        assert bad[0] == len(g["tabs"]) - 2
        return
    _both_forms(vx, g, blob, "does not balance")


@pytest.mark.parametrize("name", list(I.INNER))
def test_the_proof_bound_on_the_head_alone_is_the_blob_size(vx, oracle, name):
    g = I.group(name)
    cfg, L = pcfg(vx, g["cfg"]), vx.lib.load_library()
    ext = None if g["ext"] is None else np.array(g["ext"], dtype=np.uint64)
    for p in (g["proof"], g["proof"][:g["hd"]["o_queries"]], Z.garbled(g["proof"], g["hd"])):
        p = np.ascontiguousarray(p, dtype=np.uint64)
        need = C.c_size_t(0)
        assert L.vx_stark_inner_proof_bound(C.byref(cfg), p.ctypes.data, p.size, None if ext is None else ext.ctypes.data, C.byref(need)) == 0
        assert need.value == g["blob"].size
    need = C.c_size_t(0)
    p = np.ascontiguousarray(g["proof"][:g["hd"]["o_queries"] - 1])
    assert L.vx_stark_inner_proof_bound(C.byref(cfg), p.ctypes.data, p.size, None, C.byref(need)) == ERR_ARG
