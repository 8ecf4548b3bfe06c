"""The order of the answers of the deferred verifier, without a GPU: vx_stark_verify_deferred runs the code of the _dev verifiers --
the whole proof scanned for non-canonical words, the host pass with the Merkle openings recorded instead of walked, the recorded
openings checked afterwards, the first failing one winning over the pass's own refusal -- with the host's path check in place of the
kernel.  On the reference prover's proofs it must answer as lib.stark_verify does, code and message: for the proofs themselves, for
a sample of single-word corruptions over every kind of word, for two defects in different queries (which an implementation that
checked paths only after a clean host pass gets wrong), for truncated proofs and for a wrong expect_air."""
import numpy as np
import pytest

import verify_dev_cases as V

ERR_STATEMENT = -5


def both(vx, words, cfg, **kw):
    want = V.answer(vx.lib.stark_verify, words, cfg, **kw)
    assert V.answer(vx.lib.stark_verify_deferred, words, cfg, **kw) == want
    return want


@pytest.mark.parametrize("name", list(V.CASES))
def test_reference_proofs_are_accepted(vx, oracle, name):
    proof, cfg, air = V.case(name)
    lay = V.layout(proof)
    assert lay["n_layers"] == dict(fib5=0, lookup8=1, fib8_two_layers_cap0=2)[name] and ("row_a" in lay["queries"][0]) == (name == "lookup8")
    assert both(vx, proof, V.pcfg(vx, cfg)) == (0, "")
    assert both(vx, proof, V.pcfg(vx, cfg), expect_air=air.ID, expect_public=proof[12 + lay["n_layers"]:lay["regions"]["caps"][0][0]][:air.PUB]) == (0, "")


def test_single_word_corruptions_answer_as_the_host_verifier(vx, oracle):
    n, seen = 0, set()
    for name in V.CASES:
        proof, cfg, _ = V.case(name)
        c = V.pcfg(vx, cfg)
        for what, bad in V.sample(proof):
            code, msg = both(vx, bad, c)
            assert code != 0, (name, what)
            seen.add(msg.split("(")[0].rstrip("0123456789 "))
            n += 1
    assert n >= 200, n
    # the sample is not one refusal two hundred times: it meets the head's checks, the scan, the identity at zeta, the paths of
    # every kind of tree and the final polynomial
    for part in ("config mismatch", "non-canonical element at word", "constraint identity fails at zeta", "trace Merkle proof invalid", "auxiliary Merkle proof invalid",
                 "quotient Merkle proof invalid", "FRI layer 0 Merkle proof invalid", "FRI layer 1 Merkle proof invalid", "proof of work invalid"):
        assert any(part in s for s in seen), (part, sorted(seen))


@pytest.mark.parametrize("name", list(V.CASES))
def test_two_defects_name_the_one_the_walked_verifier_meets_first(vx, oracle, name):
    proof, cfg, _ = V.case(name)
    c, q = V.pcfg(vx, cfg), V.layout(proof)["queries"]
    # a corrupted trace-row word in query 1 (the pass stops at query 1's final polynomial) and a corrupted sibling in query 2
    bad = proof.copy()
    bad[q[1]["row_t"][0]] ^= np.uint64(1)
    bad[q[2]["sib_q"][0]] ^= np.uint64(1)
    code, msg = both(vx, bad, c)
    assert code == ERR_STATEMENT and "trace Merkle proof invalid (query 1)" in msg
    # the other way round: the pass stops at query 2, the path of query 1 was met before
    bad = proof.copy()
    bad[q[1]["sib_q"][1] - 1] ^= np.uint64(1 << 7)
    bad[q[2]["row_t"][0]] ^= np.uint64(1)
    code, msg = both(vx, bad, c)
    assert code == ERR_STATEMENT and "quotient Merkle proof invalid (query 1)" in msg
    # ... and with a layer's path in an earlier query still (where the layer's tree has a level below its cap)
    if "sibs0" not in q[0]:  # no fold layer (fib5): the final polynomial is the whole codeword
        return
    if q[0]["sibs0"][1] > q[0]["sibs0"][0]:
        bad[q[0]["sibs0"][0]] ^= np.uint64(1)
        code, msg = both(vx, bad, c)
        assert code == ERR_STATEMENT and "FRI layer 0 Merkle proof invalid (query 0)" in msg
    # a defect of the pass in an earlier query than the path's: the pass's own answer stands
    bad = proof.copy()
    bad[q[0]["evals0"][0]] ^= np.uint64(1)
    bad[q[1]["sib_t"][0]] ^= np.uint64(1)
    code, msg = both(vx, bad, c)
    assert code == ERR_STATEMENT and "(query 0)" in msg


@pytest.mark.parametrize("name", list(V.CASES))
def test_truncated_proofs_and_a_wrong_air(vx, oracle, name):
    proof, cfg, air = V.case(name)
    c, lay = V.pcfg(vx, cfg), V.layout(proof)
    cuts = [0, 1, 9, 10, 12, lay["regions"]["caps"][0][0], lay["o_queries"] - 1, lay["o_queries"], lay["o_queries"] + 1, lay["queries"][1]["row_t"][0], proof.size - 1]
    for cut in cuts:
        code, _ = both(vx, proof[:cut] if cut else np.zeros(1, dtype=np.uint64), c)
        assert code != 0, cut
    assert both(vx, np.concatenate([proof, proof[-1:]]), c)[0] != 0
    code, msg = both(vx, proof, c, expect_air=air.ID + 1)
    assert code == ERR_STATEMENT and "unexpected AIR" in msg
    if air.PUB:
        pub = proof[12 + lay["n_layers"]:][:air.PUB].copy()
        pub[0] ^= np.uint64(1)
        assert "public input 0 differs" in both(vx, proof, c, expect_public=pub)[1]
    assert "public input count differs" in both(vx, proof, c, expect_public=np.zeros(air.PUB + 1, dtype=np.uint64))[1]
    other = V.pcfg(vx, dict(cfg, num_queries=cfg["num_queries"] + 1))
    assert "config mismatch" in both(vx, proof, other)[1]
