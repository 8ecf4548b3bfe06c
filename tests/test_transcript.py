"""TranscriptAir (AIR id 23) and the transcripts group without a GPU: the restated AIR has degree 3; the block plans of synthetic chains
that hit every branch of the duplex challenger equal a direct simulation of it, their reference tables satisfy the AIR and balance
against the outside party; reference-prover groups over real inner proofs (tests/transcript_ref.py records the transcript from
oracle/stark_ref.py's own verifier) are judged by the product's vx_stark_transcripts_verify, with the whole proof and with its head
alone; every change to the blob's claims, to its length and to the head is refused; forged tables violate the rule that names them
or are proven by the reference prover and refused at the balance; and the compiled AIR accepts the constraint identity of a
reference proof of the restatement.  Everything is exact."""
import numpy as np
import pytest

import transcript_ref as T
from oracle import pyref
from oracle import stark_ref as S

P = T.P
CHAL = T.CHAL
ERR_STATEMENT = -5


def test_every_constraint_has_degree_at_most_3():
    b = T.builder()
    assert max(T.degree(e) for _, e in b.constraints) == 3


# ---- the plan against a direct simulation of the challenger (plonky2 iop/challenger.rs, as glh::Challenger states it)
class DirectChallenger:
    def __init__(self):
        self.st, self.inp, self.out, self.duplexes, self.drawn, self.n_obs = [0] * 12, [], [], [], [], 0

    def duplex(self):
        self.duplexes.append([len(self.inp), 0])
        self.st[:len(self.inp)] = self.inp
        self.inp = []
        self.st = pyref.poseidon(self.st)
        self.out = list(self.st[:8])

    def observe(self, x):
        self.out = []
        self.inp.append(int(x))
        self.n_obs += 1
        if len(self.inp) == 8:
            self.duplex()

    def challenge(self):
        if self.inp or not self.out:
            self.duplex()
        self.duplexes[-1][1] += 1
        self.drawn.append((self.n_obs, self.out.pop()))
        return self.drawn[-1][1]


def simulate(ops, words):
    ch, pos = DirectChallenger(), 0
    for j, count in enumerate(ops):
        for _ in range(count):
            if j % 2:
                ch.challenge()
            else:
                ch.observe(words[pos])
                pos += 1
    return [tuple(d) for d in ch.duplexes], ch.drawn


@pytest.mark.parametrize("name", list(T.SYNTH))
def test_plans_equal_a_direct_challenger_simulation(oracle, name):
    (ops, words), = T.synth_chains([name])
    want_plan, want_drawn = simulate(ops, words)
    assert T.plan(ops) == want_plan
    blocks, chals = T.chain_blocks(0, ops, words)
    assert chals == want_drawn and len(blocks) == len(want_plan)
    # the three rules hold on every block, and the absorb-nothing block exists exactly where more than 8 challenges follow each other
    for k, q in want_plan:
        assert (k > 0 or q > 0) and (k == 8 or q > 0)
    assert any(k == 0 for k, _ in want_plan) == (name in ("draw_9", "draw_16", "draw_17"))


def test_the_branches_the_synthetic_chains_are_chosen_for():
    assert T.plan(T.SYNTH["absorbed_8_then_1"]) == [(8, 1)]            # absorbed = 0 mod 8: the challenge pops the full block's output
    assert T.plan(T.SYNTH["absorbed_9_then_1"]) == [(8, 0), (1, 1)]    # = 1 mod 8
    assert T.plan(T.SYNTH["one_block"]) == [(3, 2)]
    assert T.plan(T.SYNTH["draw_8"])[0] == (5, 8) and T.plan(T.SYNTH["draw_9"])[:2] == [(5, 8), (0, 1)]
    assert T.plan(T.SYNTH["draw_16"])[:4] == [(8, 0), (8, 8), (0, 8), (1, 1)]
    assert T.plan(T.SYNTH["draw_17"])[:3] == [(7, 8), (0, 8), (0, 1)]
    with pytest.raises(AssertionError, match="empty sponge"):
        T.plan([0, 1])
    with pytest.raises(AssertionError, match="no duplex absorbs"):
        T.plan([8, 1, 3])


# tables: one chain of one block (exactly full at 2^5 rows); three chains of different lengths; every synthetic chain in one table;
# chains of 1 + 2 + 1 blocks exactly full at 2^7 rows (the wrap-around meets a START)
TABLES = {
    "one_block_full_32": (["one_block"], 5),
    "three_chains": (["draw_17", "one_block", "interleaved"], None),
    "all": (list(T.SYNTH), None),
    "full_128": (["absorbed_8_then_1", "absorbed_9_then_1", "one_block"], 7),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_reference_tables_satisfy_the_restated_air(oracle, name):
    names, log_n = TABLES[name]
    chains = T.synth_chains(names)
    trace, pub, claims = T.ref_table(chains, log_n)
    n_blocks = sum(len(T.plan(ops)) for ops, _ in chains)
    assert int(trace[T.ACT].sum()) == 32 * n_blocks and int(trace[T.START].sum()) == 32 * len(chains)
    if name.startswith(("one_block_full", "full")):
        assert 32 * n_blocks == trace.shape[1]
    aux, apub = T.gen_aux(trace, CHAL, pub)
    assert S.check_trace(T.air(), trace, pub, CHAL, aux, apub) is None
    assert S.ExtS(*apub) * trace.shape[1] == T.outside_sum(CHAL, claims)


# ---- reference groups over real inner proofs, judged by the product verifier
EXT = [5, P - 6, 7, 1 << 40]
_made = {}


def inner(kind, num_queries=5):
    """-> (proof by the reference prover, reference configuration, external lookup challenges or None)"""
    key = (kind, num_queries)
    if key not in _made:
        rcfg = dict(S.DEFAULT_CFG, num_queries=num_queries)
        air = S.FibAir if kind == "fib" else S.LookupAir
        trace, pub = air.trace(8)
        ext = EXT if kind == "lookup_ext" else None
        proof = S.prove(air, trace, pub, rcfg, chal_hook=(lambda p, cap: ext) if ext else None)
        _made[key] = (np.array(proof, dtype=np.uint64), rcfg, ext)
    return _made[key]


def group_of(kinds, num_queries=5):
    key = (tuple(kinds), num_queries, "group")
    if key not in _made:
        ins = [inner(k, num_queries) for k in kinds]
        _made[key] = (T.group([p for p, _, _ in ins], ins[0][1], [e for _, _, e in ins]), [p for p, _, _ in ins], [e for _, _, e in ins])
    return _made[key]


def pcfg(vx, num_queries=5):
    return vx.lib.default_stark_config(num_queries=num_queries)


@pytest.mark.parametrize("kinds", [("fib",), ("lookup",), ("lookup_ext",), ("fib", "lookup", "lookup_ext")], ids="+".join)
def test_reference_groups_pass_the_product_verifier(vx, oracle, kinds):
    g, proofs, exts = group_of(kinds)
    cfg = pcfg(vx)
    vx.lib.stark_transcripts_verify(g["blob"], proofs, cfg, exts)
    heads = [vx.lib.stark_proof_head(p, cfg) for p in proofs]
    assert all(h.size < p.size for h, p in zip(heads, proofs))
    vx.lib.stark_transcripts_verify(g["blob"], heads, cfg, exts)
    # the product's own replay hands out the same claims
    for (words, chals), p, e in zip(g["claims"], proofs, exts):
        got_w, got_c = vx.lib.stark_transcript_claims(p, cfg, e)
        assert [int(v) for v in got_w] == words and [(int(a), int(v)) for a, v in got_c] == chals
    # the outside party's sum in Python equals the table's published total
    tot, rows = T.R.published_total(T.unwrap(g["blob"])[0], 4)
    chal = S.shared_challenges_n([S.proof_peek(T.unwrap(g["blob"])[0], 4)], 4)
    assert tot * rows == T.outside_sum(chal, g["claims"])


@pytest.mark.parametrize("num_queries", [8, 9, 17])
def test_query_counts_that_cross_a_block(vx, oracle, num_queries):
    """5 queries (above) pop from the proof-of-work block; with 8, 9 and 17 queries one, one and two blocks absorb nothing"""
    g, proofs, exts = group_of(("fib",), num_queries)
    ops = g["chains"][0][0]
    assert ops[-1] == num_queries + 1  # the proof-of-work response and the indices, drawn in a row
    assert sum(k == 0 for k, _ in T.plan(ops)) == num_queries // 8
    cfg = pcfg(vx, num_queries)
    vx.lib.stark_transcripts_verify(g["blob"], proofs, cfg)
    vx.lib.stark_transcripts_verify(g["blob"], [vx.lib.stark_proof_head(proofs[0], cfg)], cfg)


def refused(vx, blob, proofs, cfg, exts=None, match=None):
    with pytest.raises(vx.VxError, match=match) as e:
        vx.lib.stark_transcripts_verify(blob, proofs, cfg, exts)
    return e.value


def test_every_change_to_the_claims_and_the_length_is_refused(vx, oracle):
    g, proofs, exts = group_of(("fib", "lookup", "lookup_ext"))
    cfg, blob = pcfg(vx), g["blob"]
    _, o_proof = T.unwrap(blob)
    for at in range(o_proof):  # magic, n, per chain the two counts and every (absorbed, value), the table's length
        bad = blob.copy()
        bad[at] ^= 1
        refused(vx, bad, proofs, cfg, exts)
    bad = blob.copy()
    bad[5] = P  # a claimed value that is no field element
    refused(vx, bad, proofs, cfg, exts, "not canonical")
    for bad in (blob[:-1], np.concatenate([blob, blob[:1]]), blob[:o_proof], blob[:3]):
        refused(vx, bad, proofs, cfg, exts)
    bad = blob.copy()
    bad[o_proof + blob[o_proof:].size // 2] ^= 1  # a word inside the table's proof
    refused(vx, bad, proofs, cfg, exts)
    # the proofs in another order, one proof fewer, another proof of the same shape
    refused(vx, blob, [proofs[0], proofs[2], proofs[1]], cfg, [None, EXT, None])
    refused(vx, blob, proofs[:2], cfg, exts[:2], "different request")
    refused(vx, blob, proofs, cfg, [None, None, None])  # the third proof absorbed its external challenges
    trace, pub = S.FibAir.trace(8, 3, 5)
    other = np.array(S.prove(S.FibAir, trace, pub, inner("fib")[1]), dtype=np.uint64)
    assert refused(vx, blob, [other, proofs[1], proofs[2]], cfg, exts).code == ERR_STATEMENT


def test_every_change_to_a_head_word_is_refused(vx, oracle):
    g, proofs, _ = group_of(("fib",))
    cfg = pcfg(vx)
    head = vx.lib.stark_proof_head(proofs[0], cfg)
    for at in range(head.size):
        bad = head.copy()
        bad[at] ^= 1
        refused(vx, g["blob"], [bad], cfg)
    bad = proofs[0].copy()
    bad[head.size + 1] ^= 1  # a whole proof is walked: a query word is read
    refused(vx, g["blob"], [bad], cfg, match="chain 0")
    for n in (head.size - 1, head.size + 1, proofs[0].size - 1):
        refused(vx, g["blob"], [proofs[0][:n]], cfg, match="truncated")


# ---- forged groups over real inner proofs: chain 0 a FibAir proof, chain 1 another FibAir proof of the same shape
def _silent(specs, words):
    return specs[:2] + [dict(k=0, q=0)] + specs[2:], words


def _split_5_3(specs, words):
    at = next(i for i, sp in enumerate(specs) if i > 0 and sp["k"] == 8 and sp["q"] == 0)
    return specs[:at] + [dict(k=5, q=0), dict(k=3, q=0)] + specs[at + 1:], words


def _out_0_first(specs, words):
    at = next(i for i, sp in enumerate(specs) if 0 < sp["q"] < 8)
    return specs[:at] + [dict(specs[at], qmask=[int(i < specs[at]["q"]) for i in range(8)])] + specs[at + 1:], words


def _second_start(specs, words):
    return specs[:2] + [dict(specs[2], start=1)] + specs[3:], words


# name -> (what happens to chain 0, the rule that objects; None: every rule holds and the balance fails)
FORGED = {
    "silent_permutation": (_silent, "absorb_or_squeeze"),
    "absorbs_5_then_3": (_split_5_3, "partial_squeezes"),
    "popped_from_out_0": (_out_0_first, "q_suffix"),
    "second_start": (_second_start, None),
    "words_of_two_chains_swapped": (None, None),
}


def two_fibs():
    if "two_fibs" not in _made:
        p0, rcfg, _ = inner("fib")
        trace, pub = S.FibAir.trace(8, 3, 5)
        p1 = np.array(S.prove(S.FibAir, trace, pub, rcfg), dtype=np.uint64)
        _made["two_fibs"] = (T.group([p0, p1], rcfg), [p0, p1], rcfg)
    return _made["two_fibs"]


@pytest.mark.parametrize("kind", list(FORGED))
def test_forged_groups_violate_their_rule_or_miss_the_balance(vx, oracle, kind):
    g, proofs, rcfg = two_fibs()
    cfg = pcfg(vx)
    vx.lib.stark_transcripts_verify(g["blob"], proofs, cfg)
    forge, want = FORGED[kind]
    specs = [[dict(k=k, q=q) for k, q in T.plan(ops)] for ops, _ in g["chains"]]
    words = [list(w) for _, w in g["chains"]]
    assert specs[0] == specs[1] and words[0] != words[1]
    if forge is None:
        words = [words[1], words[0]]
    else:
        specs[0], words[0] = forge(specs[0], words[0])
    blocks = [b for c in range(2) for b in T.run_blocks(c, specs[c], words[c])[0]]
    log_n = g["trace"].shape[1].bit_length() - 1
    trace = T.assemble(blocks, log_n if want is None else log_n + 1)
    aux, apub = T.gen_aux(trace, CHAL, g["pub"])  # the helpers follow the forged cells: only the rules and the balance can object
    bad = S.check_trace(T.air(), trace, g["pub"], CHAL, aux, apub)
    if want is not None:  # (a trace that breaks a rule has no proof: the quotient is no polynomial)
        assert bad is not None and T.rule_of(bad[0]) == want
        return
    # every rule holds: the reference prover proves the forged table, the product verifier refuses it where the bus must balance
    assert bad is None and trace.shape == g["trace"].shape and (trace != g["trace"]).any()
    assert not (S.ExtS(*apub) * trace.shape[1] == T.outside_sum(CHAL, g["claims"]))
    blob = T.wrap(T.prove_table(trace, g["pub"], rcfg), g["claims"])
    assert refused(vx, blob, proofs, cfg, match="does not balance").code == ERR_STATEMENT
    assert refused(vx, blob, [vx.lib.stark_proof_head(p, cfg) for p in proofs], cfg, match="does not balance").code == ERR_STATEMENT


def test_the_compiled_air_accepts_a_reference_proof(vx, oracle):
    """the product's host verifier runs the COMPILED constraints at zeta.  A table alone has nobody to cancel its total against, so
    the last check of a stand-alone verification refuses it -- after the constraint identity, the proof of work and the whole query
    phase have passed; with one opening word changed in the proof the identity itself fails"""
    rcfg = dict(S.DEFAULT_CFG, num_queries=8)
    trace, pub, _ = T.ref_table(T.synth_chains(["draw_17", "one_block", "interleaved"]))
    proof = np.array(S.prove(T.air(), trace, pub, rcfg), dtype=np.uint64)
    proof[1] = T.AIR_ID
    cfg = pcfg(vx, 8)
    with pytest.raises(vx.VxError, match="stand-alone proof publishes a non-zero bus total"):
        vx.lib.stark_verify(proof, cfg, expect_air=vx.lib.VX_AIR_TRANSCRIPT, expect_public=pub)
    cap_words = 4 << rcfg["cap_height"]
    o_local = 12 + int(proof[9]) + T.PUB + cap_words + 2 + cap_words + cap_words  # header, public inputs, cap, total, two caps
    for col in (T.W + 3, T.NABS, T.PREV + 1):
        bad = proof.copy()
        bad[o_local + 2 * col] ^= 1
        with pytest.raises(vx.VxError, match="constraint identity fails at zeta"):
            vx.lib.stark_verify(bad, cfg, expect_air=vx.lib.VX_AIR_TRANSCRIPT)
    with pytest.raises(vx.VxError):  # the proof is of no other table
        vx.lib.stark_verify(proof, cfg, expect_air=vx.lib.VX_AIR_LEAF_SPONGE_SET)
