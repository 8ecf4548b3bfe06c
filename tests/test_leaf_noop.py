"""LeafNoopAir (AIR id 22) without a GPU: the restated AIR has degree 3, the reference witness satisfies it for leaves of 1, 2, 3 and
4 words mixed in one table, its total is what MerkleOpenSetAir sends and FriCombineAir receives for those openings, forged rows
violate the rule that names them, a row with another word unbalances the bus, and the compiled AIR (the product's host verifier)
accepts the constraint identity of a reference-prover proof of the restatement.  Everything is exact."""
import numpy as np
import pytest

import leaf_noop_ref as N
from oracle import stark_ref as S

P = N.P
CHAL = N.CHAL
CFG = dict(S.DEFAULT_CFG, num_queries=8)

# leaves of every length, two trees, one duplicate opening, a zero word inside a row
TREES = [8, 10, 10, 9, 8, 10, 8]
INDEX = [5, 5, 300, 0, 5, (1 << 40) - 1, 77]
ROWS = [[3, P - 1], [1, 2, 3, 4], [P - 2, 0, 7, 9], [6], [3, P - 1], [11, 12, 13], [0, 0]]


def rule_of(k):
    """the name of the rule constraint k belongs to"""
    N.builder()
    return max((first, name) for name, first in N.RULES.items() if first <= k)[1]


def test_every_constraint_has_degree_at_most_3():
    b = N.builder()
    worst = max(N.degree(e) for _, e in b.constraints)
    assert worst == 3


def test_reference_trace_satisfies_the_restated_air(oracle):
    trace, pub = N.ref_trace(TREES, INDEX, ROWS)
    assert trace.shape == (N.COLS, 32) and pub == N.claims_digest(TREES, INDEX, ROWS)
    assert int(trace[N.ACT].sum()) == len(ROWS) and [int(trace[N.E:N.E + 4, i].sum()) for i in range(len(ROWS))] == [len(r) for r in ROWS]
    assert not trace[:, len(ROWS):].any()  # idle rows are all zero
    aux, apub = N.gen_aux(trace, CHAL, pub)
    assert S.check_trace(N.air(), trace, pub, CHAL, aux, apub) is None
    # every word of every row sent once, the two halves of every digest received
    tot = S.ExtS(0)
    for t, i, r in zip(TREES, INDEX, ROWS):
        tot = tot + N.opening_sum(CHAL, t, i, r)
    assert S.ExtS(*apub) * trace.shape[1] == tot


def test_a_full_table_wraps_around(oracle):
    rng = np.random.default_rng(4)
    rows = [[int(v) for v in rng.integers(0, P, size=1 + i % 4, dtype=np.uint64)] for i in range(32)]
    trees, index = [8 + i % 3 for i in range(32)], [int(v) for v in rng.integers(0, 1 << 20, size=32)]
    trace, pub = N.ref_trace(trees, index, rows)
    assert trace.shape[1] == 32 and int(trace[N.ACT].sum()) == 32
    aux, apub = N.gen_aux(trace, CHAL, pub)
    assert S.check_trace(N.air(), trace, pub, CHAL, aux, apub) is None


# a forged row in place of opening 0 (two words): (cells changed, the rule that must refuse it)
FORGERIES = {
    "word_behind_the_length": (dict(words=[3, P - 1, 5, 0]), "zero_behind_the_length"),
    "last_word_behind_the_length": (dict(words=[3, P - 1, 0, 1]), "zero_behind_the_length"),
    "gap_in_the_flags": (dict(flags=[1, 0, 1, 0], words=[3, 0, 5, 0]), "no_gap"),
    "gap_before_the_last_flag": (dict(flags=[1, 1, 0, 1], words=[3, P - 1, 0, 4]), "no_gap"),
    "first_flag_off": (dict(flags=[0, 0, 0, 0], words=[0, 0, 0, 0]), "first_word_exists"),
    "flag_not_boolean": (dict(flags=[1, 2, 0, 0]), "boolean"),
}


@pytest.mark.parametrize("kind", list(FORGERIES))
def test_forged_rows_violate_the_rule_that_names_them(oracle, kind):
    change, want = FORGERIES[kind]
    rows = [N.opening_row(t, i, r) for t, i, r in zip(TREES, INDEX, ROWS)]
    rows[0] = N.opening_row(TREES[0], INDEX[0], ROWS[0], **change)
    trace = N.assemble(rows, 5)
    pub = N.claims_digest(TREES, INDEX, ROWS)
    aux, apub = N.gen_aux(trace, CHAL, pub)  # the helpers follow the forged cells: only the row rules can object
    bad = S.check_trace(N.air(), trace, pub, CHAL, aux, apub)
    assert bad is not None and bad[1] == 0 and rule_of(bad[0]) == want


def test_an_idle_row_with_a_flag_is_refused(oracle):
    """E_0 = ACT in both directions: a row that is no opening cannot send a word"""
    rows = [N.opening_row(t, i, r) for t, i, r in zip(TREES, INDEX, ROWS)]
    ghost = [0, 8, 5, 9, 0, 0, 0, 1, 0, 0, 0]
    trace = N.assemble(rows + [ghost], 5)
    pub = N.claims_digest(TREES, INDEX, ROWS)
    bus = N._bus(CHAL)
    aux, apub = N.gen_aux(trace, CHAL, pub)
    h = N.d_row(bus, 8, 5, 0, 9).inv()  # the helper a forger would need
    aux[2, len(rows)], aux[3, len(rows)] = h.a, h.b
    bad = S.check_trace(N.air(), trace, pub, CHAL, aux, apub)
    assert bad is not None and bad[1] == len(rows) and rule_of(bad[0]) == "first_word_exists"


def test_a_changed_word_unbalances_the_bus(oracle):
    """a row that satisfies every rule but holds another word answers another opening: what it receives is not what the openings
    table sends for the leaf digest the path proves"""
    forged = [list(r) for r in ROWS]
    forged[1][2] ^= 1
    trace, pub = N.ref_trace(TREES, INDEX, forged)
    aux, apub = N.gen_aux(trace, CHAL, pub)
    assert S.check_trace(N.air(), trace, pub, CHAL, aux, apub) is None
    bus = N._bus(CHAL)

    def others(words_seen):
        """the other parties: the openings sent for the true digests, the words the combination receives"""
        tot = S.ExtS(0)
        for t, i, r, seen in zip(TREES, INDEX, ROWS, words_seen):
            w = N.padded(r)
            tot = tot + N.d_open(bus, t, i, w[0], w[1], 0).inv() + N.d_open(bus, t, i, w[2], w[3], 1).inv()
            for j, v in enumerate(seen):
                tot = tot - N.d_row(bus, t, i, j, v).inv()
        return tot

    assert not (S.ExtS(*apub) * trace.shape[1] + others(forged) == S.ExtS(0))
    assert not (S.ExtS(*apub) * trace.shape[1] + others(ROWS) == S.ExtS(0))
    trace, pub = N.ref_trace(TREES, INDEX, ROWS)  # the honest table balances against the same parties
    aux, apub = N.gen_aux(trace, CHAL, pub)
    assert S.ExtS(*apub) * trace.shape[1] + others(ROWS) == S.ExtS(0)


def test_the_compiled_air_accepts_a_reference_proof(vx, oracle):
    """the product's host verifier runs the COMPILED constraints at zeta.  A table alone has nobody to cancel its total against, so
    the last check of a stand-alone verification refuses it -- after the constraint identity, the proof of work and the whole query
    phase have passed; with one opening word changed in the proof the identity itself fails"""
    trace, pub = N.ref_trace(TREES, INDEX, ROWS)
    proof = np.array(S.prove(N.air(), trace, pub, CFG), dtype=np.uint64)
    proof[1] = N.AIR_ID
    cfg = vx.lib.default_stark_config(num_queries=CFG["num_queries"])
    with pytest.raises(vx.VxError, match="stand-alone proof publishes a non-zero bus total"):
        vx.lib.stark_verify(proof, cfg, expect_air=vx.lib.VX_AIR_LEAF_NOOP, expect_public=pub)
    cap_words = 4 << CFG["cap_height"]
    o_local = 12 + int(proof[9]) + N.PUB + cap_words + 2 + cap_words + cap_words  # header, public inputs, cap, total, two caps
    bad = proof.copy()
    bad[o_local + 2 * N.W] ^= 1  # the opening of W_0 at zeta
    with pytest.raises(vx.VxError, match="constraint identity fails at zeta"):
        vx.lib.stark_verify(bad, cfg, expect_air=vx.lib.VX_AIR_LEAF_NOOP)
    with pytest.raises(vx.VxError):  # the proof is of no other table
        vx.lib.stark_verify(proof, cfg, expect_air=vx.lib.VX_AIR_LEAF_SPONGE_SET)
