"""TranscriptAir (AIR id 23) on the GPU: the witness, the auxiliary columns, the public inputs and the returned challenges equal the
reference generator cell by cell -- the synthetic chains of every challenger branch, 64 and 65 blocks (a wave boundary of the
lane-per-block kernels), 16 and 17 chains (a block boundary of the group-per-chain kernel), tables that are exactly full --, one
block over a full table is refused, the table's STARK equals the reference prover's on the restatement word for word, and
vx_stark_transcripts_prove on vx_stark_prove proofs equals the reference group's blob word for word and passes the product verifier
with whole proofs and with heads.  The LookupAir proof under EXTERNAL lookup challenges is the reference prover's: the binding has
no entry point that proves AIR 5 under given challenges, and the two provers' proofs are equal word for word (test_gpu_stark.py)."""
import numpy as np
import pytest

import transcript_ref as T
from oracle import stark_ref as S

P = T.P
CHAL = T.CHAL

pytestmark = pytest.mark.gpu


def many(n_chains, blocks_each):
    """n_chains chains of blocks_each[c % len] blocks"""
    return [T.filler(blocks_each[c % len(blocks_each)], seed=50 + c) for c in range(n_chains)]


# name -> (chains [(ops, words)], log_n or None: the smallest)
WITNESS = {
    "one_block_full_32": (T.synth_chains(["one_block"]), 5),
    "three_chains": (T.synth_chains(["draw_17", "one_block", "interleaved"]), None),
    "every_branch": (T.synth_chains(list(T.SYNTH)), None),
    "full_64_two_chains": (T.synth_chains(["absorbed_8_then_1", "one_block"]), 6),
    "blocks_64": (many(4, [30, 2, 31, 1]), 12),
    "blocks_65": (many(4, [30, 2, 31, 2]), 12),
    "chains_16": (many(16, [1, 3, 2]), None),
    "chains_17": (many(17, [1, 3, 2]), None),
    "chains_64": (many(64, [1]), 11),
}


@pytest.mark.parametrize("name", list(WITNESS))
def test_witness_equals_the_reference(ctx, vx, oracle, name):
    chains, log_n = WITNESS[name]
    want, want_pub, claims = T.ref_table(chains, log_n)
    log_n = want.shape[1].bit_length() - 1
    if "full" in name:
        assert int(want[T.ACT].sum()) == want.shape[1]
    tb, pub, chal = ctx.transcript_air_trace([ops for ops, _ in chains], [w for _, w in chains], log_n)
    assert [[int(v) for v in c] for c in chal] == [[v for _, v in chals] for _, chals in claims]
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(T.COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_TRANSCRIPT, tb, log_n, CHAL, vx.lib.VX_TRANSCRIPT_AIR_AUX_COLS, pub)
    want_aux, want_apub = T.gen_aux(want, CHAL, want_pub)
    bad = np.argwhere(ab.download().reshape(T.AUX, -1) != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    tb.free(), ab.free()


@pytest.mark.parametrize("log_n", [5, 6])
def test_one_block_over_is_refused(ctx, vx, oracle, log_n):
    full = 1 << (log_n - 5)
    ops, words = T.filler(full + 1)
    with pytest.raises(vx.VxError, match="do not fit") as e:
        ctx.transcript_air_trace([ops], [words], log_n)
    assert e.value.code == -1  # VX_ERR_ARG
    ops, words = T.filler(full)  # the context goes on working
    tb, _, chal = ctx.transcript_air_trace([ops], [words], log_n)
    assert int(tb.download().reshape(T.COLS, -1)[T.ACT].sum()) == 1 << log_n
    assert [int(v) for v in chal[0]] == [v for _, v in T.chain_blocks(0, ops, words)[1]]
    tb.free()


def test_argument_errors(ctx, vx, oracle):
    ops, words = T.SYNTH["one_block"], T.synth_words(T.SYNTH["one_block"], 1)
    for call in (lambda: ctx.transcript_air_trace([ops], [[P] + words[1:]], 5),            # a non-canonical word
                 lambda: ctx.transcript_air_trace([ops] * 65, [words] * 65, 12),           # more than 64 chains
                 lambda: ctx.transcript_air_trace([], [], 5),                              # no chain
                 lambda: ctx.transcript_air_trace([[0, 1, 3, 1]], [words], 5),             # the first operation draws from an empty sponge
                 lambda: ctx.transcript_air_trace([[3]], [words], 5),                      # words no duplex absorbs
                 lambda: ctx.transcript_air_trace([[0, 0]], [[]], 5),                      # an empty chain
                 lambda: ctx.transcript_air_trace([ops], [words], 4),                      # fewer than 2^5 rows
                 lambda: ctx.transcript_air_trace([ops], [words], 6, out=ctx.alloc(T.COLS << 5))):  # a buffer that is too small
        with pytest.raises(vx.VxError) as e:
            call()
        assert e.value.code == -1  # VX_ERR_ARG
    tb, pub, _ = ctx.transcript_air_trace([ops], [words], 5)  # after the refusals the context makes the same table
    want, want_pub, _ = T.ref_table([(ops, words)], 5)
    assert [int(v) for v in pub] == want_pub and (tb.download().reshape(T.COLS, -1) == want).all()
    tb.free()


def test_the_table_proof_equals_the_reference_prover(ctx, vx, oracle):
    """the compiled constraints are the restated ones: the same trace proven by both provers gives the same words"""
    chains = T.synth_chains(["draw_17", "one_block", "interleaved"])
    trace, pub, _ = T.ref_table(chains)
    log_n = trace.shape[1].bit_length() - 1
    tb, gpub, _ = ctx.transcript_air_trace([ops for ops, _ in chains], [w for _, w in chains], log_n)
    over = dict(num_queries=8)
    got = ctx.stark_prove(vx.lib.VX_AIR_TRANSCRIPT, tb, log_n, gpub, ctx.stark_config(**over))
    want = np.array(S.prove(T.air(), trace, pub, dict(S.DEFAULT_CFG, **over)), dtype=np.uint64)
    assert int(got[1]) == T.AIR_ID and int(want[1]) == T.REF_ID and got.size == want.size
    got[1] = T.REF_ID
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing word of the proof: %d" % bad[0]
    got[1] = T.AIR_ID
    with pytest.raises(vx.VxError, match="stand-alone proof publishes a non-zero bus total"):
        vx.lib.stark_verify(got, ctx.stark_config(**over), expect_air=vx.lib.VX_AIR_TRANSCRIPT, expect_public=pub)
    tb.free()


# ---- the group on real inner proofs
EXT = [5, P - 6, 7, 1 << 40]
_made = {}


def inner(ctx, kind, rate_bits):
    """-> (inner proof, external lookup challenges or None)"""
    key = (kind, rate_bits)
    if key not in _made:
        over = dict(num_queries=5, rate_bits=rate_bits)
        air = S.FibAir if kind == "fib" else S.LookupAir
        trace, pub = air.trace(8)
        if kind == "lookup_ext":
            _made[key] = (np.array(S.prove(air, trace, pub, dict(S.DEFAULT_CFG, **over), chal_hook=lambda p, cap: EXT), dtype=np.uint64), EXT)
        else:
            _made[key] = (ctx.stark_prove(air.ID, ctx.from_host(trace), 8, pub, ctx.stark_config(**over)), None)
    return _made[key]


@pytest.mark.parametrize("rate_bits", [1, 2])
@pytest.mark.parametrize("kinds", [("fib",), ("lookup",), ("lookup_ext",), ("fib", "lookup", "lookup_ext")], ids="+".join)
def test_group_blob_equals_the_reference_group(ctx, vx, oracle, kinds, rate_bits):
    over = dict(num_queries=5, rate_bits=rate_bits)
    cfg, rcfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    ins = [inner(ctx, k, rate_bits) for k in kinds]
    proofs, exts = [p for p, _ in ins], [e for _, e in ins]
    want = T.group(proofs, rcfg, exts)
    got = ctx.stark_transcripts_prove(proofs, cfg, exts)
    assert got.size == want["blob"].size
    bad = np.flatnonzero(got != want["blob"])
    assert bad.size == 0, "first differing word of the blob: %d" % bad[0]
    heads = [vx.lib.stark_proof_head(p, cfg) for p in proofs]
    vx.lib.stark_transcripts_verify(got, proofs, cfg, exts)
    vx.lib.stark_transcripts_verify(got, heads, cfg, exts)
    if len(kinds) == 1:  # proven from the head alone: the same blob
        assert (ctx.stark_transcripts_prove(heads, cfg, exts) == got).all()


def test_a_false_statement_proves_nothing(ctx, vx, oracle):
    proof, _ = inner(ctx, "fib", 1)
    cfg = ctx.stark_config(num_queries=5)
    head = vx.lib.stark_proof_head(proof, cfg)
    bad = proof.copy()
    bad[head.size - 2] ^= 1  # a word of the final polynomial
    out = np.zeros(1 << 16, dtype=np.uint64)
    with pytest.raises(vx.VxError, match="proof 1") as e:
        ctx.stark_transcripts_prove([proof, bad], cfg, out=out)
    assert e.value.code == -5 and not out.any()  # VX_ERR_STATEMENT, nothing written
    got = ctx.stark_transcripts_prove([proof], cfg)  # the context goes on working
    vx.lib.stark_transcripts_verify(got, [proof], cfg)
