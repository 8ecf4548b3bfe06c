"""Declared bus messages of a run-time AIR on the GPU (k_bus_aux_prog, the interpreter of a message program): the auxiliary round of a
restated table equals the compiled table's kernel WORD FOR WORD (a field element has one canonical word: nothing here takes a
tolerance) and the plain-Python generators of tests/*_ref.py, a made-up table equals a big-integer computation, proofs under the
registered id are the compiled table's proofs except for the id word, and a false statement proves nothing."""
import numpy as np
import pytest

import bus_programs as BP
import fri_fold_ref as F
import leaf_noop_ref as N
import merkle_open_ref as M
import transcript_ref as T

P = BP.P
CHAL = BP.CHAL  # fixed canonical words, two of them close to P

pytestmark = pytest.mark.gpu

_ids = {}


def prog_id(name):
    """the restatement `name` of bus_programs.py, registered once for the module"""
    if name not in _ids:
        _ids[name] = getattr(BP, name)().register()
    return _ids[name]


def openings(n, seed=11):
    """n openings: every length in turn, three trees, a duplicate"""
    rng = np.random.default_rng(seed + n)
    rows = [[int(v) for v in rng.integers(0, P, size=1 + (i + seed) % 4, dtype=np.uint64)] for i in range(n)]
    trees, index = [8 + i % 3 for i in range(n)], [int(v) for v in rng.integers(0, 1 << 24, size=n)]
    trees[3], index[3], rows[3] = trees[0], index[0], list(rows[0])
    return trees, index, rows


def leaf_noop_table(ctx, vx, n_idx, log_n):
    tb, pub = ctx.leaf_noop_air_trace(*openings(n_idx), log_n)
    return tb, pub, vx.lib.VX_AIR_LEAF_NOOP, N.AUX, N


def transcript_table(ctx, vx, chains, log_n):
    tb, pub, _ = ctx.transcript_air_trace([ops for ops, _ in chains], [w for _, w in chains], log_n)
    return tb, pub, vx.lib.VX_AIR_TRANSCRIPT, T.AUX, T


def fri_fold_table(ctx, vx):
    """LN 9, one layer: a query is one fold row, the bit row that sends the exit and four bit rows with no message; 13 queries in 2^7 rows"""
    LN, NL, log_n, tree0 = 9, 1, 7, 3
    rng = np.random.default_rng(LN * 16 + NL)
    index = [int(v) for v in rng.integers(0, 1 << LN, size=80 // (LN - 3 * NL))]
    betas = [[int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)] for _ in range(NL)]
    leaves = np.array([F.chain_leaves(i, rng.integers(0, P, size=(NL, 16, 2), dtype=np.uint64), betas, LN) for i in index], dtype=np.uint64)
    tb, pub = ctx.fri_fold_air_trace(LN, betas, index, F.ev0_of(index, leaves), leaves, log_n, tree0)
    return tb, pub, vx.lib.VX_AIR_FRI_FOLD, F.AUX, F


def merkle_open_table(ctx, vx, D, cap_height, idx, log_n):
    leaves = np.random.default_rng(3 + 10 * D).integers(0, P, size=(1 << D, 8), dtype=np.uint64)
    tree = ctx.merkle(ctx.from_host(leaves), 1 << D, 8, vx.lib.VX_LEAVES_ROW_MAJOR, cap_height)
    tb, pub = ctx.merkle_open_air_trace(tree, idx, log_n)
    tree.free()
    return tb, pub, vx.lib.VX_AIR_MERKLE_OPEN, 4, M


# name -> (restatement, table maker, compare with the plain-Python gen_aux of the *_ref.py too)
TABLES = {
    # one helper set per row: fewer lanes than a workgroup, then several workgroups with idle rows behind the openings
    "leaf_noop_20_of_32": ("leaf_noop", lambda ctx, vx: leaf_noop_table(ctx, vx, 20, 5), True),
    "leaf_noop_300_of_512": ("leaf_noop", lambda ctx, vx: leaf_noop_table(ctx, vx, 300, 9), False),
    # one helper set per 32-row block and a step column: one lane, then a full workgroup and one lane of a second, idle blocks behind
    "transcript_one_block": ("transcript", lambda ctx, vx: transcript_table(ctx, vx, T.synth_chains(["one_block"]), 5), True),
    "transcript_65_of_128_blocks": ("transcript", lambda ctx, vx: transcript_table(ctx, vx, [T.filler(65)], 12), False),
    # 17 helpers, a public input read by the messages, rows without a message inside the active part
    "fri_fold_tree0_3": ("fri_fold", fri_fold_table, False),
    # one helper
    "merkle_open_one_block": ("merkle_open", lambda ctx, vx: merkle_open_table(ctx, vx, 1, 0, [1], 5), False),
    "merkle_open_70_of_128_blocks": ("merkle_open", lambda ctx, vx: merkle_open_table(ctx, vx, 5, 2, [0, 31, 31, 17, 5, 9, 22, 1, 16, 30, 2, 13, 8, 27], 12), False),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_the_auxiliary_round_equals_the_compiled_tables(ctx, vx, oracle, name):
    restated, make, with_ref = TABLES[name]
    tb, pub, compiled, aux_cols, R = make(ctx, vx)
    log_n = (tb.n // R.COLS).bit_length() - 1
    assert R.COLS << log_n == tb.n
    want_b, want_apub = ctx.stark_aux_trace(compiled, tb, log_n, CHAL, aux_cols, pub)
    got_b, got_apub = ctx.stark_aux_trace(prog_id(restated), tb, log_n, CHAL, aux_cols, pub)
    want, got = want_b.download().reshape(aux_cols, -1), got_b.download().reshape(aux_cols, -1)
    assert want[:-2].any() and want[-2:].any()  # the table has messages
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in got_apub] == [int(v) for v in want_apub] and (int(got_apub[0]) or int(got_apub[1]))
    if with_ref:
        trace = tb.download().reshape(R.COLS, -1)
        ref_aux, ref_apub = R.gen_aux(trace, CHAL, [int(v) for v in pub])
        assert (got == ref_aux).all() and [int(v) for v in got_apub[:2]] == ref_apub
    tb.free(), want_b.free(), got_b.free()


@pytest.mark.parametrize("log_n", [4, 7])
def test_a_made_up_table_equals_a_big_integer_computation(ctx, vx, oracle, log_n):
    """three messages (an odd count), a slot left unset, tag 0 and a tag above 13, idle rows, and on row 1 a pair of messages on one
    tuple with multiplicities +1 and -1: the helper is zero while both multiplicities are not; 16 rows (a quarter of a wave) and 128
    (two workgroups)"""
    tr, pub = BP.made_up_trace(log_n), [P - 7]
    n = tr.shape[1]
    want, want_apub = BP.aux_of_messages(lambda row: BP.made_up_messages(tr[:, row], pub), n, CHAL)
    assert want.shape[0] == 6 and not want[:4, 0].any() and not want[:2, 1].any() and not want[:2, 2].any() and want[2:4, 2].any()
    tb = ctx.from_host(tr)
    got_b, got_apub = ctx.stark_aux_trace(prog_id("made_up"), tb, log_n, CHAL, 6, pub)
    got = got_b.download().reshape(6, -1)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in got_apub[:2]] == want_apub
    tb.free(), got_b.free()


PROOFS = {"leaf_noop_rate_1": ("leaf_noop", lambda ctx, vx: leaf_noop_table(ctx, vx, 37, 6), 1),
          "leaf_noop_rate_2": ("leaf_noop", lambda ctx, vx: leaf_noop_table(ctx, vx, 37, 6), 2),
          "transcript_rate_1": ("transcript", lambda ctx, vx: transcript_table(ctx, vx, T.synth_chains(["draw_9", "one_block"]), 8), 1)}


@pytest.mark.parametrize("name", list(PROOFS))
def test_the_proof_is_the_compiled_tables_proof(ctx, vx, oracle, name):
    restated, make, rate_bits = PROOFS[name]
    tb, pub, compiled, _, R = make(ctx, vx)
    log_n = (tb.n // R.COLS).bit_length() - 1
    cfg = ctx.stark_config(num_queries=8, rate_bits=rate_bits)
    want = ctx.stark_prove(compiled, tb, log_n, pub, cfg)
    got = ctx.stark_prove(prog_id(restated), tb, log_n, pub, cfg)
    assert int(want[1]) == compiled and int(got[1]) == prog_id(restated) and got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.tolist() == [1], "differing words of the proof: %s" % bad[:4]
    # the host verifier accepts it: the one check a table alone on its bus cannot pass is the last one (tests/test_gpu_leaf_noop.py)
    with pytest.raises(vx.VxError, match="stand-alone proof publishes a non-zero bus total"):
        vx.lib.stark_verify(got, cfg, expect_air=prog_id(restated), expect_public=pub)
    tb.free()


def test_a_false_statement_proves_nothing(ctx, vx, oracle):
    """one multiplicity cell raised by one (a flag of opening 0): whatever the prover makes of it, the verifier does not get as far as
    the last check"""
    trees, index, rows = openings(20)
    trace, pub = N.ref_trace(trees, index, rows, 5)
    assert int(trace[N.E + 1, 0]) in (0, 1)
    trace[N.E + 1, 0] += 1
    cfg = ctx.stark_config(num_queries=8)
    tb = ctx.from_host(trace)
    try:
        proof = ctx.stark_prove(prog_id("leaf_noop"), tb, 5, pub, cfg)
    except vx.VxError:
        proof = None
    if proof is not None:
        with pytest.raises(vx.VxError) as e:
            vx.lib.stark_verify(proof, cfg, expect_air=prog_id("leaf_noop"), expect_public=pub)
        assert "non-zero bus total" not in str(e.value)
    tb.free()


def test_argument_errors(ctx, vx, oracle):
    trees, index, rows = openings(20)
    tb, pub = ctx.leaf_noop_air_trace(trees, index, rows, 5)
    short = ctx.alloc(N.COLS << 4)
    with pytest.raises(vx.VxError) as e:
        ctx.stark_prove(prog_id("leaf_noop"), short, 5, pub)  # a buffer of the wrong length
    assert e.value.code == -1  # VX_ERR_ARG
    with pytest.raises(vx.VxError) as e:
        ctx.stark_aux_trace(prog_id("leaf_noop"), short, 5, CHAL, N.AUX, pub)
    assert e.value.code == -1
    with pytest.raises(vx.VxError) as e:
        ctx.stark_aux_trace(prog_id("transcript"), ctx.alloc(T.COLS << 4), 4, CHAL, T.AUX, [1, 2, 3, 4])  # less than one block
    assert e.value.code == -1
    # auxiliary columns, no bus and no callback: still "verified, not proven"
    verifier_only = N.builder().register()
    with pytest.raises(vx.VxError, match="gen_aux"):
        ctx.stark_prove(verifier_only, tb, 5, pub)
    with pytest.raises(vx.VxError, match="no generator"):
        ctx.stark_aux_trace(verifier_only, tb, 5, CHAL, N.AUX, pub)
    vx.lib.air_unregister(verifier_only)
    got_b, _ = ctx.stark_aux_trace(prog_id("leaf_noop"), tb, 5, CHAL, N.AUX, pub)  # after the refusals the context goes on working
    assert got_b.download().any()
    tb.free(), short.free(), got_b.free()
