"""LeafNoopAir (AIR id 22) on the GPU: the witness, the auxiliary columns and the public inputs equal the reference generator cell by
cell -- one opening, 64 and 65 openings (across a wave boundary), tables that are exactly full --, one opening over is refused, the
table's STARK equals the reference prover's on the restatement word for word (the compiled constraints are the restated ones), and
openings outside the AIR's range are argument errors."""
import numpy as np
import pytest

import leaf_noop_ref as N
from oracle import stark_ref as S

P = N.P
CHAL = N.CHAL

pytestmark = pytest.mark.gpu


def openings(n, seed=11):
    """n openings: every length in turn, three trees, a duplicate when there is room for one"""
    rng = np.random.default_rng(seed + n)
    rows = [[int(v) for v in rng.integers(0, P, size=1 + (i + seed) % 4, dtype=np.uint64)] for i in range(n)]
    trees = [8 + i % 3 for i in range(n)]
    index = [int(v) for v in rng.integers(0, 1 << 24, size=n)]
    if n >= 4:
        trees[3], index[3], rows[3] = trees[0], index[0], list(rows[0])
    return trees, index, rows


# (openings, log_n): one; a wave and one more; exactly full at the smallest table and at one of two waves; idle rows behind a full wave;
# two workgroups of the auxiliary kernel, full and with idle rows behind the openings in the second
WITNESS = {"one": (1, 5), "wave_64": (64, 7), "wave_65": (65, 7), "full_32": (32, 5), "full_64": (64, 6), "full_512_two_blocks": (512, 9),
           "idle_behind_300_two_blocks": (300, 9)}


@pytest.mark.parametrize("name", list(WITNESS))
def test_witness_equals_the_reference(ctx, vx, name):
    n_idx, log_n = WITNESS[name]
    trees, index, rows = openings(n_idx)
    want, want_pub = N.ref_trace(trees, index, rows, log_n)
    tb, pub = ctx.leaf_noop_air_trace(trees, index, rows, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(N.COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_LEAF_NOOP, tb, log_n, CHAL, vx.lib.VX_LEAF_NOOP_AIR_AUX_COLS, pub)
    want_aux, want_apub = N.gen_aux(want, CHAL, want_pub)
    got_aux = ab.download().reshape(N.AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    tb.free(), ab.free()


@pytest.mark.parametrize("log_n", [5, 6])
def test_one_opening_over_is_refused(ctx, vx, log_n):
    trees, index, rows = openings((1 << log_n) + 1)
    with pytest.raises(vx.VxError, match="do not fit") as e:
        ctx.leaf_noop_air_trace(trees, index, rows, log_n)
    assert e.value.code == -1  # VX_ERR_ARG
    tb, _ = ctx.leaf_noop_air_trace(trees[:-1], index[:-1], rows[:-1], log_n)  # the context goes on working
    assert int(tb.download().reshape(N.COLS, -1)[N.ACT].sum()) == 1 << log_n
    tb.free()


def test_the_table_proof_equals_the_reference_prover(ctx, vx, oracle):
    """the compiled constraints are the restated ones: the same trace proven by both provers gives the same words"""
    trees, index, rows = openings(37)
    log_n = N.log_rows(37)
    trace, pub = N.ref_trace(trees, index, rows)
    tb, gpub = ctx.leaf_noop_air_trace(trees, index, rows, log_n)
    over = dict(num_queries=8)
    got = ctx.stark_prove(vx.lib.VX_AIR_LEAF_NOOP, tb, log_n, gpub, ctx.stark_config(**over))
    want = np.array(S.prove(N.air(), trace, pub, dict(S.DEFAULT_CFG, **over)), dtype=np.uint64)
    assert int(got[1]) == N.AIR_ID and int(want[1]) == N.REF_ID and got.size == want.size
    got[1] = N.REF_ID
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing word of the proof: %d" % bad[0]
    # the host verifier's compiled constraints accept it: the one check a table alone on its bus cannot pass is the last one
    got[1] = N.AIR_ID
    with pytest.raises(vx.VxError, match="stand-alone proof publishes a non-zero bus total"):
        vx.lib.stark_verify(got, ctx.stark_config(**over), expect_air=vx.lib.VX_AIR_LEAF_NOOP, expect_public=pub)
    tb.free()


def test_argument_errors(ctx, vx):
    trees, index, rows = openings(3)
    for call in (lambda: ctx.leaf_noop_air_trace(trees, index, [rows[0], [1, 2, 3, 4, 5], rows[2]], 5),  # a row of five words is hashed
                 lambda: ctx.leaf_noop_air_trace(trees, index, [rows[0], [], rows[2]], 5),               # an empty row
                 lambda: ctx.leaf_noop_air_trace(trees, index, [rows[0], [P], rows[2]], 5),              # a non-canonical word
                 lambda: ctx.leaf_noop_air_trace(trees, index, [rows[0], [1, 2, P + 1], rows[2]], 5),
                 lambda: ctx.leaf_noop_air_trace([8, 1 << 32, 8], index, rows, 5),                       # a tree id out of range
                 lambda: ctx.leaf_noop_air_trace(trees, [1, 1 << 40, 2], rows, 5),                       # a leaf index out of range
                 lambda: ctx.leaf_noop_air_trace([], [], [], 5),                                         # no opening
                 lambda: ctx.leaf_noop_air_trace(trees, index, rows, 4),                                 # fewer than 2^5 rows
                 lambda: ctx.leaf_noop_air_trace(trees, index, rows, 6, out=ctx.alloc(N.COLS << 5))):    # a buffer that is too small
        with pytest.raises(vx.VxError) as e:
            call()
        assert e.value.code == -1  # VX_ERR_ARG
    tb, pub = ctx.leaf_noop_air_trace(trees, index, rows, 5)  # after the refusals the context makes the same table
    assert [int(v) for v in pub] == N.claims_digest(trees, index, rows)
    assert (tb.download().reshape(N.COLS, -1) == N.ref_trace(trees, index, rows, 5)[0]).all()
    tb.free()
