"""Every compiled AIR's constraints on ARBITRARY data: ctx.quotient_eval (vx_quotient_eval_aux -> k_quotient<Air, R>, the `eval`
template the host verifier instantiates too) against the AIR's independent restatement (oracle/stark_ref.quotient_values), value
for value.  The proof-parity tests reach these constraints on satisfying traces only, where block-constant columns, prefix flags
and copies tie cells to each other: a compiled constraint that reads the wrong one of two tied cells yields the same proof
(tests/test_quotient_mutants.py counts such mistakes).  Here the data is uniform with a third from the edge list of the fused
multiply (quotient_arbitrary.py), public inputs, lookup challenges and published words are random, and nothing is tied.

Every case runs under three constraint-challenge pairs: random, (1, p - 1), and (0, r) -- the last constraint alone in acc[0].

  SMALL      the eight bus tables and VX_AIR_SHA_CHAIN at log_n = max(2, period) and one more, VX_AIR_LOOKUP at 2^8, rate_bits 1, 2, 3;
             VX_AIR_FIBONACCI and VX_AIR_MIX once through the new entry point (MIX at N = 512: two points per lane)
  FIXED      VX_AIR_EPOCH_END (2^9 rows), VX_AIR_SHA512[10], VX_AIR_SHA_TREE[16] (2^12): the row count is the table's period; rate_bits 1, 2
  DEVICE     VX_AIR_BLAKE_CHAIN (2^16 rows, the period of its tables; several points per lane) and VX_AIR_ED25519[16] at rate_bits 1:
             filled on the device, a window of 64 points ending at N - 1 overwritten with edge-list draws, compared at sampled
             points (0, N - 1, N - 2^r whose successor wraps to 0, 2^r - 1, every 2^b - 1 and N - 2^(b-1), over 2000 random ones) from
             the sampled rows and their successors alone

Every point is compared where N (COLS + AUX) <= 2^24 words, sampled points otherwise.

Covered through their template's smallest instantiation, which runs the same `eval` text, and not run here:
  VX_AIR_ED25519[17] (EdAir17) through VX_AIR_ED25519[16]; VX_AIR_SHA512[15] and VX_AIR_SHA512[16] through VX_AIR_SHA512[10];
  VX_AIR_SHA_TREE[256] and VX_AIR_SHA_TREE[512] through VX_AIR_SHA_TREE[16]."""
import numpy as np
import pytest

import air_program_fuzz as Z
import quotient_arbitrary as QA

P = QA.P

pytestmark = pytest.mark.gpu

N_RANDOM_POINTS = 2100  # drawn with repetition out of 2^17: at least 2000 distinct ones (asserted)
FULL_LIMIT = 1 << 24   # words of [COLS + AUX][N] up to which the host holds the whole array and every point is compared
PERIOD_5 = ["VX_AIR_MERKLE_OPEN", "VX_AIR_LEAF_SPONGE", "VX_AIR_MERKLE_OPEN_SET", "VX_AIR_LEAF_SPONGE_SET", "VX_AIR_TRANSCRIPT"]
PERIOD_0 = ["VX_AIR_FRI_FOLD", "VX_AIR_FRI_COMBINE", "VX_AIR_LEAF_NOOP"]
assert sorted(PERIOD_5 + PERIOD_0) == sorted(QA.BUS_TABLES)

# (AIR, log_n, rate_bits)
SMALL = ([(name, log_n, r) for name in PERIOD_5 for log_n in (5, 6) for r in (1, 2, 3)]
         + [(name, log_n, r) for name in PERIOD_0 for log_n in (2, 3) for r in (1, 2, 3)]
         + [("VX_AIR_SHA_CHAIN", log_n, r) for log_n in (6, 7) for r in (1, 2, 3)]
         + [("VX_AIR_LOOKUP", 8, r) for r in (1, 2, 3)]
         + [("VX_AIR_FIBONACCI", 3, 1), ("VX_AIR_MIX", 8, 1)])
FIXED = [(name, log_n, r) for name, log_n in (("VX_AIR_EPOCH_END", 9), ("VX_AIR_SHA512[10]", 10), ("VX_AIR_SHA_TREE[16]", 12)) for r in (1, 2)]
DEVICE = [("VX_AIR_BLAKE_CHAIN", 16, 1), ("VX_AIR_ED25519[16]", 16, 1)]


def case_id(c):
    return "%s-L%d-r%d" % c


def points_of(log_n, r):
    """the sampled points of a case: the fixed ones and N_RANDOM_POINTS random ones"""
    N = 1 << (log_n + r)
    rng = np.random.default_rng([log_n, r, 77])
    pts = set(QA.sample_points(rng, log_n + r, N_RANDOM_POINTS)) | {0, N - 1, N - (1 << r), (1 << r) - 1}
    return np.array(sorted(pts), dtype=np.int64)


def first_difference(got, want, points=None):
    """None, or "(challenge k, point i): got, want" of the first differing value"""
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    k, j = (int(v) for v in bad[0])
    return "(challenge %d, point %d): got %d, want %d -- %d values differ" % (k, j if points is None else int(points[j]), int(got[k, j]), int(want[k, j]), len(bad))


def compare(ctx, vx, name, log_n, r, buf, air, pub, chal, apub, pairs, lde=None, points=None, rows=None):
    """the GPU's quotient values of the buffer against the restatement's: at every point of the host array `lde`, or at `points`
    from rows = (the rows at the points, the rows at their successors)"""
    for label, alphas in pairs:
        got = ctx.quotient_eval(QA.air_id(vx.lib, name), r, buf, log_n, alphas, pub, challenges=chal, aux_public=apub)
        if points is None:
            want = QA.reference(air, lde, pub, chal, apub, alphas, log_n, r)
        else:
            want = QA.reference(air, rows[0], pub, chal, apub, alphas, log_n, r, points=points, nxt_rows=rows[1])
            got = got[:, points]
        bad = first_difference(got, want, points)
        assert bad is None, "%s at rate_bits %d, alphas %s %s: first differing %s" % (name, r, label, alphas, bad)


@pytest.mark.parametrize("case", SMALL + FIXED, ids=case_id)
def test_host_filled_table(ctx, vx, oracle, case):
    name, log_n, r = case
    air, lde, pub, chal, apub, pairs = QA.arbitrary(name, log_n, r)
    N = 1 << (log_n + r)
    buf = ctx.from_host(lde)
    try:
        if lde.size <= FULL_LIMIT:
            compare(ctx, vx, name, log_n, r, buf, air, pub, chal, apub, pairs, lde=lde)
        else:
            pts = points_of(log_n, r)
            rows = (np.ascontiguousarray(lde[:, pts]), np.ascontiguousarray(lde[:, (pts + (1 << r)) % N]))
            compare(ctx, vx, name, log_n, r, buf, air, pub, chal, apub, pairs, points=pts, rows=rows)
    finally:
        buf.free()


@pytest.mark.parametrize("case", DEVICE, ids=case_id)
def test_device_filled_table(ctx, vx, oracle, case):
    """2^17 points of a thousand columns and more never reach the host: filled with vx_fill_random, the last 64 points of every
    column overwritten with edge-list draws (so they meet the wrap-around), and only the sampled rows and their successors fetched"""
    from oracle import pyref

    name, log_n, r = case
    air = QA.restatement(name)
    cols, LN = QA.n_columns(air), log_n + r
    N = 1 << LN
    rng = np.random.default_rng(QA.seed_of(name, log_n, r))
    pub, chal, apub = QA.statement_words(rng, air)
    pairs = QA.alpha_pairs(rng)
    buf = ctx.alloc(cols * N)
    try:
        ctx.fill_random(buf, cols * N, int(rng.integers(0, 2**31)))
        window = Z.special_words(rng, cols * 64).reshape(cols, 64)
        for j in range(cols):
            buf.upload(window[j], off=j * N + N - 64)
        pts = points_of(log_n, r)
        assert {0, N - 1, N - (1 << r), (1 << r) - 1} <= set(int(p) for p in pts) and pts.size >= 2000 + 2 * LN
        succ = (pts + (1 << r)) % N

        def fetch(idx):  # vx_lde_rows takes plonky2's leaf index: row i is leaf bitrev(i)
            return np.ascontiguousarray(ctx.lde_rows(buf, LN, cols, [pyref.bitrev(int(i), LN) for i in idx]).T)

        rows = (fetch(pts), fetch(succ))
        tail = np.flatnonzero(pts >= N - 64)
        assert (rows[0][:, tail] == window[:, pts[tail] - (N - 64)]).all(), "the fetched rows are not the uploaded window"
        compare(ctx, vx, name, log_n, r, buf, air, pub, chal, apub, pairs, points=pts, rows=rows)
    finally:
        buf.free()


def test_argument_checks(ctx, vx, oracle):
    """the checks of vx_quotient_eval_aux: the counts of challenges and published words, canonical host words, the fixed row count of
    an AIR with positional columns; vx_quotient_eval still refuses an AIR with an auxiliary round"""
    name, log_n, r = "VX_AIR_LEAF_NOOP", 2, 1
    air, lde, pub, chal, apub, pairs = QA.arbitrary(name, log_n, r)
    aid, alphas = QA.air_id(vx.lib, name), pairs[0][1]
    buf = ctx.from_host(lde)
    for kw in (dict(challenges=chal[:3], aux_public=apub), dict(challenges=chal, aux_public=apub[:1]), dict(challenges=chal, aux_public=[]),
               dict(challenges=[P] + chal[1:], aux_public=apub), dict(challenges=chal, aux_public=[apub[0], P]), dict()):
        with pytest.raises(vx.VxError) as e:
            ctx.quotient_eval(aid, r, buf, log_n, alphas, pub, **kw)
        assert e.value.code == -1
    for bad_pub, bad_alphas in (([P] + pub[1:], alphas), (pub, [P, 1]), (pub[:-1], alphas)):
        with pytest.raises(vx.VxError):
            ctx.quotient_eval(aid, r, buf, log_n, bad_alphas, bad_pub, challenges=chal, aux_public=apub)
    main_only = ctx.from_host(lde[:air.COLS])
    with pytest.raises(vx.VxError):  # a buffer that holds the main columns only
        ctx.quotient_eval(aid, r, main_only, log_n, alphas, pub, challenges=chal, aux_public=apub)
    epoch = QA.restatement("VX_AIR_EPOCH_END")
    big = ctx.alloc(QA.n_columns(epoch) << 11)
    ctx.fill_random(big, big.n, 1)
    rng = np.random.default_rng(3)
    epub, echal, eapub = QA.statement_words(rng, epoch)
    with pytest.raises(vx.VxError, match="log_n must be 9"):  # 2^10 rows: the prover refuses them too
        ctx.quotient_eval(vx.lib.VX_AIR_EPOCH_END, 1, big, 10, alphas, epub, challenges=echal, aux_public=eapub)
    # the context goes on working, and an AIR without an auxiliary round gives the same values through both entry points
    compare(ctx, vx, name, log_n, r, buf, air, pub, chal, apub, pairs[:1], lde=lde)
    _, mlde, mpub, _, _, mpairs = QA.arbitrary("VX_AIR_MIX", 8, 1)
    mbuf = ctx.from_host(mlde)
    assert (ctx.quotient_eval(vx.lib.VX_AIR_MIX, 1, mbuf, 8, mpairs[0][1], mpub) == ctx.quotient_eval(vx.lib.VX_AIR_MIX, 1, mbuf, 8, mpairs[0][1], mpub, challenges=[], aux_public=[])).all()
    big.free(), buf.free(), mbuf.free(), main_only.free()


@pytest.mark.parametrize("name,log_n,r", [("VX_AIR_TRANSCRIPT", 5, 1), ("VX_AIR_SHA_CHAIN", 6, 2)])
def test_one_changed_cell_is_noticed(ctx, vx, oracle, name, log_n, r):
    """the comparison is not vacuous: with one word of the last auxiliary column changed on the device (at point N - 1, whose
    successor row is point 2^r - 1), the GPU's values leave the reference's of the unchanged data exactly at the two points whose
    rows hold that cell, under each alpha pair"""
    air, lde, pub, chal, apub, pairs = QA.arbitrary(name, log_n, r)
    N, last = 1 << (log_n + r), QA.n_columns(air) - 1
    changed = lde.copy()
    changed[last, N - 1] = (int(lde[last, N - 1]) + 1) % P
    buf = ctx.from_host(changed)
    for label, alphas in pairs:
        got = ctx.quotient_eval(QA.air_id(vx.lib, name), r, buf, log_n, alphas, pub, challenges=chal, aux_public=apub)
        want = QA.reference(air, lde, pub, chal, apub, alphas, log_n, r)
        assert first_difference(got, want) is not None, label
        assert sorted(set(int(i) for i in np.argwhere(got != want)[:, 1])) == [N - 1 - (1 << r), N - 1], label
        assert (got == QA.reference(air, changed, pub, chal, apub, alphas, log_n, r)).all(), label
    buf.free()
