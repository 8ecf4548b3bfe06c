"""FriCombineAir (AIR id 21) on the GPU: the witness, the auxiliary columns and the public inputs equal the reference generator cell by
cell at every wave and block boundary of the scan, the proof inside the blob of vx_fri_combine_prove equals the reference prover's
word for word, real vx_stark_prove proofs (with and without an auxiliary tree) are turned into claims by vx_stark_combine_claims and
their query-phase arithmetic -- combination and fold chains on one bus, no ev_0 handed over -- is proven and checked, and the
workload's shape (84 queries of 1025 row words over a 2^21 LDE, one 2^17-row table) is proven and checked by vx_fri_combine_verify."""
import numpy as np
import pytest

import fri_combine_ref as K
import fri_fold_ref as F
from oracle import stark_ref as S

P = K.P
CHAL = K.CHAL

pytestmark = pytest.mark.gpu

# absorb rows per query -> (LN, cm, ca, nq).  The witness kernel scans in waves of 64 and blocks of 256: 63 / 64 / 65 and 255 / 256 /
# 257 are the boundaries, 1025 takes five tiles.  Among them: ca = 0 (2, 257), cm = 1 (2, 64), nq = 1 (2, 65, 257) and 4, the main /
# auxiliary boundary on a wave boundary (255: 128) and off one (63: 40, 256: 200), S1's row the last lane of a wave (65) and of a tile
# (257); LN = 5 and 14
SHAPES = {2: (5, 1, 0, 1), 63: (14, 40, 19, 4), 64: (14, 1, 59, 4), 65: (5, 60, 4, 1), 255: (5, 128, 123, 4), 256: (14, 200, 52, 4), 257: (5, 256, 0, 1), 1025: (14, 745, 276, 4)}


def case_queries(rpq, LN, case):
    """-> (query indices, log_n): log_n holds at least three queries, so that `full` leaves fewer idle rows than one query takes"""
    top = (1 << LN) - 1
    rng = np.random.default_rng(rpq)
    log_n = max(5, (3 * rpq - 1).bit_length())
    if case == "single":
        return [int(rng.integers(0, top + 1))], max(5, (rpq - 1).bit_length())
    if case == "duplicates":
        i = int(rng.integers(0, top + 1))
        return [i, top // 3, i, i], max(5, (4 * rpq - 1).bit_length())
    if case == "first_and_last_index":
        return [0, top], max(5, (2 * rpq - 1).bit_length())
    if case == "full":
        return [int(v) for v in rng.integers(0, top + 1, size=(1 << log_n) // rpq)], log_n
    if case == "half_idle":
        return [int(v) for v in rng.integers(0, top + 1, size=(1 << (log_n - 1)) // rpq)], log_n
    raise ValueError(case)


@pytest.mark.parametrize("case", ["single", "duplicates", "first_and_last_index", "full", "half_idle"])
@pytest.mark.parametrize("absn", list(SHAPES))
def test_witness_equals_the_reference(ctx, vx, oracle, absn, case):
    LN, cm, ca, nq = SHAPES[absn]
    assert cm + ca + nq == absn
    rpq = absn + LN
    index, log_n = case_queries(rpq, LN, case)
    n = 1 << log_n
    if case == "full":
        assert n - len(index) * rpq < rpq
    if case == "half_idle":
        assert n // 2 - rpq < len(index) * rpq <= n // 2
    tree0 = 0 if case == "duplicates" else K.TREE0
    st = K.rand_statement(LN, cm, ca, nq, seed=absn)
    rows, ev0 = K.rand_claims(st, index, seed=absn + 1)
    want, want_pub = K.ref_trace(st, index, rows, log_n, tree0)
    tb, pub = ctx.fri_combine_air_trace(LN, st["r"], cm, ca, nq, st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"], index, rows, ev0, log_n, tree0)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(K.COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_FRI_COMBINE, tb, log_n, CHAL, vx.lib.VX_FRI_COMBINE_AIR_AUX_COLS, pub)
    want_aux, want_apub = K.gen_aux(want, CHAL, want_pub)
    got_aux = ab.download().reshape(K.AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    assert S.check_trace(K.air(), got, want_pub, CHAL, got_aux, want_apub) is None
    tb.free(), ab.free()


def prove(ctx, st, index, rows, ev0, cfg=None, out=None):
    return ctx.fri_combine_prove(st["LN"], st["cm"], st["ca"], st["nq"], st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"], index, rows, ev0, cfg, out)


def verify(vx, blob, st, index, rows, ev0, cfg=None, **over):
    a = dict(st, **over)
    vx.lib.fri_combine_verify(blob, a["LN"], a["cm"], a["ca"], a["nq"], a["alpha"], a["zeta"], a["ol"], a["on"], a["oq"], index, rows, ev0, cfg)


def flip(a, *at):
    a = np.array(a, dtype=np.uint64)
    a[at] ^= np.uint64(1)
    return a


@pytest.mark.parametrize("shape", [(5, 1, 0, 1), (9, 3, 2, 2), (6, 70, 10, 4)])
def test_proof_equals_the_reference_prover(ctx, vx, oracle, shape):
    LN, cm, ca, nq = shape
    st = K.rand_statement(LN, cm, ca, nq, seed=LN)
    rng = np.random.default_rng(LN)
    index = [0, (1 << LN) - 1] + [int(v) for v in rng.integers(0, 1 << LN, size=3)]
    index.append(index[2])  # one duplicate
    rows, ev0 = K.rand_claims(st, index)
    over = dict(num_queries=8)
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    blob = prove(ctx, st, index, rows, ev0, cfg)
    assert [int(v) for v in blob[:6]] == [K.MAGIC, LN, cm, ca, nq, len(index)] and int(blob[6]) == blob.size - K.HDR and int(blob[K.HDR + 1]) == K.AIR_ID
    assert int(blob[K.HDR + 2]) == K.log_rows(len(index), st)
    trace, pub = K.ref_trace(st, index, rows)
    want = K.prove(trace, pub, ocfg)
    got = K.unwrap(blob)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing proof word: %d" % bad[0]
    ok, chal = K.bus_check(got, ocfg["cap_height"], st, index, rows, ev0)
    assert ok
    S.verify(got, ocfg, expect_air=K.REF_ID, expect_public=pub, ext_chal=chal)
    verify(vx, blob, st, index, rows, ev0, cfg)
    with pytest.raises(vx.VxError):  # (the claims digest is a public input: a changed claim is refused there, before the bus)
        verify(vx, blob, st, index, flip(rows, 3, cm + ca + nq - 1), ev0, cfg)


@pytest.mark.parametrize("air", [S.FibAir, S.LookupAir])
def test_the_query_phase_arithmetic_of_a_real_proof(ctx, vx, oracle, air):
    """real proofs of 2^13 rows at the default arity -- a 2^14 LDE, two fold layers -- without (FibAir) and with (LookupAir) an
    auxiliary tree"""
    log_n = 13
    cfg, ocfg = ctx.stark_config(num_queries=5), dict(S.DEFAULT_CFG, num_queries=5)
    trace, pub = air.trace(log_n)
    proof = ctx.stark_prove(air.ID, ctx.from_host(trace), log_n, pub, cfg)
    c, f = vx.lib.stark_combine_claims(proof, cfg), vx.lib.stark_fri_claims(proof, cfg)
    assert (c["log_lde"], c["cm"], c["ca"] > 0, c["nq"], len(c["index"])) == (14, air.COLS, air is S.LookupAir, 4, 5)
    assert (c["ev0"] == f["ev0"]).all() and (c["index"] == f["index"]).all()
    st = dict(LN=c["log_lde"], r=ocfg["rate_bits"], cm=c["cm"], ca=c["ca"], nq=c["nq"], alpha=c["alpha"], zeta=c["zeta"], ol=c["open_local"], on=c["open_next"], oq=c["open_quot"])
    index, rows, ev0 = [int(v) for v in c["index"]], c["rows"], c["ev0"]
    assert (K.ev0_of(st, index, rows) == ev0).all()
    # the stand-alone pair
    blob = prove(ctx, st, index, rows, ev0, cfg)
    verify(vx, blob, st, index, rows, ev0, cfg)
    ok, _ = K.bus_check(K.unwrap(blob), ocfg["cap_height"], st, index, rows, ev0)
    assert ok
    with pytest.raises(vx.VxError):
        verify(vx, blob, st, index, rows, flip(ev0, 4, 0), cfg)
    # combine + fold on one bus: no ev_0 is passed
    betas, fpoly, leaves = f["betas"], f["final_poly"], f["leaves"]
    NL = len(betas)
    a = (st["LN"], st["cm"], st["ca"], st["nq"], st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"])
    gblob = ctx.fri_combine_fold_prove(*a, betas, fpoly, index, rows, leaves, cfg)
    ps, chal = K.group_prove(K.group_tables(st, betas, fpoly, index, rows, leaves), ocfg)
    want = K.group_wrap(ps, st, NL, len(index))
    assert gblob.size == want.size
    bad = np.flatnonzero(gblob != want)
    assert bad.size == 0, "first differing blob word: %d" % bad[0]
    assert K.group_sum(ps, ocfg["cap_height"], chal, st, betas, fpoly, index, rows, leaves)

    def gverify(blob_=gblob, index_=index, rows_=rows, leaves_=leaves, **over):
        s2 = dict(st, **over)
        vx.lib.fri_combine_fold_verify(blob_, s2["LN"], s2["cm"], s2["ca"], s2["nq"], s2["alpha"], s2["zeta"], s2["ol"], s2["on"], s2["oq"], betas, fpoly, index_, rows_, leaves_, cfg)

    gverify()
    for bad in (dict(rows_=flip(rows, 2, 1)), dict(leaves_=flip(leaves, 3, 1, 5)), dict(on=flip(st["on"], 0, 0)), dict(alpha=flip(st["alpha"], 1)), dict(zeta=flip(st["zeta"], 0)),
                dict(index_=index[:1] + [index[1] ^ 1] + index[2:])):
        with pytest.raises(vx.VxError):
            gverify(**bad)
    # truncation
    with pytest.raises(vx.VxError):
        vx.lib.stark_combine_claims(proof[:-9], cfg)
    with pytest.raises(vx.VxError):
        verify(vx, blob[:-9], st, index, rows, ev0, cfg)
    with pytest.raises(vx.VxError):
        gverify(blob_=gblob[:-9])


def test_workload_shape(ctx, vx, oracle):
    """84 queries of the hash-chain table's rows (745 main, 276 auxiliary, 4 quotient words) over a 2^21 LDE: 1046 rows per query,
    87864 rows in a 2^17-row table"""
    LN, cm, ca, nq = 21, 745, 276, 4
    st = K.rand_statement(LN, cm, ca, nq, seed=84)
    rng = np.random.default_rng(84)
    index = [0, (1 << LN) - 1] + [int(v) for v in rng.integers(0, 1 << LN, size=81)]
    index.append(index[7])  # one duplicate
    assert len(index) == 84
    rows, ev0 = K.rand_claims(st, index)
    blob = prove(ctx, st, index, rows, ev0)
    assert int(blob[K.HDR + 2]) == 17  # degree bits of the table
    verify(vx, blob, st, index, rows, ev0)

    def refused(index_=index, rows_=rows, ev0_=ev0, **over):
        with pytest.raises(vx.VxError):
            verify(vx, blob, st, index_, rows_, ev0_, **over)

    refused(rows_=flip(rows, 40, 800))                             # one row word
    refused(ev0_=flip(ev0, 83, 0))                                 # one ev_0
    refused(ol=flip(st["ol"], 1000, 1))                            # one opening
    refused(alpha=flip(st["alpha"], 0))
    refused(zeta=flip(st["zeta"], 1))
    refused(index_=index[:5] + [index[5] ^ 16] + index[6:])        # one index


def test_statement_and_argument_errors(ctx, vx, oracle):
    st = K.rand_statement(9, 3, 2, 2, seed=2)
    index = [17, 400]
    rows, ev0 = K.rand_claims(st, index)
    cfg = ctx.stark_config(num_queries=8)
    with pytest.raises(vx.VxError, match="query 1") as e:
        prove(ctx, st, index, rows, flip(ev0, 1, 1), cfg)  # a wrong ev_0 names its query
    assert e.value.code == -5  # VX_ERR_STATEMENT
    with pytest.raises(vx.VxError, match="query 0") as e:
        prove(ctx, st, index, flip(rows, 0, 6), ev0, cfg)  # ... and so does a wrong row word
    assert e.value.code == -5
    with pytest.raises(vx.VxError, match="outside the LDE") as e:
        prove(ctx, st, [17, 512], rows, ev0, cfg)
    assert e.value.code == -1  # VX_ERR_ARG
    with pytest.raises(vx.VxError) as e:
        ctx.fri_combine_air_trace(9, 1, 3, 2, 2, st["alpha"], st["zeta"], st["ol"], st["on"], st["oq"], index * 2, np.tile(rows, (2, 1)), np.tile(ev0, (2, 1)), 5)  # 64 rows do not fit 2^5
    assert e.value.code == -1
    with pytest.raises(vx.VxError) as e:
        prove(ctx, dict(st, cm=0, ol=st["ol"][:2], on=st["on"][:2]), index, rows[:, :4], ev0, cfg)  # no main column
    assert e.value.code == -1
    full = prove(ctx, st, index, rows, ev0, cfg)
    with pytest.raises(vx.VxError) as e:
        prove(ctx, st, index, rows, ev0, cfg, out=np.zeros(full.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == full.size  # VX_ERR_BUFSZ with the length set
