"""FriExitAir and the exit group of an inner proof on the GPU: the witness kernel (closed forms, one lane per row) against
tests/fri_exit_ref.py (the recurrences run row by row) cell for cell -- edge values, the shapes of the CPU tier with values from the
transcript claims of GPU-made inner proofs, idle blocks --, the trace's extent under poison and guard zones, the blob of
Context.fri_exits_prove against the reference group word for word, and what the device refuses.  Tables of at most 2^13 rows."""
import numpy as np
import pytest

import extents as X
import fri_exit_ref as E
import test_bus_group as BG
from oracle import stark_ref as S

Z = E.Z
P = E.P
pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATEMENT = -1, -5
LN, NL, POW_BITS, ORD_POW, ABSORBED = (E.HAND[k] for k in ("LN", "NL", "pow_bits", "ord_pow", "absorbed"))
EDGES, INDEX_VALUES, GROUP_SHAPES, final_poly = E.EDGES, E.INDEX_VALUES, E.GROUP_SHAPES, E.final_poly


def pcfg(ctx, cfg):
    cfg = dict(S.DEFAULT_CFG, **cfg)
    return ctx.stark_config(**{k: cfg[k] for k in ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")})


_proofs = {}


def gpu_proof(ctx, name):
    """the inner proof of a shape made on the GPU -- word for word the reference prover's"""
    if name not in _proofs:
        air, trace, pub, _ = Z.inner("fib8" if name == "fib8_pow0" else name)
        want = E.inner(name)
        proof = ctx.stark_prove(air.ID, ctx.from_host(trace), trace.shape[1].bit_length() - 1, pub, pcfg(ctx, want["cfg"]))
        assert proof.size == want["proof"].size and (proof == want["proof"]).all()
        _proofs[name] = proof
    return _proofs[name]


def same_cells(got, want):
    got = got.reshape(want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing cell: column %d, row %d (block row %d): %d for %d" % (bad[0][0], bad[0][1], bad[0][1] % E.BLOCK, got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("extra", [0, 1], ids=["min_log_n", "one_above"])
@pytest.mark.parametrize("case", list(EDGES))
def test_trace_parity_on_edge_values(ctx, vx, oracle, case, extra):
    pow_bits, response = EDGES[case]
    fp, values = final_poly(16), [response] + INDEX_VALUES
    log_n = vx.lib.fri_exit_log_n(len(INDEX_VALUES)) + extra
    want, want_pub = E.ref_trace(values, LN, NL, pow_bits, ORD_POW, ABSORBED, fp, log_n)
    buf, pub = ctx.fri_exit_air_trace(LN, NL, pow_bits, ORD_POW, ABSORBED, values, fp, log_n)
    assert [int(v) for v in pub] == want_pub == [int(v) for v in vx.lib.fri_exit_public(LN, NL, pow_bits, ORD_POW, ABSORBED, fp)]
    same_cells(buf.download(), want)
    buf.free()


@pytest.mark.parametrize("name", list(GROUP_SHAPES))
def test_trace_parity_on_the_claims_of_a_gpu_made_proof(ctx, vx, oracle, name):
    proof, cfg = gpu_proof(ctx, name), pcfg(ctx, E.inner(name)["cfg"])
    obs, chal = vx.lib.stark_transcript_claims(proof, cfg)
    fc = vx.lib.stark_fri_claims(proof, cfg)
    c = E.claims_of(name)
    n_q = fc["index"].size
    ord_pow = chal.shape[0] - 1 - n_q
    assert (fc["log_lde"], fc["betas"].shape[0], fc["final_poly"].shape[0]) == GROUP_SHAPES[name] and ord_pow == c["ord_pow"] and obs.size == len(c["words"])
    values = chal[ord_pow:, 1]
    assert [int(v) for v in values] == [v for _, v in c["chals"][ord_pow:]]
    for extra in (0, 1):
        log_n = vx.lib.fri_exit_log_n(n_q) + extra
        want, want_pub = E.ref_trace([int(v) for v in values], c["LN"], c["NL"], c["pow_bits"], ord_pow, obs.size, c["fpoly"], log_n)
        buf, pub = ctx.fri_exit_air_trace(fc["log_lde"], fc["betas"].shape[0], cfg.pow_bits, ord_pow, obs.size, values, fc["final_poly"], log_n)
        assert [int(v) for v in pub] == want_pub
        same_cells(buf.download(), want)
        buf.free()
    last = E.BLOCK * np.arange(2, n_q + 2) - 1  # what every index block hands to the bus: the proof's own index and exit
    assert [int(v) for v in want[E.IDX, last]] == [int(i) for i in fc["index"]]
    assert (want[E.ACC, last] == fc["ev_last"][:, 0]).all() and (want[E.ACC + 1, last] == fc["ev_last"][:, 1]).all()


@pytest.mark.parametrize("extra", [0, 1], ids=["min_log_n", "one_above"])
def test_the_trace_is_stored_whole_and_nothing_else(ctx, vx, oracle, extra):
    fp, values = final_poly(64, seed=8), [2**(64 - POW_BITS) - 1] + INDEX_VALUES[:3]  # four blocks: the minimum is a full table
    log_n = vx.lib.fri_exit_log_n(3) + extra
    n = 1 << log_n
    g = X.Guarded(ctx, E.COLS * n, shape=(E.COLS, n), name="fri exit trace")
    ctx.fri_exit_air_trace(LN, NL, POW_BITS, ORD_POW, ABSORBED, values, fp, log_n, out=g.buf)
    got = g.check()
    want, _ = E.ref_trace(values, LN, NL, POW_BITS, ORD_POW, ABSORBED, fp, log_n)
    assert E.check(want, E.public_inputs(LN, NL, POW_BITS, ORD_POW, ABSORBED, fp)) is None  # 64 Horner steps: the last on row 126
    same_cells(got, want)
    g.free()


@pytest.mark.parametrize("name", ["fib8", "lookup8", "fib8_two_layers_cap0"])
def test_group_blob_equals_the_reference_group(ctx, vx, oracle, name):
    proof = gpu_proof(ctx, name)
    g = E.group(name)
    cfg = pcfg(ctx, g["cfg"])
    blob = ctx.fri_exits_prove(proof, cfg)
    vx.lib.fri_exits_verify(blob, proof, cfg)
    ids = [vx.lib.VX_AIR_FRI_FOLD, vx.lib.VX_AIR_TRANSCRIPT, vx.lib.fri_exit_air_id()]
    got = vx.lib.split_bus_group(blob)
    assert len(got) == 3 and max(tr.shape[1] for tr, _ in g["tabs"]) <= 1 << 13
    for k, (gp, wp, i) in enumerate(zip(got, g["proofs"], ids)):
        wp = np.array(wp, dtype=np.uint64)
        wp[1] = i
        assert gp.size == wp.size, "table %d" % k
        bad = np.flatnonzero(gp != wp)
        assert bad.size == 0, "first differing word of table %d: %d" % (k, bad[0])
    want = BG.wrap(g["proofs"], ids)
    assert blob.size == want.size and (blob == want).all()
    assert (ctx.fri_exits_prove(proof, cfg) == blob).all()  # proving twice gives the same words
    tables, outside, _ = ctx.fri_exits_tables(proof, cfg)
    assert ctx.bus_group_check(tables, outside) is None
    for t in tables:
        t[1].free()


def test_device_side_refusals_leave_the_context_working(ctx, vx, oracle):
    proof = gpu_proof(ctx, "fib8")
    g = E.group("fib8")
    c, cfg = g["c"], pcfg(ctx, g["cfg"])
    blob = ctx.fri_exits_prove(proof, cfg)
    tables, outside, _ = ctx.fri_exits_tables(proof, cfg)
    # one index challenge raised by the domain size: the same low bits, another v -- only the chal message differs
    values = [v for _, v in c["chals"][c["ord_pow"]:]]
    q = next(k for k in range(1, len(values)) if values[k] + (1 << c["LN"]) < P)
    values[q] += 1 << c["LN"]
    log_n = tables[2][2]
    etr, epub = ctx.fri_exit_air_trace(c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), values, c["fpoly"], log_n)
    assert [int(v) for v in epub[:8]] == [int(v) for v in tables[2][3][:8]]
    forged = tables[:2] + [(tables[2][0], etr, log_n, tables[2][3])]
    u = ctx.bus_group_check(forged, outside)
    assert u is not None and u.n_unmatched == 2  # the chal TranscriptAir sends and the one the exit table receives
    assert (u.table == 1 and u.message >= 8) or (u.table == 2 and u.message == 0 and u.row == E.BLOCK * (q + 1) - 1)
    with pytest.raises(vx.VxError) as e:
        ctx.bus_group_prove(forged, cfg, outside)
    assert e.value.code == ERR_STATEMENT
    assert (ctx.fri_exits_prove(proof, cfg) == blob).all()
    # a proof-of-work response with a bit among its top pow_bits
    values = [v for _, v in c["chals"][c["ord_pow"]:]]
    values[0] |= 1 << (64 - c["pow_bits"])
    with pytest.raises(vx.VxError, match="proof of work invalid") as e:
        ctx.fri_exit_air_trace(c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), values, c["fpoly"], log_n, out=etr)
    assert e.value.code == ERR_STATEMENT
    for bad_values, kw in (([P] + values[1:], {}), (values[:1] + [2**64 - 1] + values[2:], {}), (None, dict(log_n=log_n - 3)), (None, dict(n_layers=0)), (None, dict(n_layers=9)), (None, dict(n_layers=2, log_lde=8))):
        a = dict(log_lde=c["LN"], n_layers=c["NL"], log_n=log_n)
        a.update(kw)
        good = [v for _, v in c["chals"][c["ord_pow"]:]]
        with pytest.raises(vx.VxError) as e:
            ctx.fri_exit_air_trace(a["log_lde"], a["n_layers"], c["pow_bits"], c["ord_pow"], len(c["words"]), good if bad_values is None else bad_values, c["fpoly"], a["log_n"], out=etr)
        assert e.value.code == ERR_ARG
    with pytest.raises(vx.VxError, match="more than 64 coefficients") as e:
        ctx.fri_exit_air_trace(c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), values, final_poly(65), log_n, out=etr)
    assert e.value.code == ERR_ARG
    assert (ctx.fri_exits_prove(proof, cfg) == blob).all()
    for t in tables + [forged[2]]:
        t[1].free()
