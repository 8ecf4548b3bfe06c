"""The whole query phase of a STARK proof on one bus, on the GPU: for real vx_stark_prove proofs the blob of vx_stark_queries_prove
equals the reference group (tests/stark_queries_ref.py: the restated AIRs under the reference prover) word for word, and
vx_stark_queries_verify accepts it with the whole proof, with the proof's head alone and with the query section replaced by junk.
Refusals: arity 3, a proof without a FRI layer, a flipped sibling (named by query and tree before anything is proven), an output
buffer one word short; after each the context proves the same blob again."""
import numpy as np
import pytest

import stark_queries_ref as Z
from oracle import stark_ref as S

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_BUFSZ, ERR_STATEMENT = -1, -4, -5


def pcfg(ctx, cfg):
    keys = ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")
    return ctx.stark_config(**{k: cfg[k] for k in keys})


def gpu_proof(ctx, name):
    air, trace, pub, cfg = Z.inner(name)
    log_n = trace.shape[1].bit_length() - 1
    return ctx.stark_prove(air.ID, ctx.from_host(trace), log_n, pub, pcfg(ctx, cfg)), cfg


@pytest.mark.parametrize("name", list(Z.SHAPES))
def test_group_blob_equals_the_reference_group(ctx, vx, oracle, name):
    proof, rcfg = gpu_proof(ctx, name)
    cfg = pcfg(ctx, rcfg)
    g = Z.group(name)  # the reference prover's inner proof is the GPU's, word for word: one reference group serves both tiers
    assert proof.size == g["proof"].size and (proof == g["proof"]).all()
    cl, hd = g["cl"], g["hd"]
    assert cl["shape"] == Z.SHAPES[name][3]
    if name == "fib8_40_queries":
        assert cl["index"].count(284) == 2  # a duplicate index is kept: both copies are proven
    blob = ctx.stark_queries_prove(proof, cfg)
    n = len(g["proofs"])
    assert [int(v) for v in blob[:Z.HDR]] == [Z.MAGIC] + cl["shape"] + [n] and n == 4 + len(Z.X.sponge_lengths(cl))
    got = Z.unwrap(blob)
    for k, (gp, wp) in enumerate(zip(got, g["proofs"])):
        wp = np.array(wp, dtype=np.uint64)
        assert gp.size == wp.size, "table %d" % k
        bad = np.flatnonzero(gp != wp)
        assert bad.size == 0, "first differing word of table %d: %d" % (k, bad[0])
    ok, _ = Z.bus_check(got, rcfg["cap_height"], cl, hd)
    assert ok
    head = vx.lib.stark_proof_head(proof, cfg)
    assert head.size == hd["o_queries"]
    vx.lib.stark_queries_verify(blob, proof, cfg)
    vx.lib.stark_queries_verify(blob, head, cfg)
    vx.lib.stark_queries_verify(blob, Z.garbled(proof, hd), cfg)
    for p in (head, Z.garbled(proof, hd)):
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(p, cfg)


def test_refusals_leave_the_context_working(ctx, vx, oracle):
    proof, rcfg = gpu_proof(ctx, "fib8")
    cfg = pcfg(ctx, rcfg)
    g = Z.group("fib8")
    blob = ctx.stark_queries_prove(proof, cfg)

    def same_again():
        assert (ctx.stark_queries_prove(proof, cfg) == blob).all()

    # arity 3: FriFoldAir is compiled for 16 values per leaf
    cfg3 = ctx.stark_config(num_queries=5, arity_bits=3)
    air, trace, pub, _ = Z.inner("fib8")
    proof3 = ctx.stark_prove(air.ID, ctx.from_host(trace), 8, pub, cfg3)
    with pytest.raises(vx.VxError) as e:
        ctx.stark_queries_prove(proof3, cfg3)
    assert e.value.code == ERR_ARG
    same_again()
    # FibAir at 2^5 has no FRI layer
    t5, p5 = S.FibAir.trace(5)
    proof5 = ctx.stark_prove(S.FibAir.ID, ctx.from_host(t5), 5, p5, cfg)
    assert int(proof5[9]) == 0
    with pytest.raises(vx.VxError) as e:
        ctx.stark_queries_prove(proof5, cfg)
    assert e.value.code == ERR_ARG
    with pytest.raises(vx.VxError) as e:
        ctx.stark_queries_prove(proof5, cfg, out=np.zeros(1 << 16, dtype=np.uint64))
    assert e.value.code == ERR_ARG
    same_again()
    # a flipped sibling: query 3, the quotient tree -- named before anything is proven
    per = len(g["cl"]["trees"])
    c = g["cl"]["claims"][3 * per + 1]
    assert c["tree"] == 10
    bad = proof.copy()
    bad[c["sib_at"] + 5] ^= 1
    with pytest.raises(vx.VxError, match=r"query 3: the path of the quotient tree") as e:
        ctx.stark_queries_prove(bad, cfg)
    assert e.value.code == ERR_STATEMENT
    c = g["cl"]["claims"][1 * per + 2]
    assert c["tree"] == 0
    bad = proof.copy()
    bad[c["sib_at"]] ^= 1
    with pytest.raises(vx.VxError, match=r"query 1: the path of FRI layer 0") as e:
        ctx.stark_queries_prove(bad, cfg)
    assert e.value.code == ERR_STATEMENT
    same_again()
    # a changed row word is an inner proof the verifier refuses
    bad = proof.copy()
    bad[g["hd"]["o_queries"]] ^= 1
    with pytest.raises(vx.VxError) as e:
        ctx.stark_queries_prove(bad, cfg)
    assert e.value.code == ERR_STATEMENT
    # an output buffer one word short
    with pytest.raises(vx.VxError) as e:
        ctx.stark_queries_prove(proof, cfg, out=np.zeros(blob.size - 1, dtype=np.uint64))
    assert e.value.code == ERR_BUFSZ and e.value.needed == blob.size
    same_again()
    vx.lib.stark_queries_verify(blob, vx.lib.stark_proof_head(proof, cfg), cfg)
