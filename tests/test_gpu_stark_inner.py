"""An inner proof's query phase AND transcript on one bus, on the GPU: for real vx_stark_prove proofs the blob of vx_stark_inner_prove
equals the reference group (tests/stark_inner_ref.py: the restated AIRs under the reference prover) table by table, word for word,
and vx_stark_inner_verify accepts it with the whole proof, with the proof's head alone and with the query section replaced by junk.
Proving twice, and on contexts of either stream mode, gives the same bytes.  Refusals: arity 3, a proof without a FRI layer, a flipped
sibling (named by query and tree before anything is proven), a flipped word of the query section, an output buffer one word short;
after each the context proves the same blob again.  Tables of at most 2^13 rows."""
import numpy as np
import pytest

import stark_inner_ref as I
from oracle import stark_ref as S
from test_gpu_table_streams import make_context

Z, T = I.Z, I.T
pytestmark = pytest.mark.gpu
ERR_ARG, ERR_BUFSZ, ERR_STATEMENT = -1, -4, -5


def pcfg(ctx, cfg):
    keys = ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")
    return ctx.stark_config(**{k: cfg[k] for k in keys})


def gpu_proof(ctx, name):
    """the inner proof made on the GPU -- word for word the reference prover's; under external lookup challenges, which
    Context.stark_prove does not take, the reference prover's itself"""
    g = I.inner(name)
    if g["ext"] is not None:
        return g["proof"].copy()
    proof = ctx.stark_prove(g["air"].ID, ctx.from_host(g["trace"]), g["trace"].shape[1].bit_length() - 1, g["pub"], pcfg(ctx, g["cfg"]))
    assert proof.size == g["proof"].size and (proof == g["proof"]).all()
    return proof


@pytest.mark.parametrize("name", list(I.INNER))
def test_group_blob_equals_the_reference_group(ctx, vx, oracle, name):
    proof = gpu_proof(ctx, name)
    g = I.group(name)
    cfg, cl, hd, ext = pcfg(ctx, g["cfg"]), g["cl"], g["hd"], g["ext"]
    words = g["chain"][1]
    blob = ctx.stark_inner_prove(proof, cfg, ext)
    n = len(g["proofs"])
    assert n == 5 + len(Z.X.sponge_lengths(cl)) and max(tr.shape[1] for tr, _ in g["tabs"]) <= 1 << 13
    assert [int(v) for v in blob[:I.HDR]] == [I.MAGIC] + cl["shape"] + [n, len(words), len(g["chals"])]
    assert I.blob_claims(blob) == g["chals"]
    got, _ = I.unwrap(blob)
    for k, (gp, wp) in enumerate(zip(got, g["proofs"])):
        wp = np.array(wp, dtype=np.uint64)
        assert gp.size == wp.size, "table %d" % k
        bad = np.flatnonzero(gp != wp)
        assert bad.size == 0, "first differing word of table %d: %d" % (k, bad[0])
    assert blob.size == g["blob"].size and (blob == g["blob"]).all()
    assert I.bus_check(got, g["cfg"]["cap_height"], cl, hd, words, g["chals"])
    head, junk = vx.lib.stark_proof_head(proof, cfg), Z.garbled(proof, hd)
    assert head.size == hd["o_queries"]
    for p in (proof, head, junk):
        vx.lib.stark_inner_verify(blob, p, cfg, ext_chal=ext)
    for p in (head, junk):
        with pytest.raises(vx.VxError):
            vx.lib.stark_verify(p, cfg)
    assert (ctx.stark_inner_prove(proof, cfg, ext) == blob).all()  # proving twice gives the same bytes


def test_own_and_shared_contexts_give_the_same_bytes(vx, oracle):
    g = I.inner("fib8")
    blobs = {}
    cs = {m: make_context(vx, m) for m in ("own", "shared")}  # two contexts in one process
    try:
        for m, c in cs.items():
            blobs[m] = c.stark_inner_prove(g["proof"], pcfg(c, g["cfg"])).copy()
    finally:
        for c in cs.values():
            c.close()
    assert blobs["own"].size == blobs["shared"].size and (blobs["own"] == blobs["shared"]).all(), "the blobs of the two modes differ"
    vx.lib.stark_inner_verify(blobs["own"], g["proof"], vx.lib.default_stark_config(num_queries=g["cfg"]["num_queries"]))


def test_refusals_leave_the_context_working(ctx, vx, oracle):
    proof = gpu_proof(ctx, "fib8")
    g = I.group("fib8")
    cfg = pcfg(ctx, g["cfg"])
    blob = ctx.stark_inner_prove(proof, cfg)

    def same_again():
        assert (ctx.stark_inner_prove(proof, cfg) == blob).all()

    # arity 3: FriFoldAir is compiled for 16 values per leaf
    cfg3 = ctx.stark_config(num_queries=5, arity_bits=3)
    proof3 = ctx.stark_prove(g["air"].ID, ctx.from_host(g["trace"]), 8, g["pub"], cfg3)
    with pytest.raises(vx.VxError) as e:
        ctx.stark_inner_prove(proof3, cfg3)
    assert e.value.code == ERR_ARG
    same_again()
    # FibAir at 2^5 has no FRI layer
    t5, p5 = S.FibAir.trace(5)
    proof5 = ctx.stark_prove(S.FibAir.ID, ctx.from_host(t5), 5, p5, cfg)
    assert int(proof5[9]) == 0
    with pytest.raises(vx.VxError) as e:
        ctx.stark_inner_prove(proof5, cfg)
    assert e.value.code == ERR_ARG
    with pytest.raises(vx.VxError, match="no query-phase group") as e:
        ctx.stark_inner_prove(proof5, cfg, out=np.zeros(1 << 16, dtype=np.uint64))
    assert e.value.code == ERR_ARG
    same_again()
    # a flipped sibling: query 3, the quotient tree -- named before anything is proven
    per = len(g["cl"]["trees"])
    c = g["cl"]["claims"][3 * per + 1]
    assert c["tree"] == 10
    bad = proof.copy()
    bad[c["sib_at"] + 5] ^= 1
    with pytest.raises(vx.VxError, match=r"stark inner: query 3: the path of the quotient tree") as e:
        ctx.stark_inner_prove(bad, cfg)
    assert e.value.code == ERR_STATEMENT
    c = g["cl"]["claims"][1 * per + 2]
    assert c["tree"] == 0
    bad = proof.copy()
    bad[c["sib_at"]] ^= 1
    with pytest.raises(vx.VxError, match=r"stark inner: query 1: the path of FRI layer 0") as e:
        ctx.stark_inner_prove(bad, cfg)
    assert e.value.code == ERR_STATEMENT
    same_again()
    # a changed word of the query section is an inner proof the verifier refuses; so is the head alone, which has no query to prove
    bad = proof.copy()
    bad[g["hd"]["o_queries"]] ^= 1
    out = np.zeros(blob.size, dtype=np.uint64)
    with pytest.raises(vx.VxError, match="stark inner:") as e:
        ctx.stark_inner_prove(bad, cfg, out=out)
    assert e.value.code == ERR_STATEMENT and not out.any()  # nothing is proven
    with pytest.raises(vx.VxError, match="truncated") as e:
        ctx.stark_inner_prove(proof[:g["hd"]["o_queries"]], cfg, out=out)
    assert e.value.code == ERR_STATEMENT
    same_again()
    # an output buffer one word short
    with pytest.raises(vx.VxError) as e:
        ctx.stark_inner_prove(proof, cfg, out=np.zeros(blob.size - 1, dtype=np.uint64))
    assert e.value.code == ERR_BUFSZ and e.value.needed == blob.size
    same_again()
    vx.lib.stark_inner_verify(blob, vx.lib.stark_proof_head(proof, cfg), cfg)
