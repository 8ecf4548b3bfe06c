"""The generic bus group (include/vx.h vx_bus_group_*) without a GPU: the product's vx_bus_group_verify accepts the two-table
reference-prover proof of tests/test_leaf_sponge.py wrapped as a VXBGRP01 blob -- the verifier being the outside party that receives
the 27 row words --, accepts the same with the openings table under a REGISTERED id (a declared run-time table) and under no other
id, refuses every way of changing the outside messages, the expectations, the header and the body, and vx_bus_group_proof_bound
states the admission rules without a GPU.  Everything is exact."""
import numpy as np
import pytest

import bus_programs as BP
import leaf_sponge_ref as R
import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CFG = dict(S.DEFAULT_CFG, num_queries=8)
D, L = 3, 9
MAGIC = int.from_bytes(b"VXBGRP01", "little")
TAG_ROW = 9


def pcfg(vx):
    return vx.lib.default_stark_config(num_queries=CFG["num_queries"])


def wrap(proofs, ids):
    """table proofs as a VXBGRP01 blob: magic, n, one length per proof, the proofs with `ids` in their id words"""
    ps = [np.array(p, dtype=np.uint64) for p in proofs]
    for p, i in zip(ps, ids):
        p[1] = i
    return np.concatenate([np.array([MAGIC, len(ps)] + [p.size for p in ps], dtype=np.uint64)] + ps)


def row_messages(idx, rows):
    """the verifier RECEIVES every word of every claimed row once: (index, position, word, -, TAG_ROW, 0 - 1)"""
    return np.array([[int(i), j, int(v), 0, TAG_ROW, P - 1] for i, r in zip(idx, rows) for j, v in enumerate(r)], dtype=np.uint64)


@pytest.fixture(scope="module")
def pair(oracle, vx):
    """ONE two-table reference-prover proof (8 leaves of 9 words, cap height 1, openings [1, 6, 3]): the proofs, both tables' public
    inputs, the outside messages, and the blob under the compiled ids"""
    leaves = np.random.default_rng(5 + 100 * L).integers(0, P, size=(1 << D, L), dtype=np.uint64)
    tree = oracle.MerkleTree(leaves, 1)
    idx = [1, 6, 3]
    rows = leaves[idx]
    p_open, p_sponge = R.prove_rows(tree, idx, rows, CFG)
    pubs = [[int(v) for v in S.proof_peek(p, CFG["cap_height"])[0]] for p in (p_open, p_sponge)]
    out = row_messages(idx, rows)
    assert out.shape == (27, 6)
    blob = wrap([p_open, p_sponge], [vx.lib.VX_AIR_MERKLE_OPEN, vx.lib.VX_AIR_LEAF_SPONGE])
    return p_open, p_sponge, pubs, out, blob


def expect_of(vx, pubs, first=None):
    return [(vx.lib.VX_AIR_MERKLE_OPEN if first is None else first, pubs[0]), (vx.lib.VX_AIR_LEAF_SPONGE, pubs[1])]


def test_reference_round_trip_through_the_product_verifier(vx, pair):
    p_open, p_sponge, pubs, out, blob = pair
    assert [int(v) for v in blob[:4]] == [MAGIC, 2, p_open.size, p_sponge.size]
    vx.lib.bus_group_verify(blob, expect_of(vx, pubs), pcfg(vx), out)
    got = vx.lib.split_bus_group(blob)
    assert len(got) == 2 and (got[0][2:] == p_open[2:]).all() and (got[1][2:] == p_sponge[2:]).all()
    # the order of the outside messages is nobody's business, and a message with multiplicity 0 says nothing
    vx.lib.bus_group_verify(blob, expect_of(vx, pubs), pcfg(vx), np.concatenate([out[::-1], np.array([[5, 5, 5, 5, 5, 0]], dtype=np.uint64)]))


def test_a_run_time_table_is_accepted_under_its_registered_id_alone(vx, pair):
    """bus_programs.merkle_open() DECLARES MerkleOpenAir's two messages; the constraints the library derives are the hand-written ones,
    so the reference prover's proof of the restatement, made under the challenges of the pair, is a proof under the registered id"""
    p_open, p_sponge, pubs, out, _ = pair
    cfg = pcfg(vx)
    mine, other = BP.merkle_open().register(), BP.leaf_noop().register()
    try:
        blob = wrap([p_open, p_sponge], [mine, vx.lib.VX_AIR_LEAF_SPONGE])
        vx.lib.bus_group_verify(blob, expect_of(vx, pubs, mine), cfg, out)
        with pytest.raises(vx.VxError, match="unexpected AIR"):
            vx.lib.bus_group_verify(blob, expect_of(vx, pubs), cfg, out)  # the compiled id is another id
        twin = BP.merkle_open().register()  # the same program registered twice has two ids
        try:
            with pytest.raises(vx.VxError, match="unexpected AIR"):
                vx.lib.bus_group_verify(blob, expect_of(vx, pubs, twin), cfg, out)
            vx.lib.bus_group_verify(wrap([p_open, p_sponge], [twin, vx.lib.VX_AIR_LEAF_SPONGE]), expect_of(vx, pubs, twin), cfg, out)
        finally:
            vx.lib.air_unregister(twin)
        with pytest.raises(vx.VxError):  # another registered program: another number of public inputs, other constraints
            vx.lib.bus_group_verify(wrap([p_open, p_sponge], [other, vx.lib.VX_AIR_LEAF_SPONGE]), [(other, pubs[0][:4]), (vx.lib.VX_AIR_LEAF_SPONGE, pubs[1])], cfg, out)
    finally:
        vx.lib.air_unregister(mine), vx.lib.air_unregister(other)
    with pytest.raises(vx.VxError, match="names no AIR") as e:  # a retired id
        vx.lib.bus_group_verify(blob, expect_of(vx, pubs, mine), cfg, out)
    assert e.value.code == -1


def test_refusals(vx, pair):
    p_open, p_sponge, pubs, out, blob = pair
    cfg = pcfg(vx)
    exp = expect_of(vx, pubs)

    def refused(blob_=blob, expect=exp, outside=out, match=None, code=-5):
        with pytest.raises(vx.VxError, match=match) as e:
            vx.lib.bus_group_verify(blob_, expect, cfg, outside)
        assert e.value.code == code

    for col in range(4):  # one outside word changed: index, position, word, the absent slot
        o = out.copy()
        o[13, col] ^= 1
        refused(outside=o, match="does not balance")
    o = out.copy()
    o[13, 4] = 8  # ... and the tag
    refused(outside=o, match="does not balance")
    refused(outside=out[:-1], match="does not balance")                       # one message dropped
    refused(outside=np.concatenate([out, out[4:5]]), match="does not balance")  # one duplicated
    o = out.copy()
    o[0, 5] = 1  # sent instead of received
    refused(outside=o, match="does not balance")
    refused(outside=(), match="does not balance")                             # a closed bus is another statement
    refused(blob_=wrap([p_sponge, p_open], [vx.lib.VX_AIR_LEAF_SPONGE, vx.lib.VX_AIR_MERKLE_OPEN]))  # the two proofs swapped
    refused(blob_=wrap([p_sponge, p_open], [vx.lib.VX_AIR_MERKLE_OPEN, vx.lib.VX_AIR_LEAF_SPONGE]))  # ... under the expected ids
    for t, q in ((0, 0), (0, 8), (1, 0), (1, 13)):  # a changed expected public input
        pb = [list(pubs[0]), list(pubs[1])]
        pb[t][q] ^= 1
        refused(expect=expect_of(vx, pb), match="public input %d differs" % q)
    refused(expect=[exp[0], (exp[1][0], pubs[1][:13])], match="public inputs")  # ... and their number
    refused(expect=exp[:1], match="different request")                        # n of 1
    refused(expect=exp + [exp[1]], match="different request")                 # n of 3
    o = out.copy()
    o[3, 2] = P
    refused(outside=o, match="outside message 3 has a non-canonical word at 2")
    o = out.copy()
    o[26, 5] = 2**64 - 1
    refused(outside=o, match="outside message 26 has a non-canonical word at 5")
    o = out.copy()
    o[7, 4] = 1 << 16
    refused(outside=o, match="outside message 7 has a tag of 2\\^16 or more")
    refused(expect=[], match="0 tables", code=-1)
    refused(expect=[exp[0]] * 17, match="17 tables", code=-1)
    refused(expect=[(vx.lib.VX_AIR_FIBONACCI, [1, 1, 2]), exp[1]], match="table 0 \\(air 1\\) has no logUp round", code=-1)
    refused(expect=[exp[0], (3, [])], match="table 1 names no AIR", code=-1)


def test_truncated_and_damaged_blobs_are_refused(vx, pair):
    p_open, p_sponge, pubs, out, blob = pair
    cfg, exp = pcfg(vx), expect_of(vx, pubs)
    hdr = 4
    for w in range(hdr):
        for bit in (0, 1, 7, 31, 63):
            bad = blob.copy()
            bad[w] ^= np.uint64(1 << bit)
            with pytest.raises(vx.VxError):
                vx.lib.bus_group_verify(bad, exp, cfg, out)
    cuts = list(range(0, hdr + 20)) + list(range(hdr + 20, blob.size, max(1, blob.size // 40))) + [hdr + p_open.size, blob.size - 1]
    for cut in cuts:
        with pytest.raises(vx.VxError):
            vx.lib.bus_group_verify(blob[:cut], exp, cfg, out)
        if cut > hdr + p_open.size:  # a consistent header over a truncated second proof
            short = blob[:cut].copy()
            short[3] = cut - hdr - p_open.size
            with pytest.raises(vx.VxError):
                vx.lib.bus_group_verify(short, exp, cfg, out)
    bad = blob.copy()  # one word of the body: the first proof's published total
    bad[hdr + 12 + int(p_open[9]) + len(pubs[0]) + (4 << CFG["cap_height"])] ^= 1
    with pytest.raises(vx.VxError):
        vx.lib.bus_group_verify(bad, exp, cfg, out)


def test_the_proof_bound_states_the_admission_rules(vx):
    lib = vx.lib
    cfg = pcfg(vx)
    ok = [(lib.VX_AIR_MERKLE_OPEN, None, 7, []), (lib.VX_AIR_LEAF_SPONGE, None, 9, []), (lib.VX_AIR_FRI_FOLD, None, 5, [])]
    want = 2 + len(ok)
    for air_id, _, log_n, _ in ok:
        need = lib.C.c_size_t(0)
        assert lib.load_library().vx_stark_proof_bound(air_id, lib.C.byref(cfg), log_n, lib.C.byref(need)) == 0
        want += need.value
    assert lib.bus_group_proof_bound(ok, cfg) == want
    mine = BP.made_up().register()  # a declared run-time table is admitted, one without an auxiliary round is not
    plain = vx.air_program.AirBuilder(2, 0)
    plain.assert_zero(plain.loc(0) * plain.loc(1))
    plain_id = plain.register()
    try:
        assert lib.bus_group_proof_bound([(mine, None, 4, [1])], cfg) > 0
        with pytest.raises(vx.VxError, match="table 0 \\(air %d" % plain_id) as e:
            lib.bus_group_proof_bound([(plain_id, None, 4, [])], cfg)
        assert e.value.code == -1
    finally:
        lib.air_unregister(mine), lib.air_unregister(plain_id)
    for tables, why in (([], "0 tables"), ([ok[0]] * (lib.VX_BUS_GROUP_MAX_TABLES + 1), "17 tables"), ([ok[0], (lib.VX_AIR_FIBONACCI, None, 7, [])], "table 1 \\(air 1"),
                        ([(lib.VX_AIR_LOOKUP, None, 8, [])], "table 0 \\(air 5"), ([ok[1], ok[0], (999, None, 7, [])], "table 2 \\(air 999"), ([(mine, None, 4, [])], "table 0")):
        with pytest.raises(vx.VxError, match=why) as e:
            lib.bus_group_proof_bound(tables, cfg)
        assert e.value.code == -1  # VX_ERR_ARG
    assert lib.bus_group_proof_bound([ok[0]] * lib.VX_BUS_GROUP_MAX_TABLES, cfg) > 0
