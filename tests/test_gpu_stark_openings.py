"""A STARK proof's Merkle openings proven from the paths it carries, on the GPU: the witness of MerkleOpenSetAir from authentication
paths (k_merkle_path_states, 16 lanes per path, and the trace kernel's second source) and of LeafSpongeSetAir from rows handed over
directly equal the reference generators cell by cell, auxiliary columns and public inputs included; the blob of
vx_stark_openings_prove over real vx_stark_prove proofs equals the reference group prover's word for word, vx_stark_openings_verify
accepts it -- with every sibling of the inner proof zeroed too -- and refuses every change, a flipped sibling is refused by the
prover with VX_ERR_STATEMENT naming the query before anything is proven; and the same trace comes out of a GPU-built tree and out
of that tree's own paths."""
import numpy as np
import pytest

import fri_queries_ref as Q
import stark_openings_ref as SO
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
CHAL = SO.CHAL

pytestmark = pytest.mark.gpu

# ---- path states and trace.  name -> (depth of every tree, the one cap height, openings (tree, leaf)).  A block of 256 lanes holds
# 16 groups of 16 lanes: 1, 15, 16 and 17 paths; cap height 0 (every sibling from the proof) and cap height = log_leaves (none);
# log_leaves 1; depths 1, 5 and 9 in one launch (the groups of a wave run 9 levels, the shorter paths idle); index 0 and the last
# index; a duplicated opening
_mixed = [(2, 0x155), (0, 1), (1, 0), (1, 31), (2, 0), (2, 511), (0, 0), (2, 0x155), (1, 17), (2, 300), (1, 8), (0, 1), (2, 77), (1, 30), (2, 256), (1, 1), (2, 510)]
PATH_CASES = {
    "one_path_depth_1": ([1], 0, [(0, 1)]),
    "one_path_cap_is_the_leaves": ([3], 3, [(0, 5)]),
    "mixed_depths_17_paths_cap_0": ([1, 5, 9], 0, _mixed),
    "mixed_depths_16_paths_cap_1": ([1, 5, 9], 1, _mixed[:16]),
    "15_paths_cap_5_of_5": ([5, 9], 5, [(t % 2, (37 * t + 3) % 32) for t in range(15)]),
    "absent_tree_between": ([5, 0, 3], 2, [(2, 7), (0, 0), (0, 31), (2, 0)]),
}
_forests = {}


def forest(oracle, name):
    """the trees of a case (oracle.MerkleTree, built once, never modified) and the paths of its openings"""
    if name not in _forests:
        depths, cap_h, openings = PATH_CASES[name]
        rng = np.random.default_rng(len(name))
        trees = [oracle.MerkleTree(rng.integers(0, P, size=(1 << d, 6), dtype=np.uint64), cap_h) if d else None for d in depths]
        digests = [[int(v) for v in trees[t].leaf_digests()[i]] for t, i in openings]
        sibs = [np.array(trees[t].prove(i), dtype=np.uint64).reshape(-1, 4) for t, i in openings]
        _forests[name] = (trees, digests, sibs)
    return _forests[name]


@pytest.mark.parametrize("name", list(PATH_CASES))
def test_path_witness_equals_the_reference(ctx, vx, oracle, name):
    depths, cap_h, openings = PATH_CASES[name]
    trees, digests, sibs = forest(oracle, name)
    tree_of, leaf_idx = [t for t, _ in openings], [i for _, i in openings]
    caps = [t.cap if t is not None else np.zeros((1 << cap_h, 4), dtype=np.uint64) for t in trees]
    want, want_pub, _ = SO.paths_ref_trace(caps, depths, tree_of, leaf_idx, digests, sibs)
    log_n = want.shape[1].bit_length() - 1
    if name.startswith("mixed"):  # ... and what a table built from the trees themselves holds
        from_trees, pub_trees = Q.open_ref_trace(trees, tree_of, leaf_idx)
        assert (from_trees == want).all() and pub_trees == want_pub
    tb, pub = ctx.merkle_paths_air_trace(caps, depths, tree_of, leaf_idx, digests, sibs, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(Q.O_COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_MERKLE_OPEN_SET, tb, log_n, CHAL, vx.lib.VX_MERKLE_OPEN_SET_AIR_AUX_COLS, pub)
    want_aux, want_apub = Q.open_gen_aux(want, CHAL)
    got_aux = ab.download().reshape(Q.O_AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    assert S.check_trace(Q.open_air(), got, want_pub, CHAL, got_aux, want_apub) is None
    tb.free(), ab.free()


def test_a_path_that_does_not_reach_its_root_is_refused(ctx, vx, oracle):
    name = "mixed_depths_17_paths_cap_0"
    depths, cap_h, openings = PATH_CASES[name]
    trees, digests, sibs = forest(oracle, name)
    tree_of, leaf_idx = [t for t, _ in openings], [i for _, i in openings]
    caps = [t.cap for t in trees]
    for k, what in ((9, "sibling"), (16, "digest"), (4, "cap")):
        d2, s2, c2 = [list(d) for d in digests], [s.copy() for s in sibs], [c.copy() for c in caps]
        if what == "sibling":
            s2[k][8, 3] ^= np.uint64(1)  # the last level of a nine-level path
        elif what == "digest":
            d2[k][0] ^= 1
        else:
            c2[2][0, 0] ^= np.uint64(1)  # every path of tree 2 ends elsewhere: the first of them is named
            k = 0
        with pytest.raises(vx.VxError, match="opening %d .*does not reach the root" % k) as e:
            ctx.merkle_paths_air_trace(c2, depths, tree_of, leaf_idx, d2, s2, 12)
        assert e.value.code == -5  # VX_ERR_STATEMENT
    with pytest.raises(vx.VxError) as e:
        ctx.merkle_paths_air_trace(caps, depths, tree_of, leaf_idx, digests, sibs, 10)  # 105 levels need 2^12 rows
    assert e.value.code == -1
    with pytest.raises(vx.VxError) as e:
        ctx.merkle_paths_air_trace(caps, depths, [1] + tree_of[1:], [32] + leaf_idx[1:], digests, [sibs[2]] + sibs[1:], 12)  # not a leaf of tree 1
    assert e.value.code == -1
    tb, _ = ctx.merkle_paths_air_trace(caps, depths, tree_of, leaf_idx, digests, sibs, 12)  # the context is usable after every refusal
    tb.free()


# ---- the sponge from rows: a single partial block, a seven-word block, exactly one block, a one-word tail, two and four full blocks,
# four blocks and a one-word tail; 1, 16 and 17 leaves (a block of 256 lanes holds 16 groups)
@pytest.mark.parametrize("n_leaves", [1, 16, 17])
@pytest.mark.parametrize("L", [5, 7, 8, 9, 16, 32, 33])
def test_sponge_witness_from_rows_equals_the_reference(ctx, vx, oracle, L, n_leaves):
    rng = np.random.default_rng(100 * L + n_leaves)
    rows = rng.integers(0, P, size=(n_leaves, L), dtype=np.uint64)
    rows[0, 0], rows[-1, -1] = 0, P - 1
    tree_of = [[9, 3, 8][k % 3] for k in range(n_leaves)]
    leaf_idx = [int(v) for v in rng.integers(0, 1 << 20, size=n_leaves)]
    leaf_idx[0] = 0
    if n_leaves > 1:
        rows[1], tree_of[1], leaf_idx[1] = rows[0], tree_of[0], leaf_idx[0]  # a duplicate
    want, want_pub, digs = Q.sponge_ref_trace(tree_of, leaf_idx, rows)
    log_n = want.shape[1].bit_length() - 1
    tb, pub = ctx.leaf_sponge_rows_air_trace(tree_of, leaf_idx, rows, log_n)
    assert [int(v) for v in pub] == want_pub
    got = tb.download().reshape(Q.S_COLS, -1)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first differing (column, row): %s" % bad[:1]
    assert [[int(v) for v in d] for d in digs] == [SO.leaf_digest(r) for r in rows]
    ab, apub = ctx.stark_aux_trace(vx.lib.VX_AIR_LEAF_SPONGE_SET, tb, log_n, CHAL, vx.lib.VX_LEAF_SPONGE_SET_AIR_AUX_COLS, pub)
    want_aux, want_apub = Q.sponge_gen_aux(want, CHAL, want_pub)
    got_aux = ab.download().reshape(Q.S_AUX, -1)
    bad = np.argwhere(got_aux != want_aux)
    assert bad.size == 0, "first differing auxiliary (column, row): %s" % bad[:1]
    assert [int(v) for v in apub[:2]] == want_apub
    assert S.check_trace(Q.sponge_air(), got, want_pub, CHAL, got_aux, want_apub) is None
    tb.free(), ab.free()


def test_sponge_from_rows_refuses_bad_arguments(ctx, vx):
    rows = np.arange(16, dtype=np.uint64).reshape(2, 8)
    for kw in (dict(rows=rows[:, :4]), dict(log_n=5), dict(rows=np.array([[P] + [0] * 7, [0] * 8], dtype=np.uint64))):
        args = dict(tree_of=[0, 1], leaf_idx=[3, 4], rows=rows, log_n=6)
        args.update(kw)
        with pytest.raises(vx.VxError) as e:
            ctx.leaf_sponge_rows_air_trace(**args)
        assert e.value.code == -1


# ---- real vx_stark_prove proofs, five queries each
PROOFS = {
    "fib_2^5": (S.FibAir, 5, {}),                    # no FRI layer, every tree a no-op tree: the openings table alone
    "fib_2^8": (S.FibAir, 8, {}),                    # one layer: a sponge table of 32-word leaves
    "lookup_2^8": (S.LookupAir, 8, {}),              # auxiliary columns: leaf lengths 6, 7 and 32, four tables
    "fib_2^8_arity_3": (S.FibAir, 8, dict(arity_bits=3)),  # 16-word layer leaves
    "fib_2^8_rate_2": (S.FibAir, 8, dict(rate_bits=2)),    # an LDE of 2^10
}
SHAPES = {"fib_2^5": ([6, 2, 0, 4, 0, 4, 5], []), "fib_2^8": ([9, 2, 0, 4, 1, 4, 5], [32]), "lookup_2^8": ([9, 7, 6, 4, 1, 4, 5], [6, 7, 32]),
          "fib_2^8_arity_3": ([9, 2, 0, 3, 1, 4, 5], [16]), "fib_2^8_rate_2": ([10, 2, 0, 4, 1, 4, 5], [32])}


def flipped(words, at):
    w = np.array(words, dtype=np.uint64)
    w[at] ^= np.uint64(1)
    return w


@pytest.mark.parametrize("name", list(PROOFS))
def test_openings_of_real_proofs(ctx, vx, oracle, name):
    air, log_n, over = PROOFS[name]
    over = dict(over, num_queries=5)
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    trace, pub = air.trace(log_n)
    proof = ctx.stark_prove(air.ID, ctx.from_host(trace), log_n, pub, cfg)
    blob = ctx.stark_openings_prove(proof, cfg)
    # ---- the blob is the reference group's, word for word
    cl = SO.extract(proof, ocfg)
    tabs, lens = SO.tables(cl)
    assert (cl["shape"], lens) == SHAPES[name]
    n_tab = 1 + len(lens)
    assert [int(v) for v in blob[:SO.HDR]] == [SO.MAGIC] + cl["shape"] + [n_tab]
    want = SO.prove(tabs, ocfg)
    got = SO.unwrap(blob)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size, k
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "table %d: first differing proof word: %d" % (k, bad[0])
    assert [int(g[2]) for g in got] == [t.shape[1].bit_length() - 1 for t, _ in tabs]
    ok, chal = SO.bus_check(got, ocfg["cap_height"], cl)
    assert ok
    for p, a, (_, tpub) in zip(got, SO.airs(n_tab), tabs):
        S.verify(p, ocfg, expect_air=a.ID, expect_public=tpub, ext_chal=chal)
    # ---- the verifier accepts, reads no sibling, and refuses every change
    vx.lib.stark_openings_verify(blob, proof, cfg, expect_air=air.ID, expect_public=pub)
    vx.lib.stark_openings_verify(blob, SO.zero_siblings(proof, cl), cfg)
    with pytest.raises(vx.VxError):
        vx.lib.stark_verify(SO.zero_siblings(proof, cl), cfg)

    def refused(blob_=blob, proof_=proof, match=None):
        with pytest.raises(vx.VxError, match=match) as e:
            vx.lib.stark_openings_verify(blob_, proof_, cfg)
        assert e.value.code == -5

    LN, cm, ca, a, NL, cap_h, n_q = cl["shape"]
    q0 = int(min(c["sib_at"] for c in cl["claims"])) - cm
    refused(proof_=flipped(proof, q0 + 1))                                        # one row word
    if NL:
        refused(proof_=flipped(proof, cl["claims"][-1]["sib_at"] - 3))            # one layer-leaf word
    refused(proof_=flipped(proof, 12 + NL + len(pub) + 5))                        # one cap word
    other_trace, other_pub = air.trace(log_n, 3, 1) if air is S.FibAir else air.trace(log_n, seed=12)
    other = ctx.stark_prove(air.ID, ctx.from_host(other_trace), log_n, other_pub, cfg)
    refused(proof_=other)                                                         # the blob of another proof of the same shape
    refused(blob_=blob[:-9], match="inconsistent")                                # truncated by 9 words
    at = SO.HDR + n_tab
    offsets = [0, 1, SO.HDR - 1, SO.HDR]
    for k in range(n_tab):
        offsets += [at + 2, at + int(blob[SO.HDR + k]) - 1]
        at += int(blob[SO.HDR + k])
    for w in offsets:
        refused(blob_=flipped(blob, w))
    # ---- the prover refuses a proof whose path does not reach its root, naming the query, before anything is proven
    per = len(cl["trees"])
    c = cl["claims"][3 * per + per - 1]  # the last tree of query 3: the layer, or the quotient tree
    with pytest.raises(vx.VxError, match="query 3: the path of %s" % ("FRI layer 0" if NL else "the quotient tree")) as e:
        ctx.stark_openings_prove(flipped(proof, c["sib_at"] + c["sib"].size - 1), cfg)
    assert e.value.code == -5  # VX_ERR_STATEMENT
    with pytest.raises(vx.VxError) as e:
        ctx.stark_openings_prove(flipped(proof, q0 + 1), cfg)  # a changed row is not the proof's any more: the inner verifier says so
    assert e.value.code == -5
    with pytest.raises(vx.VxError) as e:
        ctx.stark_openings_prove(proof, cfg, out=np.zeros(blob.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == blob.size  # VX_ERR_BUFSZ with the length set
    again = ctx.stark_openings_prove(proof, cfg)  # the context is usable after every refusal
    assert (again == blob).all()


def test_more_than_eight_layers_are_refused(ctx, vx):
    over = dict(arity_bits=1, final_poly_bits=0, cap_height=0, num_queries=2, pow_bits=0)
    cfg = ctx.stark_config(**over)
    trace, pub = S.FibAir.trace(10)
    proof = ctx.stark_prove(S.FibAir.ID, ctx.from_host(trace), 10, pub, cfg)  # ten layers
    assert int(proof[9]) == 10
    with pytest.raises(vx.VxError) as e:
        ctx.stark_openings_prove(proof, cfg)
    assert e.value.code == -1  # VX_ERR_ARG
    with pytest.raises(vx.VxError, match="fold layers") as e:
        vx.lib.stark_merkle_claims(proof, cfg)
    assert e.value.code == -1


def test_arity_1_layer_leaves_are_their_own_digests(ctx, vx, oracle):
    """arity_bits 1: a layer leaf is 4 words, so the layer trees are no-op trees as well and the openings table is alone"""
    over = dict(arity_bits=1, final_poly_bits=3, num_queries=3, pow_bits=4)
    cfg, ocfg = ctx.stark_config(**over), dict(S.DEFAULT_CFG, **over)
    trace, pub = S.FibAir.trace(5)
    proof = ctx.stark_prove(S.FibAir.ID, ctx.from_host(trace), 5, pub, cfg)
    cl = SO.extract(proof, ocfg)
    assert cl["shape"] == [6, 2, 0, 1, 2, 4, 3] and SO.sponge_lengths(cl) == []
    blob = ctx.stark_openings_prove(proof, cfg)
    assert int(blob[SO.HDR - 1]) == 1
    vx.lib.stark_openings_verify(blob, SO.zero_siblings(proof, cl), cfg, expect_air=S.FibAir.ID, expect_public=pub)
    with pytest.raises(vx.VxError):
        vx.lib.stark_openings_verify(blob, flipped(proof, cl["claims"][-1]["sib_at"] - 1), cfg)  # a layer-leaf word


# ---- unchanged: the same table from a GPU-built tree and from that tree's own paths
def test_the_trace_from_trees_equals_the_trace_from_their_paths(ctx, vx):
    rng = np.random.default_rng(5)
    depths, cap_h, L = [3, 6], 2, 9
    data = [rng.integers(0, P, size=(1 << d, L), dtype=np.uint64) for d in depths]
    bufs = [ctx.from_host(d) for d in data]
    trees = [ctx.merkle(b, 1 << d, L, vx.lib.VX_LEAVES_ROW_MAJOR, cap_h) for b, d in zip(bufs, depths)]
    openings = [(1, 0), (0, 7), (1, 63), (1, 21), (0, 0), (1, 21)]
    tree_of, leaf_idx = [t for t, _ in openings], [i for _, i in openings]
    log_n = 10  # 32 x (6 + 3 + 6 + 6 + 3 + 6) = 960 rows
    ta, pub_a = ctx.merkle_open_set_air_trace(trees, tree_of, leaf_idx, log_n)
    leaf_digests = [t.leaf_digests() for t in trees]
    digests = [leaf_digests[t][i] for t, i in openings]
    sibs = [trees[t].open([i])[0] for t, i in openings]
    tb, pub_b = ctx.merkle_paths_air_trace([t.cap() for t in trees], depths, tree_of, leaf_idx, digests, sibs, log_n)
    assert (pub_a == pub_b).all()
    a, b = ta.download(), tb.download()
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "first differing trace word: %d" % bad[0]
    assert int(a.reshape(Q.O_COLS, -1)[Q.M.ACT].sum()) == 32 * 30
    ta.free(), tb.free()
    for t in trees:
        t.free()
    for b_ in bufs:
        b_.free()
