"""Verifying on the GPU.  k_merkle_check on its own (Context.merkle_check) against forests built by the oracle: every leaf length
at which the sponge takes another path, depths 1, 5 and 9 in one launch, cap height 0 and cap height = log_leaves, 1 / 15 / 16 / 17
claims (a block holds 16 groups), the first and the last index, a duplicate; every refusal names the smallest failing claim and
leaves the context usable.  Then the three _dev verifiers: for the reference prover's proofs, the corruption sample and the double
defects of tests/test_verify_deferred.py, and for header_range and rotate blobs proven here and tampered with, they answer as the host
verifiers do -- the same code, the same message, word for word."""
import numpy as np
import pytest

import verify_dev_cases as V

P = V.P
ERR_ARG, ERR_STATEMENT = -1, -5
pytestmark = pytest.mark.gpu

# ---- the kernel alone.  name -> (per tree (log_leaves, leaf_len), the one cap height, openings (tree, leaf)).
_mixed = [(2, 0x155), (0, 1), (1, 0), (1, 31), (2, 0), (2, 511), (0, 0), (2, 0x155), (1, 17), (2, 300), (1, 8), (0, 1), (2, 77), (1, 30), (2, 256), (1, 1), (2, 510)]
LENS = [1, 4, 5, 7, 8, 9, 16, 32, 33]  # noop, noop, a partial block, seven words, exactly one block, a one-word tail, two blocks, four, four and a tail
FORESTS = {
    "every_leaf_length": ([(3, n) for n in LENS], 1, [(t, i) for t in range(len(LENS)) for i in (0, 7, 5)]),
    "every_leaf_length_interleaved": ([(3, n) for n in LENS], 0, [((5 * k) % len(LENS), (3 * k) % 8) for k in range(20)]),  # waves whose groups differ in steps
    "depths_1_5_9_cap_0_17_claims": ([(1, 6), (5, 6), (9, 6)], 0, _mixed),
    "depths_1_5_9_cap_1_16_claims": ([(1, 6), (5, 6), (9, 6)], 1, _mixed[:16]),
    "15_claims_cap_5_of_5": ([(5, 9), (9, 3)], 5, [(t % 2, (37 * t + 3) % 32) for t in range(15)]),
    "one_claim_depth_1": ([(1, 2)], 0, [(0, 1)]),
    "one_claim_cap_is_the_leaves": ([(3, 12)], 3, [(0, 5)]),
    "no_sibling_at_all_17_claims": ([(4, 5), (4, 1)], 4, [(k % 2, (7 * k) % 16) for k in range(17)]),
}
_forests = {}


def forest(oracle, name):
    """the trees of a case (oracle.MerkleTree, built once, never modified) -> the arguments of Context.merkle_check"""
    if name not in _forests:
        shapes, cap_h, openings = FORESTS[name]
        rng = np.random.default_rng(len(name))
        trees = []
        for d, n in shapes:
            rows = rng.integers(0, P, size=(1 << d, n), dtype=np.uint64)
            rows[0, 0], rows[-1, -1] = 0, P - 1
            trees.append(oracle.MerkleTree(rows, cap_h))
        leaves = [trees[t].leaves[i].copy() for t, i in openings]
        sibs = [np.array(trees[t].prove(i), dtype=np.uint64).reshape(-1, 4) for t, i in openings]
        for (t, i), row, sb in zip(openings, leaves, sibs):
            assert sb.shape[0] == shapes[t][0] - cap_h and oracle.merkle_verify(row, i, sb, trees[t].cap)
        _forests[name] = (np.stack([t.cap for t in trees]), [d for d, _ in shapes], [t for t, _ in openings], [i for _, i in openings], leaves, sibs)
    caps, log_leaves, tree_of, leaf_idx, leaves, sibs = _forests[name]
    return caps.copy(), log_leaves, tree_of, leaf_idx, [r.copy() for r in leaves], [s.copy() for s in sibs]


@pytest.mark.parametrize("name", list(FORESTS))
def test_merkle_check_accepts_the_oracles_paths(ctx, oracle, name):
    assert ctx.merkle_check(*forest(oracle, name)) is None


@pytest.mark.parametrize("n_claims", [0, 1, 15, 16, 17])
def test_merkle_check_at_the_edges_of_a_block(ctx, oracle, n_claims):
    caps, ll, tr, ix, lv, sb = forest(oracle, "depths_1_5_9_cap_0_17_claims")
    assert ctx.merkle_check(caps, ll, tr[:n_claims], ix[:n_claims], lv[:n_claims], sb[:n_claims]) is None
    if n_claims:  # the last claim of the batch is a live group: its failure is seen
        lv[n_claims - 1][0] ^= np.uint64(1)
        assert ctx.merkle_check(caps, ll, tr[:n_claims], ix[:n_claims], lv[:n_claims], sb[:n_claims]) == n_claims - 1


def test_merkle_check_names_the_smallest_failing_claim(ctx, vx, oracle):
    name = "depths_1_5_9_cap_0_17_claims"
    openings = FORESTS[name][2]
    assert openings[9] == (2, 300) and openings[0] == openings[7]  # a nine-level path; a duplicated claim
    again = lambda: ctx.merkle_check(*forest(oracle, name)) is None  # noqa: E731
    caps, ll, tr, ix, lv, sb = forest(oracle, name)
    lv[4][5] ^= np.uint64(1 << 33)  # a leaf word
    assert ctx.merkle_check(caps, ll, tr, ix, lv, sb) == 4 and again()
    caps, ll, tr, ix, lv, sb = forest(oracle, name)
    sb[9][8, 3] ^= np.uint64(1)  # the last level of the longest path
    assert ctx.merkle_check(caps, ll, tr, ix, lv, sb) == 9 and again()
    caps, ll, tr, ix, lv, sb = forest(oracle, name)
    caps[2, 0, 0] ^= np.uint64(1)  # every path of tree 2 ends elsewhere: the first of them is named
    assert ctx.merkle_check(caps, ll, tr, ix, lv, sb) == 0 and again()
    caps, ll, tr, ix, lv, sb = forest(oracle, name)
    sb[13][0, 0] ^= np.uint64(1)
    lv[7][0] ^= np.uint64(1)
    sb[16][2, 1] ^= np.uint64(1)  # three failing claims, in other blocks and other trees: the smallest index
    assert ctx.merkle_check(caps, ll, tr, ix, lv, sb) == 7 and again()
    # the leaf lengths: the last word of every row matters (the tail of a partial block, the one-word tail)
    name = "every_leaf_length"
    for k in range(len(FORESTS[name][2])):
        caps, ll, tr, ix, lv, sb = forest(oracle, name)
        lv[k][-1] = np.uint64((int(lv[k][-1]) + 1) % P)
        assert ctx.merkle_check(caps, ll, tr, ix, lv, sb) == k
    # VX_ERR_ARG: non-canonical words anywhere, an index outside its tree, a tree above its cap, a tree that is not there
    name = "depths_1_5_9_cap_1_16_claims"
    for where in ("leaf", "sibling", "cap", "index", "tree", "depth"):
        caps, ll, tr, ix, lv, sb = forest(oracle, name)
        ll = list(ll)
        if where == "leaf":
            lv[3][2] = np.uint64(P)
        elif where == "sibling":
            sb[9][7, 0] = np.uint64(2**64 - 1)
        elif where == "cap":
            caps[1, 1, 3] = np.uint64(P + 5)
        elif where == "index":
            ix = [32 if k == 3 else v for k, v in enumerate(ix)]  # claim 3 opens tree 1 of 32 leaves
        elif where == "tree":
            tr = [3 if k == 5 else v for k, v in enumerate(tr)]
        else:
            ll[0] = 0  # below the cap height
        with pytest.raises(vx.VxError) as e:
            ctx.merkle_check(caps, ll, tr, ix, lv, sb)
        assert e.value.code == ERR_ARG, (where, e.value)
        assert ctx.merkle_check(*forest(oracle, name)) is None
    caps, ll, tr, ix, lv, sb = forest(oracle, name)
    with pytest.raises(vx.VxError) as e:  # lengths that do not add up: a path one level short
        ctx.merkle_check(caps, ll, tr, ix, lv, sb[:-1] + [sb[-1][:-1]])
    assert e.value.code == ERR_ARG
    assert ctx.merkle_check(caps, ll, tr, ix, lv, sb) is None


# ---- vx_stark_verify_dev: the proofs and the sample of the CPU file
def both(ctx, vx, words, cfg, **kw):
    want = V.answer(vx.lib.stark_verify, words, cfg, **kw)
    assert V.answer(ctx.stark_verify, words, cfg, **kw) == want
    return want


@pytest.mark.parametrize("name", list(V.CASES))
def test_stark_verify_dev_answers_as_the_host_verifier(ctx, vx, oracle, name):
    proof, cfg, air = V.case(name)
    c, lay = V.pcfg(vx, cfg), V.layout(proof)
    assert both(ctx, vx, proof, c) == (0, "") and both(ctx, vx, proof, c, expect_air=air.ID) == (0, "")
    merkle = 0
    for what, bad in V.sample(proof):
        code, msg = both(ctx, vx, bad, c)
        assert code != 0, what
        merkle += "Merkle proof invalid" in msg
    assert merkle >= 12  # rows, layer evaluations and siblings end at the kernel's answer
    q = lay["queries"]
    bad = proof.copy()
    bad[q[1]["row_t"][0]] ^= np.uint64(1)
    bad[q[2]["sib_q"][0]] ^= np.uint64(1)
    assert "trace Merkle proof invalid (query 1)" in both(ctx, vx, bad, c)[1]
    bad = proof.copy()
    bad[q[1]["sib_q"][1] - 1] ^= np.uint64(1 << 7)
    bad[q[2]["row_t"][0]] ^= np.uint64(1)
    assert "quotient Merkle proof invalid (query 1)" in both(ctx, vx, bad, c)[1]
    for cut in (10, lay["o_queries"], q[1]["row_t"][0], proof.size - 1):
        assert both(ctx, vx, proof[:cut], c)[0] != 0
    assert "unexpected AIR" in both(ctx, vx, proof, c, expect_air=air.ID + 1)[1]
    assert both(ctx, vx, proof, c) == (0, "")  # the context is usable after every refusal


# ---- the circuit verifiers: the smallest requests the prover tests prove
QUERIES = 6
_blobs = {}


def hr_blob(ctx, vx, kind):
    """-> (blob, the positional arguments of header_range_verify behind it, its keyword arguments)"""
    if kind not in _blobs:
        ch = vx.synth.Chain(16, profile="Ptiny", stride=512)
        just = None if kind == "plain" else vx.lib.PackedJustification(vx.synth.Justification(ch.target_block, ch.target_hash, n_auth=9, n_signed=7), 12)
        out96, blob = ctx.header_range_prove(ctx.from_host(ch.headers), 512, ch.sizes, 16, ch.trusted_block, ch.trusted_hash, ch.target_block, ctx.stark_config(num_queries=QUERIES),
                                             just=just, n_segments=2 if kind == "two_segments" else 1)
        kw = {} if just is None else dict(authority_set_hash=just.sh.tobytes(), authority_set_id=just.struct.authority_set_id)
        _blobs[kind] = (blob.copy(), (16, ch.trusted_block, ch.trusted_hash, ch.target_block, out96), kw)
    return _blobs[kind]


def hr_tables(vx, blob):
    """(offset, length) of every table of a header_range blob, in the order the verifier reads them: segments, Merkle, commitment, Ed25519, SHA-512"""
    S, F = int(blob[16]), vx.lib.HR_FIXED
    lens = [int(v) for v in blob[F:F + S]] + [int(v) for v in blob[17:21]]  # blob order: segments, commitment, Merkle, Ed25519, SHA-512
    offs = np.cumsum([F + S] + lens[:-1])
    tabs = [(int(o), n) for o, n in zip(offs, lens)]
    return [t for t in tabs[:S] + [tabs[S + 1], tabs[S], tabs[S + 2], tabs[S + 3]] if t[1]]


def tampered(blob, tables):
    """the two tamperings of a blob whose tables lie at `tables`: a sibling of the last table's last query flipped; a row word of the
    first table's query 0 and a sibling of the second table's query 0"""
    lay = [V.layout(blob[o:o + n]) for o, n in tables]
    a = blob.copy()
    a[tables[-1][0] + lay[-1]["queries"][-1]["sib_q"][1] - 1] ^= np.uint64(1)
    b = blob.copy()
    b[tables[0][0] + lay[0]["queries"][0]["row_t"][0]] ^= np.uint64(1)
    b[tables[1][0] + lay[1]["queries"][0]["sib_t"][0]] ^= np.uint64(1)
    return a, b, len(lay[-1]["queries"]) - 1


@pytest.mark.parametrize("kind", ["plain", "justified", "two_segments"])
def test_header_range_verify_dev_answers_as_the_host_verifier(ctx, vx, kind):
    blob, args, kw = hr_blob(ctx, vx, kind)
    cfg = ctx.stark_config(num_queries=QUERIES)
    host = lambda b, a=args, k=kw: V.answer(vx.lib.header_range_verify, b, *a, cfg, **k)  # noqa: E731
    dev = lambda b, a=args, k=kw: V.answer(ctx.header_range_verify, b, *a, cfg, **k)  # noqa: E731
    assert host(blob) == dev(blob) == (0, "")
    tables = hr_tables(vx, blob)
    assert len(tables) == dict(plain=2, justified=5, two_segments=6)[kind]
    last, first, q_last = tampered(blob, tables)
    code, msg = dev(last)
    assert (code, msg) == host(last) and code == ERR_STATEMENT and "quotient Merkle proof invalid (query %d)" % q_last in msg
    code, msg = dev(first)
    assert (code, msg) == host(first) and code == ERR_STATEMENT and "trace Merkle proof invalid (query 0)" in msg
    # another request, another claimed output, a truncated blob, and a table proof whose host pass is refused BEHIND a table with a bad path
    mh, tb, th, tg, out = args
    for other in ((mh, tb, th, tg + 1, out), (mh, tb, bytes([th[0] ^ 1]) + th[1:], tg, out), (mh, tb, th, tg, out[:95] + bytes([out[95] ^ 1]))):
        assert dev(blob, other) == host(blob, other) != (0, "")
    assert "different request" in dev(blob, (mh, tb + 1, th, tg, out))[1]
    assert dev(blob[:-1]) == host(blob[:-1]) != (0, "")
    bad = first.copy()
    bad[tables[-1][0] + 3] ^= np.uint64(1)  # the last table's header
    assert dev(bad) == host(bad) and "trace Merkle proof invalid (query 0)" in dev(bad)[1]
    bad = blob.copy()
    bad[tables[0][0] + 3] ^= np.uint64(1)  # ... and the other way round: the first table's head is refused, no table behind it is read
    bad[tables[1][0] + V.layout(blob[tables[1][0]:sum(tables[1])])["queries"][0]["sib_t"][0]] ^= np.uint64(1)
    assert dev(bad) == host(bad) and "Merkle" not in dev(bad)[1]
    assert dev(blob) == (0, "")


def test_rotate_verify_dev_answers_as_the_host_verifier(ctx, vx):
    cfg = ctx.stark_config(num_queries=QUERIES)
    e = vx.synth.EpochEndHeader(140000, 5)
    sj = vx.synth.Justification(140000, e.hash, n_auth=7, n_signed=5, set_id=3)
    out32, blob = ctx.rotate_prove(ctx.from_host(e.padded), e.size, 140000, 5, e.start_position, e.new_pubkeys, vx.lib.PackedJustification(sj, 12), cfg)
    blob = blob.copy()
    host = lambda b, sid=3, sh=sj.authority_set_hash, o=out32: V.answer(vx.lib.rotate_verify, b, sid, sh, o, cfg)  # noqa: E731
    dev = lambda b, sid=3, sh=sj.authority_set_hash, o=out32: V.answer(ctx.rotate_verify, b, sid, sh, o, cfg)  # noqa: E731
    assert host(blob) == dev(blob) == (0, "")
    # blob order: header hash, current set, new set, Ed25519, SHA-512, epoch end; read as (header hash, epoch end, new set), then (current set, Ed25519, SHA-512)
    lens = [int(blob[k]) for k in (16, 17, 18, 19, 24, 27)]
    offs = [int(v) for v in np.cumsum([28] + lens[:-1])]
    tables = [(offs[k], lens[k]) for k in (0, 5, 2, 1, 3, 4)]
    last, first, q_last = tampered(blob, tables)
    code, msg = dev(last)
    assert (code, msg) == host(last) and code == ERR_STATEMENT and "quotient Merkle proof invalid (query %d)" % q_last in msg
    code, msg = dev(first)
    assert (code, msg) == host(first) and code == ERR_STATEMENT and "trace Merkle proof invalid (query 0)" in msg
    # a path of the second group fails and a table of the first group is refused by its own pass: the first group's answer
    bad = last.copy()
    lay = V.layout(blob[tables[1][0]:sum(tables[1])])
    pub = lay["regions"]["public"][1][0]  # the total the epoch-end table publishes
    bad[tables[1][0] + pub] ^= np.uint64(1)
    assert dev(bad) == host(bad) != (0, "") and "quotient Merkle" not in dev(bad)[1]
    assert dev(blob, sid=4) == host(blob, sid=4) and "different request" in dev(blob, sid=4)[1]
    assert dev(blob[:-1]) == host(blob[:-1]) != (0, "")
    assert dev(blob) == (0, "")
