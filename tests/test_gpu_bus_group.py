"""The generic bus group on the GPU (vx_bus_group_prove / _check): two run-time tables of different heights close a bus between them
and are proven together, in either order; a compiled table with a run-time one gives the proofs of the compiled pair word for word --
which are the reference prover's and the ones inside vx_merkle_rows_prove's blob --; and the balance check on the device (the records
kernels of both kinds of table, the sort, the match) names the message without a partner exactly: table, row, ordinal, net
multiplicity and the number of unmatched tuples are compared with a count in Python integers.  Nothing here takes a tolerance."""
import collections
import hashlib

import numpy as np
import pytest

import bus_programs as BP
import leaf_sponge_ref as R
import merkle_open_ref as M
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
TAG, TAG_ROW, TAG_OPEN = 20, 9, 8

pytestmark = pytest.mark.gpu

_ids = {}


def builder(vx, kind):
    """a table of three columns (t, v, m) that sends (t, v) under tag 20 with multiplicity m in {0, 2}, or receives it with m in {0, 1}"""
    b = vx.air_program.AirBuilder(3, 0)
    t, v, m = b.loc(0), b.loc(1), b.loc(2)
    if kind == "sender":
        b.assert_zero(m * (m - 2))
        b.send(TAG, [t, v], m)
    else:
        b.assert_zero(m * (m - 1))
        b.receive(TAG, [t, v], m)
    return b


def air_id(vx, name):
    """registered once for the module: the two made-up tables and the restated MerkleOpenAir of bus_programs.py"""
    if name not in _ids:
        _ids[name] = BP.merkle_open().register() if name == "merkle_open" else builder(vx, name).register()
    return _ids[name]


def closed_pair(seed=3):
    """sender [3][2^5]: rows 0..9 send (i, v_i) twice, the rest is idle with arbitrary cells; receiver [3][2^7] (two workgroups of the
    records kernel): tuple i is taken once on row 5 i + 2 and once on row 127 - 3 i, everything else is idle"""
    rng = np.random.default_rng(seed)
    snd = rng.integers(0, P, size=(3, 32), dtype=np.uint64)
    snd[2] = 0
    snd[0, :10], snd[2, :10] = np.arange(10), 2
    snd[1, 3] = P - 1
    rcv = rng.integers(0, P, size=(3, 128), dtype=np.uint64)
    rcv[2] = 0
    for i in range(10):
        for row in (5 * i + 2, 127 - 3 * i):
            rcv[0, row], rcv[1, row], rcv[2, row] = snd[0, i], snd[1, i], 1
    return snd, rcv


def balance(tables, outside=()):
    """the balance with Python integers: tables = [[(row, ordinal, (t0, t1, t2, t3, tag), m)]] -> None or (n_unmatched, table, message, row, net)"""
    net, low = collections.defaultdict(int), {}
    parties = list(tables) + [[(i, 0, tuple(int(x) for x in w[:5]), int(w[5])) for i, w in enumerate(outside)]]
    for k, msgs in enumerate(parties):
        for row, ordinal, tup, m in msgs:
            if m % P:
                net[tup] = (net[tup] + m) % P
                low[tup] = min(low.get(tup, (99, 0, 0)), (k, row, ordinal))
    bad = [t for t in net if net[t]]
    if not bad:
        return None
    first = min(bad, key=lambda t: low[t])
    return (len(bad), low[first][0], low[first][2], low[first][1], net[first])


def made_up_messages(tr, sign):
    return [(row, 0, (int(tr[0, row]), int(tr[1, row]), 0, 0, TAG), sign * int(tr[2, row]) % P) for row in range(tr.shape[1])]


def test_two_run_time_tables_close_a_bus_between_them(ctx, vx):
    snd, rcv = closed_pair()
    sid, rid = air_id(vx, "sender"), air_id(vx, "receiver")
    sb, rb = ctx.from_host(snd), ctx.from_host(rcv)
    cfg = ctx.stark_config(num_queries=8)
    tables = [(sid, sb, 5, []), (rid, rb, 7, [])]
    assert balance([made_up_messages(snd, 1), made_up_messages(rcv, -1)]) is None
    assert ctx.bus_group_check(tables) is None
    blob = ctx.bus_group_prove(tables, cfg)
    assert [int(v) for v in blob[:2]] == [vx.lib.BGRP_MAGIC, 2] and int(blob[2]) + int(blob[3]) == blob.size - 4 <= vx.lib.bus_group_proof_bound(tables, cfg) - 4
    p_s, p_r = vx.lib.split_bus_group(blob)
    assert [int(p_s[1]), int(p_s[2]), int(p_r[1]), int(p_r[2])] == [sid, 5, rid, 7]
    vx.lib.bus_group_verify(blob, [(sid, []), (rid, [])], cfg)
    assert (sb.download().reshape(3, -1) == snd).all() and (rb.download().reshape(3, -1) == rcv).all()  # the traces are left intact
    # the other order is another transcript: another blob, which verifies under the swapped expectations only
    other = ctx.bus_group_prove(tables[::-1], cfg)
    assert other.size == blob.size and (other[4:] != np.concatenate([p_r, p_s])).any()
    vx.lib.bus_group_verify(other, [(rid, []), (sid, [])], cfg)
    for b, exp in ((other, [(sid, []), (rid, [])]), (blob, [(rid, []), (sid, [])])):
        with pytest.raises(vx.VxError):
            vx.lib.bus_group_verify(b, exp, cfg)
    # neither table is a statement alone: its own proof of the pair is under shared challenges, and alone its bus does not close
    with pytest.raises(vx.VxError):
        vx.lib.bus_group_verify(np.concatenate([blob[:1], np.array([1, p_s.size], dtype=np.uint64), p_s]), [(sid, [])], cfg)
    with pytest.raises(vx.VxError, match="message 0 of table 0 .air %d. at row 0 has no partner .net multiplicity 2; 10 unmatched tuples" % sid) as e:
        ctx.bus_group_prove(tables[:1], cfg)
    assert e.value.code == -5  # VX_ERR_STATEMENT
    # ... unless the outside party takes what it sends: n = 1 is the same path, under the one-table transcript
    outside = [[i, int(snd[1, i]), 0, 0, TAG, P - 2] for i in range(10)]
    assert ctx.bus_group_check(tables[:1], outside) is None
    alone = ctx.bus_group_prove(tables[:1], cfg, outside)
    vx.lib.bus_group_verify(alone, [(sid, [])], cfg, outside)
    with pytest.raises(vx.VxError, match="does not balance"):
        vx.lib.bus_group_verify(alone, [(sid, [])], cfg, outside[:9])
    sb.free(), rb.free()


def test_sixteen_tables_meet_on_one_bus(ctx, vx):
    """VX_BUS_GROUP_MAX_TABLES tables, each on a context of its own: eight copies of the sender and of the receiver (every tuple is sent
    16 times and taken 16 times); a seventeenth table is refused"""
    snd, rcv = closed_pair()
    sid, rid = air_id(vx, "sender"), air_id(vx, "receiver")
    sb, rb = ctx.from_host(snd), ctx.from_host(rcv)
    cfg = ctx.stark_config(num_queries=8)
    tables = [(sid, sb, 5, []), (rid, rb, 7, [])] * 8
    assert len(tables) == vx.lib.VX_BUS_GROUP_MAX_TABLES and ctx.bus_group_check(tables) is None
    got = ctx.bus_group_check(tables[:-1])  # the last receiver left out: every tuple keeps a net of 2, and table 0 is named
    assert tuple(got) == (10, 0, 0, 0, 2)
    blob = ctx.bus_group_prove(tables, cfg)
    assert int(blob[1]) == 16 and len(vx.lib.split_bus_group(blob)) == 16
    vx.lib.bus_group_verify(blob, [(t[0], []) for t in tables], cfg)
    with pytest.raises(vx.VxError, match="17 tables") as e:
        ctx.bus_group_prove(tables + tables[:1], cfg)
    assert e.value.code == -1
    sb.free(), rb.free()


CHANGES = {
    # name -> (what is done to the receiver's trace, what is done to the outside messages)
    "one_receive_of_another_value": (lambda r: r.__setitem__((1, 127 - 3 * 4), (int(r[1, 127 - 3 * 4]) + 1) % P), None),
    "one_receive_missing": (lambda r: r.__setitem__((2, 5 * 7 + 2), 0), None),
    "an_idle_row_receives": (lambda r: r.__setitem__((2, 64), 1), None),
    "the_outside_party_sends_an_unknown_tuple": (None, [[7, 7, 7, 7, 7, 3]]),
    "the_outside_party_takes_a_tuple_a_third_time": (None, [[0, 0, 0, 0, 1 << 15, 0], [4, None, 0, 0, TAG, P - 1]]),
    "two_outside_messages_cancel": (None, [[9, 8, 7, 6, 5, 4], [9, 8, 7, 6, 5, P - 4]]),
}


@pytest.mark.parametrize("name", list(CHANGES))
@pytest.mark.parametrize("order", ["sender_first", "receiver_first"])
def test_the_balance_check_names_the_message_without_a_partner(ctx, vx, name, order):
    snd, rcv = closed_pair()
    on_receiver, outside = CHANGES[name]
    if on_receiver:
        on_receiver(rcv)
    outside = [[int(snd[1, w[0]]) if x is None else x for x in w] for w in (outside or [])]
    sid, rid = air_id(vx, "sender"), air_id(vx, "receiver")
    sb, rb = ctx.from_host(snd), ctx.from_host(rcv)
    tables, msgs = [(sid, sb, 5, []), (rid, rb, 7, [])], [made_up_messages(snd, 1), made_up_messages(rcv, -1)]
    if order == "receiver_first":
        tables, msgs = tables[::-1], msgs[::-1]
    want = balance(msgs, outside)
    assert (want is None) == (name == "two_outside_messages_cancel")
    got = ctx.bus_group_check(tables, outside)
    assert (None if got is None else tuple(got)) == want
    if want is not None:  # the prover says the same and proves nothing
        who = "outside message %d has no partner" % want[3] if want[1] == 2 else "message 0 of table %d .air %d. at row %d has no partner" % (want[1], tables[want[1]][0], want[3])
        with pytest.raises(vx.VxError, match="%s .net multiplicity %d; %d unmatched tuples" % (who, want[4], want[0])) as e:
            ctx.bus_group_prove(tables, ctx.stark_config(num_queries=8), outside)
        assert e.value.code == -5
    sb.free(), rb.free()


IDX = [0, 31, 31, 17]  # four of the openings of tests/test_gpu_air_bus_program.py's merkle_open_70_of_128_blocks, one duplicated


@pytest.fixture(scope="module")
def rows_case(ctx, vx, oracle):
    """a tree of depth 5 with cap height 2 and leaves of 9 words; MerkleOpenAir (20 path blocks in 2^10 rows) and LeafSpongeAir (8 sponge
    blocks in 2^8 rows) from the trace entry points; the outside party receives every word of every opened row"""
    D, L, cap_height = 5, 9, 2
    leaves = np.random.default_rng(3 + 10 * D).integers(0, P, size=(1 << D, L), dtype=np.uint64)
    data = ctx.from_host(leaves)
    gtree = ctx.merkle(data, 1 << D, L, vx.lib.VX_LEAVES_ROW_MAJOR, cap_height)
    lo, ls = M.log_rows(len(IDX), D), R.log_rows(len(IDX), L)
    assert (lo, ls) == (10, 8)
    ob, opub = ctx.merkle_open_air_trace(gtree, IDX, lo)
    sb, spub = ctx.leaf_sponge_air_trace(data, 1 << D, L, vx.lib.VX_LEAVES_ROW_MAJOR, IDX, ls)
    outside = [[i, j, int(v), 0, TAG_ROW, P - 1] for i in IDX for j, v in enumerate(leaves[i])]
    yield dict(leaves=leaves, data=data, gtree=gtree, rtree=oracle.MerkleTree(leaves, cap_height), open=(ob, lo, [int(v) for v in opub]), sponge=(sb, ls, [int(v) for v in spub]),
               outside=outside, D=D, L=L)
    ob.free(), sb.free(), gtree.free(), data.free()


def test_a_compiled_table_with_a_run_time_one_gives_the_compiled_pairs_proofs(ctx, vx, rows_case):
    c = rows_case
    (ob, lo, opub), (sb, ls, spub) = c["open"], c["sponge"]
    cfg, ocfg = ctx.stark_config(num_queries=8), dict(S.DEFAULT_CFG, num_queries=8)
    mine, MO, LS = air_id(vx, "merkle_open"), vx.lib.VX_AIR_MERKLE_OPEN, vx.lib.VX_AIR_LEAF_SPONGE
    compiled = [(MO, ob, lo, opub), (LS, sb, ls, spub)]
    mixed = [(mine, ob, lo, opub), (LS, sb, ls, spub)]
    assert ctx.bus_group_check(compiled, c["outside"]) is None and ctx.bus_group_check(mixed, c["outside"]) is None
    want = vx.lib.split_bus_group(ctx.bus_group_prove(compiled, cfg, c["outside"]))
    blob = ctx.bus_group_prove(mixed, cfg, c["outside"])
    got = vx.lib.split_bus_group(blob)
    # (a) block_log 5 and a compiled table beside a run-time one: the second proofs are equal, the first differ in the id word
    assert got[1].size == want[1].size and (got[1] == want[1]).all()
    assert got[0].size == want[0].size and np.flatnonzero(got[0] != want[0]).tolist() == [1] and [int(got[0][1]), int(want[0][1])] == [mine, MO]
    vx.lib.bus_group_verify(blob, [(mine, opub), (LS, spub)], cfg, c["outside"])
    with pytest.raises(vx.VxError, match="unexpected AIR"):
        vx.lib.bus_group_verify(blob, [(MO, opub), (LS, spub)], cfg, c["outside"])
    # (b) both are the two-table reference prover's proofs word for word
    ref = R.prove_rows(c["rtree"], IDX, c["leaves"][IDX], ocfg)
    for g, w, ref_id, what in zip(want, ref, (M.REF_ID, R.REF_ID), ("MerkleOpenAir", "LeafSpongeAir")):
        g = g.copy()
        g[1] = ref_id
        assert g.size == w.size, what
        bad = np.flatnonzero(g != np.asarray(w, dtype=np.uint64))
        assert bad.size == 0, "first differing word of the %s proof: %d" % (what, bad[0])
    # (c) ... and the ones inside vx_merkle_rows_prove's blob for the same request, whose tables have the same public inputs
    rows_blob = ctx.merkle_rows_prove(c["gtree"], c["data"], c["L"], vx.lib.VX_LEAVES_ROW_MAJOR, IDX, cfg)
    inner = R.HDR, R.HDR + int(rows_blob[4])
    p_open, p_sponge = rows_blob[inner[0]: inner[1]], rows_blob[inner[1]:]
    at = 12 + int(p_open[9])
    assert [int(v) for v in p_open[at: at + 9]] == opub and [int(v) for v in p_sponge[12 + int(p_sponge[9]): 12 + int(p_sponge[9]) + 14]] == spub
    assert p_open.size == want[0].size and (p_open == want[0]).all() and p_sponge.size == want[1].size and (p_sponge == want[1]).all()
    vx.lib.merkle_rows_verify(np.concatenate([rows_blob[:4], np.array([want[0].size, want[1].size], dtype=np.uint64), want[0], want[1]]), c["gtree"].cap(), c["D"], IDX, c["leaves"][IDX], cfg)


def compiled_messages(c):
    """MerkleOpenAir's and LeafSpongeAir's messages from the traces, read independently of the library (air_merkle_open.cuh / air_leaf_sponge.cuh state them)"""
    (ob, lo, _), (sb, ls, spub) = c["open"], c["sponge"]
    ot, st = ob.download().reshape(M.COLS, -1), sb.download().reshape(R.COLS, -1)
    om, sm = [], []
    for row in range(0, ot.shape[1], 32):
        m, r, leaf = int(ot[M.FIRSTB, row]), int(ot[M.R, row]), [int(ot[M.LEAF + j, row]) for j in range(4)]
        om += [(row, 0, (r, leaf[0], leaf[1], 0, TAG_OPEN), m), (row, 1, (r, leaf[2], leaf[3], 1, TAG_OPEN), m)]
    for row in range(0, st.shape[1], 32):
        cell = lambda j: int(st[j, row])  # noqa: E731
        act, last = cell(R.ACT), cell(R.LASTB)
        for i in range(8):
            sm.append((row, i, (cell(R.IDX), 8 * cell(R.POS) + i, cell(R.MSG + i), 0, TAG_ROW), (act - last + last * spub[2 + i]) % P))
        dig = [cell(R.DIG + j) for j in range(4)]
        sm += [(row, 8, (cell(R.IDX), dig[0], dig[1], 0, TAG_OPEN), -last % P), (row, 9, (cell(R.IDX), dig[2], dig[3], 1, TAG_OPEN), -last % P)]
    return om, sm


def test_the_balance_check_reads_the_compiled_tables_messages(ctx, vx, rows_case):
    """the records of k_bus_records<Air> (block tables, a duplicated opening: tuples of multiplicity 2 on either side) and of the
    interpreter on the same trace, against the messages read from the traces in Python"""
    c = rows_case
    (ob, lo, opub), (sb, ls, spub) = c["open"], c["sponge"]
    om, sm = compiled_messages(c)
    assert sum(1 for m in om if m[3]) == 8 and sum(1 for m in sm if m[3]) == 4 * 9 + 8
    out = c["outside"]
    assert balance([om, sm], out) is None
    for first in (vx.lib.VX_AIR_MERKLE_OPEN, air_id(vx, "merkle_open")):
        tables = [(first, ob, lo, opub), (vx.lib.VX_AIR_LEAF_SPONGE, sb, ls, spub)]
        assert ctx.bus_group_check(tables, out) is None
        # a claim the tables do not prove, a claim dropped (its words are sent and nobody takes them), the sponge table alone, the
        # openings table alone with the rows, a closed bus claimed for an open one
        wrong = [list(w) for w in out]
        wrong[20][2] ^= 1
        for tabs, msgs, outside in ((tables, [om, sm], wrong), (tables, [om, sm], out[9:]), (tables[1:], [sm], out), (tables[:1], [om], out), (tables, [om, sm], [])):
            want = balance(msgs, outside)
            got = ctx.bus_group_check(tabs, outside)
            assert want is not None and tuple(got) == want, (first, want)
    with pytest.raises(vx.VxError, match="table 0 .air %d. at row 0 has no partner" % vx.lib.VX_AIR_LEAF_SPONGE) as e:  # the sponge's first row word
        ctx.bus_group_prove(tables[1:], ctx.stark_config(num_queries=8), out[1:])
    assert e.value.code == -5


def test_argument_errors(ctx, vx, rows_case):
    c = rows_case
    (ob, lo, opub), (sb, ls, spub) = c["open"], c["sponge"]
    MO, LS = vx.lib.VX_AIR_MERKLE_OPEN, vx.lib.VX_AIR_LEAF_SPONGE
    cfg = ctx.stark_config(num_queries=8)
    good = [(MO, ob, lo, opub), (LS, sb, ls, spub)]
    fib = ctx.from_host(np.ones((2, 32), dtype=np.uint64))
    bad_word = [list(w) for w in c["outside"]]
    bad_word[2][1] = P
    bad_tag = [list(w) for w in c["outside"]]
    bad_tag[5][4] = 1 << 16
    for tables, outside, why in (([], c["outside"], "0 tables"),
                                 (good + [(vx.lib.VX_AIR_FIBONACCI, fib, 5, [1, 1, 2])], c["outside"], "table 2 .air 1. has no logUp round"),
                                 ([(MO, ob, lo - 1, opub), good[1]], c["outside"], "trace of table 0 is not cols << log_n"),
                                 ([good[0], (LS, ob, ls, spub)], c["outside"], "trace of table 1 is not cols << log_n"),
                                 ([(MO, ob, lo, opub[:8]), good[1]], c["outside"], "table 0 .air 16. takes 9 public inputs, 8 given"),
                                 ([good[0], (777, sb, ls, spub)], c["outside"], "table 1 names no AIR"),
                                 (good, bad_word, "outside message 2 has a non-canonical word at 1"),
                                 (good, bad_tag, "outside message 5 has a tag of 2.16 or more")):
        for call in (lambda: ctx.bus_group_prove(tables, cfg, outside), lambda: ctx.bus_group_check(tables, outside)):
            with pytest.raises(vx.VxError, match=why) as e:
                call()
            assert e.value.code == -1, why  # VX_ERR_ARG
    # a compiled table without a message list: the check refuses it by name, the prover proves and closes the bus on the totals
    blake = ctx.alloc(vx.lib.VX_BLAKE_AIR_COLS << 16)
    with pytest.raises(vx.VxError, match="table 0 .air 6. has no message list") as e:
        ctx.bus_group_check([(vx.lib.VX_AIR_BLAKE_CHAIN, blake, 16, [0] * 20)])
    assert e.value.code == -1
    blake.free()
    full = ctx.bus_group_prove(good, cfg, c["outside"])
    with pytest.raises(vx.VxError) as e:
        ctx.bus_group_prove(good, cfg, c["outside"], out=np.zeros(full.size - 1, dtype=np.uint64))
    assert e.value.code == -4 and e.value.needed == full.size  # VX_ERR_BUFSZ with the length set
    assert ctx.bus_group_check(good, c["outside"]) is None  # after the refusals the context goes on working
    fib.free()


def test_a_table_without_a_message_list_is_closed_on_its_published_total(ctx, vx):
    """BlakeChainAir (a periodic lookup table, no message list) stand-alone (no tree, no window: nothing leaves the table) publishes a
    zero total: the group of one proves and verifies as a closed bus; with an outside message the totals do not cancel and no blob is
    written"""
    ch = vx.synth.Chain(1, profile="Ptiny", stride=512)
    hb = ctx.from_host(ch.headers)
    tb, pub, _ = ctx.blake_chain_trace(hb, 512, ch.sizes, ch.trusted_hash, ch.trusted_block + 1, 16)
    pub = [int(x) for x in pub]
    cfg = ctx.stark_config(num_queries=8)
    tables = [(vx.lib.VX_AIR_BLAKE_CHAIN, tb, 16, pub)]
    blob = ctx.bus_group_prove(tables, cfg)
    vx.lib.bus_group_verify(blob, [(vx.lib.VX_AIR_BLAKE_CHAIN, pub)], cfg)
    with pytest.raises(vx.VxError, match="the bus does not close") as e:
        ctx.bus_group_prove(tables, cfg, [[1, 2, 3, 4, 5, 1]])
    assert e.value.code == -5
    tb.free(), hb.free()


TAG_BYTE, TAG_KEY, TAG_EDMSG, TAG_EDH = 2, 5, 6, 7


def test_the_sha_tree_table_alone_closes_its_bus_against_the_root_bytes(ctx, vx):
    """ShaTreeAir16 (2^12 rows, the list reads periodic columns and its last helper holds one message): the word messages between a
    node and its parent close inside the table, the outside party sends the root bytes of the 5 headers; a byte left out is named by
    the cell that would have received it, found here from the oracle's periodic columns"""
    from oracle import sha_tree_air as T

    air = T.make_air(16)
    ch = vx.synth.Chain(5, profile="Ptiny", stride=512)
    tr, pub = T.gen_trace(ch.state_roots, ch.data_roots, 16)
    tb = ctx.from_host(tr)
    tables = [(vx.lib.VX_AIR_SHA_TREE[16], tb, 12, pub)]
    outside = [[leaf, k, bytes(root)[k], tree, TAG_BYTE, 1] for tree, roots in enumerate((ch.state_roots, ch.data_roots)) for leaf, root in enumerate(roots) for k in range(32)]
    assert len(outside) == 5 * 2 * 32
    assert ctx.bus_group_check(tables, outside) is None
    per = [np.asarray(c) for c in air.periodic_values()]
    for tree, leaf, k in ((0, 0, 0), (1, 3, 17), (1, 4, 31)):
        at = (tree * 5 + leaf) * 32 + k
        assert outside[at][:2] == [leaf, k] and outside[at][3] == tree
        rows = np.flatnonzero((per[T.P_PBL] + per[T.P_PBR] == 1) & (per[T.P_TREE] == tree) & (per[T.P_CID] == leaf) & (per[T.P_JJ] == k // 4))
        assert rows.size == 1
        got = ctx.bus_group_check(tables, outside[:at] + outside[at + 1:])
        assert tuple(got) == (1, 0, 1 + k % 4, int(rows[0]), P - 1)
    tb.free()
    tr0, pub0 = T.gen_trace([], [], 16)  # no leaf enabled: only the word messages, and nothing outside
    tb0 = ctx.from_host(tr0)
    assert pub0[16] == 0 and ctx.bus_group_check([(vx.lib.VX_AIR_SHA_TREE[16], tb0, 12, pub0)]) is None
    tb0.free()


def test_the_epoch_end_table_alone_closes_its_bus_against_bytes_and_keys(ctx, vx):
    """EpochEndAir (2^9 rows, 22 helpers) on the header of tests/test_gpu_epoch_air.py with one new authority: the outside party sends
    the bytes of the window and takes the four quarters of every key; a quarter left out names the validator's row and that key message"""
    n_new = 1
    e = vx.synth.EpochEndHeader(140000, n_new, logs_before=0)
    hb = ctx.from_host(e.padded)
    buf, pub, wlen = ctx.epoch_end_trace(hb, e.start_position, n_new, bus_on=1)
    tables = [(vx.lib.VX_AIR_EPOCH_END, buf, 9, [int(x) for x in pub])]
    window = bytes(e.bytes[e.start_position + 1: e.start_position + 1 + wlen])
    sent = [[0, k, window[k], 1, TAG_BYTE, 1] for k in range(wlen)]
    u32 = lambda b: int.from_bytes(b, "little")  # noqa: E731
    taken = [[4 * i + q, u32(key[8 * q: 8 * q + 4]), u32(key[8 * q + 4: 8 * q + 8]), 0, TAG_KEY, P - 1] for i, key in enumerate(bytes(k) for k in e.new_pubkeys) for q in range(4)]
    assert len(sent) == wlen and len(taken) == 4 * n_new
    assert ctx.bus_group_check(tables, sent + taken) is None
    for q in (0, 3):
        got = ctx.bus_group_check(tables, sent + taken[:q] + taken[q + 1:])
        assert tuple(got) == (1, 0, 40 + q, 1, 1)  # the one validator is row 1; its key quarter q is sent once
    buf0, pub0, _ = ctx.epoch_end_trace(hb, e.start_position, n_new, bus_on=0)
    assert ctx.bus_group_check([(vx.lib.VX_AIR_EPOCH_END, buf0, 9, [int(x) for x in pub0])]) is None
    buf.free(), buf0.free(), hb.free()


def outside_of(trace, periodic, pub, lookup):
    """the other side of every message a table has, from the oracle's trace and the oracle's reading of a row (m, tag, tuple):
    -> [[t0, t1, t2, t3, tag, -m]], and the rows they belong to"""
    out, rows = [], []
    for row, loc in enumerate(trace.T.tolist()):
        m, tag, tup = lookup(loc, [int(c[row % len(c)]) for c in periodic], pub)
        if m % P:
            out.append([int(t) % P for t in tup] + [int(tag) % P, -m % P])
            rows.append(row)
    return out, rows


def test_the_sha_chain_table_alone_closes_its_bus_against_the_keys(ctx, vx):
    """ShaChainAir (one helper of one message, the list reads three periodic columns), 3 keys in 2^9 rows -- blocks FIRST, DATA, PAD,
    DATA, PAD and 3 IDLE -- with flags 1, 0, 1.  Mode 1: the outside party takes the four quarters of the two flagged keys; mode 2: it
    sends those of all three, whatever the flags; mode 0: nobody says anything.  A quarter left out is named by the row it sits on"""
    from oracle import sha_air as A

    keys, flags = [hashlib.sha256(b"key %d" % i).digest() for i in range(3)], [1, 0, 1]
    u32 = lambda b: int.from_bytes(b, "little")  # noqa: E731
    quarters = lambda i, m: [[4 * i + j, u32(keys[i][8 * j: 8 * j + 4]), u32(keys[i][8 * j + 4: 8 * j + 8]), 0, TAG_KEY, m] for j in range(4)]  # noqa: E731
    tb, pub, _ = ctx.sha_chain_trace(keys, 9, signed=flags, bus_on=1)
    want, wpub, _ = A.gen_trace(keys, 9, signed=flags, bus_on=1)
    assert (tb.download().reshape(A.CHAIN_COLS, 512) == want).all() and [int(x) for x in pub] == wpub
    table = lambda mode: [(vx.lib.VX_AIR_SHA_CHAIN, tb, 9, wpub[:9] + [mode])]  # noqa: E731
    # mode 1: the flagged keys are sent from rows 0, 2, 4, 6 of the FIRST block and rows 8, 10, 12, 14 of the second DATA block
    taken, rows = outside_of(want, A.chain_periodic_values(), wpub[:9] + [1], A.key_lookup)
    assert taken == quarters(0, P - 1) + quarters(2, P - 1) and len(taken) == 8
    assert rows == [0, 2, 4, 6] + [64 * 3 + r for r in (8, 10, 12, 14)]
    assert ctx.bus_group_check(table(1), taken) is None
    assert tuple(ctx.bus_group_check(table(1), taken[:1] + taken[2:])) == (1, 0, 0, 2, 1)  # key 0, quarter 1
    assert tuple(ctx.bus_group_check(table(1), taken[:7])) == (1, 0, 0, 64 * 3 + 14, 1)  # key 2, quarter 3
    # mode 2: every key is received
    sent, rows = outside_of(want, A.chain_periodic_values(), wpub[:9] + [2], A.key_lookup)
    assert sent == quarters(0, 1) + quarters(1, 1) + quarters(2, 1) and len(sent) == 12
    assert ctx.bus_group_check(table(2), sent) is None
    assert rows[5] == 64 + 10 and tuple(ctx.bus_group_check(table(2), sent[:5] + sent[6:])) == (1, 0, 0, 64 + 10, P - 1)  # key 1, quarter 1
    # mode 0
    assert outside_of(want, A.chain_periodic_values(), wpub[:9] + [0], A.key_lookup) == ([], [])
    assert ctx.bus_group_check(table(0)) is None
    tb.free()


def test_the_epoch_end_and_sha_chain_tables_close_the_key_bus_between_them(ctx, vx):
    """the rotation's key bus as a group of two compiled lists: EpochEndAir sends the quarters of the one new key, ShaChainAir (mode 2,
    2^6 rows, committing that key) receives them, the outside party sends the window bytes alone.  With another key in the commitment
    table all eight key messages are without a partner and the lowest origin is named"""
    e = vx.synth.EpochEndHeader(140000, 1, logs_before=0)
    hb = ctx.from_host(e.padded)
    buf, pub, wlen = ctx.epoch_end_trace(hb, e.start_position, 1, bus_on=1)
    window = bytes(e.bytes[e.start_position + 1: e.start_position + 1 + wlen])
    sent = [[0, k, window[k], 1, TAG_BYTE, 1] for k in range(wlen)]
    key = bytes(e.new_pubkeys[0])
    tb, spub, _ = ctx.sha_chain_trace([key], 6, bus_on=2)
    epoch, chain = (vx.lib.VX_AIR_EPOCH_END, buf, 9, [int(x) for x in pub]), (vx.lib.VX_AIR_SHA_CHAIN, tb, 6, [int(x) for x in spub])
    assert len(sent) == wlen > 0 and ctx.bus_group_check([epoch, chain], sent) is None and ctx.bus_group_check([chain, epoch], sent) is None
    other = hashlib.sha256(key).digest()
    assert all(other[8 * q: 8 * q + 8] != key[8 * q: 8 * q + 8] for q in range(4))
    ob, opub, _ = ctx.sha_chain_trace([other], 6, bus_on=2)
    wrong = (vx.lib.VX_AIR_SHA_CHAIN, ob, 6, [int(x) for x in opub])
    assert tuple(ctx.bus_group_check([epoch, wrong], sent)) == (8, 0, 40, 1, 1)  # the validator's row of the epoch-end table, its first key message
    assert tuple(ctx.bus_group_check([wrong, epoch], sent)) == (8, 0, 0, 0, P - 1)  # row 0 of the FIRST block takes quarter 0
    buf.free(), tb.free(), ob.free(), hb.free()


def test_the_sha512_table_alone_closes_its_bus_against_messages_and_digests(ctx, vx):
    """Sha512Air10 (2^10 rows, 6 slots; one message whose tag is weighted by the row's selectors): 3 signatures with flags 1, 0, 1 fill
    two compact slots.  The outside party sends the four parts of R || A of either slot and takes the six parts of its digest; slots
    2 .. 5 and the rows behind the last slot say nothing"""
    from oracle import sha512_air as H

    msg = b"\x01" + bytes(range(32)) + (100000).to_bytes(4, "little") + (7).to_bytes(8, "little") + (3).to_bytes(8, "little")
    keys, sigs, flags = [hashlib.sha256(b"A %d" % i).digest() for i in range(3)], [hashlib.sha512(b"R S %d" % i).digest() for i in range(3)], [1, 0, 1]
    slots = [(sg[:32], k) for k, sg, f in zip(keys, sigs, flags) if f]
    tb, pub = ctx.sha512_trace(keys, sigs, msg, flags, 10, bus_on=1)
    want, wpub, dig = H.gen_trace(slots, msg, 10, bus_on=1)
    assert (tb.download().reshape(H.COLS, 1024) == want).all() and [int(x) for x in pub] == wpub
    outside, rows = outside_of(want, H.periodic_values(1024), wpub, H.bus_lookup)
    assert len(outside) == 20 and rows == [160 * s + r for s in range(2) for r in [0, 2, 4, 6] + list(range(154, 160))]
    assert [w[4:] for w in outside] == ([[TAG_EDMSG, 1]] * 4 + [[TAG_EDH, P - 1]] * 6) * 2
    # two of them from the bytes: part 2 of slot 1's R || A (bytes 32 .. 47: the first half of A, three / three / two 16-bit limbs), and
    # part 5 of slot 0's digest (the high half of word 7; halves 16 and 17 do not exist)
    head, le = slots[1][0] + slots[1][1], lambda b: int.from_bytes(b, "little")  # noqa: E731
    assert outside[10 + 2] == [4 * 1 + 2, le(head[32:38]), le(head[38:44]), le(head[44:48]), TAG_EDMSG, 1]
    assert dig[0] == hashlib.sha512(slots[0][0] + slots[0][1] + msg).digest() and outside[9] == [5, int.from_bytes(dig[0][56:60], "big"), 0, 0, TAG_EDH, P - 1]
    table = [(vx.lib.VX_AIR_SHA512[10], tb, 10, wpub)]
    assert ctx.bus_group_check(table, outside) is None
    assert tuple(ctx.bus_group_check(table, outside[:12] + outside[13:])) == (1, 0, 0, 164, P - 1)
    assert tuple(ctx.bus_group_check(table, outside[:9] + outside[10:])) == (1, 0, 0, 159, 1)
    assert outside_of(want, H.periodic_values(1024), wpub[:14] + [0], H.bus_lookup) == ([], [])
    assert ctx.bus_group_check([(vx.lib.VX_AIR_SHA512[10], tb, 10, wpub[:14] + [0])]) is None
    tb.free()
