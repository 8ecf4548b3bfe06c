"""TEST INFRASTRUCTURE for declared bus messages (include/vx.h vx_air_register_bus): the restatements of tests/*_ref.py with their
hand-written bus block (the last 2 N_HELP + 2 base-field assertions) dropped and the messages DECLARED instead, a made-up table, and the
big-integer reading of a declaration that the tests compare the library with.  No tests here."""
import numpy as np

import fri_fold_ref as F
import leaf_noop_ref as N
import merkle_open_ref as M
import transcript_ref as T
import vx_import
from oracle import stark_ref as S

P = N.P
CHAL = N.CHAL


def _drop_bus_block(b, n_help):
    del b.constraints[-(2 * n_help + 2):]
    return b


def leaf_noop():
    """LeafNoopAir: the two halves of the digest received, the words that exist sent"""
    b = _drop_bus_block(N.builder(), N.N_HELP)
    act, tree, idx = b.loc(N.ACT), b.loc(N.TREE), b.loc(N.IDX)
    w, e = [b.loc(N.W + j) for j in range(4)], [b.loc(N.E + j) for j in range(4)]
    b.receive(N.TAG_OPEN, [idx, w[0], w[1], tree + tree], act)
    b.receive(N.TAG_OPEN, [idx, w[2], w[3], tree + tree + 1], act)
    for j in range(4):
        b.send(N.TAG_ROW, [idx, None if j == 0 else b.const(j), w[j], tree], e[j])
    return b


def transcript():
    """TranscriptAir: eight absorbed words received with multiplicity W_i, eight outputs sent with multiplicity Q_i"""
    b = _drop_bus_block(T.builder(), T.N_HELP)
    loc = b.loc
    chain, nabs, nch = loc(T.CHAIN), loc(T.NABS), loc(T.NCH)
    sw = loc(T.W)
    for i in range(1, 8):
        sw = sw + loc(T.W + i)
    absorbed = nabs + sw
    for i in range(8):
        b.receive(T.TAG_OBS, [chain, nabs + i, loc(T.MSG + i)], loc(T.W + i))
    for i in range(8):
        b.send(T.TAG_CHAL, [chain, nch + (7 - i), absorbed, loc(T.OUT + i)], loc(T.Q + i))
    b.bus(block_log=5, step_periodic=16)
    return b


def fri_fold():
    """FriFoldAir: 32 leaf words received on a fold row; the entry received on the first row, the exit sent on the first bit row"""
    b = _drop_bus_block(F.builder(), F.N_HELP)
    loc = b.loc
    tree, q, idx, fold = b.pub(F.PUB_TREE0) + loc(F.CNT), loc(F.Q), loc(F.IDX), loc(F.FOLD)
    for j in range(32):
        b.receive(F.TAG_ROW, [q, b.const(j), loc(F.LEAF + j), tree], fold)
    b.receive(F.TAG_FRI, [idx, loc(F.EV), loc(F.EV + 1)], loc(F.FIRST))
    b.send(F.TAG_FRI, [idx, loc(F.EV), loc(F.EV + 1), b.const(1)], loc(F.FBIT))
    return b


def merkle_open():
    """MerkleOpenAir: the two halves of the opened leaf digest sent on a path's first block"""
    b = _drop_bus_block(M.builder(), 1)
    loc = b.loc
    b.send(M.TAG_OPEN, [loc(M.R), loc(M.LEAF), loc(M.LEAF + 1)], loc(M.FIRSTB))
    b.send(M.TAG_OPEN, [loc(M.R), loc(M.LEAF + 2), loc(M.LEAF + 3), b.const(1)], loc(M.FIRSTB))
    b.bus(block_log=5, step_periodic=16)
    return b


TAG_A, TAG_B = 0, 300  # tag 0 (its term is absent) and a tag above the library's own 13
MADE_UP_COLS = 6


def made_up():
    """A table of 6 columns (m0, m1, m2, u, v, w) with THREE messages (an odd count: helper 1 holds one), a slot left unset, tag 0 and a
    tag above 13.  Messages 0 and 1 name the same tuple (u, -, v) under the same tag, so a row with m0 = 1, m1 = P - 1 has a zero
    helper with both multiplicities non-zero.  Its one own constraint, 0 * w, holds on every trace."""
    ap = vx_import.load().air_program
    b = ap.AirBuilder(MADE_UP_COLS, 1)
    m0, m1, m2, u, v, w = (b.loc(j) for j in range(6))
    b.assert_zero(b.const(0) * w)
    b.send(TAG_B, [u, None, v], m0)
    b.send(TAG_B, [u, None, v], m1)
    b.send(TAG_A, [u * 3 + b.pub(0), v, None, w - 1], m2)
    return b


def made_up_trace(log_n, seed=5):
    """random rows; idle rows (all three multiplicities zero) at every third position; row 1 the cancelling pair; row 2 message 2 alone"""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    tr = rng.integers(0, P, size=(MADE_UP_COLS, n), dtype=np.uint64)
    tr[:3] = rng.integers(0, 3, size=(3, n), dtype=np.uint64)
    tr[:3, ::3] = 0
    tr[0, 1], tr[1, 1], tr[2, 1] = 1, P - 1, 0
    tr[0, 2], tr[1, 2], tr[2, 2] = 0, 0, 2
    return tr


def made_up_messages(row, pub):
    """the declaration read with Python integers: [(tag, [t0..t3 or None], m)] of one row"""
    m0, m1, m2, u, v, w = (int(x) for x in row)
    return [(TAG_B, [u, None, v, None], m0), (TAG_B, [u, None, v, None], m1), (TAG_A, [(3 * u + int(pub[0])) % P, v, None, (w - 1) % P], m2)]


def aux_of_messages(messages_of_row, n, chal, rows_per_helper=1):
    """the auxiliary columns of the compiled layout from a per-row message list, with big integers (oracle.stark_ref.ExtS): helper e =
    m_2e / D_2e + m_2e+1 / D_2e+1, the running sum behind them -> (aux [2 N_HELP + 2][n], [total / n])"""
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g = [None, gamma, gamma * gamma, gamma * gamma * gamma]
    g4 = g[2] * g[2]
    incs, aux = [], None
    for blk in range(n // rows_per_helper):
        row = blk * rows_per_helper
        msgs = messages_of_row(row)
        n_help = (len(msgs) + 1) // 2
        if aux is None:
            aux = np.zeros((2 * n_help + 2, n), dtype=np.uint64)
        tot = S.ExtS(0)
        for e in range(n_help):
            h = S.ExtS(0)
            for tag, slots, m in msgs[2 * e: 2 * e + 2]:
                d = beta + g4 * int(tag)
                for j, t in enumerate(slots):
                    if t is not None:
                        d = d + (g[j] * int(t) if j else S.ExtS(int(t)))
                if m % P:
                    h = h + d.inv() * (m % P)
            aux[2 * e, row: row + rows_per_helper], aux[2 * e + 1, row: row + rows_per_helper] = h.a, h.b
            tot = tot + h
        incs.append(tot)
    total = S.ExtS(0)
    for t in incs:
        total = total + t
    apub = total * pow(n, P - 2, P)
    z, zc = S.ExtS(0), aux.shape[0] - 2
    for i in range(n):
        aux[zc, i], aux[zc + 1, i] = z.a, z.b
        if i % rows_per_helper == 0:
            z = z + incs[i // rows_per_helper]
        z = z - apub
    return aux, [apub.a, apub.b]
