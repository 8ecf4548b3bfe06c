"""TEST INFRASTRUCTURE for LeafNoopAir (csrc/air_leaf_noop.cuh, AIR id 22): the AIR restated INDEPENDENTLY as a constraint program
(air_program.AirBuilder / X2, the same constraint order as the compiled eval, so oracle.air_program.ProgramAir runs it through
oracle/stark_ref.py unchanged), a reference trace generator and gen_aux in plain Python, the claims digest and the bus terms of one
opening (what the table receives from MerkleOpenSetAir and what it sends to FriCombineAir).  No tests here."""
import numpy as np

import fri_fold_ref as F
import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = F.P
AIR_ID = 22        # the compiled AIR
REF_ID = 1022      # the program restatement in the reference prover's registry (never registered with the product)
ACT, TREE, IDX, W, E, COLS = 0, 1, 2, 3, 7, 11
N_HELP, AUX, PUB = 3, 8, 4
TAG_OPEN, TAG_ROW = 8, 9
CHAL = F.CHAL
degree = F.degree
RULES = {}  # rule name -> index of its first constraint (filled by the builder)


def builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(COLS, PUB, aux_cols=AUX, n_challenges=4, n_aux_public=1)
    loc = b.loc
    act, tree, idx = loc(ACT), loc(TREE), loc(IDX)
    w, e = [loc(W + j) for j in range(4)], [loc(E + j) for j in range(4)]

    def rule(name):
        RULES[name] = len(b.constraints)

    # 1. boolean cells
    rule("boolean")
    b.assert_zero(act * (act - 1))
    for j in range(4):
        b.assert_zero(e[j] * (e[j] - 1))
    # 2. the length
    rule("first_word_exists")
    b.assert_zero(e[0] - act)
    rule("no_gap")
    for j in range(3):
        b.assert_zero(e[j + 1] * (1 - e[j]))
    rule("zero_behind_the_length")
    for j in range(4):
        b.assert_zero((1 - e[j]) * w[j])
    # 3. the bus
    rule("bus")
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    dlo = beta + idx + gamma * w[0] + g2 * w[1] + g3 * (tree + tree) + g4 * TAG_OPEN
    dhi = beta + idx + gamma * w[2] + g2 * w[3] + g3 * (tree + tree + 1) + g4 * TAG_OPEN
    h0 = X2(b.aux(0), b.aux(1))
    b.assert_zero_x2(h0 * dlo * dhi + (dlo + dhi) * act)
    hsum = h0
    for k in range(2):
        da, db = (beta + idx + gamma * j + g2 * w[j] + g3 * tree + g4 * TAG_ROW for j in (2 * k, 2 * k + 1))
        h = X2(b.aux(2 + 2 * k), b.aux(3 + 2 * k))
        b.assert_zero_x2(h * da * db - db * e[2 * k] - da * e[2 * k + 1])
        hsum = hsum + h
    rule("running_sum")
    z, zn = X2(b.aux(6), b.aux(7)), X2(b.aux_nxt(6), b.aux_nxt(7))
    b.assert_zero_x2(zn - z - hsum + X2(b.apub(0), b.apub(1)))
    return b


_air = None


def air():
    """the restatement as an AIR object of the reference prover (registered there under REF_ID)"""
    global _air
    if _air is None:
        b = builder()
        code, consts, _ = b.assemble()
        _air = ProgramAir(REF_ID, b.cols, b.n_public, code, consts, b.periodic, b.aux_cols, b.n_challenges, b.n_aux_public, gen_aux=gen_aux)
        S.register_air(_air)
    return _air


# ---- witness
def log_rows(n_idx):
    return max(5, (n_idx - 1).bit_length())


def padded(row):
    return [int(v) for v in row] + [0] * (4 - len(row))


def opening_row(tree, index, row, flags=None, words=None):
    """the eleven cells of one opening.  Forgeries: flags -- other E cells; words -- other W cells"""
    assert 1 <= len(row) <= 4
    return [1, int(tree), int(index)] + (padded(row) if words is None else list(words)) + ([int(j < len(row)) for j in range(4)] if flags is None else list(flags))


def assemble(rows, log_n):
    """rows (lists of eleven cells) followed by idle rows -> trace [11][2^log_n]"""
    n = 1 << log_n
    assert len(rows) <= n
    tr = np.zeros((COLS, n), dtype=np.uint64)
    if rows:
        tr[:, :len(rows)] = np.array(rows, dtype=np.uint64).T
    return tr


def claims_digest(tree_of, leaf_idx, rows):
    words = []
    for t, i, r in zip(tree_of, leaf_idx, rows):
        words += [int(t), int(i), len(r)] + padded(r)
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def ref_trace(tree_of, leaf_idx, rows, log_n=None, digest=None):
    """opening i: the row rows[i] (1..4 words) of leaf leaf_idx[i] of tree tree_of[i] -> (trace [11][2^log_n], the 4 public inputs)"""
    log_n = log_rows(len(rows)) if log_n is None else log_n
    pub = claims_digest(tree_of, leaf_idx, rows) if digest is None else [int(v) for v in digest]
    return assemble([opening_row(t, i, r) for t, i, r in zip(tree_of, leaf_idx, rows)], log_n), pub


def _bus(chal):
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g2 = gamma * gamma
    return beta, gamma, g2, g2 * gamma, g2 * g2


def d_open(bus, tree, index, da, db, half):
    beta, gamma, g2, g3, g4 = bus
    return beta + int(index) + gamma * int(da) + g2 * int(db) + g3 * (2 * int(tree) + half) + g4 * TAG_OPEN


def d_row(bus, tree, index, position, word):
    beta, gamma, g2, g3, g4 = bus
    return beta + int(index) + gamma * int(position) + g2 * int(word) + g3 * int(tree) + g4 * TAG_ROW


def row_helpers(bus, cell):
    """the three helpers of one row from its cells (cell(column) -> int)"""
    if not cell(ACT):
        return [S.ExtS(0)] * N_HELP
    tree, idx = cell(TREE), cell(IDX)
    w, e = [cell(W + j) for j in range(4)], [cell(E + j) for j in range(4)]
    hs = [(d_open(bus, tree, idx, w[0], w[1], 0).inv() + d_open(bus, tree, idx, w[2], w[3], 1).inv()) * (P - 1)]
    for k in range(2):
        hs.append(d_row(bus, tree, idx, 2 * k, w[2 * k]).inv() * e[2 * k] + d_row(bus, tree, idx, 2 * k + 1, w[2 * k + 1]).inv() * e[2 * k + 1])
    return hs


def gen_aux(trace, chal, pub=None):
    """-> (aux [8][n]: three helpers, Z; [S / n])"""
    n = trace.shape[1]
    bus = _bus(chal)
    aux = np.zeros((AUX, n), dtype=np.uint64)
    incs = []
    for i in range(n):
        hs = row_helpers(bus, lambda j: int(trace[j, i]))
        tot = S.ExtS(0)
        for k, h in enumerate(hs):
            aux[2 * k, i], aux[2 * k + 1, i] = h.a, h.b
            tot = tot + h
        incs.append(tot)
    tot = S.ExtS(0)
    for h in incs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[6, i], aux[7, i] = z.a, z.b
        z = z + incs[i] - apub
    return aux, [apub.a, apub.b]


def opening_sum(chal, tree, index, row):
    """what one opening adds to the table's total: every word sent, the two halves of the digest received"""
    bus, w = _bus(chal), padded(row)
    tot = S.ExtS(0) - d_open(bus, tree, index, w[0], w[1], 0).inv() - d_open(bus, tree, index, w[2], w[3], 1).inv()
    for j, v in enumerate(row):
        tot = tot + d_row(bus, tree, index, j, v).inv()
    return tot
