"""TEST INFRASTRUCTURE for MerkleOpenAir (csrc/air_merkle_open.cuh, AIR id 16): the AIR restated INDEPENDENTLY as a constraint
program (air_program.AirBuilder / X2, the same constraint order as the compiled eval, so oracle.air_program.ProgramAir runs it
through oracle/stark_ref.py unchanged), a reference trace generator and gen_aux in plain Python on oracle.pyref.poseidon's
constants and oracle.MerkleTree, the claims digest, the blob wrapper and the verifier's side of the bus.  No tests here."""
import numpy as np

import vx_import
from oracle import oracle as O
from oracle import pyref
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = 2**64 - 2**32 + 1
AIR_ID = 16        # the compiled AIR
REF_ID = 1016      # the program restatement in the reference prover's registry (never registered with the product)
BIT, SIB, CUR, LEAF, R, LVL, ACT, END, FIRSTB, COLS = 48, 49, 53, 57, 61, 62, 63, 64, 65, 66
TAG_OPEN = 8
MAGIC, HDR = int.from_bytes(b"VXMOPEN1", "little"), 4
MDS_CIRC, MDS_DIAG = pyref.MDS_CIRC, pyref.MDS_DIAG
# the shapes both tiers check: name -> (D = log2(n_leaves), cap height, leaf indices); fixed lookup challenges for the witness checks
CASES = {
    "D3_Q1": (3, 0, [5]),
    "D3_Q3_idle_tail": (3, 0, [1, 6, 3]),
    "D2_Q4_no_idle_block": (2, 0, [2, 0, 3, 1]),
    "duplicate_index": (3, 0, [4, 4]),
    "first_and_last_leaf": (3, 0, [0, 7]),
    "cap_height_1": (3, 1, [1, 6, 3]),
    "cap_height_2": (3, 2, [1, 6, 3]),
}
CHAL = [0x1234567890ABCDEF % P, 77, P - 5, 0xFEDCBA9876543210 % P]


def periodic():
    rc = pyref._constants()
    per = [[rc[12 * r + i] if r < 30 else 0 for r in range(32)] for i in range(12)]
    per.append([1 if (r < 4 or 26 <= r < 30) else 0 for r in range(32)])  # 12 full
    per.append([1 if r < 30 else 0 for r in range(32)])                   # 13 a round row
    per.append([1 if r == 30 else 0 for r in range(32)])                  # 14 the output row
    per.append([1 if r == 31 else 0 for r in range(32)])                  # 15 the spare row
    per.append([1 if r == 0 else 0 for r in range(32)])                   # 16 the first row
    return per


def builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(COLS, 9, periodic=periodic(), aux_cols=4, n_challenges=4, n_aux_public=1)
    full, rnd, out, spare, first = (b.per(q) for q in range(12, 17))
    # 1. the permutation
    x = [b.loc(i) + b.per(i) for i in range(12)]
    a, bb, t = [b.loc(12 + i) for i in range(12)], [b.loc(24 + i) for i in range(12)], [b.loc(36 + i) for i in range(12)]
    for i in range(12):
        b.assert_zero(a[i] - x[i] * x[i])
    for i in range(12):
        b.assert_zero(bb[i] - a[i] * a[i])
    for i in range(12):
        b.assert_zero(t[i] - x[i] * a[i] * bb[i])
    y = [t[0]] + [full * t[i] + (1 - full) * x[i] for i in range(1, 12)]
    for row in range(12):
        acc = y[row] * (MDS_CIRC[0] + MDS_DIAG[row])
        for i in range(1, 12):
            acc = acc + y[(i + row) % 12] * MDS_CIRC[i]
        b.assert_zero(rnd * (b.nxt(row) - acc))
    for i in range(12):
        b.assert_zero(out * (b.nxt(i) - b.loc(i)))
    # 2. shape columns constant over a block
    for j in range(BIT, COLS):
        b.assert_zero((1 - spare) * (b.nxt(j) - b.loc(j)))
    # 3. flags
    bit, act, end, r, lvl = b.loc(BIT), b.loc(ACT), b.loc(END), b.loc(R), b.loc(LVL)
    cont = act - end
    b.assert_zero(bit * (bit - 1))
    b.assert_zero(act * (act - 1))
    b.assert_zero(end * (end - 1))
    b.assert_zero(end * (1 - act))
    # 4. block input
    for i in range(4):
        b.assert_zero(first * (b.loc(i) - b.loc(CUR + i) - bit * (b.loc(SIB + i) - b.loc(CUR + i))))
    for i in range(4):
        b.assert_zero(first * (b.loc(4 + i) - b.loc(SIB + i) + bit * (b.loc(SIB + i) - b.loc(CUR + i))))
    for i in range(8, 12):
        b.assert_zero(first * b.loc(i))
    # 5. spare row -> next block
    sc, sn = spare * cont, spare * (1 - cont)
    for i in range(4):
        b.assert_zero(sc * (b.nxt(CUR + i) - b.loc(i)))
    for i in range(4):
        b.assert_zero(sc * (b.nxt(LEAF + i) - b.loc(LEAF + i)))
    b.assert_zero(sc * (r - 2 * b.nxt(R) - bit))
    b.assert_zero(sc * (b.nxt(LVL) - lvl - 1))
    b.assert_zero(sc * (1 - b.nxt(ACT)))
    for i in range(4):
        b.assert_zero(sn * (b.nxt(CUR + i) - b.nxt(LEAF + i)))
    b.assert_zero(sn * (b.nxt(LVL) - 1))
    b.assert_zero(spare * (b.nxt(FIRSTB) - b.nxt(ACT) * (1 - cont)))
    # 6. top of a path
    b.assert_zero(end * (r - bit))
    b.assert_zero(end * (lvl - b.pub(4)))
    for i in range(4):
        b.assert_zero(spare * end * (b.loc(i) - b.pub(i)))
    # 7. the bus
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    dlo = beta + r + gamma * b.loc(LEAF) + g2 * b.loc(LEAF + 1) + g4 * TAG_OPEN
    dhi = beta + r + gamma * b.loc(LEAF + 2) + g2 * b.loc(LEAF + 3) + g3 + g4 * TAG_OPEN
    h, z, zn = X2(b.aux(0), b.aux(1)), X2(b.aux(2), b.aux(3)), X2(b.aux_nxt(2), b.aux_nxt(3))
    b.assert_zero_x2(h * dlo * dhi - (dlo + dhi) * b.loc(FIRSTB))
    b.assert_zero_x2(zn - z - h * first + X2(b.apub(0), b.apub(1)))
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
def block_rows(s):
    """the 32 rows x 48 columns of one permutation block for the input state s -> (rows [48][32], output state)"""
    rc = pyref._constants()
    rows = np.zeros((48, 32), dtype=np.uint64)
    s = list(s)
    for r in range(32):
        x = [(s[i] + (rc[12 * r + i] if r < 30 else 0)) % P for i in range(12)]
        a = [v * v % P for v in x]
        b4 = [v * v % P for v in a]
        t = [x[i] * a[i] % P * b4[i] % P for i in range(12)]
        for i in range(12):
            rows[i, r], rows[12 + i, r], rows[24 + i, r], rows[36 + i, r] = s[i], a[i], b4[i], t[i]
        if r < 30:
            fl = r < 4 or r >= 26
            y = [t[0]] + [t[i] if fl else x[i] for i in range(1, 12)]
            s = [(sum(y[(i + q) % 12] * MDS_CIRC[i] for i in range(12)) + y[q] * MDS_DIAG[q]) % P for q in range(12)]
    return rows, s


def tree_nodes(tree):
    """every level of an oracle.MerkleTree, the levels above its cap included: nodes[l][k] = 4 ints; nodes[D] = [root]"""
    D = tree.n.bit_length() - 1
    nodes, off, cur = [], 0, tree.n
    for _ in range(D - tree.cap_height + 1):
        nodes.append([[int(v) for v in tree.levels[off + 4 * k: off + 4 * k + 4]] for k in range(cur)])
        off += 4 * cur
        cur >>= 1
    while len(nodes[-1]) > 1:
        lv = nodes[-1]
        nodes.append([[int(v) for v in O.two_to_one(lv[2 * k], lv[2 * k + 1])] for k in range(len(lv) // 2)])
    return nodes


def fold_cap(cap):
    lv = [[int(v) for v in d] for d in np.asarray(cap, dtype=np.uint64).reshape(-1, 4)]
    while len(lv) > 1:
        lv = [[int(v) for v in O.two_to_one(lv[2 * k], lv[2 * k + 1])] for k in range(len(lv) // 2)]
    return lv[0]


def claims_digest(idx, digests):
    words = []
    for i, d in zip(idx, np.asarray(digests, dtype=np.uint64).reshape(-1, 4)):
        words += [int(i)] + [int(v) for v in d]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def log_rows(n_idx, D):
    return max(5, (32 * n_idx * D - 1).bit_length())


def path_blocks(nodes, idx, leaf=None, levels=None, start=0):
    """the blocks of one path as dicts: from level `start` (node idx >> start, or `leaf` as the entering digest) up `levels` levels"""
    D = len(nodes) - 1
    levels = D - start if levels is None else levels
    cur = list(nodes[start][idx >> start]) if leaf is None else [int(v) for v in leaf]
    lf, out = list(cur), []
    for k in range(levels):
        l = start + k
        node = idx >> l
        bit, sib = node & 1, list(nodes[l][node ^ 1])
        out.append(dict(cur=cur, sib=sib, bit=bit, leaf=lf, r=node, lvl=k + 1, act=1, end=int(k == levels - 1), firstb=int(k == 0)))
        _, s = block_rows((sib + cur if bit else cur + sib) + [0, 0, 0, 0])
        cur = s[:4]
    return out


def assemble(blocks, log_n):
    """blocks (dicts of path_blocks) followed by idle blocks -> trace [66][2^log_n]"""
    n = 1 << log_n
    assert 32 * len(blocks) <= n
    tr = np.zeros((COLS, n), dtype=np.uint64)
    idle = dict(cur=[0] * 4, sib=[0] * 4, bit=0, leaf=[0] * 4, r=0, lvl=1, act=0, end=0, firstb=0)
    idle_rows = None
    for b in range(n // 32):
        blk = blocks[b] if b < len(blocks) else idle
        if blk is idle and idle_rows is not None:
            rows = idle_rows
        else:
            s = (blk["sib"] + blk["cur"] if blk["bit"] else blk["cur"] + blk["sib"]) + [0, 0, 0, 0]
            rows, _ = block_rows(blk.get("state", s))
            if blk is idle:
                idle_rows = rows
        sl = slice(32 * b, 32 * b + 32)
        tr[:48, sl] = rows
        tr[BIT, sl], tr[R, sl], tr[LVL, sl], tr[ACT, sl], tr[END, sl], tr[FIRSTB, sl] = blk["bit"], blk["r"], blk["lvl"], blk["act"], blk["end"], blk["firstb"]
        for i in range(4):
            tr[SIB + i, sl], tr[CUR + i, sl], tr[LEAF + i, sl] = blk["sib"][i], blk["cur"][i], blk["leaf"][i]
    return tr


def public_inputs(nodes, idx, digests=None):
    D = len(nodes) - 1
    digests = [nodes[0][i] for i in idx] if digests is None else digests
    return list(nodes[D][0]) + [D] + claims_digest(idx, digests)


def ref_trace(tree, idx, log_n=None):
    """-> (trace [66][2^log_n], the 9 public inputs, the leaf digests of the openings)"""
    nodes = tree_nodes(tree)
    D = len(nodes) - 1
    log_n = log_rows(len(idx), D) if log_n is None else log_n
    blocks = [blk for i in idx for blk in path_blocks(nodes, int(i))]
    return assemble(blocks, log_n), public_inputs(nodes, idx), np.array([nodes[0][int(i)] for i in idx], dtype=np.uint64)


def _denoms(chal, index, d):
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    return (beta + int(index) + gamma * int(d[0]) + g2 * int(d[1]) + g4 * TAG_OPEN,
            beta + int(index) + gamma * int(d[2]) + g2 * int(d[3]) + g3 + g4 * TAG_OPEN)


def gen_aux(trace, chal, pub=None):
    """-> (aux [4][n]: h (constant over a block), Z; [S / n])"""
    n = trace.shape[1]
    aux = np.zeros((4, n), dtype=np.uint64)
    hs = []
    for b in range(n // 32):
        row = 32 * b
        fb = int(trace[FIRSTB, row])
        h = S.ExtS(0)
        if fb:
            dlo, dhi = _denoms(chal, trace[R, row], [trace[LEAF + i, row] for i in range(4)])
            h = (dlo.inv() + dhi.inv()) * fb
        hs.append(h)
        aux[0, row: row + 32], aux[1, row: row + 32] = h.a, h.b
    tot = S.ExtS(0)
    for h in hs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[2, i], aux[3, i] = z.a, z.b
        if i % 32 == 0:
            z = z + hs[i // 32]
        z = z - apub
    return aux, [apub.a, apub.b]


def chal_hook(pub, cap):
    """one table on its own bus: the shared-challenge transcript of its (public inputs, trace cap)"""
    return S.shared_challenges_n([(pub, cap)], 4)


def prove(trace, pub, cfg=None):
    """the reference prover on the program restatement -> table proof (id word REF_ID)"""
    return S.prove(air(), trace, pub, cfg, chal_hook=chal_hook)


def wrap(proof, log_leaves, n_idx, air_id=AIR_ID):
    """a table proof as a blob of the product, with the compiled AIR's id in its id word"""
    p = np.array(proof, dtype=np.uint64)
    p[1] = air_id
    return np.concatenate([np.array([MAGIC, log_leaves, n_idx, p.size], dtype=np.uint64), p])


def unwrap(blob, air_id=REF_ID):
    """the table proof inside a blob, with the reference registry's id in its id word"""
    p = np.array(blob[HDR:], dtype=np.uint64)
    assert int(blob[0]) == MAGIC and int(blob[3]) == p.size
    p[1] = air_id
    return p


def bus_check(proof, cfg_cap_height, idx, digests):
    """the verifier's side of the bus in Python: published total x rows == sum over the claims of 1 / D_lo + 1 / D_hi"""
    pub, cap = S.proof_peek(proof, cfg_cap_height)
    chal = chal_hook(pub, cap)
    pos = 10 + int(proof[9]) + 2 + len(pub) + (4 << cfg_cap_height)
    apub = S.ExtS(int(proof[pos]), int(proof[pos + 1]))
    tot = S.ExtS(0)
    for i, d in zip(idx, np.asarray(digests, dtype=np.uint64).reshape(-1, 4)):
        dlo, dhi = _denoms(chal, i, d)
        tot = tot + dlo.inv() + dhi.inv()
    return apub * (1 << int(proof[2])) == tot, chal
