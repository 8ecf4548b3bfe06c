"""TEST INFRASTRUCTURE for LeafSpongeAir (csrc/air_leaf_sponge.cuh, AIR id 17): the AIR restated INDEPENDENTLY as a constraint
program (air_program.AirBuilder / X2, the same constraint order as the compiled eval, so oracle.air_program.ProgramAir runs it
through oracle/stark_ref.py unchanged), a reference trace generator and gen_aux in plain Python, the row-claims digest, the
two-table reference prover (MerkleOpenAir's restatement of merkle_open_ref first, then this one, under the shared challenges of
both), the blob wrapper and the verifier's side of the row bus.  No tests here."""
import numpy as np

import merkle_open_ref as M
import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = 2**64 - 2**32 + 1
AIR_ID = 17        # the compiled AIR
REF_ID = 1017      # the program restatement in the reference prover's registry (never registered with the product)
MSG, IDX, POS, ACT, FIRSTB, LASTB, NXL, DIG, COLS = 48, 56, 57, 58, 59, 60, 61, 62, 66
N_HELP, AUX, PUB = 5, 12, 14
TAG_OPEN, TAG_ROW = 8, 9
MAGIC, HDR = int.from_bytes(b"VXMROWS1", "little"), 6
CHAL = M.CHAL
# the leaf lengths both tiers check: a single partial block, exactly one block, a one-word tail, two full blocks, two full blocks
# and a five-word tail
LENGTHS = [5, 8, 9, 16, 21]


def n_blocks(L):
    return (L + 7) // 8


def tail_flags(L):
    t = L % 8
    return [int(i < (t or 8)) for i in range(8)]


def degree(e):
    """total degree of an air_program expression in the trace cells, a periodic column counting as one factor"""
    if e.op in ("loc", "nxt", "per"):
        return 1
    if e.op in ("add", "sub"):
        return max(degree(e.a), degree(e.b))
    if e.op == "mul":
        return degree(e.a) + degree(e.b)
    return 0


def builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(COLS, PUB, periodic=M.periodic(), aux_cols=AUX, n_challenges=4, n_aux_public=1)
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
        acc = y[row] * (M.MDS_CIRC[0] + M.MDS_DIAG[row])
        for i in range(1, 12):
            acc = acc + y[(i + row) % 12] * M.MDS_CIRC[i]
        b.assert_zero(rnd * (b.nxt(row) - acc))
    for i in range(12):
        b.assert_zero(out * (b.nxt(i) - b.loc(i)))
    # 2. shape columns constant over a block
    for j in range(MSG, COLS):
        b.assert_zero((1 - spare) * (b.nxt(j) - b.loc(j)))
    # 3. flags
    idx, pos, act, firstb, last, nxl = (b.loc(j) for j in (IDX, POS, ACT, FIRSTB, LASTB, NXL))
    cont = act - last
    w = [b.pub(2 + i) for i in range(8)]
    b.assert_zero(act * (act - 1))
    b.assert_zero(last * (last - 1))
    b.assert_zero(last * (1 - act))
    # 4. block input: the rate part is MSG
    for i in range(8):
        b.assert_zero(first * (b.loc(i) - b.loc(MSG + i)))
    # 5. spare row -> next block
    sc, sn = spare * cont, spare * (1 - cont)
    for i in range(8, 12):
        b.assert_zero(sc * (b.nxt(i) - b.loc(i)))
    for i in range(8, 12):
        b.assert_zero(sn * b.nxt(i))
    b.assert_zero(sc * (b.nxt(IDX) - idx))
    b.assert_zero(sc * (b.nxt(POS) - pos - 1))
    b.assert_zero(sc * (1 - b.nxt(ACT)))
    b.assert_zero(spare * (b.nxt(FIRSTB) - b.nxt(ACT) * (1 - cont)))
    b.assert_zero(spare * (nxl - cont * b.nxt(LASTB)))
    for i in range(4):
        b.assert_zero(spare * (b.loc(DIG + i) - b.loc(i)))
    sl = spare * nxl
    for i in range(8):
        b.assert_zero(sl * ((b.nxt(MSG + i) - b.loc(i)) * (1 - w[i])))
    # 6. exactly B blocks per leaf; a single-block leaf keeps zero behind its tail
    b.assert_zero(firstb * pos)
    b.assert_zero(last * (pos + 1 - b.pub(1)))
    fl = firstb * last
    for i in range(8):
        b.assert_zero(fl * (b.loc(MSG + i) * (1 - w[i])))
    # 7. the bus
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    pos8 = pos * 8

    def d_row(i):
        return beta + idx + gamma * (pos8 + i) + g2 * b.loc(MSG + i) + g4 * TAG_ROW

    hsum = X2(0, 0)
    for e in range(4):
        ma, mb = cont + last * w[2 * e], cont + last * w[2 * e + 1]
        da, db = d_row(2 * e), d_row(2 * e + 1)
        h = X2(b.aux(2 * e), b.aux(2 * e + 1))
        b.assert_zero_x2(h * da * db - db * ma - da * mb)
        hsum = hsum + h
    dlo = beta + idx + gamma * b.loc(DIG) + g2 * b.loc(DIG + 1) + g4 * TAG_OPEN
    dhi = beta + idx + gamma * b.loc(DIG + 2) + g2 * b.loc(DIG + 3) + g3 + g4 * TAG_OPEN
    h = X2(b.aux(8), b.aux(9))
    b.assert_zero_x2(h * dlo * dhi + (dlo + dhi) * last)
    hsum = hsum + h
    z, zn = X2(b.aux(10), b.aux(11)), X2(b.aux_nxt(10), b.aux_nxt(11))
    b.assert_zero_x2(zn - z - hsum * first + X2(b.apub(0), b.apub(1)))
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
def log_rows(n_idx, L):
    return max(5, (32 * n_idx * n_blocks(L) - 1).bit_length())


def leaf_blocks(index, row):
    """the blocks of one leaf as dicts -> (blocks, digest): the sponge in overwrite mode, 8 words per permutation"""
    L, B = len(row), n_blocks(len(row))
    state, out = [0] * 12, []
    for k in range(B):
        words = [int(v) for v in row[8 * k: 8 * k + 8]]
        state[:len(words)] = words
        _, nxt = M.block_rows(state)
        out.append(dict(state=list(state), msg=list(state[:8]), idx=int(index), pos=k, act=1, firstb=int(k == 0), lastb=int(k == B - 1), nxl=int(k == B - 2), dig=nxt[:4]))
        state = nxt
    return out, state[:4]


_idle = None


def idle_block():
    global _idle
    if _idle is None:
        _, nxt = M.block_rows([0] * 12)
        _idle = dict(state=[0] * 12, msg=[0] * 8, idx=0, pos=0, act=0, firstb=0, lastb=0, nxl=0, dig=nxt[:4])
    return _idle


def assemble(blocks, log_n):
    """blocks (dicts of leaf_blocks) followed by idle blocks -> trace [66][2^log_n]"""
    n = 1 << log_n
    assert 32 * len(blocks) <= n
    tr = np.zeros((COLS, n), dtype=np.uint64)
    idle_rows = None
    for b in range(n // 32):
        blk = blocks[b] if b < len(blocks) else idle_block()
        if blk is idle_block() and idle_rows is not None:
            rows = idle_rows
        else:
            rows, _ = M.block_rows(blk["state"])
            if blk is idle_block():
                idle_rows = rows
        sl = slice(32 * b, 32 * b + 32)
        tr[:48, sl] = rows
        for j, key in ((IDX, "idx"), (POS, "pos"), (ACT, "act"), (FIRSTB, "firstb"), (LASTB, "lastb"), (NXL, "nxl")):
            tr[j, sl] = blk[key]
        for i in range(8):
            tr[MSG + i, sl] = blk["msg"][i]
        for i in range(4):
            tr[DIG + i, sl] = blk["dig"][i]
    return tr


def claims_digest(idx, rows):
    words = []
    for i, r in zip(idx, rows):
        words += [int(i)] + [int(v) for v in r]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def public_inputs(idx, rows):
    L = len(rows[0])
    return [L, n_blocks(L)] + tail_flags(L) + claims_digest(idx, rows)


def ref_trace(idx, rows, log_n=None):
    """idx: leaf indices; rows: the opened rows [n_idx][L] -> (trace [66][2^log_n], the 14 public inputs, the digests [n_idx][4])"""
    L = len(rows[0])
    log_n = log_rows(len(idx), L) if log_n is None else log_n
    blocks, digs = [], []
    for i, r in zip(idx, rows):
        bl, d = leaf_blocks(i, r)
        blocks += bl
        digs.append(d)
    return assemble(blocks, log_n), public_inputs(idx, rows), np.array(digs, dtype=np.uint64)


def _bus(chal):
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g2 = gamma * gamma
    return beta, gamma, g2, g2 * gamma, g2 * g2


def d_row(chal, index, position, word):
    beta, gamma, g2, _, g4 = _bus(chal)
    return beta + int(index) + gamma * int(position) + g2 * int(word) + g4 * TAG_ROW


def block_helpers(chal, wflags, cell, tail_sent=False):
    """the five helpers of one block from its shape cells (cell(column) -> int); tail_sent forges: every word of a last block sent"""
    act, last = cell(ACT), cell(LASTB)
    if not act:
        return [S.ExtS(0)] * N_HELP
    hs = []
    for e in range(4):
        m = [1 if (not last or wflags[i] or tail_sent) else 0 for i in (2 * e, 2 * e + 1)]
        d = [d_row(chal, cell(IDX), 8 * cell(POS) + i, cell(MSG + i)) for i in (2 * e, 2 * e + 1)]
        hs.append(d[0].inv() * m[0] + d[1].inv() * m[1])
    dlo, dhi = M._denoms(chal, cell(IDX), [cell(DIG + i) for i in range(4)])
    hs.append((dlo.inv() + dhi.inv()) * (P - 1 if last else 0))
    return hs


def gen_aux(trace, chal, pub=None, tail_sent=False):
    """-> (aux [12][n]: five helpers (constant over a block), Z; [S / n]).  pub: the public inputs (the tail flags are read)"""
    n = trace.shape[1]
    wflags = [1] * 8 if pub is None else [int(v) for v in pub[2:10]]
    aux = np.zeros((AUX, n), dtype=np.uint64)
    incs = []
    for b in range(n // 32):
        row = 32 * b
        hs = block_helpers(chal, wflags, lambda j: int(trace[j, row]), tail_sent)
        tot = S.ExtS(0)
        for e, h in enumerate(hs):
            aux[2 * e, row: row + 32], aux[2 * e + 1, row: row + 32] = h.a, h.b
            tot = tot + h
        incs.append(tot)
    tot = S.ExtS(0)
    for h in incs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[10, i], aux[11, i] = z.a, z.b
        if i % 32 == 0:
            z = z + incs[i // 32]
        z = z - apub
    return aux, [apub.a, apub.b]


# ---- two tables on one bus
def trace_cap(trace, cfg):
    """the cap of a trace's commitment, as the provers compute it (the shared challenges need every table's cap first)"""
    cfg = dict(S.DEFAULT_CFG, **(cfg or {}))
    leaves, _ = O.lde_from_values(np.ascontiguousarray(trace, dtype=np.uint64), cfg["rate_bits"], S.G)
    return O.MerkleTree(leaves, cfg["cap_height"]).cap.reshape(-1)


def shared_challenges(tables):
    """tables: [(public inputs, trace cap)] in bus order -- openings, then sponge"""
    return S.shared_challenges_n(tables, 4)


def prove(open_trace, open_pub, sponge_trace, sponge_pub, cfg=None):
    """the reference prover on both restatements under the challenges both tables share -> (MerkleOpenAir proof, LeafSpongeAir
    proof), id words M.REF_ID / REF_ID"""
    chal = shared_challenges([(open_pub, trace_cap(open_trace, cfg)), (sponge_pub, trace_cap(sponge_trace, cfg))])
    hook = lambda pub, cap: chal  # noqa: E731
    return S.prove(M.air(), open_trace, open_pub, cfg, chal_hook=hook), S.prove(air(), sponge_trace, sponge_pub, cfg, chal_hook=hook)


def prove_rows(tree, idx, rows, cfg=None):
    """both traces of the openings idx of an oracle.MerkleTree whose leaves `rows` are, and both proofs"""
    open_trace, open_pub, _ = M.ref_trace(tree, idx)
    sponge_trace, sponge_pub, _ = ref_trace(idx, rows)
    return prove(open_trace, open_pub, sponge_trace, sponge_pub, cfg)


def wrap(p_open, p_sponge, log_leaves, leaf_len, n_idx):
    """two table proofs as a blob of the product, with the compiled AIRs' ids in their id words"""
    a, b = np.array(p_open, dtype=np.uint64), np.array(p_sponge, dtype=np.uint64)
    a[1], b[1] = M.AIR_ID, AIR_ID
    return np.concatenate([np.array([MAGIC, log_leaves, leaf_len, n_idx, a.size, b.size], dtype=np.uint64), a, b])


def unwrap(blob):
    """the two table proofs inside a blob, with the reference registry's ids in their id words"""
    assert int(blob[0]) == MAGIC and int(blob[4]) + int(blob[5]) == blob.size - HDR
    a, b = np.array(blob[HDR: HDR + int(blob[4])], dtype=np.uint64), np.array(blob[HDR + int(blob[4]):], dtype=np.uint64)
    a[1], b[1] = M.REF_ID, REF_ID
    return a, b


def published_total(proof, cap_h):
    """(S / n of a table proof, its rows)"""
    pub, _ = S.proof_peek(proof, cap_h)
    pos = 10 + int(proof[9]) + 2 + len(pub) + (4 << cap_h)
    return S.ExtS(int(proof[pos]), int(proof[pos + 1])), 1 << int(proof[2])


def bus_check(p_open, p_sponge, cap_h, idx, rows):
    """the verifier's side of the row bus in Python: the two published totals x rows == sum over the claims of 1 / D_row"""
    chal = shared_challenges([S.proof_peek(p_open, cap_h), S.proof_peek(p_sponge, cap_h)])
    (so, no), (ss, ns) = published_total(p_open, cap_h), published_total(p_sponge, cap_h)
    tot = S.ExtS(0)
    for i, r in zip(idx, rows):
        for j, v in enumerate(r):
            tot = tot + d_row(chal, i, j, v).inv()
    return so * no + ss * ns == tot, chal
