"""TEST INFRASTRUCTURE for the FRI query phase on one bus (csrc/vx_fri_queries.hip): MerkleOpenSetAir (AIR id 19) and
LeafSpongeSetAir (AIR id 20) restated INDEPENDENTLY as constraint programs (air_program.AirBuilder / X2, the same constraint order
as the compiled evals, so oracle.air_program.ProgramAir runs them through oracle/stark_ref.py unchanged), reference trace generators
and gen_aux in plain Python, the claims digests of the set tables, the statement digest, the three-table reference prover
(openings, sponge, FriFoldAir's restatement of fri_fold_ref, under the challenges all three share), the blob wrapper and the
verifier's side of the bus.  No tests here."""
import numpy as np

import fri_fold_ref as F
import leaf_sponge_ref as R
import merkle_open_ref as M
import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = 2**64 - 2**32 + 1
OPEN_ID, SPONGE_ID = 19, 20              # the compiled AIRs
OPEN_REF_ID, SPONGE_REF_ID = 1019, 1020  # the restatements in the reference prover's registry (never registered with the product)
# MerkleOpenSetAir: MerkleOpenAir's columns, then
O_TREE, O_ROOT, O_DEPTH, O_COLS, O_AUX, O_PUB = 66, 67, 71, 72, 6, 4
# LeafSpongeSetAir: LeafSpongeAir's columns, then
S_TREE, S_COLS, S_AUX, S_PUB = 66, 67, 12, 14
TAG_OPEN, TAG_ROW, TAG_FRI, TAG_ROOT = 8, 9, 10, 11
MAGIC, HDR = int.from_bytes(b"VXFQRY01", "little"), 7
CHAL = M.CHAL
LEAF_LEN = 32  # a FRI leaf: 16 extension values
degree = R.degree


def _permutation(b):
    """constraints 0..59 of both AIRs: one PoseidonAir block"""
    full, rnd, out = b.per(12), b.per(13), b.per(14)
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


def _bus_x2(b, X2):
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    return beta, gamma, g2, g2 * gamma, g2 * g2


OPEN_RULES, SPONGE_RULES = {}, {}  # rule name -> index of its first constraint (filled by the builders)


def open_builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(O_COLS, O_PUB, periodic=M.periodic(), aux_cols=O_AUX, n_challenges=4, n_aux_public=1)
    mark = lambda name: OPEN_RULES.__setitem__(name, len(b.constraints))  # noqa: E731
    spare, first = b.per(15), b.per(16)
    _permutation(b)
    # 2. the 24 shape columns are constant over a block
    mark("block_constant")
    for j in range(M.BIT, O_COLS):
        b.assert_zero((1 - spare) * (b.nxt(j) - b.loc(j)))
    # 3. flags
    bit, act, end, r, lvl, tree, depth = (b.loc(j) for j in (M.BIT, M.ACT, M.END, M.R, M.LVL, O_TREE, O_DEPTH))
    cont = act - end
    mark("flags")
    b.assert_zero(bit * (bit - 1))
    b.assert_zero(act * (act - 1))
    b.assert_zero(end * (end - 1))
    b.assert_zero(end * (1 - act))
    # 4. block input
    mark("block_input")
    for i in range(4):
        b.assert_zero(first * (b.loc(i) - b.loc(M.CUR + i) - bit * (b.loc(M.SIB + i) - b.loc(M.CUR + i))))
    for i in range(4):
        b.assert_zero(first * (b.loc(4 + i) - b.loc(M.SIB + i) + bit * (b.loc(M.SIB + i) - b.loc(M.CUR + i))))
    for i in range(8, 12):
        b.assert_zero(first * b.loc(i))
    # 5. spare row -> next block
    sc, sn = spare * cont, spare * (1 - cont)
    mark("carry")
    for i in range(4):
        b.assert_zero(sc * (b.nxt(M.CUR + i) - b.loc(i)))
    for i in range(4):
        b.assert_zero(sc * (b.nxt(M.LEAF + i) - b.loc(M.LEAF + i)))
    b.assert_zero(sc * (r - 2 * b.nxt(M.R) - bit))
    b.assert_zero(sc * (b.nxt(M.LVL) - lvl - 1))
    b.assert_zero(sc * (1 - b.nxt(M.ACT)))
    mark("tree_carried")
    b.assert_zero(sc * (b.nxt(O_TREE) - tree))
    mark("path_start")
    for i in range(4):
        b.assert_zero(sn * (b.nxt(M.CUR + i) - b.nxt(M.LEAF + i)))
    b.assert_zero(sn * (b.nxt(M.LVL) - 1))
    b.assert_zero(spare * (b.nxt(M.FIRSTB) - b.nxt(M.ACT) * (1 - cont)))
    # 6. top of a path: no index bit left, the level is DEPTH, the output is ROOT
    mark("no_bit_left")
    b.assert_zero(end * (r - bit))
    mark("level_is_depth")
    b.assert_zero(end * (lvl - depth))
    mark("output_is_root")
    for i in range(4):
        b.assert_zero(spare * end * (b.loc(i) - b.loc(O_ROOT + i)))
    # 7. the bus: the opening under FIRSTB, the root under END
    beta, gamma, g2, g3, g4 = _bus_x2(b, X2)
    t2 = tree * 2
    dlo = beta + r + gamma * b.loc(M.LEAF) + g2 * b.loc(M.LEAF + 1) + g3 * t2 + g4 * TAG_OPEN
    dhi = beta + r + gamma * b.loc(M.LEAF + 2) + g2 * b.loc(M.LEAF + 3) + g3 * (t2 + 1) + g4 * TAG_OPEN
    rlo = beta + t2 + gamma * b.loc(O_ROOT) + g2 * b.loc(O_ROOT + 1) + g3 * depth + g4 * TAG_ROOT
    rhi = beta + (t2 + 1) + gamma * b.loc(O_ROOT + 2) + g2 * b.loc(O_ROOT + 3) + g3 * depth + g4 * TAG_ROOT
    h, h2 = X2(b.aux(0), b.aux(1)), X2(b.aux(2), b.aux(3))
    z, zn = X2(b.aux(4), b.aux(5)), X2(b.aux_nxt(4), b.aux_nxt(5))
    mark("helper_open")
    b.assert_zero_x2(h * dlo * dhi - (dlo + dhi) * b.loc(M.FIRSTB))
    mark("helper_root")
    b.assert_zero_x2(h2 * rlo * rhi - (rlo + rhi) * end)
    mark("running_sum")
    b.assert_zero_x2(zn - z - (h + h2) * first + X2(b.apub(0), b.apub(1)))
    return b


def sponge_builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(S_COLS, S_PUB, periodic=M.periodic(), aux_cols=S_AUX, n_challenges=4, n_aux_public=1)
    mark = lambda name: SPONGE_RULES.__setitem__(name, len(b.constraints))  # noqa: E731
    spare, first = b.per(15), b.per(16)
    _permutation(b)
    mark("block_constant")
    for j in range(R.MSG, S_COLS):
        b.assert_zero((1 - spare) * (b.nxt(j) - b.loc(j)))
    idx, pos, act, firstb, last, nxl, tree = (b.loc(j) for j in (R.IDX, R.POS, R.ACT, R.FIRSTB, R.LASTB, R.NXL, S_TREE))
    cont = act - last
    w = [b.pub(2 + i) for i in range(8)]
    mark("flags")
    b.assert_zero(act * (act - 1))
    b.assert_zero(last * (last - 1))
    b.assert_zero(last * (1 - act))
    mark("block_input")
    for i in range(8):
        b.assert_zero(first * (b.loc(i) - b.loc(R.MSG + i)))
    sc, sn = spare * cont, spare * (1 - cont)
    mark("carry")
    for i in range(8, 12):
        b.assert_zero(sc * (b.nxt(i) - b.loc(i)))
    for i in range(8, 12):
        b.assert_zero(sn * b.nxt(i))
    b.assert_zero(sc * (b.nxt(R.IDX) - idx))
    b.assert_zero(sc * (b.nxt(R.POS) - pos - 1))
    b.assert_zero(sc * (1 - b.nxt(R.ACT)))
    mark("tree_carried")
    b.assert_zero(sc * (b.nxt(S_TREE) - tree))
    mark("leaf_shape")
    b.assert_zero(spare * (b.nxt(R.FIRSTB) - b.nxt(R.ACT) * (1 - cont)))
    b.assert_zero(spare * (nxl - cont * b.nxt(R.LASTB)))
    for i in range(4):
        b.assert_zero(spare * (b.loc(R.DIG + i) - b.loc(i)))
    sl = spare * nxl
    for i in range(8):
        b.assert_zero(sl * ((b.nxt(R.MSG + i) - b.loc(i)) * (1 - w[i])))
    b.assert_zero(firstb * pos)
    b.assert_zero(last * (pos + 1 - b.pub(1)))
    fl = firstb * last
    for i in range(8):
        b.assert_zero(fl * (b.loc(R.MSG + i) * (1 - w[i])))
    # the bus: eight words of tree TREE sent, the digest of a leaf of tree TREE received
    beta, gamma, g2, g3, g4 = _bus_x2(b, X2)
    pos8, t2 = pos * 8, tree * 2

    def d_row_(i):
        return beta + idx + gamma * (pos8 + i) + g2 * b.loc(R.MSG + i) + g3 * tree + g4 * TAG_ROW

    hsum = X2(0, 0)
    mark("helpers")
    for e in range(4):
        ma, mb = cont + last * w[2 * e], cont + last * w[2 * e + 1]
        da, db = d_row_(2 * e), d_row_(2 * e + 1)
        h = X2(b.aux(2 * e), b.aux(2 * e + 1))
        b.assert_zero_x2(h * da * db - db * ma - da * mb)
        hsum = hsum + h
    dlo = beta + idx + gamma * b.loc(R.DIG) + g2 * b.loc(R.DIG + 1) + g3 * t2 + g4 * TAG_OPEN
    dhi = beta + idx + gamma * b.loc(R.DIG + 2) + g2 * b.loc(R.DIG + 3) + g3 * (t2 + 1) + g4 * TAG_OPEN
    h = X2(b.aux(8), b.aux(9))
    b.assert_zero_x2(h * dlo * dhi + (dlo + dhi) * last)
    hsum = hsum + h
    z, zn = X2(b.aux(10), b.aux(11)), X2(b.aux_nxt(10), b.aux_nxt(11))
    mark("running_sum")
    b.assert_zero_x2(zn - z - hsum * first + X2(b.apub(0), b.apub(1)))
    return b


_airs = {}


def _air(key, ref_id, builder, gen):
    if key not in _airs:
        b = builder()
        code, consts, _ = b.assemble()
        _airs[key] = ProgramAir(ref_id, b.cols, b.n_public, code, consts, b.periodic, b.aux_cols, b.n_challenges, b.n_aux_public, gen_aux=gen)
        S.register_air(_airs[key])
    return _airs[key]


def open_air():
    return _air("open", OPEN_REF_ID, open_builder, open_gen_aux)


def sponge_air():
    return _air("sponge", SPONGE_REF_ID, sponge_builder, sponge_gen_aux)


# ---- denominators
def _bus(chal):
    return F._bus(chal)


def d_open(bus, tree, index, da, db, half):
    beta, gamma, g2, g3, g4 = bus
    return beta + int(index) + gamma * int(da) + g2 * int(db) + g3 * (2 * int(tree) + half) + g4 * TAG_OPEN


def d_root(bus, tree, ra, rb, half, depth):
    beta, gamma, g2, g3, g4 = bus
    return beta + (2 * int(tree) + half) + gamma * int(ra) + g2 * int(rb) + g3 * int(depth) + g4 * TAG_ROOT


d_row, d_fri = F.d_row, F.d_fri


# ---- the layer trees of a commit phase
def layer_rows(layers):
    """F.commit_phase's layers as Merkle leaves: layer l -> rows [2^(LN - 4 (l + 1))][32]"""
    return [np.ascontiguousarray(lv, dtype=np.uint64).reshape(lv.shape[0], 32) for lv in layers]


def layer_values(layers):
    """... as the values the layer trees are built from: natural order, [2^(LN - 4 l)][2] (leaf j holds positions bitrev(16 j + t))"""
    out = []
    for lv in layers:
        flat = np.ascontiguousarray(lv, dtype=np.uint64).reshape(-1, 2)
        out.append(flat[S.bitrev_perm(flat.shape[0].bit_length() - 1)])
    return out


def layer_trees(layers, cap_height):
    return [O.MerkleTree(rows, cap_height) for rows in layer_rows(layers)]


def openings_of(index, NL):
    """one opening per (query, layer), queries outermost -> (tree_of, leaf_idx)"""
    tree_of = [l for _ in index for l in range(NL)]
    leaf_idx = [int(i) >> (4 * (l + 1)) for i in index for l in range(NL)]
    return tree_of, leaf_idx


# ---- MerkleOpenSetAir witness
def open_log_rows(nodes, tree_of):
    return max(5, (32 * sum(len(nodes[t]) - 1 for t in tree_of) - 1).bit_length())


def open_blocks(nodes, tree, idx, **kw):
    """the blocks of one path of tree `tree` (nodes: M.tree_nodes of every tree); kw as M.path_blocks (forgeries)"""
    nd = nodes[tree]
    blocks = M.path_blocks(nd, idx, **kw)
    for blk in blocks:
        blk.update(tree=tree, root=list(nd[-1][0]), depth=len(nd) - 1)
    return blocks


def open_assemble(blocks, log_n):
    tr = np.zeros((O_COLS, 1 << log_n), dtype=np.uint64)
    tr[:M.COLS] = M.assemble(blocks, log_n)
    for b, blk in enumerate(blocks):
        sl = slice(32 * b, 32 * b + 32)
        tr[O_TREE, sl], tr[O_DEPTH, sl] = blk["tree"], blk["depth"]
        for i in range(4):
            tr[O_ROOT + i, sl] = blk["root"][i]
    return tr


def open_claims_digest(tree_of, leaf_idx, digests):
    words = []
    for t, i, d in zip(tree_of, leaf_idx, digests):
        words += [int(t), int(i)] + [int(v) for v in d]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def open_ref_trace(trees, tree_of, leaf_idx, log_n=None):
    """trees: oracle.MerkleTree per tree -> (trace [72][2^log_n], the 4 public inputs: the claims digest)"""
    nodes = [M.tree_nodes(t) for t in trees]
    log_n = open_log_rows(nodes, tree_of) if log_n is None else log_n
    blocks = [blk for t, i in zip(tree_of, leaf_idx) for blk in open_blocks(nodes, int(t), int(i))]
    return open_assemble(blocks, log_n), open_claims_digest(tree_of, leaf_idx, [nodes[t][0][int(i)] for t, i in zip(tree_of, leaf_idx)])


def open_gen_aux(trace, chal, pub=None):
    """-> (aux [6][n]: h, h2 (constant over a block), Z; [S / n])"""
    n = trace.shape[1]
    bus = _bus(chal)
    aux = np.zeros((O_AUX, n), dtype=np.uint64)
    incs = []
    for b in range(n // 32):
        row = 32 * b
        cell = lambda j: int(trace[j, row])  # noqa: E731
        h, h2 = S.ExtS(0), S.ExtS(0)
        if cell(M.FIRSTB):
            h = (d_open(bus, cell(O_TREE), cell(M.R), cell(M.LEAF), cell(M.LEAF + 1), 0).inv()
                 + d_open(bus, cell(O_TREE), cell(M.R), cell(M.LEAF + 2), cell(M.LEAF + 3), 1).inv()) * cell(M.FIRSTB)
        if cell(M.END):
            h2 = (d_root(bus, cell(O_TREE), cell(O_ROOT), cell(O_ROOT + 1), 0, cell(O_DEPTH)).inv()
                  + d_root(bus, cell(O_TREE), cell(O_ROOT + 2), cell(O_ROOT + 3), 1, cell(O_DEPTH)).inv()) * cell(M.END)
        aux[0, row: row + 32], aux[1, row: row + 32], aux[2, row: row + 32], aux[3, row: row + 32] = h.a, h.b, h2.a, h2.b
        incs.append(h + h2)
    return _close(aux, 4, incs, n)


def _close(aux, zcol, incs, n):
    tot = S.ExtS(0)
    for h in incs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[zcol, i], aux[zcol + 1, i] = z.a, z.b
        if i % 32 == 0:
            z = z + incs[i // 32]
        z = z - apub
    return aux, [apub.a, apub.b]


# ---- LeafSpongeSetAir witness
def sponge_log_rows(n_idx, L=LEAF_LEN):
    return R.log_rows(n_idx, L)


def sponge_blocks(tree, index, row):
    blocks, dig = R.leaf_blocks(index, row)
    for blk in blocks:
        blk["tree"] = tree
    return blocks, dig


def sponge_assemble(blocks, log_n):
    tr = np.zeros((S_COLS, 1 << log_n), dtype=np.uint64)
    tr[:R.COLS] = R.assemble(blocks, log_n)
    for b, blk in enumerate(blocks):
        tr[S_TREE, 32 * b: 32 * b + 32] = blk["tree"]
    return tr


def sponge_claims_digest(tree_of, leaf_idx, rows):
    words = []
    for t, i, r in zip(tree_of, leaf_idx, rows):
        words += [int(t), int(i)] + [int(v) for v in r]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def sponge_public(L, digest):
    return [L, R.n_blocks(L)] + R.tail_flags(L) + [int(v) for v in digest]


def sponge_ref_trace(tree_of, leaf_idx, rows, log_n=None):
    """rows: the opened rows [n_idx][L] -> (trace [67][2^log_n], the 14 public inputs, the digests [n_idx][4])"""
    L = len(rows[0])
    log_n = sponge_log_rows(len(leaf_idx), L) if log_n is None else log_n
    blocks, digs = [], []
    for t, i, r in zip(tree_of, leaf_idx, rows):
        bl, d = sponge_blocks(int(t), int(i), r)
        blocks += bl
        digs.append(d)
    return sponge_assemble(blocks, log_n), sponge_public(L, sponge_claims_digest(tree_of, leaf_idx, rows)), np.array(digs, dtype=np.uint64)


def sponge_gen_aux(trace, chal, pub=None):
    """-> (aux [12][n]: five helpers (constant over a block), Z; [S / n]).  pub: the public inputs (the tail flags are read)"""
    n = trace.shape[1]
    wflags = [1] * 8 if pub is None else [int(v) for v in pub[2:10]]
    bus = _bus(chal)
    aux = np.zeros((S_AUX, n), dtype=np.uint64)
    incs = []
    for b in range(n // 32):
        row = 32 * b
        cell = lambda j: int(trace[j, row])  # noqa: E731
        hs = [S.ExtS(0)] * 5
        if cell(R.ACT):
            last, tree, idx = cell(R.LASTB), cell(S_TREE), cell(R.IDX)
            hs = []
            for e in range(4):
                h = S.ExtS(0)
                for i in (2 * e, 2 * e + 1):
                    if not last or wflags[i]:
                        h = h + d_row(bus, tree, idx, 8 * cell(R.POS) + i, cell(R.MSG + i)).inv()
                hs.append(h)
            h = S.ExtS(0)
            if last:
                h = (d_open(bus, tree, idx, cell(R.DIG), cell(R.DIG + 1), 0).inv() + d_open(bus, tree, idx, cell(R.DIG + 2), cell(R.DIG + 3), 1).inv()) * (P - 1)
            hs.append(h)
        tot = S.ExtS(0)
        for e, h in enumerate(hs):
            aux[2 * e, row: row + 32], aux[2 * e + 1, row: row + 32] = h.a, h.b
            tot = tot + h
        incs.append(tot)
    return _close(aux, 10, incs, n)


# ---- the statement and the three tables
def final_len_words(final_poly):
    return [int(v) for v in np.asarray(final_poly, dtype=np.uint64).reshape(-1)]


def statement_digest(LN, betas, final_poly, roots, index, ev0):
    """hash_n_to_hash_no_pad(log_lde, NL, n_q, betas, final_poly, the NL roots, (index, ev_0) of every query)"""
    words = [LN, len(betas), len(index)]
    for be in betas:
        words += [int(be[0]), int(be[1])]
    words += final_len_words(final_poly)
    for r in roots:
        words += [int(v) for v in r]
    for i, e in zip(index, ev0):
        words += [int(i), int(e[0]), int(e[1])]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def roots_of(trees):
    return [M.fold_cap(t.cap) for t in trees]


def tables(LN, betas, final_poly, layers, trees, index):
    """the three traces and their public inputs in this circuit (every digest is the statement digest)
    -> ([(trace, pub)] openings, sponge, fold; ev0 [n][2])"""
    NL = len(betas)
    ev0, leaves = F.claims_from(layers, index)
    tree_of, leaf_idx = openings_of(index, NL)
    rows = [layer_rows(layers)[t][i] for t, i in zip(tree_of, leaf_idx)]
    stmt = statement_digest(LN, betas, final_poly, roots_of(trees), index, ev0)
    otr, _ = open_ref_trace(trees, tree_of, leaf_idx)
    str_, _, _ = sponge_ref_trace(tree_of, leaf_idx, rows)
    ftr, fpub = F.ref_trace(index, leaves, betas, LN)
    return [(otr, list(stmt)), (str_, sponge_public(LEAF_LEN, stmt)), (ftr, fpub[:F.PUB_DIGEST] + list(stmt))], ev0


def shared_challenges(tabs, cfg=None):
    return S.shared_challenges_n([(pub, R.trace_cap(tr, cfg)) for tr, pub in tabs], 4)


def prove(tabs, cfg=None, chal=None):
    """the reference prover on the three restatements under the challenges all tables share -> three proofs (id words REF ids)"""
    chal = shared_challenges(tabs, cfg) if chal is None else chal
    hook = lambda pub, cap: chal  # noqa: E731
    return [S.prove(a, tr, pub, cfg, chal_hook=hook) for a, (tr, pub) in zip((open_air(), sponge_air(), F.air()), tabs)]


def wrap(proofs, LN, NL, n_q):
    """three table proofs as a blob of the product, with the compiled AIRs' ids in their id words"""
    ps = [np.array(p, dtype=np.uint64) for p in proofs]
    for p, i in zip(ps, (OPEN_ID, SPONGE_ID, F.AIR_ID)):
        p[1] = i
    return np.concatenate([np.array([MAGIC, LN, NL, n_q] + [p.size for p in ps], dtype=np.uint64)] + ps)


def unwrap(blob):
    """the three table proofs inside a blob, with the reference registry's ids in their id words"""
    assert int(blob[0]) == MAGIC and sum(int(v) for v in blob[4:7]) == blob.size - HDR
    out, at = [], HDR
    for k, i in enumerate((OPEN_REF_ID, SPONGE_REF_ID, F.REF_ID)):
        p = np.array(blob[at: at + int(blob[4 + k])], dtype=np.uint64)
        p[1] = i
        out.append(p)
        at += p.size
    return out


def outside_sum(chal, LN, NL, final_poly, roots, index, ev0):
    """what the verifier puts on the bus: - 1 / D_fri(index, ev_0, 0) + 1 / D_fri(index, final(x_NL), 1) + the two halves of
    (root, depth) of every layer, per query"""
    bus = _bus(chal)
    tot = S.ExtS(0)
    for i, e in zip(index, ev0):
        fe = F.final_eval(final_poly, int(i), LN, NL)
        tot = tot - d_fri(bus, i, e[0], e[1], 0).inv() + d_fri(bus, i, fe.a, fe.b, 1).inv()
        for l in range(NL):
            r, depth = roots[l], LN - 4 * (l + 1)
            tot = tot + d_root(bus, l, r[0], r[1], 0, depth).inv() + d_root(bus, l, r[2], r[3], 1, depth).inv()
    return tot


def tables_sum(aux_pubs, tabs):
    tot = S.ExtS(0)
    for apub, (tr, _) in zip(aux_pubs, tabs):
        tot = tot + S.ExtS(*apub) * tr.shape[1]
    return tot


def bus_check(proofs, cap_h, LN, NL, final_poly, roots, index, ev0):
    """the verifier's side of the bus in Python on three proofs: the published totals x rows == outside_sum"""
    chal = S.shared_challenges_n([S.proof_peek(p, cap_h) for p in proofs], 4)
    tot = S.ExtS(0)
    for p in proofs:
        s, n = R.published_total(p, cap_h)
        tot = tot + s * n
    return tot == outside_sum(chal, LN, NL, final_poly, roots, index, ev0), chal
