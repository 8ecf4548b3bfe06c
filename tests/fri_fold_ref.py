"""TEST INFRASTRUCTURE for FriFoldAir (csrc/air_fri_fold.cuh, AIR id 18): the AIR restated INDEPENDENTLY as a constraint program
(air_program.AirBuilder / X2, the same constraint order as the compiled eval, so oracle.air_program.ProgramAir runs it through
oracle/stark_ref.py unchanged), a reference trace generator and gen_aux in plain Python, the claims digest, the one-table reference
prover, the blob wrapper, the verifier's side of the bus, and a FRI commit phase on a random polynomial to cut claims from.
No tests here."""
import numpy as np

import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = 2**64 - 2**32 + 1
AIR_ID = 18        # the compiled AIR
REF_ID = 1018      # the program restatement in the reference prover's registry (never registered with the product)
# main columns
ACT, FOLD, FIRST, LAST, FBIT, CNT, R, Q, IDX = range(9)
B, OH, LSEL = 9, 13, 29                      # 4 bits, the 16-cell one-hot of `within`, the 8-cell one-hot of the layer
Y, SI, S1, S2, S3, Y0 = 37, 38, 39, 40, 41, 42
A, A1, A2, A3, A4 = 43, 44, 45, 46, 47
BE, EV, LEAF, V1, V2, V3, V4, COLS = 48, 56, 58, 90, 106, 114, 118, 120
VLEV = [LEAF, V1, V2, V3, V4]
N_HELP, AUX = 17, 36
PUB_NL, PUB_ROWS, PUB_WINV, PUB_TREE0, PUB_BETA, PUB_DIGEST, PUB = 0, 1, 2, 3, 4, 20, 24
MAX_LAYERS = 8
TAG_ROW, TAG_FRI = 9, 10
MAGIC, HDR = int.from_bytes(b"VXFFOLD1", "little"), 5
CHAL = [0x1234567890ABCDEF % P, 77, P - 5, 0xFEDCBA9876543210 % P]
HALF, INV7 = pow(2, P - 2, P), pow(7, P - 2, P)
G16 = O.root(4)


def brev(x, bits):
    r = 0
    for i in range(bits):
        r = (r << 1) | ((x >> i) & 1)
    return r


def fold_const(j, k):
    """1 / (2 g^(2^j brev(k, 3 - j))): the compile-time factor of pair k of fold level j"""
    return HALF * pow(G16, (16 - (1 << j) * brev(k, 3 - j)) % 16, P) % P


def degree(e):
    """total degree of an air_program expression in the trace cells (a challenge or a public input counts 0)"""
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
    b = ap.AirBuilder(COLS, PUB, aux_cols=AUX, n_challenges=4, n_aux_public=1)
    loc, nxt = b.loc, b.nxt

    def x2(col, row=loc):
        return X2(row(col), row(col + 1))

    def total(terms):
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        return acc

    act, fold, first, last, cnt, r, q, idx = (loc(j) for j in (ACT, FOLD, FIRST, LAST, CNT, R, Q, IDX))
    bits = [loc(B + i) for i in range(4)]
    oh = [loc(OH + t) for t in range(16)]
    sel = [loc(LSEL + i) for i in range(MAX_LAYERS)]
    cont = act - last
    # 1. boolean cells
    for v in [act, fold, last] + bits + oh + sel:
        b.assert_zero(v * (v - 1))
    # 2. the shape of a query: fold rows, then bit rows
    b.assert_zero(fold * (1 - act))
    b.assert_zero(last * (1 - act))
    b.assert_zero(last * fold)
    for i in range(1, 4):
        b.assert_zero((act - fold) * bits[i])
    b.assert_zero(first * (1 - fold))
    b.assert_zero(nxt(FIRST) - nxt(ACT) * (1 - cont))
    b.assert_zero(nxt(FBIT) - fold * (1 - nxt(FOLD)))
    b.assert_zero(nxt(FOLD) * (1 - nxt(FIRST)) * (1 - fold))
    b.assert_zero(fold * (1 - nxt(FOLD)) * (cnt + 1 - b.pub(PUB_NL)))
    b.assert_zero(cont * (1 - nxt(ACT)))
    # 3. the row counter and the index digits
    within = bits[0] + bits[1] * 2 + bits[2] * 4 + bits[3] * 8
    b.assert_zero(first * cnt)
    b.assert_zero(cont * (nxt(CNT) - cnt - 1))
    b.assert_zero(last * (cnt + 1 - b.pub(PUB_ROWS)))
    b.assert_zero(r - within - q * (fold * 14 + 2))
    b.assert_zero(cont * (nxt(R) - q))
    b.assert_zero(last * q)
    b.assert_zero(first * (r - idx))
    b.assert_zero(cont * (nxt(IDX) - idx))
    # 4. the one-hots
    b.assert_zero(total(oh) - fold)
    b.assert_zero(total([oh[t] * t for t in range(1, 16)]) - fold * within)
    b.assert_zero(total(sel) - fold)
    b.assert_zero(total([sel[i] * i for i in range(1, MAX_LAYERS)]) - fold * cnt)
    # 5. the point, by inverses
    y, si, s1, s2, s3, y0 = (loc(j) for j in (Y, SI, S1, S2, S3, Y0))
    b.assert_zero(si - y * total([oh[t] * pow(G16, brev(t, 4), P) for t in range(16)]))
    b.assert_zero(s1 - si * si)
    b.assert_zero(s2 - s1 * s1)
    b.assert_zero(s3 - s2 * s2)
    b.assert_zero(fold * (nxt(Y) - s3 * s3))
    b.assert_zero(first * (y - y0))
    b.assert_zero(cont * (nxt(Y0) - y0))
    # 6. 1 / x_0 is bound to the index: square and multiply over the bits
    acc = [loc(A + i) for i in range(5)]
    wm1 = b.pub(PUB_WINV) - 1
    b.assert_zero(first * (acc[0] - 1))
    for i in range(4):
        b.assert_zero(acc[i + 1] - acc[i] * acc[i] * (bits[i] * wm1 + 1))
    b.assert_zero(cont * (nxt(A) - acc[1] - fold * (acc[4] - acc[1])))
    b.assert_zero(last * (y0 - acc[1] * INV7))
    # 7. beta_l and its squares
    be = [x2(BE + 2 * j) for j in range(4)]
    b.assert_zero_x2(be[0] - X2(total([sel[i] * b.pub(PUB_BETA + 2 * i) for i in range(MAX_LAYERS)]), total([sel[i] * b.pub(PUB_BETA + 2 * i + 1) for i in range(MAX_LAYERS)])))
    for j in range(3):
        b.assert_zero_x2(be[j + 1] - be[j] * be[j])
    # 8. the value entering the layer is the leaf's slot `within`; the value leaving it enters the next row
    ev = x2(EV)
    pick = X2(total([oh[t] * loc(LEAF + 2 * t) for t in range(16)]), total([oh[t] * loc(LEAF + 2 * t + 1) for t in range(16)]))
    b.assert_zero_x2(pick - ev * fold)
    b.assert_zero_x2((x2(EV, nxt) - x2(V4)) * fold)
    # 9. the fold: four arity-2 levels
    s = [si, s1, s2, s3]
    for j in range(4):
        for k in range(8 >> j):
            u, w = x2(VLEV[j] + 4 * k), x2(VLEV[j] + 4 * k + 2)
            b.assert_zero_x2(x2(VLEV[j + 1] + 2 * k) - (u + w) * HALF - be[j] * (u - w) * (s[j] * fold_const(j, k)))
    # 10. the bus
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    tree = b.pub(PUB_TREE0) + cnt
    hsum = X2(0, 0)
    for e in range(16):
        da, db = (beta + q + gamma * (2 * e + c) + g2 * loc(LEAF + 2 * e + c) + g3 * tree + g4 * TAG_ROW for c in (0, 1))
        h = X2(b.aux(2 * e), b.aux(2 * e + 1))
        b.assert_zero_x2(h * da * db + (da + db) * fold)
        hsum = hsum + h
    base = beta + idx + gamma * loc(EV) + g2 * loc(EV + 1) + g4 * TAG_FRI
    de, dx = base, base + g3
    h = X2(b.aux(32), b.aux(33))
    b.assert_zero_x2(h * de * dx - de * loc(FBIT) + dx * first)
    hsum = hsum + h
    z, zn = X2(b.aux(34), b.aux(35)), X2(b.aux_nxt(34), b.aux_nxt(35))
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


# ---- the fold
def ext(v):
    return S.ExtS(int(v[0]), int(v[1]))


def x_inv_of(index, LN):
    """1 / x_0 for a query index of an LDE of 2^LN points: x_0 = 7 w^bitrev(index)"""
    return INV7 * pow(O.root(LN), P - 1 - brev(index, LN), P) % P


def fold_leaf(leaf, within, beta, x_inv):
    """leaf: 16 ExtS in leaf order, x_inv = 1 / x (x the point of slot `within`) -> (the interpolant of the coset at beta, the cells
    of the four levels)"""
    s, be, vals, cells = x_inv * pow(G16, brev(within, 4), P) % P, beta, list(leaf), []
    for j in range(4):
        vals = [(vals[2 * k] + vals[2 * k + 1]) * HALF + be * (vals[2 * k] - vals[2 * k + 1]) * (s * fold_const(j, k) % P) for k in range(8 >> j)]
        cells.append(vals)
        s, be = s * s % P, be * be
    return vals[0], cells


def fold_query(index, leaves, betas, LN):
    """leaves [NL][16][2] -> ev_NL, every leaf's slot `within` taken as the value entering its layer"""
    xi, ev = x_inv_of(index, LN), None
    for l in range(len(leaves)):
        ev, _ = fold_leaf([ext(v) for v in leaves[l]], (index >> (4 * l)) & 15, ext(betas[l]), xi)
        xi = pow(xi, 16, P)
    return ev


def chain_leaves(index, leaves, betas, LN):
    """random leaves made a chain: slot `within` of leaf l + 1 becomes the fold of leaf l (a copy is returned)"""
    leaves = np.array(leaves, dtype=np.uint64).reshape(len(betas), 16, 2)
    xi = x_inv_of(index, LN)
    for l in range(len(betas) - 1):
        ev, _ = fold_leaf([ext(v) for v in leaves[l]], (index >> (4 * l)) & 15, ext(betas[l]), xi)
        leaves[l + 1, (index >> (4 * (l + 1))) & 15] = [ev.a, ev.b]
        xi = pow(xi, 16, P)
    return leaves


# ---- witness
def log_rows(n_queries, LN, NL):
    return max(5, (n_queries * (LN - 3 * NL) - 1).bit_length())


def query_rows(index, leaves, betas, LN, tree0=0, r_start=None, y_index=None, n_rows=None):
    """the NL + FB rows of one query as columns [COLS][rows].  Forgeries: r_start -- the R / IDX chain starts from another value
    and is continued by field division; y_index -- 1 / x_0 and the points come from another index; n_rows -- the query ends early"""
    NL = len(betas)
    rows = LN - 3 * NL if n_rows is None else n_rows
    t = np.zeros((COLS, rows), dtype=np.uint64)
    winv = pow(O.root(LN), P - 2, P)
    y0 = x_inv_of(index if y_index is None else y_index, LN)
    rr, yy, acc, ev = (index if r_start is None else r_start) % P, y0, 1, None
    claimed, inv16 = rr, pow(16, P - 2, P)
    for k in range(rows):
        is_fold = k < NL
        nb = 4 if is_fold else 1
        pos = 4 * k if is_fold else 4 * NL + (k - NL)
        bits = [(index >> (pos + i)) & 1 for i in range(nb)] + [0] * (4 - nb)
        within = sum(bits[i] << i for i in range(4))
        qq = (rr - within) * (inv16 if is_fold else HALF) % P
        t[ACT, k], t[FOLD, k], t[FIRST, k], t[LAST, k], t[FBIT, k] = 1, is_fold, k == 0, k == rows - 1, k == NL
        t[CNT, k], t[R, k], t[Q, k], t[IDX, k] = k, rr, qq, claimed
        for i in range(4):
            t[B + i, k] = bits[i]
        a = [acc]
        for i in range(4):
            a.append(a[-1] * a[-1] % P * (winv if bits[i] else 1) % P)
        for i in range(5):
            t[A + i, k] = a[i]
        acc = a[4] if is_fold else a[1]
        t[Y, k], t[Y0, k] = yy, y0
        if is_fold:
            leaf = [ext(v) for v in leaves[k]]
            if ev is None:
                ev = leaf[within]
            t[EV, k], t[EV + 1, k] = ev.a, ev.b
            t[OH + within, k], t[LSEL + k, k] = 1, 1
            s = yy * pow(G16, brev(within, 4), P) % P
            be = ext(betas[k])
            for j in range(4):
                t[SI + j, k] = s
                t[BE + 2 * j, k], t[BE + 2 * j + 1, k] = be.a, be.b
                s, be = s * s % P, be * be
            yy = s
            for i in range(16):
                t[LEAF + 2 * i, k], t[LEAF + 2 * i + 1, k] = leaf[i].a, leaf[i].b
            ev, cells = fold_leaf(leaf, within, ext(betas[k]), t[Y, k].item())
            for j in range(4):
                for i, v in enumerate(cells[j]):
                    t[VLEV[j + 1] + 2 * i, k], t[VLEV[j + 1] + 2 * i + 1, k] = v.a, v.b
        else:
            t[EV, k], t[EV + 1, k] = ev.a, ev.b
        rr = qq
    return t


def assemble(queries, log_n):
    """the rows of the queries (arrays of query_rows) followed by idle rows -> trace [COLS][2^log_n]"""
    n = 1 << log_n
    tr = np.zeros((COLS, n), dtype=np.uint64)
    at = 0
    for qr in queries:
        assert at + qr.shape[1] <= n
        tr[:, at: at + qr.shape[1]] = qr
        at += qr.shape[1]
    return tr


def claims_digest(index, ev0, leaves):
    """hash_n_to_hash_no_pad over (index, ev_0, leaf_0 .. leaf_{NL-1}) of every query in order"""
    words = []
    for i, e, lv in zip(index, ev0, leaves):
        words += [int(i), int(e[0]), int(e[1])] + [int(v) for v in np.asarray(lv, dtype=np.uint64).reshape(-1)]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def public_inputs(index, ev0, leaves, betas, LN, tree0=0):
    NL = len(betas)
    pub = [NL, LN - 3 * NL, pow(O.root(LN), P - 2, P), tree0]
    for l in range(MAX_LAYERS):
        pub += [int(betas[l][0]), int(betas[l][1])] if l < NL else [0, 0]
    return pub + claims_digest(index, ev0, leaves)


def ev0_of(index, leaves):
    return [[int(v) for v in np.asarray(lv, dtype=np.uint64).reshape(-1, 16, 2)[0, i & 15]] for i, lv in zip(index, leaves)]


def ref_trace(index, leaves, betas, LN, log_n=None, tree0=0):
    """index: query indices; leaves [n_queries][NL][16][2] -> (trace [COLS][2^log_n], the 24 public inputs)"""
    NL = len(betas)
    log_n = log_rows(len(index), LN, NL) if log_n is None else log_n
    leaves = np.asarray(leaves, dtype=np.uint64).reshape(len(index), NL, 16, 2)
    tr = assemble([query_rows(int(i), lv, betas, LN, tree0) for i, lv in zip(index, leaves)], log_n)
    return tr, public_inputs(index, ev0_of(index, leaves), leaves, betas, LN, tree0)


def _bus(chal):
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g2 = gamma * gamma
    return beta, gamma, g2, g2 * gamma, g2 * g2


def d_row(bus, tree, index, position, word):
    beta, gamma, g2, g3, g4 = bus
    return beta + int(index) + gamma * int(position) + g2 * int(word) + g3 * int(tree) + g4 * TAG_ROW


def d_fri(bus, index, va, vb, end):
    beta, gamma, g2, g3, g4 = bus
    return beta + int(index) + gamma * int(va) + g2 * int(vb) + g3 * int(end) + g4 * TAG_FRI


def gen_aux(trace, chal, pub=None):
    """-> (aux [36][n]: 17 helpers, Z; [S / n]).  pub: the public inputs (TREE0 is read)"""
    n = trace.shape[1]
    tree0 = 0 if pub is None else int(pub[PUB_TREE0])
    bus = _bus(chal)
    aux = np.zeros((AUX, n), dtype=np.uint64)
    incs = []
    for i in range(n):
        cell = lambda j: int(trace[j, i])  # noqa: E731
        tot = S.ExtS(0)
        if cell(ACT):
            hs = []
            for e in range(16):
                h = S.ExtS(0)
                if cell(FOLD):
                    d = [d_row(bus, tree0 + cell(CNT), cell(Q), 2 * e + c, cell(LEAF + 2 * e + c)) for c in (0, 1)]
                    h = (d[0].inv() + d[1].inv()) * (P - 1)
                hs.append(h)
            h = S.ExtS(0)
            if cell(FIRST):
                h = h - d_fri(bus, cell(IDX), cell(EV), cell(EV + 1), 0).inv()
            if cell(FBIT):
                h = h + d_fri(bus, cell(IDX), cell(EV), cell(EV + 1), 1).inv()
            hs.append(h)
            for e, h in enumerate(hs):
                aux[2 * e, i], aux[2 * e + 1, i] = h.a, h.b
                tot = tot + h
        incs.append(tot)
    tot = S.ExtS(0)
    for h in incs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[34, i], aux[35, i] = z.a, z.b
        z = z + incs[i] - apub
    return aux, [apub.a, apub.b]


# ---- one table on its own bus
def chal_hook(pub, cap):
    return S.shared_challenges_n([(pub, cap)], 4)


def prove(trace, pub, cfg=None):
    """the reference prover on the program restatement -> table proof (id word REF_ID)"""
    return S.prove(air(), trace, pub, cfg, chal_hook=chal_hook)


def wrap(proof, log_lde, n_layers, n_queries, air_id=AIR_ID):
    """a table proof as a blob of the product, with the compiled AIR's id in its id word"""
    p = np.array(proof, dtype=np.uint64)
    p[1] = air_id
    return np.concatenate([np.array([MAGIC, log_lde, n_layers, n_queries, p.size], dtype=np.uint64), p])


def unwrap(blob, air_id=REF_ID):
    """the table proof inside a blob, with the reference registry's id in its id word"""
    p = np.array(blob[HDR:], dtype=np.uint64)
    assert int(blob[0]) == MAGIC and int(blob[4]) == p.size
    p[1] = air_id
    return p


def final_eval(final_poly, index, LN, NL):
    """final_poly(x_NL), x_NL = x_0^(16^NL) from the index by one exponentiation"""
    x = 7 * pow(O.root(LN), brev(index, LN), P) % P
    x = pow(x, 16 ** NL, P)
    acc = S.ExtS(0)
    for c in reversed(np.asarray(final_poly, dtype=np.uint64).reshape(-1, 2)):
        acc = acc * x + ext(c)
    return acc


def bus_check(proof, cap_h, index, ev0, leaves, final_poly, LN, NL, tree0=0):
    """the verifier's side of the bus in Python: published total x rows == sum over the claims of - 1 / D_row over every leaf word,
    - 1 / D_fri(index, ev_0, 0), + 1 / D_fri(index, final_poly(x_NL), 1)"""
    pub, cap = S.proof_peek(proof, cap_h)
    chal = chal_hook(pub, cap)
    bus = _bus(chal)
    pos = 10 + int(proof[9]) + 2 + len(pub) + (4 << cap_h)
    apub = S.ExtS(int(proof[pos]), int(proof[pos + 1]))
    tot = S.ExtS(0)
    for i, e, lv in zip(index, ev0, np.asarray(leaves, dtype=np.uint64).reshape(len(index), NL, 32)):
        for l in range(NL):
            for j in range(32):
                tot = tot - d_row(bus, tree0 + l, int(i) >> (4 * (l + 1)), j, lv[l, j]).inv()
        fe = final_eval(final_poly, int(i), LN, NL)
        tot = tot - d_fri(bus, i, e[0], e[1], 0).inv() + d_fri(bus, i, fe.a, fe.b, 1).inv()
    return apub * (1 << int(proof[2])) == tot, chal


# ---- a commit phase to cut claims from
def commit_phase(LN, NL, seed=1, rate_bits=1):
    """FRI's commit phase (arity 16) on a random polynomial of degree < 2^(LN - rate_bits) over the coset 7 <w_2^LN> ->
    (betas [NL][2], final_poly [2^(LN - 4 NL - rate_bits)][2], layers: the leaves [2^(LN - 4 (l + 1))][16][2] of layer l)"""
    rng = np.random.default_rng(seed)
    n = 1 << (LN - rate_bits)
    coeffs = np.zeros(2 << LN, dtype=np.uint64)
    coeffs[: 2 * n] = rng.integers(0, P, size=2 * n, dtype=np.uint64)
    shift, cur, layers, betas = S.G, LN, [], []
    values = O.ext_coset_ntt(coeffs, shift)
    for l in range(NL):
        layers.append(values.reshape(-1, 2)[S.bitrev_perm(cur)].reshape(-1, 16, 2))
        beta = [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)]
        betas.append(beta)
        coeffs = O.fri_fold_coeffs(coeffs, 4, np.array(beta, dtype=np.uint64))
        shift, cur = pow(shift, 16, P), cur - 4
        if l + 1 < NL:
            values = O.ext_coset_ntt(coeffs, shift)
    final_len = (1 << cur) >> rate_bits
    assert (coeffs[2 * final_len:] == 0).all()
    return betas, np.array(coeffs[: 2 * final_len], dtype=np.uint64).reshape(-1, 2), layers


def claims_from(layers, index):
    """-> (ev_0 [n][2], leaves [n][NL][16][2]) of the queries `index`"""
    leaves = np.array([[layers[l][int(i) >> (4 * (l + 1))] for l in range(len(layers))] for i in index], dtype=np.uint64)
    return np.array(ev0_of(index, leaves), dtype=np.uint64), leaves
