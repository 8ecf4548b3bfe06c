"""TEST INFRASTRUCTURE for FriCombineAir (csrc/air_fri_combine.cuh, AIR id 21): the AIR restated INDEPENDENTLY as a constraint program
(air_program.AirBuilder / X2, the same constraint order as the compiled eval, so oracle.air_program.ProgramAir runs it through
oracle/stark_ref.py unchanged), a reference trace generator and gen_aux in plain Python, the digests, the one-table reference prover,
the blob wrappers, the verifier's side of the bus, the claims of a reference-prover proof, and the two-table (combine + fold) prover
with the group's sum.  No tests here."""
import numpy as np

import fri_fold_ref as F
import leaf_sponge_ref as R
import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = F.P
AIR_ID = 21        # the compiled AIR
REF_ID = 1021      # the program restatement in the reference prover's registry (never registered with the product)
ACT, TM, TA, TQ, FIRST, LAST, FBIT, CNT, POS, W, IDX, RR, Q, B, A, A1 = range(16)
AP, SS, S1, D0, D1, EV, COLS = 16, 18, 20, 22, 24, 26, 28
AUX = 4
PUB_ROWS, PUB_CM, PUB_CA, PUB_NQ, PUB_TREE0, PUB_W, PUB_ALPHA, PUB_ALPHAC, PUB_ZETA, PUB_ZETAN, PUB_Y0, PUB_Y1, PUB_DIGEST, PUB = 0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 22
TREE0 = 8
MAGIC, HDR = int.from_bytes(b"VXFCOMB1", "little"), 7
GMAGIC, GHDR = int.from_bytes(b"VXFCFLD1", "little"), 9
CHAL = F.CHAL
brev, degree, ext = F.brev, F.degree, F.ext


def builder():
    ap_ = vx_import.load().air_program
    X2 = ap_.X2
    b = ap_.AirBuilder(COLS, PUB, aux_cols=AUX, n_challenges=4, n_aux_public=1)
    loc, nxt, pub = b.loc, b.nxt, b.pub

    def x2(col, row=loc):
        return X2(row(col), row(col + 1))

    def p2(i):
        return X2(pub(i), pub(i + 1))

    act, tm, ta, tq, first, last, fbit, cnt, pos, w = (loc(j) for j in (ACT, TM, TA, TQ, FIRST, LAST, FBIT, CNT, POS, W))
    idx, r, q, bb, a, a1 = (loc(j) for j in (IDX, RR, Q, B, A, A1))
    abs_, nabs = tm + ta + tq, nxt(TM) + nxt(TA) + nxt(TQ)
    bit, cont = act - abs_, act - last
    # 1. boolean cells; at most one tree
    for v in (act, tm, ta, tq, abs_, last, bb):
        b.assert_zero(v * (v - 1))
    # 2. the shape of a query
    b.assert_zero(abs_ * (1 - act))
    b.assert_zero(last * (1 - act))
    b.assert_zero(last * abs_)
    b.assert_zero(first * (1 - tm))
    b.assert_zero(nxt(FIRST) - nxt(ACT) * (1 - cont))
    b.assert_zero(nxt(FBIT) - abs_ * (1 - nabs))
    b.assert_zero(cont * (1 - nxt(ACT)))
    b.assert_zero(tm * (1 - nabs))
    b.assert_zero(ta * (1 - nxt(TA) - nxt(TQ)))
    b.assert_zero(nxt(TM) * (1 - nxt(FIRST)) * (1 - tm))
    b.assert_zero(nxt(TA) * (1 - tm - ta))
    b.assert_zero(nxt(TQ) * (1 - abs_))
    b.assert_zero(bit * cont * nabs)
    b.assert_zero(tm * nxt(TQ) * pub(PUB_CA))
    # 3. a tree ends only at its public length; POS starts at 0 in each tree and counts up
    b.assert_zero(tm * (1 - nxt(TM)) * (pos + 1 - pub(PUB_CM)))
    b.assert_zero(ta * (1 - nxt(TA)) * (pos + 1 - pub(PUB_CA)))
    b.assert_zero(tq * (1 - nxt(TQ)) * (pos + 1 - pub(PUB_NQ)))
    same = tm * nxt(TM) + ta * nxt(TA) + tq * nxt(TQ)
    b.assert_zero(same * (nxt(POS) - pos - 1))
    b.assert_zero((nabs - same) * nxt(POS))
    # 4. the row counter
    b.assert_zero(first * cnt)
    b.assert_zero(cont * (nxt(CNT) - cnt - 1))
    b.assert_zero(last * (cnt + 1 - pub(PUB_ROWS)))
    # 5. the word, the power of alpha, the sums
    ap, s, s1 = x2(AP), x2(SS), x2(S1)
    nap = x2(AP, nxt)
    b.assert_zero(bit * w)
    b.assert_zero_x2(X2(ap.a - 1, ap.b) * first)
    b.assert_zero_x2((nap - ap * p2(PUB_ALPHA)) * (abs_ * nabs))
    b.assert_zero_x2(X2(s.a - w, s.b) * first)
    b.assert_zero_x2((x2(SS, nxt) - s - nap * nxt(W)) * cont)
    b.assert_zero_x2((x2(S1, nxt) - s1) * cont)
    b.assert_zero_x2((s - s1) * ((tm + ta) * nxt(TQ)))
    # 6. the index bits
    b.assert_zero(r - q - q - bb)
    b.assert_zero(bit * cont * (nxt(RR) - q))
    b.assert_zero(last * q)
    b.assert_zero(fbit * (r - idx))
    b.assert_zero(cont * (nxt(IDX) - idx))
    # 7. x_0 is bound to the index
    b.assert_zero(fbit * (a - 1))
    b.assert_zero(a1 - a * a * (bb * (pub(PUB_W) - 1) + 1))
    b.assert_zero(bit * cont * (nxt(A) - a1))
    # 8. the last row
    ev, d0, d1 = x2(EV), x2(D0), x2(D1)
    x = a1 * 7
    zeta, zetan = p2(PUB_ZETA), p2(PUB_ZETAN)
    t0, t1 = d0 * X2(x - zeta.a, 0 - zeta.b), d1 * X2(x - zetan.a, 0 - zetan.b)
    b.assert_zero_x2(X2(t0.a - 1, t0.b) * last)
    b.assert_zero_x2(X2(t1.a - 1, t1.b) * last)
    b.assert_zero_x2((ev - p2(PUB_ALPHAC) * (s - p2(PUB_Y0)) * d0 - (s1 - p2(PUB_Y1)) * d1) * last)
    # 9. the bus
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    tree = pub(PUB_TREE0) + ta + tq + tq
    dr = beta + idx + gamma * pos + g2 * w + g3 * tree + g4 * F.TAG_ROW
    df = beta + idx + gamma * loc(EV) + g2 * loc(EV + 1) + g4 * F.TAG_FRI
    h = X2(b.aux(0), b.aux(1))
    b.assert_zero_x2(h * dr * df + df * abs_ - dr * last)
    z, zn = X2(b.aux(2), b.aux(3)), X2(b.aux_nxt(2), b.aux_nxt(3))
    b.assert_zero_x2(zn - z - h + X2(b.apub(0), b.apub(1)))
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


# ---- the statement: st = dict(LN, r, cm, ca, nq, alpha [2], zeta [2], ol [c][2], on [c][2], oq [nq][2])
def rand_statement(LN, cm, ca, nq, seed=3, r=1):
    rng = np.random.default_rng(seed)
    g = lambda *shape: rng.integers(0, P, size=shape, dtype=np.uint64)  # noqa: E731
    return dict(LN=LN, r=r, cm=cm, ca=ca, nq=nq, alpha=g(2), zeta=g(2), ol=g(cm + ca, 2), on=g(cm + ca, 2), oq=g(nq, 2))


def reduced(st):
    """-> (alpha^c, zeta w_n, y0, y1): what prover and verifier compute once per proof"""
    alpha, c = ext(st["alpha"]), st["cm"] + st["ca"]
    ap, y0, y1 = S.ExtS(1), S.ExtS(0), S.ExtS(0)
    for j in range(c):
        y0, y1, ap = y0 + ap * ext(st["ol"][j]), y1 + ap * ext(st["on"][j]), ap * alpha
    alphac = ap
    for j in range(st["nq"]):
        y0, ap = y0 + ap * ext(st["oq"][j]), ap * alpha
    return alphac, ext(st["zeta"]) * O.root(st["LN"] - st["r"]), y0, y1


def x_of(index, LN):
    return 7 * pow(O.root(LN), brev(int(index), LN), P) % P


def combine(st, index, row):
    """ev_0 of one query: alpha^c (s0 - y0) / (x - zeta) + (s1 - y1) / (x - zeta')"""
    alphac, zetan, y0, y1 = reduced(st)
    alpha, c = ext(st["alpha"]), st["cm"] + st["ca"]
    s, ap, s1 = S.ExtS(0), S.ExtS(1), None
    for j, wd in enumerate(row):
        s, ap = s + ap * int(wd), ap * alpha
        if j + 1 == c:
            s1 = s
    x = S.ExtS(x_of(index, st["LN"]))
    return alphac * (s - y0) * (x - ext(st["zeta"])).inv() + (s1 - y1) * (x - zetan).inv()


def rand_claims(st, index, seed=7):
    """random rows and their ev_0 -> (rows [n][c + nq], ev0 [n][2])"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, P, size=(len(index), st["cm"] + st["ca"] + st["nq"]), dtype=np.uint64)
    return rows, ev0_of(st, index, rows)


def ev0_of(st, index, rows):
    return np.array([[e.a, e.b] for e in (combine(st, i, rw) for i, rw in zip(index, rows))], dtype=np.uint64)


def log_rows(n_queries, st):
    return max(5, (n_queries * (st["cm"] + st["ca"] + st["nq"] + st["LN"]) - 1).bit_length())


def query_rows(st, index, row, trees=None, pos=None, ap_stall=None, s1_row=None, flip_bit=None, a_start=1):
    """the c + nq + LN rows of one query as columns [COLS][rows].  Forgeries: trees / pos -- another tree or position per absorb row;
    ap_stall -- AP is not advanced into that row; s1_row -- S1 is the sum at another row; flip_bit -- that index bit is consumed
    flipped while R starts from the claimed index and is continued by field division; a_start -- the accumulator's first value"""
    LN, cm, ca, nq = st["LN"], st["cm"], st["ca"], st["nq"]
    c, index = cm + ca, int(index)
    absn = len(row)
    if trees is None:
        trees = [0] * cm + [1] * ca + [2] * nq
    if pos is None:
        pos = [0] * absn
        for j in range(1, absn):
            pos[j] = pos[j - 1] + 1 if trees[j] == trees[j - 1] else 0
    alphac, zetan, y0, y1 = reduced(st)
    alpha, w = ext(st["alpha"]), O.root(LN)
    n = absn + LN
    t = np.zeros((COLS, n), dtype=np.uint64)
    t[ACT], t[IDX], t[CNT] = 1, index, np.arange(n)
    t[FIRST, 0], t[LAST, n - 1], t[FBIT, absn] = 1, 1, 1
    ap, s, sums = S.ExtS(1), S.ExtS(0), []
    for j in range(absn):
        if j and j != ap_stall:
            ap = ap * alpha
        s = s + ap * int(row[j])
        sums.append(s)
        t[TM + trees[j], j], t[POS, j], t[W, j] = 1, pos[j], int(row[j])
        t[AP, j], t[AP + 1, j], t[SS, j], t[SS + 1, j] = ap.a, ap.b, s.a, s.b
    s1 = sums[c - 1 if s1_row is None else s1_row]
    t[S1], t[S1 + 1] = s1.a, s1.b
    t[SS, absn:], t[SS + 1, absn:] = s.a, s.b
    used = index if flip_bit is None else index ^ (1 << flip_bit)
    rr, acc, half = index, a_start, pow(2, P - 2, P)
    for j in range(LN):
        k, bit = absn + j, (used >> j) & 1
        qq = (rr - bit) * half % P
        nxt_acc = acc * acc % P * (w if bit else 1) % P
        t[RR, k], t[Q, k], t[B, k], t[A, k], t[A1, k] = rr, qq, bit, acc, nxt_acc
        rr, acc = qq, nxt_acc
    x = S.ExtS(7 * acc % P)
    d0, d1 = (x - ext(st["zeta"])).inv(), (x - zetan).inv()
    ev = alphac * (s - y0) * d0 + (s1 - y1) * d1
    for col, v in ((D0, d0), (D1, d1), (EV, ev)):
        t[col, n - 1], t[col + 1, n - 1] = v.a, v.b
    return t


def assemble(queries, log_n):
    n = 1 << log_n
    tr = np.zeros((COLS, n), dtype=np.uint64)
    at = 0
    for qr in queries:
        assert at + qr.shape[1] <= n
        tr[:, at: at + qr.shape[1]] = qr
        at += qr.shape[1]
    return tr


def statement_words(st, n_queries):
    w = [st["LN"], st["r"], st["cm"], st["ca"], st["nq"], n_queries] + [int(v) for v in st["alpha"]] + [int(v) for v in st["zeta"]]
    for k in ("ol", "on", "oq"):
        w += [int(v) for v in np.asarray(st[k], dtype=np.uint64).reshape(-1)]
    return w


def claims_digest(st, index, rows, ev0):
    w = statement_words(st, len(index))
    for i, rw, e in zip(index, rows, ev0):
        w += [int(i)] + [int(v) for v in rw] + [int(e[0]), int(e[1])]
    return [int(v) for v in O.hash_no_pad(np.array(w, dtype=np.uint64))]


def public_head(st, tree0):
    alphac, zetan, y0, y1 = reduced(st)
    pub = [st["cm"] + st["ca"] + st["nq"] + st["LN"], st["cm"], st["ca"], st["nq"], tree0, O.root(st["LN"])] + [int(v) for v in st["alpha"]] + [alphac.a, alphac.b]
    return pub + [int(v) for v in st["zeta"]] + [zetan.a, zetan.b, y0.a, y0.b, y1.a, y1.b]


def public_inputs(st, index, rows, ev0, tree0=TREE0):
    return public_head(st, tree0) + claims_digest(st, index, rows, ev0)


def ref_trace(st, index, rows, log_n=None, tree0=TREE0):
    """-> (trace [COLS][2^log_n], the 22 public inputs); ev_0 is what the rows combine to"""
    log_n = log_rows(len(index), st) if log_n is None else log_n
    tr = assemble([query_rows(st, i, rw) for i, rw in zip(index, rows)], log_n)
    return tr, public_inputs(st, index, rows, ev0_of(st, index, rows), tree0)


def gen_aux(trace, chal, pub=None):
    """-> (aux [4][n]: the helper, Z; [S / n]).  pub: the public inputs (TREE0 is read)"""
    n = trace.shape[1]
    tree0 = TREE0 if pub is None else int(pub[PUB_TREE0])
    bus = F._bus(chal)
    aux = np.zeros((AUX, n), dtype=np.uint64)
    incs = []
    for i in range(n):
        cell = lambda j: int(trace[j, i])  # noqa: E731
        h = S.ExtS(0)
        if cell(TM) or cell(TA) or cell(TQ):
            h = h - F.d_row(bus, tree0 + cell(TA) + 2 * cell(TQ), cell(IDX), cell(POS), cell(W)).inv()
        if cell(LAST):
            h = h + F.d_fri(bus, cell(IDX), cell(EV), cell(EV + 1), 0).inv()
        aux[0, i], aux[1, i] = h.a, h.b
        incs.append(h)
    tot = S.ExtS(0)
    for h in incs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[2, i], aux[3, i] = z.a, z.b
        z = z + incs[i] - apub
    return aux, [apub.a, apub.b]


# ---- one table on its own bus
def chal_hook(pub, cap):
    return S.shared_challenges_n([(pub, cap)], 4)


def prove(trace, pub, cfg=None):
    return S.prove(air(), trace, pub, cfg, chal_hook=chal_hook)


def wrap(proof, st, n_queries, air_id=AIR_ID):
    p = np.array(proof, dtype=np.uint64)
    p[1] = air_id
    return np.concatenate([np.array([MAGIC, st["LN"], st["cm"], st["ca"], st["nq"], n_queries, p.size], dtype=np.uint64), p])


def unwrap(blob, air_id=REF_ID):
    p = np.array(blob[HDR:], dtype=np.uint64)
    assert int(blob[0]) == MAGIC and int(blob[HDR - 1]) == p.size
    p[1] = air_id
    return p


def published(proof, cap_h, n_pub):
    pos = 10 + int(proof[9]) + 2 + n_pub + (4 << cap_h)
    return S.ExtS(int(proof[pos]), int(proof[pos + 1])) * (1 << int(proof[2]))


def row_terms(bus, st, index, row, tree0=TREE0):
    """sum over the row words of 1 / D_row(tree0 + t, index, position, word)"""
    cm, c = st["cm"], st["cm"] + st["ca"]
    tot = S.ExtS(0)
    for j, wd in enumerate(row):
        t, pos = (0, j) if j < cm else (1, j - cm) if j < c else (2, j - c)
        tot = tot + F.d_row(bus, tree0 + t, index, pos, wd).inv()
    return tot


def bus_check(proof, cap_h, st, index, rows, ev0, tree0=TREE0):
    """the verifier's side of the bus: published total x rows == sum over the claims of - 1 / D_row over every row word
    + 1 / D_fri(index, ev_0, 0)"""
    pub, cap = S.proof_peek(proof, cap_h)
    chal = chal_hook(pub, cap)
    bus = F._bus(chal)
    tot = S.ExtS(0)
    for i, rw, e in zip(index, rows, ev0):
        tot = tot - row_terms(bus, st, int(i), rw, tree0) + F.d_fri(bus, i, e[0], e[1], 0).inv()
    return published(proof, cap_h, len(pub)) == tot, chal


# ---- the claims of a reference-prover proof (the transcript replayed; nothing is verified here)
def claims_of(proof, cfg=None):
    """-> (st, index, rows, first: per query (the 15 other values of the first FRI leaf, its siblings), the first layer's cap)"""
    cfg = dict(S.DEFAULT_CFG, **(cfg or {}))
    pr = [int(x) for x in np.asarray(proof, dtype=np.uint64)]
    _, air_id, L, cm, nq, r, cap_h, n_queries, _, n_layers = pr[:10]
    a = S.AIRS[air_id]
    ca, pos = getattr(a, "AUX", 0), 10
    arities = pr[pos: pos + n_layers]
    final_len, n_pub = pr[pos + n_layers: pos + n_layers + 2]
    pos += n_layers + 2

    def take(k):
        nonlocal pos
        pos += k
        return pr[pos - k: pos]

    pub, cw, c, LN = take(n_pub), 4 << cap_h, cm + ca, L + r
    ch = O.Challenger()
    if pub:
        ch.observe(np.array(pub, dtype=np.uint64))
    ch.observe(np.array(take(cw), dtype=np.uint64))
    if ca:
        for _ in range(a.CHAL):
            ch.challenge()
        ch.observe(np.array(take(2 * a.AUXPUB), dtype=np.uint64))
        ch.observe(np.array(take(cw), dtype=np.uint64))
    ch.challenge(), ch.challenge()
    ch.observe(np.array(take(cw), dtype=np.uint64))
    zeta = [ch.challenge(), ch.challenge()]
    ol, on, oq = (np.array(take(2 * k), dtype=np.uint64).reshape(-1, 2) for k in (c, c, nq))
    for o in (ol, oq, on):
        ch.observe(o.reshape(-1))
    alpha = [ch.challenge(), ch.challenge()]
    caps = []
    for _ in arities:
        caps.append(np.array(take(cw), dtype=np.uint64).reshape(-1, 4))
        ch.observe(caps[-1].reshape(-1))
        ch.challenge(), ch.challenge()
    ch.observe(np.array(take(2 * final_len), dtype=np.uint64))
    ch.observe(np.array(take(1), dtype=np.uint64))
    ch.challenge()
    st = dict(LN=LN, r=r, cm=cm, ca=ca, nq=nq, alpha=np.array(alpha, dtype=np.uint64), zeta=np.array(zeta, dtype=np.uint64), ol=ol, on=on, oq=oq)
    index, rows, first, depth0 = [], [], [], LN - cap_h
    for _ in range(n_queries):
        index.append(ch.challenge() % (1 << LN))
        row = take(cm)
        take(4 * depth0)
        if ca:
            row += take(ca)
            take(4 * depth0)
        row += take(nq)
        take(4 * depth0)
        rows.append(row)
        cur = LN
        for l, ab in enumerate(arities):
            others = take(2 * ((1 << ab) - 1))
            sib = take(4 * (cur - ab - cap_h))
            if l == 0:
                first.append((others, np.array(sib, dtype=np.uint64).reshape(-1, 4)))
            cur -= ab
    assert pos == len(pr)
    return st, index, np.array(rows, dtype=np.uint64), first, caps[0]


# ---- FriCombineAir + FriFoldAir on one bus (combine first): TAG_FRI end 0 closes between the tables
def group_statement(st, betas, fpoly, index, rows, leaves):
    w = statement_words(st, len(index)) + [len(betas)] + [int(v) for b in betas for v in b] + [int(v) for v in np.asarray(fpoly, dtype=np.uint64).reshape(-1)]
    for i, rw, lv in zip(index, rows, leaves):
        w += [int(i)] + [int(v) for v in rw] + [int(v) for v in np.asarray(lv, dtype=np.uint64).reshape(-1)]
    return [int(v) for v in O.hash_no_pad(np.array(w, dtype=np.uint64))]


def group_tables(st, betas, fpoly, index, rows, leaves):
    """-> [(combine trace, public inputs), (fold trace, public inputs)], both with the statement digest"""
    stmt = group_statement(st, betas, fpoly, index, rows, leaves)
    ctr, cpub = ref_trace(st, index, rows)
    ftr, fpub = F.ref_trace(index, leaves, betas, st["LN"])
    return [(ctr, cpub[:PUB_DIGEST] + stmt), (ftr, fpub[:F.PUB_DIGEST] + stmt)]


def group_prove(tabs, cfg=None):
    chal = S.shared_challenges_n([(pub, R.trace_cap(tr, cfg)) for tr, pub in tabs], 4)
    hook = lambda pub, cap: chal  # noqa: E731
    return [S.prove(a, tr, pub, cfg, chal_hook=hook) for a, (tr, pub) in zip((air(), F.air()), tabs)], chal


def group_wrap(proofs, st, NL, n_queries):
    ps = [np.array(p, dtype=np.uint64) for p in proofs]
    for p, i in zip(ps, (AIR_ID, F.AIR_ID)):
        p[1] = i
    return np.concatenate([np.array([GMAGIC, st["LN"], st["cm"], st["ca"], st["nq"], NL, n_queries, ps[0].size, ps[1].size], dtype=np.uint64)] + ps)


def group_unwrap(blob):
    assert int(blob[0]) == GMAGIC
    l0, l1 = int(blob[GHDR - 2]), int(blob[GHDR - 1])
    assert GHDR + l0 + l1 == blob.size
    ps = [np.array(blob[GHDR: GHDR + l0], dtype=np.uint64), np.array(blob[GHDR + l0:], dtype=np.uint64)]
    ps[0][1], ps[1][1] = REF_ID, F.REF_ID
    return ps


def group_sum(proofs, cap_h, chal, st, betas, fpoly, index, rows, leaves):
    """sum over the tables of total x rows == sum over the queries of - the row words - the leaf words + 1 / D_fri(index, final_poly(x_NL), 1)"""
    bus, NL, LN = F._bus(chal), len(betas), st["LN"]
    got = published(proofs[0], cap_h, PUB) + published(proofs[1], cap_h, F.PUB)
    tot = S.ExtS(0)
    for i, rw, lv in zip(index, rows, np.asarray(leaves, dtype=np.uint64).reshape(len(index), NL, 32)):
        tot = tot - row_terms(bus, st, int(i), rw)
        for l in range(NL):
            for j in range(32):
                tot = tot - F.d_row(bus, l, int(i) >> (4 * (l + 1)), j, lv[l, j]).inv()
        fe = F.final_eval(fpoly, int(i), LN, NL)
        tot = tot + F.d_fri(bus, i, fe.a, fe.b, 1).inv()
    return got == tot
