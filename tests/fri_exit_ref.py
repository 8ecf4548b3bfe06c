"""TEST INFRASTRUCTURE for FriExitAir (the shipped constraint program air_library.fri_exit_builder(), csrc/fri_exit_layout.h) and the
exit group of an inner proof [FriFoldAir, TranscriptAir, FriExitAir]: the AIR restated INDEPENDENTLY with its bus block written out by
hand (so oracle.air_program.ProgramAir runs it through oracle/stark_ref.py, and the constraints the library DERIVES from the declared
messages are compared with these), a reference trace that RUNS the recurrences row by row (the witness kernel uses closed forms),
gen_aux in plain Python, the public inputs, forge hooks, the group's statement digest, reference prover and the outside party's sum.
The fold and transcript tables are fri_fold_ref's and transcript_ref's.  No tests here."""
import numpy as np

import fri_fold_ref as F
import leaf_sponge_ref as R
import stark_inner_ref as I
import stark_queries_ref as Z
import transcript_ref as T
import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = F.P
REF_ID = 1024      # the restatement in the reference prover's registry (never registered with the product)
BLOCK, HROW, MAX_FINAL = 128, 63, 64
BIT, V, FL, C, EF, C2, G, EB, W, X, IDX, TT, HF, K, CA, CB, ACC, ACT, ISPOW, ORD, COLS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21
PER_FIRST, PER_LAST, PER_BIT, PER_WEIGHT, PER_HIGH, PER_HOLD, PER_LOW, PER_PRE, PER_R62, PERIODIC = range(10)
PUB_ORD_POW, PUB_ABSORBED, PUB_POW_BITS, PUB_SKIP, PUB_FB, PUB_W, PUB_G, PUB_FINAL_LEN, PUB_DIGEST, PUB = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12
N_HELP, AUX = 2, 6
TAG_FRI, TAG_CHAL, TAG_FIN = 10, 13, 14
CHAL = F.CHAL
degree = F.degree


# the hand-made statement and values both tiers build traces from, and the shapes of the groups: name -> (LN, NL, final_len)
HAND = dict(LN=9, NL=1, pow_bits=16, ord_pow=20, absorbed=300)
INDEX_VALUES = [0, 1, 2**32 - 1, 2**32, P - 1, 2**9 - 1, 2**9, 2**63]
EDGES = {"response_0": (16, 0), "response_max": (16, 2**48 - 1), "pow_bits_0_top_bit_set": (0, 2**63 + 12345)}  # name -> (pow_bits, the PoW response)
GROUP_SHAPES = {"fib8": (9, 1, 16), "fib8_two_layers_cap0": (9, 2, 1), "fib9_two_layers_cap1": (10, 2, 2), "fib8_rate2": (10, 1, 16), "fib8_40_queries": (9, 1, 16), "fib8_pow0": (9, 1, 16)}


def final_poly(n, seed=3):
    return np.random.default_rng(seed).integers(0, P, size=(n, 2), dtype=np.uint64)


def periodic():
    rows = range(BLOCK)
    cols = [[0] * BLOCK for _ in range(PERIODIC)]
    for r in rows:
        cols[PER_FIRST][r], cols[PER_LAST][r] = int(r == 0), int(r == BLOCK - 1)
        cols[PER_BIT][r], cols[PER_WEIGHT][r] = int(r < 64), (2 ** (63 - r) if r < 64 else 0)
        cols[PER_HIGH][r], cols[PER_HOLD][r], cols[PER_LOW][r] = int(0 < r < 32), int(32 <= r <= 62), int(32 <= r <= 63)
        cols[PER_PRE][r], cols[PER_R62][r] = int(r < HROW), int(r == HROW - 1)
    return cols


def builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(COLS, PUB, periodic=periodic(), aux_cols=AUX, n_challenges=4, n_aux_public=1)
    loc, nxt, per, pub = b.loc, b.nxt, b.per, b.pub
    first, last = per(PER_FIRST), per(PER_LAST)
    act, ispow = loc(ACT), loc(ISPOW)
    index_block = act - ispow
    # booleans
    for cell in (loc(BIT), loc(FL), loc(EF), loc(FL) + loc(EF), loc(HF), act, ispow):
        b.assert_zero(cell * (cell - 1))
    b.assert_zero(ispow * (1 - act))
    b.assert_zero((1 - per(PER_BIT)) * loc(BIT))
    # blocks
    b.assert_zero((1 - last) * (nxt(ACT) - act))
    b.assert_zero((1 - last) * (nxt(ISPOW) - ispow))
    b.assert_transition(nxt(ORD) - loc(ORD) - last)
    b.assert_first(loc(ORD) - pub(PUB_ORD_POW))
    b.assert_first(ispow - act)
    b.assert_transition(last * nxt(ISPOW))
    # the value and its canonical form
    b.assert_zero(nxt(V) - (1 - last) * loc(V) - loc(BIT) * per(PER_WEIGHT))
    b.assert_zero(nxt(TT) - first * loc(BIT) - loc(TT) * (per(PER_HIGH) * loc(BIT) + per(PER_HOLD)))
    b.assert_zero(per(PER_LOW) * loc(TT) * loc(BIT))
    # the two prefix flags with their counters
    for flag, flag_n, count, length in ((loc(FL), nxt(FL), C, ispow * pub(PUB_POW_BITS) + index_block * pub(PUB_SKIP)), (loc(FL) + loc(EF), nxt(FL) + nxt(EF), C2, index_block * pub(PUB_FB))):
        own = loc(FL) if count == C else loc(EF)
        b.assert_zero(last * own)
        b.assert_zero(flag_n * (1 - flag - last))
        b.assert_zero(first * (loc(count) - length))
        b.assert_zero((1 - last) * (nxt(count) - loc(count) + own))
        b.assert_zero(last * loc(count))
    # flag x bit
    b.assert_zero(loc(G) - loc(BIT) + loc(FL) * loc(BIT))
    b.assert_zero(loc(EB) - loc(EF) * loc(BIT))
    b.assert_zero(ispow * (loc(BIT) - loc(G)))
    # index and point
    b.assert_zero(nxt(IDX) - (1 - last) * loc(IDX) - loc(G) * per(PER_WEIGHT))
    b.assert_zero(nxt(W) - loc(FL) * pub(PUB_W) - loc(EF) * loc(W) * loc(W))
    b.assert_zero(nxt(X) - loc(FL) * pub(PUB_G) - (1 - loc(FL) - last) * loc(X) - loc(X) * loc(EB) * (loc(W) - 1))
    # Horner
    b.assert_zero(per(PER_PRE) * loc(HF))
    b.assert_zero(last * loc(HF))
    b.assert_zero(nxt(HF) * (1 - loc(HF) - per(PER_R62)))
    b.assert_zero(first * (loc(K) - index_block * pub(PUB_FINAL_LEN)))
    b.assert_zero((1 - last) * (nxt(K) - loc(K) + loc(HF)))
    b.assert_zero(last * loc(K))
    for j in range(2):
        b.assert_zero(nxt(ACC + j) - (1 - last) * loc(ACC + j) - loc(HF) * (loc(ACC + j) * (loc(X) - 1) + loc(CA + j)))
    # the bus, by hand: helper 0 = chal and fin (both received), helper 1 = the exit (received)
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    d_chal = beta + gamma * loc(ORD) + g2 * pub(PUB_ABSORBED) + g3 * loc(V) + g4 * TAG_CHAL
    d_fin = beta + (loc(K) - 1) + gamma * loc(CA) + g2 * loc(CB) + g4 * TAG_FIN
    d_fri = beta + loc(IDX) + gamma * loc(ACC) + g2 * loc(ACC + 1) + g3 + g4 * TAG_FRI
    h0, h1 = X2(b.aux(0), b.aux(1)), X2(b.aux(2), b.aux(3))
    b.assert_zero_x2(h0 * d_chal * d_fin + d_fin * (last * act) + d_chal * loc(HF))
    b.assert_zero_x2(h1 * d_fri + (last * index_block))
    z, zn = X2(b.aux(4), b.aux(5)), X2(b.aux_nxt(4), b.aux_nxt(5))
    b.assert_zero_x2(zn - z - (h0 + h1) + X2(b.apub(0), b.apub(1)))
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


# ---- witness: the recurrences run row by row
def log_rows(n_queries):
    return max(8, (BLOCK * (1 + n_queries) - 1).bit_length())


def statement_of(LN, NL, pow_bits, ord_pow, absorbed, final_poly):
    """the eight public inputs before the digest"""
    fp = np.asarray(final_poly, dtype=np.uint64).reshape(-1, 2)
    return [int(ord_pow), int(absorbed), int(pow_bits), 64 - LN, LN - 4 * NL, pow(O.root(LN), 16 ** NL, P), pow(7, 16 ** NL, P), fp.shape[0]]


def public_inputs(LN, NL, pow_bits, ord_pow, absorbed, final_poly, digest=None):
    head = statement_of(LN, NL, pow_bits, ord_pow, absorbed, final_poly)
    if digest is None:
        digest = O.hash_no_pad(np.array(head + [int(w) for w in np.asarray(final_poly, dtype=np.uint64).reshape(-1)], dtype=np.uint64))
    return head + [int(w) for w in digest]


def run_block(v, ordinal, ispow, head, final_poly, bits=None, length=None, eb_flip=None, k_jump=None):
    """the 128 rows of one active block as columns [COLS][128], every column advanced by its own transition rule.  head: the eight
    statement words.  Forgeries: bits -- the 64 bit cells (MSB first) instead of v's; length -- the prefix flag's length instead
    of the public one; eb_flip -- the exponent step whose bit the point takes inverted; k_jump -- the Horner step at which K drops by 2"""
    _, _, pow_bits, skip, fb, w_fb, g7, final_len = head
    fp = [(int(a), int(b)) for a, b in np.asarray(final_poly, dtype=np.uint64).reshape(-1, 2)]
    bits = [(int(v) >> (63 - r)) & 1 for r in range(64)] if bits is None else list(bits)
    L = (pow_bits if ispow else skip) if length is None else length
    n_exp, k = (0, 0) if ispow else (fb, final_len)
    t = np.zeros((COLS, BLOCK), dtype=np.uint64)
    val = idx = tt = w = x = 0
    c, c2, acc = L, n_exp, (0, 0)
    for r in range(BLOCK):
        last = r == BLOCK - 1
        bit = bits[r] if r < 64 else 0
        f, ef = int(r < L), int(L <= r < L + n_exp)
        g, took = (0 if f else bit), (bit if ef else 0)
        if ef and eb_flip == r - L:
            took = 1 - took
        hf = int(HROW <= r < BLOCK - 1 and k > 0)
        co = fp[k - 1] if hf else (0, 0)
        for col, cell in ((BIT, bit), (V, val), (FL, f), (C, c), (EF, ef), (C2, c2), (G, g), (EB, took), (W, w), (X, x), (IDX, idx), (TT, tt), (HF, hf), (K, k), (CA, co[0]), (CB, co[1]),
                          (ACC, acc[0]), (ACC + 1, acc[1]), (ACT, 1), (ISPOW, int(ispow)), (ORD, ordinal)):
            t[col, r] = cell % P
        weight = 2 ** (63 - r) if r < 64 else 0
        val, idx = (val + bit * weight) % P, (idx + g * weight) % P
        tt = bit if r == 0 else tt * bit if r < 32 else tt if r <= 62 else 0
        w, x = (w_fb if f else w * w % P if ef else 0), (g7 if f else 0 if last else x * (w if took else 1) % P)
        c, c2 = c - f, c2 - ef
        if hf:
            acc = ((acc[0] * x + co[0]) % P, (acc[1] * x + co[1]) % P)
            k -= 2 if k_jump == r - HROW else 1
    return t


def ref_trace(values, LN, NL, pow_bits, ord_pow, absorbed, final_poly, log_n=None, digest=None, forge=None):
    """values: the PoW response, then one index challenge per query -> (trace [COLS][2^log_n], the 12 public inputs).
    forge: {block number: keyword arguments of block_rows, or ispow=...}"""
    forge = forge or {}
    head = statement_of(LN, NL, pow_bits, ord_pow, absorbed, final_poly)
    log_n = log_rows(len(values) - 1) if log_n is None else log_n
    n = 1 << log_n
    assert BLOCK * len(values) <= n, "the blocks do not fit"
    tr = np.zeros((COLS, n), dtype=np.uint64)
    for blk in range(n // BLOCK):
        sl = slice(BLOCK * blk, BLOCK * (blk + 1))
        if blk < len(values):
            kw = dict(forge.get(blk, {}))
            tr[:, sl] = run_block(values[blk], ord_pow + blk, kw.pop("ispow", blk == 0), head, final_poly, **kw)
        else:
            tr[ORD, sl] = ord_pow + blk
    return tr, public_inputs(LN, NL, pow_bits, ord_pow, absorbed, final_poly, digest)


def _bus(chal):
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g2 = gamma * gamma
    return beta, gamma, g2, g2 * gamma, g2 * g2


def d_fin(bus, k, ca, cb):
    beta, gamma, g2, _, g4 = bus
    return beta + int(k) + gamma * int(ca) + g2 * int(cb) + g4 * TAG_FIN


def gen_aux(trace, chal, pub=None):
    """-> (aux [6][n]: helper 0 = chal and fin, helper 1 = the exit, Z; [S / n]).  pub: the public inputs (ABSORBED is read)"""
    n = trace.shape[1]
    absorbed = int(pub[PUB_ABSORBED])
    bus = _bus(chal)
    aux = np.zeros((AUX, n), dtype=np.uint64)
    incs = []
    for i in range(n):
        cell = lambda j: int(trace[j, i])  # noqa: E731
        h0, h1 = S.ExtS(0), S.ExtS(0)
        if i % BLOCK == BLOCK - 1 and cell(ACT):
            h0 = h0 - T.d_chal(bus, 0, cell(ORD), absorbed, cell(V)).inv()
            if cell(ACT) != cell(ISPOW):
                h1 = h1 - F.d_fri(bus, cell(IDX), cell(ACC), cell(ACC + 1), 1).inv() * ((cell(ACT) - cell(ISPOW)) % P)
        if cell(HF):
            h0 = h0 - d_fin(bus, (cell(K) - 1) % P, cell(CA), cell(CB)).inv() * cell(HF)
        aux[0, i], aux[1, i], aux[2, i], aux[3, i] = h0.a, h0.b, h1.a, h1.b
        incs.append(h0 + h1)
    tot = S.ExtS(0)
    for h in incs:
        tot = tot + h
    apub = tot * pow(n, P - 2, P)
    z = S.ExtS(0)
    for i in range(n):
        aux[4, i], aux[5, i] = z.a, z.b
        z = z + incs[i] - apub
    return aux, [apub.a, apub.b]


def check(trace, pub, chal=CHAL):
    """None, or the first (constraint, row) the reference prover's own row check refuses"""
    aux, apub = gen_aux(trace, chal, pub)
    return S.check_trace(air(), trace, pub, chal, aux, apub)


def prove_alone(trace, pub, cfg=None):
    """the reference prover on the restatement as a stand-alone table: the lookup challenges are DRAWN, as vx_stark_verify draws them
    (id word REF_ID); it proves whatever it is handed"""
    return np.array(S.prove(air(), trace, pub, cfg), dtype=np.uint64)


# ---- the exit group of an inner proof: [FriFoldAir, TranscriptAir, FriExitAir] on one bus, the verifier outside
def statement_words(LN, pow_bits, ord_pow, words, chals, index, ev0, leaves):
    """everything the outside party states: LN, pow_bits, ORD_POW, n_obs, n_queries, NL; the observed words; (absorbed, value) of the
    challenges below ORD_POW; per query (index, ev_0, leaves)"""
    lv = np.asarray(leaves, dtype=np.uint64).reshape(len(index), -1)
    w = [LN, pow_bits, ord_pow, len(words), len(index), lv.shape[1] // 32] + [int(x) for x in words]
    for a, v in chals[:ord_pow]:
        w += [int(a), int(v)]
    for i, e, l in zip(index, ev0, lv):
        w += [int(i), int(e[0]), int(e[1])] + [int(x) for x in l]
    return w


def statement_digest(*args):
    return [int(v) for v in O.hash_no_pad(np.array(statement_words(*args), dtype=np.uint64))]


def outside_sum(chal, ord_pow, words, chals, final_poly, index, ev0, leaves, fin_mult=None):
    """what the verifier adds: the leaves and entries of the fold chains SENT (-), every observed word SENT (-), the challenges below
    ORD_POW RECEIVED (+), every final-polynomial coefficient SENT n_queries times (-).  No index is reduced, no point raised, no
    polynomial evaluated."""
    bus, tot = _bus(chal), S.ExtS(0)
    lv = np.asarray(leaves, dtype=np.uint64).reshape(len(index), -1, 32)
    for q, (i, e) in enumerate(zip(index, ev0)):
        for l in range(lv.shape[1]):
            for j in range(32):
                tot = tot - F.d_row(bus, l, int(i) >> (4 * (l + 1)), j, lv[q, l, j]).inv()
        tot = tot - F.d_fri(bus, i, e[0], e[1], 0).inv()
    tot = tot + T.outside_sum(chal, [(words, chals[:ord_pow])])
    for k, c in enumerate(np.asarray(final_poly, dtype=np.uint64).reshape(-1, 2)):
        tot = tot - d_fin(bus, k, c[0], c[1]).inv() * (len(index) if fin_mult is None else fin_mult)
    return tot


SHAPES = ["fib8", "fib8_two_layers_cap0", "fib9_two_layers_cap1", "fib8_rate2", "fib8_40_queries", "fib8_pow0", "lookup8"]
_inner, _claims, _groups = {}, {}, {}


def inner(name):
    """-> dict(proof: the reference prover's inner proof, cfg) -- stark_inner_ref's where it has the shape, fib8 at pow_bits = 0 here"""
    if name not in _inner:
        if name in I.INNER:
            g = I.inner(name)
            _inner[name] = dict(proof=g["proof"], cfg=g["cfg"])
        else:
            air_, trace, pub, cfg = Z.inner("fib8" if name == "fib8_pow0" else name)
            if name == "fib8_pow0":
                cfg = dict(cfg, pow_bits=0)
            _inner[name] = dict(proof=np.array(S.prove(air_, trace, pub, cfg), dtype=np.uint64), cfg=cfg)
    return _inner[name]


def claims_of(name):
    """the claims of a shape's inner proof, made once"""
    if name not in _claims:
        g = inner(name)
        _claims[name] = claims(g["proof"], g["cfg"])
    return _claims[name]


def claims(proof, cfg):
    """what prover and verifier hold of an inner proof: dict(LN, NL, pow_bits, index, ev0, leaves [n_q][NL][32], betas, fpoly, ops, words,
    chals [(absorbed, value)], ord_pow)"""
    cl, hd, st, _, leaves = Z.claims(proof, cfg)
    ops, words, values = T.record(proof, cfg)
    chals = T.chain_blocks(0, ops, words)[1]
    assert [v for _, v in chals] == values
    index = [int(i) for i in cl["index"]]
    N = 1 << cl["shape"][0]
    ord_pow = len(chals) - 1 - len(index)
    assert [v % N for _, v in chals[ord_pow + 1:]] == index and all(a == len(words) for a, _ in chals[ord_pow:])
    return dict(LN=cl["shape"][0], NL=cl["shape"][4], pow_bits=dict(S.DEFAULT_CFG, **cfg)["pow_bits"], index=index, ev0=F.ev0_of(index, leaves.reshape(len(index), -1, 16, 2)), leaves=leaves,
                betas=hd["betas"], fpoly=hd["fpoly"], ops=ops, words=words, chals=chals, ord_pow=ord_pow)


def tables(c, cfg, forge=None, exit_values=None):
    """-> ([(trace, public inputs)] of FriFoldAir, TranscriptAir, FriExitAir with the group's digest as their last four words, the digest)"""
    stmt = statement_digest(c["LN"], c["pow_bits"], c["ord_pow"], c["words"], c["chals"], c["index"], c["ev0"], c["leaves"])
    ftr, fpub = F.ref_trace(c["index"], c["leaves"], c["betas"], c["LN"], Z.table_log(F.log_rows(len(c["index"]), c["LN"], c["NL"]), cfg))
    ttr, _, _ = T.ref_table([(c["ops"], c["words"])], I.transcript_log(c["ops"], cfg))
    values = [v for _, v in c["chals"][c["ord_pow"]:]] if exit_values is None else exit_values
    etr, epub = ref_trace(values, c["LN"], c["NL"], c["pow_bits"], c["ord_pow"], len(c["words"]), c["fpoly"], Z.table_log(log_rows(len(c["index"])), cfg), stmt, forge)
    return [(ftr, fpub[:F.PUB_DIGEST] + stmt), (ttr, list(stmt)), (etr, epub)], stmt


def airs():
    return [F.air(), T.air(), air()]


def group(name):
    """the reference exit group of a shape, made once: dict(proof, cfg, c: claims, tabs, stmt, proofs: the three table proofs)"""
    if name not in _groups:
        g = dict(inner(name))
        c = claims_of(name)
        tabs, stmt = tables(c, g["cfg"])
        g.update(c=c, tabs=tabs, stmt=stmt, proofs=Z.prove(tabs, airs(), g["cfg"]))
        _groups[name] = g
    return _groups[name]


def totals(proofs, cap_h):
    """(sum over the tables of published total x rows, the shared challenges) of a group's table proofs"""
    chal = S.shared_challenges_n([S.proof_peek(p, cap_h) for p in proofs], 4)
    tot = S.ExtS(0)
    for p in proofs:
        s, n = R.published_total(p, cap_h)
        tot = tot + s * n
    return tot, chal
