"""TEST INFRASTRUCTURE for a STARK proof's Merkle openings proven from the paths it carries (csrc/vx_stark_groups.hip): the claims
of a proof restated INDEPENDENTLY (the proof walked word by word, the transcript replayed for the query indices and the running
evaluation that fills a layer leaf's `within` slot), path -> blocks from the leaf digest, the siblings and the fold of the cap with
oracle.two_to_one, the statement digest, the group's tables and reference prover, the blob wrapper and the verifier's side of the
bus.  The AIRs (MerkleOpenSetAir, LeafSpongeSetAir), the sponge blocks and the bus denominators are fri_queries_ref / merkle_open_ref /
leaf_sponge_ref.  No tests here."""
import numpy as np

import fri_queries_ref as Q
import leaf_sponge_ref as R
import merkle_open_ref as M
from oracle import oracle as O
from oracle import pyref
from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
MAGIC, HDR = int.from_bytes(b"VXSOPEN1", "little"), 9  # magic, 7 shape words, the table count; then one length per table
TREE0 = 8  # main / auxiliary / quotient = 8 / 9 / 10; layer l = l
NQ = 4
CHAL = M.CHAL


def log_leaves_of(cl, tree):
    LN, _, _, a, _, _, _ = cl["shape"]
    return LN if tree >= TREE0 else LN - a * (tree + 1)


# ---- the claims of a proof
def extract(proof, cfg=None, ext_chal=None):
    """-> dict(shape [LN, cm, ca, a, NL, cap_h, n_queries], trees (ids of a query's trees in record order), caps {tree: [2^cap_h][4]},
    index [n_queries], claims: one dict(tree, index, leaf, sib [depth][4], sib_at (its first word in the proof)) per (query, tree),
    queries outermost).  Nothing is verified here (S.verify does that): the transcript is replayed for what the claims need."""
    cfg = dict(S.DEFAULT_CFG, **(cfg or {}))
    pr = [int(x) for x in np.asarray(proof, dtype=np.uint64)]
    pos = 0

    def take(k):
        nonlocal pos
        out = pr[pos:pos + k]
        pos += k
        return out

    def take_ext(k):
        w = take(2 * k)
        return [S.ExtS(w[2 * i], w[2 * i + 1]) for i in range(k)]

    _, air_id, L, cm, nq, r, cap_h, n_queries, _, n_layers = take(10)
    air = S.AIRS[air_id]
    arities = take(n_layers)
    final_len, n_pub = take(2)
    pub = take(n_pub)
    ca = getattr(air, "AUX", 0)
    LN, cap_words = L + r, 4 << cap_h
    N, c = 1 << LN, cm + ca
    ch = O.Challenger()
    if pub:
        ch.observe(np.array(pub, dtype=np.uint64))
    caps = {TREE0: np.array(take(cap_words), dtype=np.uint64).reshape(-1, 4)}
    ch.observe(caps[TREE0].reshape(-1))
    if ca:
        if ext_chal is not None:
            ch.observe(np.array([int(x) % P for x in ext_chal], dtype=np.uint64))
        else:
            for _ in range(air.CHAL):
                ch.challenge()
        aux_pub = take(2 * air.AUXPUB)
        if aux_pub:
            ch.observe(np.array(aux_pub, dtype=np.uint64))
        caps[TREE0 + 1] = np.array(take(cap_words), dtype=np.uint64).reshape(-1, 4)
        ch.observe(caps[TREE0 + 1].reshape(-1))
    ch.challenge(), ch.challenge()
    caps[TREE0 + 2] = np.array(take(cap_words), dtype=np.uint64).reshape(-1, 4)
    ch.observe(caps[TREE0 + 2].reshape(-1))
    zeta = S._ext_challenge(ch)
    zeta_next = zeta * O.root(L)
    o_local, o_next, o_quot = take_ext(c), take_ext(c), take_ext(nq)
    for e in o_local + o_quot + o_next:
        S._observe_ext(ch, e)
    alpha = S._ext_challenge(ch)
    betas = []
    for l in range(n_layers):
        caps[l] = np.array(take(cap_words), dtype=np.uint64).reshape(-1, 4)
        ch.observe(caps[l].reshape(-1))
        betas.append(S._ext_challenge(ch))
    for e in take_ext(final_len):
        S._observe_ext(ch, e)
    ch.observe(np.array(take(1), dtype=np.uint64))
    ch.challenge()
    apow, y0, y1 = S.ExtS(1), S.ExtS(0), S.ExtS(0)
    for j in range(c + nq):
        if j < c:
            y0, y1 = y0 + apow * o_local[j], y1 + apow * o_next[j]
        else:
            y0 = y0 + apow * o_quot[j - c]
        apow = apow * alpha
    alpha_c, depth0, wN = alpha ** c, LN - cap_h, O.root(LN)
    a = cfg["arity_bits"]
    trees = [TREE0] + ([TREE0 + 1] if ca else []) + [TREE0 + 2] + list(range(n_layers))
    index, claims = [], []

    def sibs(depth):
        at = pos
        return np.array(take(4 * depth), dtype=np.uint64).reshape(-1, 4), at

    for _ in range(n_queries):
        x_index = ch.challenge() % N
        index.append(x_index)
        row_t = take(cm)
        sb, at = sibs(depth0)
        claims.append(dict(tree=TREE0, index=x_index, leaf=row_t, sib=sb, sib_at=at))
        row = list(row_t)
        if ca:
            row_a = take(ca)
            sb, at = sibs(depth0)
            claims.append(dict(tree=TREE0 + 1, index=x_index, leaf=row_a, sib=sb, sib_at=at))
            row += row_a
        row_q = take(nq)
        sb, at = sibs(depth0)
        claims.append(dict(tree=TREE0 + 2, index=x_index, leaf=row_q, sib=sb, sib_at=at))
        x = S.G * pow(wN, pyref.bitrev(x_index, LN), P) % P
        s1, ap = S.ExtS(0), S.ExtS(1)
        for j in range(c):
            s1, ap = s1 + ap * row[j], ap * alpha
        s0 = s1
        for j in range(nq):
            s0, ap = s0 + ap * row_q[j], ap * alpha
        ev = alpha_c * (s0 - y0) * (S.ExtS(x) - zeta).inv() + (s1 - y1) * (S.ExtS(x) - zeta_next).inv()
        cur_log, xi = LN, x_index
        for l, ar in enumerate(arities):
            arity = 1 << ar
            within = xi & (arity - 1)
            others = take_ext(arity - 1)
            leaf = others[:within] + [ev] + others[within:]
            flat = [v for e in leaf for v in (e.a, e.b)]
            sb, at = sibs(cur_log - ar - cap_h)
            claims.append(dict(tree=l, index=xi >> ar, leaf=flat, sib=sb, sib_at=at))
            out = O.fri_compute_evaluation(x, within, ar, np.array(flat, dtype=np.uint64), betas[l].arr())
            ev = S.ExtS(int(out[0]), int(out[1]))
            x = pow(x, arity, P)
            xi >>= ar
            cur_log -= ar
    assert pos == len(pr)
    return dict(shape=[LN, cm, ca, a, n_layers, cap_h, n_queries], trees=trees, caps=caps, index=index, claims=claims)


# ---- path -> blocks
def leaf_digest(row):
    """hash_or_noop: a row of at most 4 words is its own digest, zero-padded"""
    row = [int(v) for v in row]
    if len(row) <= 4:
        return row + [0] * (4 - len(row))
    return [int(v) for v in O.hash_no_pad(np.array(row, dtype=np.uint64))]


def cap_levels(cap):
    """the fold of a cap: levels[0] = the cap, levels[-1] = [root]"""
    lv = [[[int(v) for v in d] for d in np.asarray(cap, dtype=np.uint64).reshape(-1, 4)]]
    while len(lv[-1]) > 1:
        cur = lv[-1]
        lv.append([[int(v) for v in O.two_to_one(cur[2 * k], cur[2 * k + 1])] for k in range(len(cur) // 2)])
    return lv


def path_blocks(tree, idx, digest, sib, cap, log_leaves, depth=None):
    """the blocks of one path from what a proof carries: the leaf digest, the siblings below the cap, the cap (its fold gives the
    siblings above).  depth: the DEPTH cells (a forgery: a path labelled with another tree's depth)"""
    up = cap_levels(cap)
    low = log_leaves - (len(up) - 1)
    assert len(sib) == low
    cur, lf, out = [int(v) for v in digest], [int(v) for v in digest], []
    for l in range(log_leaves):
        node = idx >> l
        bit = node & 1
        s = [int(v) for v in sib[l]] if l < low else list(up[l - low][node ^ 1])
        out.append(dict(cur=cur, sib=s, bit=bit, leaf=lf, r=node, lvl=l + 1, act=1, end=int(l == log_leaves - 1), firstb=int(l == 0), tree=tree, root=list(up[-1][0]),
                        depth=log_leaves if depth is None else depth))
        cur = [int(v) for v in (O.two_to_one(s, cur) if bit else O.two_to_one(cur, s))]
    return out, cur


def open_log_rows(n_levels):
    return max(5, (32 * n_levels - 1).bit_length())


def paths_ref_trace(caps, log_leaves, tree_of, leaf_idx, digests, sibs, log_n=None):
    """the openings table from paths -> (trace [72][2^log_n], the 4 public inputs: the claims digest, every path's end)"""
    blocks, ends = [], []
    for t, i, d, s in zip(tree_of, leaf_idx, digests, sibs):
        bl, end = path_blocks(int(t), int(i), d, s, caps[int(t)], log_leaves[int(t)])
        blocks += bl
        ends.append(end)
    log_n = open_log_rows(len(blocks)) if log_n is None else log_n
    return Q.open_assemble(blocks, log_n), Q.open_claims_digest(tree_of, leaf_idx, digests), ends


# ---- the statement and the tables of the group
def roots_of(cl):
    return [cap_levels(cl["caps"][t])[-1][0] for t in cl["trees"]]


def statement_digest(cl):
    """hash_n_to_hash_no_pad(the shape words, the folded root of every tree in record order, per query the index and the leaf words
    of every tree in record order)"""
    words = list(cl["shape"])
    for r in roots_of(cl):
        words += r
    per = len(cl["trees"])
    for q, i in enumerate(cl["index"]):
        words.append(int(i))
        for c in cl["claims"][q * per: (q + 1) * per]:
            words += [int(v) for v in c["leaf"]]
    return [int(v) for v in O.hash_no_pad(np.array(words, dtype=np.uint64))]


def sponge_lengths(cl):
    return sorted(set(len(c["leaf"]) for c in cl["claims"] if len(c["leaf"]) > 4))


def tables(cl):
    """the traces and public inputs of the group in bus order: the openings, then one sponge table per leaf length above 4, ascending
    -> ([(trace, pub)], the leaf lengths of the sponge tables)"""
    stmt = statement_digest(cl)
    blocks = []
    for c in cl["claims"]:
        bl, end = path_blocks(c["tree"], c["index"], leaf_digest(c["leaf"]), c["sib"], cl["caps"][c["tree"]], log_leaves_of(cl, c["tree"]))
        assert end == bl[0]["root"], "the path of tree %d at %d does not reach its root" % (c["tree"], c["index"])
        blocks += bl
    tabs = [(Q.open_assemble(blocks, open_log_rows(len(blocks))), list(stmt))]
    lens = sponge_lengths(cl)
    for L in lens:
        sel = [c for c in cl["claims"] if len(c["leaf"]) == L]
        tr, _, _ = Q.sponge_ref_trace([c["tree"] for c in sel], [c["index"] for c in sel], [c["leaf"] for c in sel])
        tabs.append((tr, Q.sponge_public(L, stmt)))
    return tabs, lens


def airs(n_tables):
    return [Q.open_air()] + [Q.sponge_air()] * (n_tables - 1)


def shared_challenges(tabs, cfg=None):
    return S.shared_challenges_n([(pub, R.trace_cap(tr, cfg)) for tr, pub in tabs], 4)


def prove(tabs, cfg=None, chal=None):
    """the reference prover on the restatements under the challenges all tables share -> the table proofs (id words REF ids)"""
    chal = shared_challenges(tabs, cfg) if chal is None else chal
    hook = lambda pub, cap: chal  # noqa: E731
    return [S.prove(a, tr, pub, cfg, chal_hook=hook) for a, (tr, pub) in zip(airs(len(tabs)), tabs)]


def wrap(proofs, shape):
    """the table proofs as a blob of the product, with the compiled AIRs' ids in their id words"""
    ps = [np.array(p, dtype=np.uint64) for p in proofs]
    for k, p in enumerate(ps):
        p[1] = Q.OPEN_ID if k == 0 else Q.SPONGE_ID
    return np.concatenate([np.array([MAGIC] + list(shape) + [len(ps)] + [p.size for p in ps], dtype=np.uint64)] + ps)


def unwrap(blob):
    """the table proofs inside a blob, with the reference registry's ids in their id words"""
    n = int(blob[HDR - 1])
    assert int(blob[0]) == MAGIC and 1 <= n <= 4 and sum(int(v) for v in blob[HDR: HDR + n]) == blob.size - HDR - n
    out, at = [], HDR + n
    for k in range(n):
        p = np.array(blob[at: at + int(blob[HDR + k])], dtype=np.uint64)
        p[1] = Q.OPEN_REF_ID if k == 0 else Q.SPONGE_REF_ID
        out.append(p)
        at += p.size
    return out


def outside_sum(chal, cl):
    """what the verifier puts on the bus, per claim: the two halves of (root, depth); every word of a row longer than 4 words; the two
    halves of the opening of a row that is its own digest"""
    bus = Q._bus(chal)
    roots = dict(zip(cl["trees"], roots_of(cl)))
    tot = S.ExtS(0)
    for c in cl["claims"]:
        t, i, r, depth = c["tree"], c["index"], roots[c["tree"]], log_leaves_of(cl, c["tree"])
        tot = tot + Q.d_root(bus, t, r[0], r[1], 0, depth).inv() + Q.d_root(bus, t, r[2], r[3], 1, depth).inv()
        if len(c["leaf"]) > 4:
            for j, w in enumerate(c["leaf"]):
                tot = tot + Q.d_row(bus, t, i, j, w).inv()
        else:
            d = leaf_digest(c["leaf"])
            tot = tot + Q.d_open(bus, t, i, d[0], d[1], 0).inv() + Q.d_open(bus, t, i, d[2], d[3], 1).inv()
    return tot


def bus_check(proofs, cap_h, cl):
    """the verifier's side of the bus in Python on the table proofs: the published totals x rows == outside_sum"""
    chal = S.shared_challenges_n([S.proof_peek(p, cap_h) for p in proofs], 4)
    tot = S.ExtS(0)
    for p in proofs:
        s, n = R.published_total(p, cap_h)
        tot = tot + s * n
    return tot == outside_sum(chal, cl), chal


def zero_siblings(proof, cl):
    """the proof with every sibling word zeroed"""
    p = np.array(proof, dtype=np.uint64)
    for c in cl["claims"]:
        p[c["sib_at"]: c["sib_at"] + c["sib"].size] = 0
    return p
