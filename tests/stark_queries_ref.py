"""TEST INFRASTRUCTURE for the whole query phase of a STARK proof on one bus (csrc/vx_stark_groups.hip): the head of a proof walked
word by word with its transcript replayed (alpha, zeta, the openings, betas, the final polynomial, where the query records start),
the claims of the group (the Merkle side is stark_openings_ref.extract; the rows the combination reads and the leaves the folds
read are taken from it), the statement digest, the five to seven tables and the group's reference prover, blob wrap and unwrap, the
outside party's sum and a helper that garbles the query section of a proof.  The AIRs are the restatements of fri_queries_ref
(MerkleOpenSetAir, LeafSpongeSetAir), leaf_noop_ref, fri_combine_ref and fri_fold_ref.  No tests here."""
import numpy as np

import fri_combine_ref as K
import fri_fold_ref as F
import fri_queries_ref as Q
import leaf_noop_ref as N
import leaf_sponge_ref as R
import stark_openings_ref as X
from oracle import oracle as O
from oracle import stark_ref as S

P = F.P
MAGIC, HDR = int.from_bytes(b"VXSQRY01", "little"), 9  # magic, 7 shape words, the table count; then one length per table
TREE0, NQ = X.TREE0, X.NQ
CHAL = F.CHAL


# ---- the head of a proof
def head(proof, cfg=None, ext_chal=None):
    """-> dict(alpha, zeta: [2]; ol, on [c][2], oq [4][2]; betas [NL][2]; fpoly [final_len][2]; o_queries: where the query records
    start; q_words: the words of one record).  Nothing is verified."""
    cfg = dict(S.DEFAULT_CFG, **(cfg or {}))
    pr = [int(x) for x in np.asarray(proof, dtype=np.uint64)]
    _, air_id, L, cm, nq, r, cap_h, n_queries, _, n_layers = pr[:10]
    air = S.AIRS[air_id]
    ca, pos = getattr(air, "AUX", 0), 10
    arities = pr[pos: pos + n_layers]
    final_len, n_pub = pr[pos + n_layers: pos + n_layers + 2]
    pos += n_layers + 2

    def take(k):
        nonlocal pos
        pos += k
        return np.array(pr[pos - k: pos], dtype=np.uint64)

    cw, c, LN = 4 << cap_h, cm + ca, L + r
    ch = O.Challenger()
    pub = take(n_pub)
    if n_pub:
        ch.observe(pub)
    ch.observe(take(cw))
    if ca:
        if ext_chal is not None:
            ch.observe(np.array([int(x) % P for x in ext_chal], dtype=np.uint64))
        else:
            for _ in range(air.CHAL):
                ch.challenge()
        ch.observe(take(2 * air.AUXPUB))
        ch.observe(take(cw))
    ch.challenge(), ch.challenge()
    ch.observe(take(cw))
    zeta = [ch.challenge(), ch.challenge()]
    ol, on, oq = (take(2 * k).reshape(-1, 2) for k in (c, c, nq))
    for o in (ol, oq, on):
        ch.observe(o.reshape(-1))
    alpha = [ch.challenge(), ch.challenge()]
    betas = []
    for _ in arities:
        ch.observe(take(cw))
        betas.append([ch.challenge(), ch.challenge()])
    fpoly = take(2 * final_len).reshape(-1, 2)
    take(1)
    depth0, q_words, cur = LN - cap_h, 0, LN
    q_words = cm + nq + 8 * depth0 + (ca + 4 * depth0 if ca else 0)
    for ab in arities:
        cur -= ab
        q_words += 2 * ((1 << ab) - 1) + 4 * (cur - cap_h)
    assert pos + n_queries * q_words == len(pr)
    return dict(alpha=alpha, zeta=zeta, ol=ol, on=on, oq=oq, betas=betas, fpoly=fpoly, o_queries=pos, q_words=q_words, r=r)


def claims(proof, cfg=None, ext_chal=None):
    """-> (cl: stark_openings_ref.extract, hd: head, st: the combine statement, rows [n_q][c + 4], leaves [n_q][NL][32])"""
    cl, hd = X.extract(proof, cfg, ext_chal), head(proof, cfg, ext_chal)
    LN, cm, ca, _, NL, _, n_q = cl["shape"]
    per = len(cl["trees"])
    rows, leaves = [], []
    for q in range(n_q):
        rec = cl["claims"][q * per: (q + 1) * per]
        rows.append([int(v) for c in rec if c["tree"] >= TREE0 for v in c["leaf"]])
        leaves.append([[int(v) for v in c["leaf"]] for c in rec if c["tree"] < TREE0])
    st = dict(LN=LN, r=hd["r"], cm=cm, ca=ca, nq=NQ, alpha=np.array(hd["alpha"], dtype=np.uint64), zeta=np.array(hd["zeta"], dtype=np.uint64), ol=hd["ol"], on=hd["on"], oq=hd["oq"])
    return cl, hd, st, np.array(rows, dtype=np.uint64), np.array(leaves, dtype=np.uint64).reshape(n_q, NL, 32)


def statement_digest(cl, hd):
    """hash_n_to_hash_no_pad(the 7 shape words, alpha, zeta, the openings local / next / quotient, betas, the final polynomial, the
    folded root of every tree in record order, the index of every query): no row word, no leaf word"""
    w = list(cl["shape"]) + list(hd["alpha"]) + list(hd["zeta"])
    for part in (hd["ol"], hd["on"], hd["oq"], hd["betas"], hd["fpoly"]):
        w += [int(v) for v in np.asarray(part, dtype=np.uint64).reshape(-1)]
    for r in X.roots_of(cl):
        w += r
    w += [int(i) for i in cl["index"]]
    return [int(v) for v in O.hash_no_pad(np.array(w, dtype=np.uint64))]


# ---- the tables of the group, in bus order
def table_log(log_n, cfg=None):
    """the rows (log2) a table of at least 2^log_n rows is proven at: the next size whose FRI plan under the configuration leaves a
    final polynomial (with arity 4, final_poly_bits 0 and cap height 0 a table of 2^7 rows would be folded below degree one)"""
    cfg = dict(S.DEFAULT_CFG, **(cfg or {}))
    while True:
        d = log_n
        while d > cfg["final_poly_bits"] and d + cfg["rate_bits"] - cfg["arity_bits"] >= cfg["cap_height"]:
            d -= cfg["arity_bits"]
        if d >= 0:
            return log_n
        log_n += 1


def tables(cl, hd, st, rows, leaves, forge=None, cfg=None):
    """-> ([(trace, public inputs)], [AIR], the leaf lengths of the sponge tables).  forge(kind, ...) hooks let a test change what ONE
    table holds: forge = dict(sponge=f(tree, index, leaf) -> leaf, noop=f(tree, index, leaf) -> (tree, leaf), rows=f(rows) -> rows)"""
    forge = forge or {}
    stmt = statement_digest(cl, hd)
    blocks = []
    for c in cl["claims"]:
        bl, end = X.path_blocks(c["tree"], c["index"], X.leaf_digest(c["leaf"]), c["sib"], cl["caps"][c["tree"]], X.log_leaves_of(cl, c["tree"]))
        assert end == bl[0]["root"], "the path of tree %d at %d does not reach its root" % (c["tree"], c["index"])
        blocks += bl
    tabs, airs = [(Q.open_assemble(blocks, table_log(X.open_log_rows(len(blocks)), cfg)), list(stmt))], [Q.open_air()]
    lens = X.sponge_lengths(cl)
    fs = forge.get("sponge", lambda t, i, leaf: leaf)
    for L in lens:
        sel = [c for c in cl["claims"] if len(c["leaf"]) == L]
        tr, _, _ = Q.sponge_ref_trace([c["tree"] for c in sel], [c["index"] for c in sel], [fs(c["tree"], c["index"], list(c["leaf"])) for c in sel],
                                      table_log(Q.sponge_log_rows(len(sel), L), cfg))
        tabs.append((tr, Q.sponge_public(L, stmt)))
        airs.append(Q.sponge_air())
    fn = forge.get("noop", lambda t, i, leaf: (t, leaf))
    sel = [(c["index"],) + tuple(fn(c["tree"], c["index"], list(c["leaf"]))) for c in cl["claims"] if len(c["leaf"]) <= 4]
    tabs.append(N.ref_trace([t for _, t, _ in sel], [i for i, _, _ in sel], [leaf for _, _, leaf in sel], table_log(N.log_rows(len(sel)), cfg), digest=stmt))
    airs.append(N.air())
    ctr, cpub = K.ref_trace(st, cl["index"], forge.get("rows", lambda x: x)(rows), table_log(K.log_rows(len(cl["index"]), st), cfg))
    tabs.append((ctr, cpub[:K.PUB_DIGEST] + stmt))
    airs.append(K.air())
    ftr, fpub = F.ref_trace(cl["index"], leaves, hd["betas"], st["LN"], table_log(F.log_rows(len(cl["index"]), st["LN"], len(hd["betas"])), cfg))
    tabs.append((ftr, fpub[:F.PUB_DIGEST] + stmt))
    airs.append(F.air())
    return tabs, airs, lens


def shared_challenges(tabs, cfg=None):
    return S.shared_challenges_n([(pub, R.trace_cap(tr, cfg)) for tr, pub in tabs], 4)


def prove(tabs, airs, cfg=None, chal=None):
    """the reference prover on the restatements under the challenges all tables share -> the table proofs (id words REF ids)"""
    chal = shared_challenges(tabs, cfg) if chal is None else chal
    hook = lambda pub, cap: chal  # noqa: E731
    return [S.prove(a, tr, pub, cfg, chal_hook=hook) for a, (tr, pub) in zip(airs, tabs)]


def _ids(n, ref):
    mid = [Q.SPONGE_REF_ID if ref else Q.SPONGE_ID] * (n - 4)
    return ([Q.OPEN_REF_ID] + mid + [N.REF_ID, K.REF_ID, F.REF_ID]) if ref else ([Q.OPEN_ID] + mid + [N.AIR_ID, K.AIR_ID, F.AIR_ID])


def wrap(proofs, shape):
    """the table proofs as a blob of the product, with the compiled AIRs' ids in their id words"""
    ps = [np.array(p, dtype=np.uint64) for p in proofs]
    for p, i in zip(ps, _ids(len(ps), False)):
        p[1] = i
    return np.concatenate([np.array([MAGIC] + list(shape) + [len(ps)] + [p.size for p in ps], dtype=np.uint64)] + ps)


def unwrap(blob):
    """the table proofs inside a blob, with the reference registry's ids in their id words"""
    n = int(blob[HDR - 1])
    assert int(blob[0]) == MAGIC and 5 <= n <= 7 and sum(int(v) for v in blob[HDR: HDR + n]) == blob.size - HDR - n
    out, at = [], HDR + n
    for k, i in enumerate(_ids(n, True)):
        p = np.array(blob[at: at + int(blob[HDR + k])], dtype=np.uint64)
        p[1] = i
        out.append(p)
        at += p.size
    return out


def outside_sum(chal, cl, hd):
    """what the verifier receives, per query: the two halves of (root, depth) of every tree of the record, and the exit of the fold
    chain fri(index, final_poly(x_NL), 1).  It sends nothing."""
    bus = Q._bus(chal)
    LN, NL = cl["shape"][0], cl["shape"][4]
    roots = dict(zip(cl["trees"], X.roots_of(cl)))
    tot = S.ExtS(0)
    for i in cl["index"]:
        for t in cl["trees"]:
            r, depth = roots[t], X.log_leaves_of(cl, t)
            tot = tot + Q.d_root(bus, t, r[0], r[1], 0, depth).inv() + Q.d_root(bus, t, r[2], r[3], 1, depth).inv()
        fe = F.final_eval(hd["fpoly"], int(i), LN, NL)
        tot = tot + F.d_fri(bus, i, fe.a, fe.b, 1).inv()
    return tot


def tables_sum(tabs, airs, chal):
    """sum over the tables of total x rows from their auxiliary generators, and the first (table, constraint, row) a row check refuses"""
    tot, bad = S.ExtS(0), None
    for k, (a, (tr, pub)) in enumerate(zip(airs, tabs)):
        aux, apub = a.gen_aux(tr, chal, pub)
        tot = tot + S.ExtS(*apub) * tr.shape[1]
        if bad is None:
            b = S.check_trace(a, tr, pub, chal, aux, apub)
            bad = None if b is None else (k,) + tuple(b)
    return tot, bad


def bus_check(proofs, cap_h, cl, hd):
    """the verifier's side of the bus in Python on the table proofs: the published totals x rows == outside_sum"""
    chal = S.shared_challenges_n([S.proof_peek(p, cap_h) for p in proofs], 4)
    tot = S.ExtS(0)
    for p in proofs:
        s, n = R.published_total(p, cap_h)
        tot = tot + s * n
    return tot == outside_sum(chal, cl, hd), chal


def garbled(proof, hd, seed=1):
    """the proof with every word of its query section replaced by junk (non-canonical words among it)"""
    p = np.array(proof, dtype=np.uint64)
    junk = np.random.default_rng(seed).integers(0, 1 << 63, size=p.size - hd["o_queries"], dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    p[hd["o_queries"]:] = junk
    return p


# ---- the inner proofs both tiers use: name -> (AIR, log_n, configuration overrides, the shape words [LN, cm, ca, a, NL, cap_h, n_q])
SHAPES = {
    "fib8": ("FibAir", 8, dict(num_queries=5), [9, 2, 0, 4, 1, 4, 5]),                                             # five tables; main and quotient through the noop table
    "lookup8": ("LookupAir", 8, dict(num_queries=5), [9, 7, 6, 4, 1, 4, 5]),                                       # seven tables; sponge lengths 6, 7, 32
    "fib8_two_layers_cap0": ("FibAir", 8, dict(num_queries=5, final_poly_bits=0, cap_height=0), [9, 2, 0, 4, 2, 0, 5]),  # ONE bit row per fold query
    "fib9_two_layers_cap1": ("FibAir", 9, dict(num_queries=5, final_poly_bits=1, cap_height=1), [10, 2, 0, 4, 2, 1, 5]),  # two bit rows
    "fib8_rate2": ("FibAir", 8, dict(num_queries=5, rate_bits=2), [10, 2, 0, 4, 1, 4, 5]),                         # LDE of 2^10
    "fib8_40_queries": ("FibAir", 8, dict(num_queries=40), [9, 2, 0, 4, 1, 4, 40]),                                # an index drawn twice
}


def inner(name):
    """-> (the AIR, its trace, its public inputs, the reference configuration) of a shape"""
    air_name, log_n, over, _ = SHAPES[name]
    air = getattr(S, air_name)
    trace, pub = air.trace(log_n)
    return air, trace, pub, dict(S.DEFAULT_CFG, **over)


_groups = {}


def group(name):
    """the reference group of a shape, made once: dict(proof: the reference prover's inner proof, cfg, cl, hd, st, rows, leaves, tabs,
    airs, proofs: the table proofs, blob)"""
    if name not in _groups:
        air, trace, pub, cfg = inner(name)
        proof = np.array(S.prove(air, trace, pub, cfg), dtype=np.uint64)
        cl, hd, st, rows, leaves = claims(proof, cfg)
        tabs, airs, _ = tables(cl, hd, st, rows, leaves, cfg=cfg)
        proofs = prove(tabs, airs, cfg)
        _groups[name] = dict(proof=proof, cfg=cfg, cl=cl, hd=hd, st=st, rows=rows, leaves=leaves, tabs=tabs, airs=airs, proofs=proofs, blob=wrap(proofs, cl["shape"]))
    return _groups[name]
