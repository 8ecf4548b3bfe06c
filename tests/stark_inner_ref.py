"""TEST INFRASTRUCTURE for an inner proof's query phase AND transcript on one bus (csrc/vx_stark_groups.hip): nothing is restated
here that tests/ already has.  The claims, rows, leaves and the five to seven query-phase tables are stark_queries_ref's, the chain,
its plan and the transcript table are transcript_ref's (recorded from oracle/stark_ref.py's own verifier); new are the ONE statement
digest, the group's table list with forge hooks, the blob's wrap and unwrap, and the outside party's sum -- the sum of the two
existing ones.  No tests here."""
import numpy as np

import stark_queries_ref as Z
import transcript_ref as T
from oracle import oracle as O
from oracle import stark_ref as S

P = Z.P
MAGIC, HDR = int.from_bytes(b"VXSINR01", "little"), 11  # magic, 7 shape words, the table count, n_obs, n_chal; then the claims, one length per table
CHAL = Z.CHAL
EXT = [5, P - 6, 7, 1 << 40]  # external lookup challenges (tests/test_transcript.py's)


def statement_digest(shape, words, chals):
    """hash_n_to_hash_no_pad(the 7 shape words, n_obs, n_chal, the observed words in order, (absorbed, value) of every challenge)"""
    w = [int(v) for v in shape] + [len(words), len(chals)] + [int(v) for v in words]
    for a, v in chals:
        w += [int(a), int(v)]
    return [int(v) for v in O.hash_no_pad(np.array(w, dtype=np.uint64))]


def transcript_log(ops, cfg=None):
    return T.table_log(T.log_rows(len(T.plan(ops))), cfg)


def tables(cl, hd, st, rows, leaves, chain, chals=None, forge=None, cfg=None):
    """-> ([(trace, public inputs)], [AIR], the digest).  chain: (ops, words) of the inner transcript; chals: the CLAIMED challenges
    [(absorbed, value)] the digest is made of (None: the ones the chain yields).  forge: the hooks of stark_queries_ref.tables, and
    transcript=f(ops, words) -> (ops, words): what the transcript table holds instead.  A changed `hd` (betas) reaches the fold table."""
    forge = forge or {}
    ops, words = chain
    if chals is None:
        chals = T.chain_blocks(0, ops, words)[1]
    stmt = statement_digest(cl["shape"], words, chals)
    tabs, airs, _ = Z.tables(cl, hd, st, rows, leaves, forge, cfg)
    tabs = [(tr, [int(v) for v in pub[:-4]] + stmt) for tr, pub in tabs]  # every table ends on four digest words it does not constrain
    f_ops, f_words = forge.get("transcript", lambda o, w: (o, w))(list(ops), list(words))
    trace, _, _ = T.ref_table([(f_ops, f_words)], transcript_log(ops, cfg))
    return tabs + [(trace, list(stmt))], airs + [T.air()], stmt


def prove(tabs, airs, cfg=None):
    """the reference prover on the restatements under the challenges all tables share -> the table proofs (id words REF ids)"""
    return Z.prove(tabs, airs, cfg)


def _ids(n, ref):
    return Z._ids(n - 1, ref) + [T.REF_ID if ref else T.AIR_ID]


def wrap(proofs, shape, n_obs, chals):
    """the table proofs as a blob of the product, with the compiled AIRs' ids in their id words"""
    ps = [np.array(p, dtype=np.uint64) for p in proofs]
    for p, i in zip(ps, _ids(len(ps), False)):
        p[1] = i
    req = list(shape) + [len(ps), int(n_obs), len(chals)]
    for a, v in chals:
        req += [int(a), int(v)]
    return np.concatenate([np.array([MAGIC] + req + [p.size for p in ps], dtype=np.uint64)] + ps)


def unwrap(blob):
    """-> (the table proofs with the reference registry's ids, where the lengths start in the blob)"""
    n, n_chal = int(blob[8]), int(blob[10])
    o_len = HDR + 2 * n_chal
    assert int(blob[0]) == MAGIC and 6 <= n <= 8 and sum(int(v) for v in blob[o_len: o_len + n]) == blob.size - o_len - n
    out, at = [], o_len + n
    for k, i in enumerate(_ids(n, True)):
        p = np.array(blob[at: at + int(blob[o_len + k])], dtype=np.uint64)
        p[1] = i
        out.append(p)
        at += p.size
    return out, o_len


def blob_claims(blob):
    n_chal = int(blob[10])
    return [(int(blob[HDR + 2 * j]), int(blob[HDR + 2 * j + 1])) for j in range(n_chal)]


def outside_sum(chal, cl, hd, words, chals):
    """the outside party of both halves: the roots and the fold exits received; the observed words sent, the challenges received"""
    return Z.outside_sum(chal, cl, hd) + T.outside_sum(chal, [(words, chals)])


def bus_check(proofs, cap_h, cl, hd, words, chals):
    """the verifier's side of the bus in Python on the table proofs: the published totals x rows == outside_sum"""
    chal = S.shared_challenges_n([S.proof_peek(p, cap_h) for p in proofs], 4)
    tot = S.ExtS(0)
    for p in proofs:
        s, n = Z.R.published_total(p, cap_h)
        tot = tot + s * n
    return tot == outside_sum(chal, cl, hd, words, chals)


# ---- the inner proofs both tiers use: name -> (the shape of stark_queries_ref.SHAPES, external lookup challenges,
# (observed words, challenges, duplexes, log2 of the transcript table's rows, tables))
INNER = {
    "fib8": ("fib8", None, (244, 14, 32, 10, 6)),                          # EXACTLY 2^10 rows: a full transcript table, no idle block
    "lookup8": ("lookup8", None, (349, 18, 45, 11, 8)),                    # drawn lookup challenges
    "lookup8_ext": ("lookup8", EXT, None),                                 # ... absorbed instead
    "fib8_two_layers_cap0": ("fib8_two_layers_cap0", None, (38, 16, 7, 8, 6)),  # two fold layers
}
_inner, _groups = {}, {}


def inner(name):
    """-> dict(proof: the reference prover's inner proof, cfg, ext, air, trace, pub)"""
    if name not in _inner:
        shape, ext, _ = INNER[name]
        air, trace, pub, cfg = Z.inner(shape)
        proof = S.prove(air, trace, pub, cfg, chal_hook=(lambda p, cap: ext) if ext else None)
        _inner[name] = dict(proof=np.array(proof, dtype=np.uint64), cfg=cfg, ext=ext, air=air, trace=trace, pub=pub)
    return _inner[name]


def group(name):
    """the reference group of an inner proof, made once: dict(proof, cfg, ext, cl, hd, st, rows, leaves, chain: (ops, words), chals,
    tabs, airs, stmt, proofs: the table proofs, blob)"""
    if name not in _groups:
        g = dict(inner(name))
        cl, hd, st, rows, leaves = Z.claims(g["proof"], g["cfg"], g["ext"])
        ops, words, values = T.record(g["proof"], g["cfg"], g["ext"])
        chals = T.chain_blocks(0, ops, words)[1]
        assert [v for _, v in chals] == values  # the plan's chain draws what the reference verifier drew
        tabs, airs, stmt = tables(cl, hd, st, rows, leaves, (ops, words), chals, cfg=g["cfg"])
        proofs = prove(tabs, airs, g["cfg"])
        g.update(cl=cl, hd=hd, st=st, rows=rows, leaves=leaves, chain=(ops, words), chals=chals, tabs=tabs, airs=airs, stmt=stmt, proofs=proofs,
                 blob=wrap(proofs, cl["shape"], len(words), chals))
        _groups[name] = g
    return _groups[name]
