"""What tests/test_verify_deferred.py (CPU) and tests/test_gpu_verify_dev.py share: the reference prover's proofs (made once, never
modified), where every kind of word lies in a proof, and the sample of single-word corruptions both files judge against
lib.stark_verify."""
import numpy as np

from oracle import stark_ref as S

P = 2**64 - 2**32 + 1
NQ = 4

# name -> (AIR, log_n, what differs from the default configuration).  lookup8 has an auxiliary tree; the third has two fold layers and
# no cap above the roots (the shapes of tests/stark_queries_ref.py, which tests/test_stark_inner.py proves over)
CASES = {
    "fib5": ("FibAir", 5, dict(num_queries=6)),
    "lookup8": ("LookupAir", 8, dict(num_queries=5)),
    "fib8_two_layers_cap0": ("FibAir", 8, dict(num_queries=5, final_poly_bits=0, cap_height=0)),
}
_proofs = {}


def case(name):
    """-> (proof words, the reference configuration, the AIR)"""
    if name not in _proofs:
        air_name, log_n, over = CASES[name]
        air = getattr(S, air_name)
        trace, pub = air.trace(log_n)
        cfg = dict(S.DEFAULT_CFG, **over)
        proof = np.array(S.prove(air, trace, pub, cfg), dtype=np.uint64)
        proof.setflags(write=False)
        _proofs[name] = (proof, cfg, air)
    return _proofs[name]


def pcfg(vx, cfg):
    keys = ("rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits", "final_poly_bits")
    return vx.lib.default_stark_config(**{k: cfg[k] for k in keys})


def layout(proof):
    """Where the words of a vx_stark_prove proof lie, from its header and its length alone (the number of auxiliary columns is not in
    the header: the length settles it) -> dict(regions: name -> [(start, end)], queries: per query dict(name -> (start, end)),
    o_queries).  Names: header, public, caps, openings, final_poly, nonce, rows, layer_evals, siblings."""
    pr = [int(v) for v in proof]
    _, _, L, cm, nq, r, cap_h, n_queries, _, n_layers = pr[:10]
    arities = pr[10:10 + n_layers]
    final_len, n_pub = pr[10 + n_layers:12 + n_layers]
    LN, cw = L + r, 4 << cap_h
    depth0 = LN - cap_h
    depths, cur = [], LN
    for a in arities:
        cur -= a
        depths.append(cur - cap_h)
    layer_words = sum(2 * ((1 << a) - 1) + 4 * d for a, d in zip(arities, depths))
    # without auxiliary columns ...
    head0 = 12 + n_layers + n_pub + cw * (2 + n_layers) + 2 * (2 * cm + nq) + 2 * final_len + 1
    q0 = cm + nq + 8 * depth0 + layer_words
    rest = len(pr) - head0 - n_queries * q0
    ca = auxpub = 0
    if rest:  # ... and with ca of them: a third cap, 2 auxpub published words, 4 ca opening words; per query ca words and a third path
        rest -= cw + n_queries * 4 * depth0
        ca, auxpub = rest // (4 + n_queries), (rest % (4 + n_queries)) // 2
        assert ca >= 1 and rest == ca * (4 + n_queries) + 2 * auxpub and auxpub <= 4
    c = cm + ca
    reg = {k: [] for k in ("header", "public", "caps", "openings", "final_poly", "nonce", "rows", "layer_evals", "siblings")}
    at = 0

    def take(name, n):
        nonlocal at
        if n:
            reg[name].append((at, at + n))
        at += n
        return (at - n, at)

    take("header", 12 + n_layers), take("public", n_pub), take("caps", cw)
    if ca:
        take("public", 2 * auxpub), take("caps", cw)
    take("caps", cw), take("openings", 2 * (2 * c + nq)), take("caps", n_layers * cw), take("final_poly", 2 * final_len), take("nonce", 1)
    o_queries, queries = at, []
    for _ in range(n_queries):
        q = dict(row_t=take("rows", cm), sib_t=take("siblings", 4 * depth0))
        if ca:
            q.update(row_a=take("rows", ca), sib_a=take("siblings", 4 * depth0))
        q.update(row_q=take("rows", nq), sib_q=take("siblings", 4 * depth0))
        for l, (a, d) in enumerate(zip(arities, depths)):
            q["evals%d" % l], q["sibs%d" % l] = take("layer_evals", 2 * ((1 << a) - 1)), take("siblings", 4 * d)
        queries.append(q)
    assert at == len(pr), (at, len(pr))
    return dict(regions=reg, queries=queries, o_queries=o_queries, n_layers=n_layers)


def sample(proof, per_region=12):
    """The single-word corruptions of a proof: (what, the corrupted words).  Every header word and per_region positions spread over
    every other kind of word, each with one bit flipped (bits 0, 5 and 40 in turn); and sibling words made non-canonical -- p plus
    the word's low 16 bits: p added to a word of full size would wrap, and no sibling is below 2^32."""
    lay, out, k = layout(proof), [], 0
    for name, spans in lay["regions"].items():
        words = [w for a, b in spans for w in range(a, b)]
        picks = words if name == "header" or len(words) <= per_region else [words[(i * (len(words) - 1)) // (per_region - 1)] for i in range(per_region)]
        for w in sorted(set(picks)):
            bad = proof.copy()
            bad[w] ^= np.uint64(1 << (0, 5, 40)[k % 3])
            out.append(("%s word %d bit %d" % (name, w, (0, 5, 40)[k % 3]), bad))
            k += 1
    sibs = [w for a, b in lay["regions"]["siblings"] for w in range(a, b)]
    for w in (sibs[0], sibs[len(sibs) // 2], sibs[-1]):
        bad = proof.copy()
        bad[w] = np.uint64(P + (int(proof[w]) & 0xFFFF))
        out.append(("sibling word %d non-canonical" % w, bad))
    return out


def answer(fn, *args, **kw):
    """(code, message) of a verifier call: (0, "") when it accepts"""
    try:
        fn(*args, **kw)
    except Exception as e:  # VxError: the binding's one exception
        return (e.code, str(e))
    return (0, "")
