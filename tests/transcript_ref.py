"""TEST INFRASTRUCTURE for TranscriptAir (csrc/air_transcript.cuh, AIR id 23) and the group of vx_stark_transcripts_prove: the AIR
restated INDEPENDENTLY as a constraint program (air_program.AirBuilder / X2, the same constraint order as the compiled eval, so
oracle.air_program.ProgramAir runs it through oracle/stark_ref.py unchanged), the block plan of a chain from its run lengths (a
counter machine: no hashing), a reference trace generator and gen_aux in plain Python, the statement digest, the transcript of a
proof RECORDED from oracle/stark_ref.py's own verifier (its challenger is wrapped, nothing about the order is restated), the group's
reference prover, blob wrap and unwrap and the outside party's sum.  Independent of the C++.  No tests here."""
import numpy as np

import leaf_sponge_ref as R
import merkle_open_ref as M
import vx_import
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import ProgramAir

P = M.P
AIR_ID = 23        # the compiled AIR
REF_ID = 1023      # the program restatement in the reference prover's registry (never registered with the product)
MSG, W, OUT, Q, PREV, CHAIN, ACT, START, NABS, NCH, COLS = 48, 56, 64, 72, 80, 88, 89, 90, 91, 92, 93
N_HELP, AUX, PUB = 8, 18, 4
TAG_OBS, TAG_CHAL = 12, 13
MAGIC = int.from_bytes(b"VXSTRN01", "little")
CHAL = M.CHAL
degree = R.degree
RULES = {}  # rule name -> index of its first constraint (filled by the builder)


def builder():
    ap = vx_import.load().air_program
    X2 = ap.X2
    b = ap.AirBuilder(COLS, PUB, periodic=M.periodic(), aux_cols=AUX, n_challenges=4, n_aux_public=1)
    full, rnd, out, spare, first = (b.per(q) for q in range(12, 17))
    loc, nxt = b.loc, b.nxt

    def rule(name):
        RULES[name] = len(b.constraints)

    # 1. the permutation
    rule("permutation")
    x = [loc(i) + b.per(i) for i in range(12)]
    a, bb, t = [loc(12 + i) for i in range(12)], [loc(24 + i) for i in range(12)], [loc(36 + i) for i in range(12)]
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
        b.assert_zero(rnd * (nxt(row) - acc))
    for i in range(12):
        b.assert_zero(out * (nxt(i) - loc(i)))
    # 2. shape columns constant over a block
    rule("block_constant")
    for j in range(MSG, COLS):
        b.assert_zero((1 - spare) * (nxt(j) - loc(j)))
    # 3. flags
    chain, act, start, nabs, nch = (loc(j) for j in (CHAIN, ACT, START, NABS, NCH))
    w, q = [loc(W + i) for i in range(8)], [loc(Q + i) for i in range(8)]
    rule("boolean")
    b.assert_zero(act * (act - 1))
    b.assert_zero(start * (start - 1))
    b.assert_zero(start * (1 - act))
    for i in range(8):
        b.assert_zero(w[i] * (w[i] - 1))
    for i in range(8):
        b.assert_zero(q[i] * (q[i] - 1))
    rule("w_prefix")
    for i in range(7):
        b.assert_zero(w[i + 1] * (1 - w[i]))
    rule("q_suffix")
    for i in range(7):
        b.assert_zero(q[i] * (1 - q[i + 1]))
    rule("idle")
    b.assert_zero((1 - act) * w[0])
    b.assert_zero((1 - act) * q[7])
    # 4. the plan
    rule("absorb_or_squeeze")
    b.assert_zero(act * (1 - w[0]) * (1 - q[7]))
    rule("partial_squeezes")
    b.assert_zero(act * (1 - w[7]) * (1 - q[7]))
    rule("start")
    b.assert_zero((act - w[0]) * start)
    b.assert_zero(start * nabs)
    b.assert_zero(start * nch)
    # 5. block input
    rule("input")
    for i in range(8):
        b.assert_zero(first * (loc(i) - loc(MSG + i)))
    rule("kept_words")
    for i in range(8):
        b.assert_zero((1 - w[i]) * (loc(MSG + i) - (act - start) * loc(PREV + i)))
    # 6. spare row -> next block
    sw, sq = w[0], q[0]
    for i in range(1, 8):
        sw, sq = sw + w[i], sq + q[i]
    cn = nxt(ACT) - nxt(START)
    sc, sn = spare * cn, spare * (1 - cn)
    rule("output")
    for i in range(8):
        b.assert_zero(spare * (loc(OUT + i) - loc(i)))
    rule("previous_output")
    for i in range(8):
        b.assert_zero(sc * (nxt(PREV + i) - loc(i)))
    for i in range(8):
        b.assert_zero(sn * nxt(PREV + i))
    rule("capacity")
    for i in range(8, 12):
        b.assert_zero(sc * (nxt(i) - loc(i)))
    for i in range(8, 12):
        b.assert_zero(sn * nxt(i))
    rule("contiguous")
    b.assert_zero(sc * (1 - act))
    b.assert_zero(sc * (nxt(CHAIN) - chain))
    rule("counters")
    b.assert_zero(sc * (nxt(NABS) - nabs - sw))
    b.assert_zero(sc * (nxt(NCH) - nch - sq))
    rule("squeezed_dry")
    b.assert_zero(spare * (nxt(ACT) - nxt(W)) * (1 - q[0]))
    # 7. the bus
    rule("bus")
    beta, gamma = X2(b.chal(0), b.chal(1)), X2(b.chal(2), b.chal(3))
    g2 = gamma * gamma
    g3, g4 = g2 * gamma, g2 * g2
    absorbed = nabs + sw

    def d_obs(i):
        return beta + chain + gamma * (nabs + i) + g2 * loc(MSG + i) + g4 * TAG_OBS

    def d_chal(i):
        return beta + chain + gamma * (nch + (7 - i)) + g2 * absorbed + g3 * loc(OUT + i) + g4 * TAG_CHAL

    hsum = X2(0, 0)
    for e in range(4):
        da, db = d_obs(2 * e), d_obs(2 * e + 1)
        h = X2(b.aux(2 * e), b.aux(2 * e + 1))
        b.assert_zero_x2(h * da * db + db * w[2 * e] + da * w[2 * e + 1])
        hsum = hsum + h
    for e in range(4):
        da, db = d_chal(2 * e), d_chal(2 * e + 1)
        h = X2(b.aux(8 + 2 * e), b.aux(9 + 2 * e))
        b.assert_zero_x2(h * da * db - db * q[2 * e] - da * q[2 * e + 1])
        hsum = hsum + h
    rule("running_sum")
    z, zn = X2(b.aux(16), b.aux(17)), X2(b.aux_nxt(16), b.aux_nxt(17))
    b.assert_zero_x2(zn - z - hsum * first + X2(b.apub(0), b.apub(1)))
    return b


def rule_of(k):
    """the name of the rule constraint k belongs to"""
    if not RULES:
        builder()
    return max((first, name) for name, first in RULES.items() if first <= k)[1]


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


# ---- the plan of a chain: which duplex absorbs how many words and yields how many challenges
def plan(ops):
    """ops: run lengths, observe count, challenge count, observe count, ... -> [(k, q)] per duplex.  A counter machine of the duplex
    challenger: an observation fills the buffer and voids the output, a full buffer or a challenge on a non-empty buffer or an
    empty output duplexes.  Words left in the buffer at the end are never absorbed: refused."""
    n_in, n_out, blocks = 0, 0, []
    for j, count in enumerate(ops):
        for _ in range(int(count)):
            if j % 2 == 0:
                n_out, n_in = 0, n_in + 1
                if n_in == 8:
                    blocks.append([8, 0])
                    n_in, n_out = 0, 8
            else:
                if n_in > 0 or n_out == 0:
                    assert blocks or n_in > 0, "the first operation draws from an empty sponge"
                    blocks.append([n_in, 0])
                    n_in, n_out = 0, 8
                blocks[-1][1] += 1
                n_out -= 1
    assert n_in == 0, "the chain ends on observed words that no duplex absorbs"
    return [tuple(b) for b in blocks]


def run_blocks(chain, specs, words):
    """the blocks of one chain from per-block specs dict(k, q[, qmask][, start]) -> (blocks, challenges [(absorbed, value)]).  A
    spec with `start` begins again from the zero state with both counters at zero (block 0 always does); qmask: the Q cells,
    default the last q.  Forgeries pass their own specs; honest chains those of plan()."""
    state, prev, nabs, nch, pos, blocks, chals = [0] * 12, [0] * 8, 0, 0, 0, [], []
    for j, sp in enumerate(specs):
        k, start = sp["k"], int(sp.get("start", j == 0))
        qmask = list(sp.get("qmask", [int(i >= 8 - sp["q"]) for i in range(8)]))
        if start:
            state, prev, nabs, nch = [0] * 12, [0] * 8, 0, 0
        state[:k] = [int(v) for v in words[pos: pos + k]]
        assert len(words) - pos >= k
        pos += k
        rows, out = M.block_rows(state)
        blocks.append(dict(rows=rows, msg=list(state[:8]), w=[int(i < k) for i in range(8)], q=qmask, prev=list(prev), out=list(out[:8]), chain=int(chain), act=1, start=start,
                           nabs=nabs, nch=nch))
        t = 0
        for i in range(7, -1, -1):
            if qmask[i]:
                chals.append((nabs + k, int(out[i])))
                t += 1
        nabs, nch, state, prev = nabs + k, nch + t, list(out), list(out[:8])
    assert pos == len(words)
    return blocks, chals


def chain_blocks(chain, ops, words):
    return run_blocks(chain, [dict(k=k, q=q) for k, q in plan(ops)], words)


_idle = None


def idle_block():
    global _idle
    if _idle is None:
        rows, out = M.block_rows([0] * 12)
        _idle = dict(rows=rows, msg=[0] * 8, w=[0] * 8, q=[0] * 8, prev=[0] * 8, out=list(out[:8]), chain=0, act=0, start=0, nabs=0, nch=0)
    return _idle


def log_rows(n_blocks):
    return max(5, (32 * n_blocks - 1).bit_length())


def assemble(blocks, log_n):
    """blocks (dicts of run_blocks) followed by idle blocks -> trace [93][2^log_n]"""
    n = 1 << log_n
    assert 32 * len(blocks) <= n, "the blocks do not fit"
    tr = np.zeros((COLS, n), dtype=np.uint64)
    for b in range(n // 32):
        blk = blocks[b] if b < len(blocks) else idle_block()
        sl = slice(32 * b, 32 * b + 32)
        tr[:48, sl] = blk["rows"]
        for col, key in ((MSG, "msg"), (W, "w"), (OUT, "out"), (Q, "q"), (PREV, "prev")):
            for i in range(8):
                tr[col + i, sl] = blk[key][i]
        for col, key in ((CHAIN, "chain"), (ACT, "act"), (START, "start"), (NABS, "nabs"), (NCH, "nch")):
            tr[col, sl] = blk[key]
    return tr


def statement_digest(claims):
    """claims: [(words, [(absorbed, value)])] per chain -> hash_n_to_hash_no_pad(n, per chain n_obs and n_chal, per chain the
    observed words, per chain (absorbed, value) of every challenge)"""
    w = [len(claims)]
    for words, chals in claims:
        w += [len(words), len(chals)]
    for words, _ in claims:
        w += [int(v) for v in words]
    for _, chals in claims:
        for a, v in chals:
            w += [int(a), int(v)]
    return [int(v) for v in O.hash_no_pad(np.array(w, dtype=np.uint64))]


def ref_table(chains, log_n=None):
    """chains: [(ops, words)] -> (trace, the 4 public inputs, claims [(words, [(absorbed, value)])])"""
    blocks, claims = [], []
    for c, (ops, words) in enumerate(chains):
        bl, chals = chain_blocks(c, ops, words)
        blocks += bl
        claims.append(([int(v) for v in words], chals))
    return assemble(blocks, log_rows(len(blocks)) if log_n is None else log_n), statement_digest(claims), claims


def _bus(chal):
    beta, gamma = S.ExtS(chal[0], chal[1]), S.ExtS(chal[2], chal[3])
    g2 = gamma * gamma
    return beta, gamma, g2, g2 * gamma, g2 * g2


def d_obs(bus, chain, position, word):
    beta, gamma, g2, _, g4 = bus
    return beta + int(chain) + gamma * int(position) + g2 * int(word) + g4 * TAG_OBS


def d_chal(bus, chain, ordinal, absorbed, word):
    beta, gamma, g2, g3, g4 = bus
    return beta + int(chain) + gamma * int(ordinal) + g2 * int(absorbed) + g3 * int(word) + g4 * TAG_CHAL


def block_helpers(bus, cell):
    """the eight helpers of one block from its shape cells (cell(column) -> int)"""
    if not cell(ACT):
        return [S.ExtS(0)] * N_HELP
    chain, nabs, nch = cell(CHAIN), cell(NABS), cell(NCH)
    absorbed = nabs + sum(cell(W + i) for i in range(8))
    hs = []
    for e in range(4):
        hs.append((d_obs(bus, chain, nabs + 2 * e, cell(MSG + 2 * e)).inv() * cell(W + 2 * e) + d_obs(bus, chain, nabs + 2 * e + 1, cell(MSG + 2 * e + 1)).inv() * cell(W + 2 * e + 1)) * (P - 1))
    for e in range(4):
        hs.append(d_chal(bus, chain, nch + 7 - 2 * e, absorbed, cell(OUT + 2 * e)).inv() * cell(Q + 2 * e)
                  + d_chal(bus, chain, nch + 6 - 2 * e, absorbed, cell(OUT + 2 * e + 1)).inv() * cell(Q + 2 * e + 1))
    return hs


def gen_aux(trace, chal, pub=None):
    """-> (aux [18][n]: eight helpers (constant over a block), Z; [S / n])"""
    n = trace.shape[1]
    bus = _bus(chal)
    aux = np.zeros((AUX, n), dtype=np.uint64)
    incs = []
    for b in range(n // 32):
        row = 32 * b
        hs = block_helpers(bus, lambda j: int(trace[j, row]))
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
        aux[16, i], aux[17, i] = z.a, z.b
        if i % 32 == 0:
            z = z + incs[i // 32]
        z = z - apub
    return aux, [apub.a, apub.b]


def outside_sum(chal, claims):
    """what the party outside the table adds: per chain every absorbed word SENT (-), every challenge RECEIVED (+)"""
    bus, tot = _bus(chal), S.ExtS(0)
    for c, (words, chals) in enumerate(claims):
        for i, v in enumerate(words):
            tot = tot - d_obs(bus, c, i, v).inv()
        for j, (a, v) in enumerate(chals):
            tot = tot + d_chal(bus, c, j, a, v).inv()
    return tot


# ---- the transcript of a proof, recorded from the reference verifier's own challenger
class _Recorder(O.Challenger):
    log = None

    def observe(self, v):
        v = np.atleast_1d(np.asarray(v, dtype=np.uint64)).reshape(-1)
        _Recorder.log.append(("obs", [int(x) for x in v]))
        super().observe(v)

    def challenge(self):
        c = super().challenge()
        _Recorder.log.append(("chal", c))
        return c


def record(proof, cfg=None, ext_chal=None):
    """runs oracle.stark_ref.verify on the proof with its challenger wrapped -> (ops: run lengths, words: everything absorbed in
    order, values: every challenge in order).  The order is stark_ref's, nothing is restated."""
    _Recorder.log, keep = [], O.Challenger
    O.Challenger = _Recorder
    try:
        S.verify(proof, cfg, ext_chal=ext_chal)
    finally:
        O.Challenger = keep
    ops, words, values = [0], [], []
    for kind, v in _Recorder.log:
        if (kind == "chal") != (len(ops) % 2 == 0):
            ops.append(0)
        if kind == "obs":
            ops[-1] += len(v)
            words += v
        else:
            ops[-1] += 1
            values.append(v)
    return ops, words, values


# ---- the group: one table on its bus, the verifier outside
def table_log(log_n, cfg=None):
    """the rows (log2) a table of at least 2^log_n rows is proven at: the next size whose FRI plan leaves a final polynomial"""
    cfg = dict(S.DEFAULT_CFG, **(cfg or {}))
    while True:
        d = log_n
        while d > cfg["final_poly_bits"] and d + cfg["rate_bits"] - cfg["arity_bits"] >= cfg["cap_height"]:
            d -= cfg["arity_bits"]
        if d >= 0:
            return log_n
        log_n += 1


def prove_table(trace, pub, cfg=None):
    """the reference prover on the restatement under the challenges of a table alone on its bus (id word REF_ID)"""
    chal = S.shared_challenges_n([(pub, R.trace_cap(trace, cfg))], 4)
    return S.prove(air(), trace, pub, cfg, chal_hook=lambda p, cap: chal)


def wrap(proof, claims):
    """the table proof as a blob of the product, with the compiled AIR's id in its id word"""
    p = np.array(proof, dtype=np.uint64)
    p[1] = AIR_ID
    req = [len(claims)]
    for words, chals in claims:
        req += [len(words), len(chals)]
        for a, v in chals:
            req += [int(a), int(v)]
    return np.concatenate([np.array([MAGIC] + req + [p.size], dtype=np.uint64), p])


def unwrap(blob):
    """-> (the table proof with the reference registry's id, where it starts in the blob)"""
    n, at = int(blob[1]), 2
    for _ in range(n):
        at += 2 + 2 * int(blob[at + 1])
    assert int(blob[0]) == MAGIC and int(blob[at]) == blob.size - at - 1
    p = np.array(blob[at + 1:], dtype=np.uint64)
    p[1] = REF_ID
    return p, at + 1


def group(proofs, cfg=None, ext_chals=None):
    """the reference group of inner proofs (made under the reference configuration cfg) -> dict(chains [(ops, words)], claims, trace,
    pub, table: the table proof, blob)"""
    ext_chals = ext_chals or [None] * len(proofs)
    chains = []
    for p, e in zip(proofs, ext_chals):
        ops, words, values = record(p, cfg, e)
        chains.append((ops, words))
    blocks = sum(len(plan(ops)) for ops, _ in chains)
    trace, pub, claims = ref_table(chains, table_log(log_rows(blocks), cfg))
    table = prove_table(trace, pub, cfg)
    return dict(chains=chains, claims=claims, trace=trace, pub=pub, table=table, blob=wrap(table, claims))


# ---- the synthetic chains both tiers use: name -> ops.  Every branch of the challenger: a challenge on a full buffer (absorbed = 0
# mod 8: no block of its own) and on one word (= 1 mod 8); 1, 8, 9, 16, 17 challenges in a row (9 and 17 need absorb-nothing blocks)
SYNTH = {
    "absorbed_8_then_1": [8, 1],
    "absorbed_9_then_1": [9, 1],
    "one_block": [3, 2],
    "draw_8": [5, 8, 2, 1],
    "draw_9": [5, 9, 2, 1],
    "draw_16": [16, 16, 1, 1],
    "draw_17": [7, 17, 9, 3],
    "interleaved": [1, 1, 1, 1, 8, 2, 15, 0, 1, 4],
    "zero_runs": [4, 0, 4, 3, 0, 2, 12, 1],
}


def synth_words(ops, seed):
    n = sum(int(v) for v in ops[0::2])
    rng = np.random.default_rng(seed)
    w = [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]
    if n >= 3:
        w[0], w[1], w[2] = P - 1, 0, 1
    return w


def synth_chains(names):
    return [(SYNTH[name], synth_words(SYNTH[name], 100 + k)) for k, name in enumerate(names)]


def filler(n_blocks, seed=9):
    """a chain of exactly n_blocks blocks: full absorptions, one challenge at the end"""
    ops = [8 * n_blocks, 1]
    return ops, synth_words(ops, seed)
