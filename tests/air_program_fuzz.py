"""TEST INFRASTRUCTURE: seeded generators of constraint programs (include/vx.h `vx_air_program`) that no builder would write, for
the differential tests of the three evaluators of the format -- the GPU interpreter k_quotient_prog, the host interpreter
air_program_eval and the reference reading oracle/air_program.py.  No tests here.

raw_program     straight-line instruction words over the whole register file: aliased destinations, values kept live across
                assertions, register 31, edge-valued constants.  Evaluated on ARBITRARY data (vx_quotient_eval needs no witness).
relabel         renames the registers of a program by a permutation of 0..31 (the semantics do not change).
recurrence_air  a random SATISFIABLE AIR with its trace and public inputs, for whole proofs.
special_lde     [cols][N] canonical words, a third of them from the edge list of the fused multiply.

Everything is deterministic in its seed; RAW_CASES / RECURRENCE_CASES / SNIPPETS are the exact lists the CPU tier
(test_air_program_fuzz.py, which asserts their coverage) and the GPU tier (test_gpu_air_program_fuzz.py) share."""
import numpy as np

from test_gpu_field_mul_edges import EDGES

P = 2**64 - 2**32 + 1
LOC, NXT, PER, PUB, CONST, ADD, SUB, MUL, ASSERT, ASSERT_TRANSITION, ASSERT_FIRST, ASSERT_LAST = range(1, 13)
ASSERTS = (ASSERT, ASSERT_TRANSITION, ASSERT_FIRST, ASSERT_LAST)
MAX_REGS = 32
N_RANDOM_CONSTS = 16


def insn(op, d=0, a=0, b=0):
    return op | (d << 8) | (a << 16) | (b << 32)


def decode(w):
    w = int(w)
    return w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFFFF, (w >> 32) & 0xFFFF


def special_words(rng, n):
    """n uniform canonical words, one third of them replaced by draws from the edge list."""
    v = rng.integers(0, P, size=n, dtype=np.uint64)
    edges = np.array(EDGES, dtype=np.uint64)
    return np.where(rng.integers(0, 3, size=n) == 0, edges[rng.integers(0, edges.size, size=n)], v)


def special_lde(rng, cols, N):
    """[cols][N] words for vx_quotient_eval: uniform, a third from the edge list; point 0 of every column is p - 1, point 1 is 0."""
    a = special_words(rng, cols * N).reshape(cols, N)
    a[:, 0], a[:, 1] = P - 1, 0
    return np.ascontiguousarray(a)


def periodic_columns(rng, period_logs):
    return [[int(v) for v in special_words(rng, 1 << pl)] for pl in period_logs]


def raw_program(rng, cols, n_periodic, n_public, n_code, n_regs=MAX_REGS):
    """-> (code uint64[n_code], consts uint64[], n_constraints).  The degree of every register is tracked as vx_air_register tracks
    it (columns and periodic columns 1, public inputs and constants 0, MUL adds, ADD / SUB take the larger), so registration
    accepts the program: a MUL that would pass degree 3 becomes an ADD, ASSERT takes degree <= 3, the other three <= 2.
    Registers are never recycled: a value stays readable until an instruction happens to write its register again."""
    consts = [int(e) for e in EDGES] + [int(v) for v in rng.integers(0, P, size=N_RANDOM_CONSTS, dtype=np.uint64)]
    deg = [-1] * n_regs
    code, n_constraints, last_asserted = [], 0, None

    def pick_hi(n):  # an index below n, the last one a quarter of the time
        return n - 1 if rng.integers(0, 4) == 0 else int(rng.integers(0, n))

    def load():
        kinds = [LOC, NXT, CONST] + ([PER] if n_periodic else []) + ([PUB] if n_public else [])
        op = kinds[int(rng.integers(0, len(kinds)))]
        d = int(rng.integers(0, n_regs))
        a = {LOC: lambda: pick_hi(cols), NXT: lambda: pick_hi(cols), PER: lambda: int(rng.integers(0, n_periodic)),
             PUB: lambda: pick_hi(n_public), CONST: lambda: int(rng.integers(0, len(consts)))}[op]()
        deg[d] = 1 if op in (LOC, NXT, PER) else 0
        code.append(insn(op, d, a))
        return d

    while len(code) < n_code:
        live = [r for r in range(n_regs) if deg[r] >= 0]
        u = rng.random()
        if len(live) < 2 or u < 0.3:
            d = load()
        elif u < 0.8:
            a = live[int(rng.integers(0, len(live)))]
            b = a if rng.integers(0, 4) == 0 else live[int(rng.integers(0, len(live)))]
            d = a if rng.integers(0, 4) == 0 else int(rng.integers(0, n_regs))
            op = (ADD, SUB, MUL)[int(rng.integers(0, 3))]
            if op == MUL and deg[a] + deg[b] > 3:
                op = ADD
            deg[d] = deg[a] + deg[b] if op == MUL else max(deg[a], deg[b])
            code.append(insn(op, d, a, b))
        else:
            kind = ASSERTS[int(rng.integers(0, 4))]
            lim = 3 if kind == ASSERT else 2
            fit = [r for r in live if deg[r] <= lim]
            if not fit:
                d = load()
            else:
                # a quarter of the assertions read the register the previous assertion read, if nothing has written it since
                again = last_asserted is not None and deg[last_asserted] <= lim and rng.integers(0, 4) == 0
                a = last_asserted if again else fit[int(rng.integers(0, len(fit)))]
                code.append(insn(kind, 0, a))
                n_constraints += 1
                last_asserted = a
                continue
        if d == last_asserted:
            last_asserted = None
    return np.array(code, dtype=np.uint64), np.array(consts, dtype=np.uint64), n_constraints


def relabel(code, perm):
    """The same program with register r renamed perm[r]: d of loads and arithmetic, a / b of arithmetic, a of assertions."""
    out = []
    for w in code:
        op, d, a, b = decode(w)
        if op in (ADD, SUB, MUL):
            out.append(insn(op, perm[d], perm[a], perm[b]))
        elif op in ASSERTS:
            out.append(insn(op, 0, perm[a]))
        else:
            out.append(insn(op, perm[d], a))
    return np.array(out, dtype=np.uint64)


def registers_written(code):
    return sorted({decode(w)[1] for w in code if decode(w)[0] not in ASSERTS})


def permutation_onto_31(rng, code):
    """A random permutation of 0..31 that sends one of the registers the code writes to register 31."""
    perm = [int(v) for v in rng.permutation(MAX_REGS)]
    used = registers_written(code)
    u = used[int(rng.integers(0, len(used)))]
    j = perm.index(MAX_REGS - 1)
    perm[u], perm[j] = perm[j], perm[u]
    return perm


def coverage(code):
    """What a program exercises, as the CPU tier asserts it: the opcodes present, whether register 31 is written, whether some
    arithmetic instruction has d == a / a == b / d == a == b, a MUL d, a, a with d != a, and whether two assertions read one register with no write to it in between."""
    ops, d_eq_a, a_eq_b, twice, in_place, square = set(), False, False, False, False, False
    asserted = set()  # registers asserted since their last write
    for w in code:
        op, d, a, b = decode(w)
        ops.add(op)
        if op in (ADD, SUB, MUL):
            d_eq_a |= d == a
            a_eq_b |= a == b
            in_place |= d == a == b               # ADD d, d, d and its kin
            square |= op == MUL and a == b != d   # MUL d, a, a
        if op in ASSERTS:
            twice |= a in asserted
            asserted.add(a)
        else:
            asserted.discard(d)
    return dict(ops=ops, reg31=MAX_REGS - 1 in registers_written(code), d_eq_a=d_eq_a, a_eq_b=a_eq_b, asserted_twice=twice, in_place=in_place, square=square)


# ---- the raw-program cases of the GPU tier: (seed, log_n, rate_bits, cols, n_public, period logs, n_code, n_regs)
RAW_CASES = [
    (101, 2, 1, 1, 0, (0, 2), 400, 6),                # N = 8 < block; smallest table; six registers, then relabelled onto 32
    (102, 3, 3, 4, 1, (0,), 400, 17),                 # N = 64 = one wave; seventeen registers, then relabelled
    (103, 5, 2, 7, 64, (0, 5), 400, 32),              # N = 128; the public-input limit
    (104, 6, 1, 7, 5, (0, 6, 6), 400, 32),            # host-interpolated periods only; period = n
    (105, 7, 1, 5, 3, (0, 6, 7, 7), 400, 32),         # both sides of the `pl <= 6` split in one table; N = 256 = one block
    (106, 8, 2, 33, 9, (0, 6, 7, 8), 400, 32),        # table offsets at rate_bits 2
    (107, 9, 3, 300, 17, (0, 6, 7, 9), 400, 32),      # wide rows; column * N indexing; rate_bits 3
    (108, 9, 1, 3, 2, (), 20000, 32),                 # a long scalar-fetched program
]
RAW_IDS = ["s%d-L%d-r%d-c%d-pub%d-%dinsn" % (c[0], c[1], c[2], c[3], c[4], c[6]) for c in RAW_CASES]


def other_rate(r):
    """The second rate_bits every raw case is evaluated at."""
    return r % 3 + 1


class RawCase:
    """One row of RAW_CASES materialised: the program, its variants (the relabelled one when it uses fewer than 32 registers),
    periodic columns, public inputs, and the challenge pairs / LDE data of the GPU comparison -- all from the case's seed."""

    def __init__(self, case):
        self.seed, self.log_n, self.rate_bits, self.cols, self.n_public, self.period_logs, self.n_code, self.n_regs = case
        rng = np.random.default_rng(self.seed)
        self.code, self.consts, self.n_constraints = raw_program(rng, self.cols, len(self.period_logs), self.n_public, self.n_code, self.n_regs)
        self.periodic = periodic_columns(rng, self.period_logs)
        self.public = [int(v) for v in special_words(rng, self.n_public)]
        self.variants = [(self.code, self.n_regs)]
        if self.n_regs < MAX_REGS:
            self.variants.append((relabel(self.code, permutation_onto_31(rng, self.code)), MAX_REGS))
        self.alphas = [[P - 1, 2**32], [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)]]
        self.lde_seed = int(rng.integers(0, 2**31))

    def lde(self, rate_bits):
        return special_lde(np.random.default_rng([self.lde_seed, rate_bits]), self.cols, 1 << (self.log_n + rate_bits))


# ---- hand-assembled aliasing snippets (two columns): (name, code, consts, n_regs)
SNIPPETS = [
    ("add_mul_in_place", [insn(LOC, 0, 0), insn(ADD, 0, 0, 0), insn(MUL, 0, 0, 0), insn(ASSERT, 0, 0)], [], 1),
    ("r31_asserted_three_times", [insn(LOC, 31, 0), insn(LOC, 0, 1), insn(SUB, 31, 31, 0), insn(ASSERT_TRANSITION, 0, 31), insn(ASSERT_FIRST, 0, 31),
                                  insn(ASSERT_LAST, 0, 31)], [], 32),
    ("const_2_63_squared_twice", [insn(CONST, 5, 0), insn(MUL, 5, 5, 5), insn(MUL, 5, 5, 5), insn(LOC, 6, 1), insn(MUL, 6, 6, 5), insn(ASSERT, 0, 6)], [2**63], 7),
]


# ---- random satisfiable AIRs
# expressions as nested tuples -- ("loc", j) ("per", q) ("pub", i) ("const", v) ("add" | "sub" | "mul", x, y) -- lowered twice:
# to the builder's Expr (a tuple used twice becomes ONE Expr object, which the builder evaluates once) and to Python integers
def _to_expr(b, t, memo):
    if id(t) not in memo:
        if t[0] in ("add", "sub", "mul"):
            x, y = _to_expr(b, t[1], memo), _to_expr(b, t[2], memo)
            memo[id(t)] = x + y if t[0] == "add" else x - y if t[0] == "sub" else x * y
        else:
            memo[id(t)] = getattr(b, t[0])(t[1])
    return memo[id(t)]


def _eval(t, loc, per, pub):
    if t[0] in ("add", "sub", "mul"):
        x, y = _eval(t[1], loc, per, pub), _eval(t[2], loc, per, pub)
        return (x + y if t[0] == "add" else x - y if t[0] == "sub" else x * y) % P
    return {"loc": loc, "per": per, "pub": pub}[t[0]][t[1]] if t[0] != "const" else t[1]


def _random_expr(rng, cols, n_per):
    """A random expression of degree <= 2 over the local row, the periodic columns, the first `cols` public inputs and constants."""
    def deg1():
        if n_per and rng.integers(0, 3) == 0:
            return ("per", int(rng.integers(0, n_per)))
        return ("loc", int(rng.integers(0, cols)))

    def deg0():
        return ("pub", int(rng.integers(0, cols))) if rng.integers(0, 2) else ("const", int(EDGES[int(rng.integers(0, len(EDGES)))]))

    def term():
        k = int(rng.integers(0, 6))
        if k == 0:
            return ("mul", deg1(), deg1())
        if k == 1:
            return ("mul", deg1(), deg0())
        if k == 2:
            return deg1()
        if k == 3:
            return deg0()
        if k == 4:
            u = ("add", deg1(), deg0())
            return ("mul", u, u)  # a shared sub-expression, squared
        return ("mul", ("add", deg1(), deg0()), ("sub", deg1(), deg0()))

    e = term()
    for _ in range(int(rng.integers(0, 4))):
        e = ("add" if rng.integers(0, 2) else "sub", e, term())
    return e


def recurrence_air(ap, seed, log_n, bump=0):
    """-> (builder, trace [cols][2^log_n], public inputs): 1-6 columns, 0-3 periodic columns of periods in {1, ..., 2^log_n}; per
    column k a random E_k of degree <= 2 with
        first row:  loc k = pub k          between rows:  nxt k = E_k          last row:  loc k = pub(cols + k)
    and one degree-3 constraint that holds on EVERY row (the wrap-around row included):
        s (s - 1) (x_0 - c)  with periodic column 0 a 0/1 selector,  or
        t (t - 1) (t - 2)    with t the last column, fed from a periodic column with values in {0, 1, 2} (t' = per q) -- or, without
                             periodic columns, alternating between 1 and 2 (t' = 3 - t).
    The trace iterates the recurrence in Python integers; its last row goes into the public inputs.  bump: added to E_0 (the twin
    program of the rejection test; the random draws do not depend on it)."""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    cols, n_per = int(rng.integers(1, 7)), int(rng.integers(0, 4))
    periodic = periodic_columns(rng, [int(rng.integers(0, log_n + 1)) for _ in range(n_per)])
    variant = "alternate" if n_per == 0 else ("selector", "fed")[int(rng.integers(0, 2))]
    E = [_random_expr(rng, cols, n_per) for _ in range(cols)]
    row0 = [int(v) for v in special_words(rng, cols)]
    t = cols - 1
    if variant == "selector":
        periodic[0] = [int(v) for v in rng.integers(0, 2, size=len(periodic[0]))]
        c3 = int(EDGES[int(rng.integers(0, len(EDGES)))])
        s = ("per", 0)
        cubic = ("mul", ("mul", s, ("sub", s, ("const", 1))), ("sub", ("loc", 0), ("const", c3)))
    else:
        if variant == "fed":
            q = int(rng.integers(0, n_per))
            periodic[q] = [int(v) for v in rng.integers(0, 3, size=len(periodic[q]))]
            E[t], row0[t] = ("per", q), int(rng.integers(0, 3))
        else:
            E[t], row0[t] = ("sub", ("const", 3), ("loc", t)), int(rng.integers(1, 3))
        x = ("loc", t)
        cubic = ("mul", ("mul", x, ("sub", x, ("const", 1))), ("sub", x, ("const", 2)))
    if bump:
        E[0] = ("add", E[0], ("const", bump))
    trace = np.zeros((cols, n), dtype=np.uint64)
    row = row0
    for i in range(n):
        trace[:, i] = row
        per = [col[i % len(col)] for col in periodic]
        row = [_eval(E[k], row, per, row0) for k in range(cols)]
    public = row0 + [int(v) for v in trace[:, n - 1]]

    b = ap.AirBuilder(cols, 2 * cols, periodic=periodic)
    memo = {}
    cubic_at = int(rng.integers(0, cols + 1))
    for k in range(cols):
        if k == cubic_at:
            b.assert_zero(_to_expr(b, cubic, memo))
        b.assert_first(b.loc(k) - b.pub(k))
        b.assert_transition(b.nxt(k) - _to_expr(b, E[k], memo))
        b.assert_last(b.loc(k) - b.pub(cols + k))
    if cubic_at == cols:
        b.assert_zero(_to_expr(b, cubic, memo))
    b.cubic_kind = variant  # which degree-3 constraint this AIR got (the CPU tier asserts that the seed list has all three)
    return b, trace, public


# (seed, log_n) of the proofs both tiers make; the seeds of RATE_SEEDS are proven at the higher rates too
RECURRENCE_CASES = [(201, 3), (214, 3), (208, 3), (204, 4), (206, 4), (230, 4), (203, 5), (223, 5), (215, 5), (217, 6), (211, 6), (229, 6)]
RATE_SEEDS = (201, 206, 217)


class RecurrenceCase:
    """One proof case: the builder's program relabelled through a permutation that puts a used register on 31 (so it registers with
    n_regs = 32), and its twin (E_0 + 1) relabelled the same way."""

    def __init__(self, ap, seed, log_n):
        self.seed, self.log_n = seed, log_n
        self.builder, self.trace, self.public = recurrence_air(ap, seed, log_n)
        code, self.consts, _ = self.builder.assemble()
        perm = permutation_onto_31(np.random.default_rng([seed, 31]), code)
        self.code = relabel(code, perm)
        twin, _, _ = recurrence_air(ap, seed, log_n, bump=1)
        twin_code, self.twin_consts, _ = twin.assemble()
        self.twin_code = relabel(twin_code, perm)
        self.cols, self.n_public, self.periodic = self.builder.cols, self.builder.n_public, self.builder.periodic
