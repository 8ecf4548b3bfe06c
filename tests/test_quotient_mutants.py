"""What the arbitrary data of test_gpu_quotient_arbitrary.py can tell apart, measured on the CPU: for each bus table (the AIRs
whose restatement is a constraint program) every single-instruction MUTANT of the program is evaluated by
oracle/stark_ref.quotient_values on that data at log_n 5, rate_bits 1 (64 points), and a mutant SURVIVES when every quotient value
equals the original program's.  A compiled `eval` with the same mistake would survive the GPU comparison exactly then.

The mutants of instruction k:
  col+1     LOC / NXT a      -> the same load of column a + 1 (the last column wraps to column 0)
  loc<->nxt LOC a <-> NXT a
  const+1   CONST c          -> the constant c + 1
  add<->sub ADD <-> SUB

Conditions: no col+1 and no loc<->nxt mutant survives; the add<->sub / const+1 survivors are exactly those listed in EQUIVALENT, each
with the reason it is the same polynomial.  Anything else is a failure of the data generator.

test_an_honest_trace_leaves_column_mistakes_unseen documents the gap the arbitrary-data test closes: on the honest trace of the
Transcript proof-parity test (test_gpu_transcript.test_the_table_proof_equals_the_reference_prover) col+1 mutants DO survive --
reading the neighbour of a block-constant, prefix-flag or copied cell changes nothing there.

Every mutant is evaluated (k = 1, no sub-sampling): a mutant re-evaluates only the instructions that depend on the mutated one and
adds the change of each touched constraint, weighted as ConstraintConsumer weighs it, to the original accumulators -- the same
field elements as a full evaluation, which CHECK_EVERY-th mutants and all survivors are checked against by running
quotient_values on the mutated program itself."""
import heapq
from collections import defaultdict

import numpy as np
import pytest

import air_program_fuzz as Z
import quotient_arbitrary as QA
from oracle import oracle as O
from oracle import stark_ref as S
from oracle.air_program import APUB, CHAL, ProgramAir

P = QA.P
LOC, NXT, PER, PUB, CONST, ADD, SUB, MUL = Z.LOC, Z.NXT, Z.PER, Z.PUB, Z.CONST, Z.ADD, Z.SUB, Z.MUL
ASSERT, ASSERT_TRANSITION, ASSERT_FIRST, ASSERT_LAST = Z.ASSERTS
LOG_N, RATE_BITS = 5, 1
CHECK_EVERY = 101

# AIR -> {instruction index: why ADD <-> SUB there is the same polynomial}.  No const+1 mutant survives anywhere.  The test also folds
# constants through the program and confirms that the second operand of each listed instruction is the constant 0.
ADD_0 = "adds a register that is the constant 0 (a message field or counter offset of 0): x + 0 = x - 0"
MUL_0 = "adds a challenge times a register that is the constant 0 (a bus-message field that is 0 in this message): x + g 0 = x - g 0"
EQUIVALENT = {
    "VX_AIR_LEAF_SPONGE": {2591: ADD_0, 2688: ADD_0},
    "VX_AIR_FRI_FOLD": {1661: MUL_0, 1703: MUL_0, 1767: MUL_0, 1809: MUL_0},
    "VX_AIR_LEAF_SPONGE_SET": {2609: ADD_0, 2725: ADD_0},
    "VX_AIR_LEAF_NOOP": {286: MUL_0, 326: MUL_0, 392: MUL_0, 432: MUL_0},
    "VX_AIR_TRANSCRIPT": {3135: ADD_0, 3223: ADD_0, 4628: ADD_0, 4750: ADD_0},
}


def mutants(air):
    """-> [(kind, instruction index, mutated instruction word)]; a const+1 word reads constant index len(consts), see mutated()"""
    cols, out = QA.n_columns(air), []
    for k, w in enumerate(air.code):
        op, d, a, b = Z.decode(w)
        if op in (LOC, NXT):
            out.append(("col+1", k, Z.insn(op, d, (a + 1) % cols)))
            out.append(("loc<->nxt", k, Z.insn(LOC + NXT - op, d, a)))
        elif op == CONST:
            out.append(("const+1", k, Z.insn(CONST, d, len(air.consts))))
        elif op in (ADD, SUB):
            out.append(("add<->sub", k, Z.insn(ADD + SUB - op, d, a, b)))
    return out


def mutated(air, k, word):
    """the program with instruction k replaced, as an AIR of the reference prover"""
    code = list(air.code)
    code[k] = word
    consts = list(air.consts)
    if Z.decode(word)[0] == CONST:
        consts.append((air.consts[Z.decode(air.code[k])[2]] + 1) % P)
    return ProgramAir(air.ID, air.COLS, air.PUB, code, consts, air.periodic_values(), air.AUX, air.CHAL, air.AUXPUB)


class Run:
    """One evaluation of a program on [cols][N] values with the value of every instruction kept, so that a mutant re-evaluates only
    what depends on the mutated instruction."""

    def __init__(self, air, lde, pub, chal, apub, alphas, log_n=LOG_N, r=RATE_BITS):
        self.air, self.args = air, (pub, alphas, log_n, r, chal, apub)
        self.lde = lde
        n, N = 1 << log_n, lde.shape[1]
        assert N == n << r
        self.full = lambda x: np.full(N, int(x) % P, dtype=np.uint64)
        self.loads = {LOC: lde, NXT: np.roll(lde, -(1 << r), axis=1), PER: [S.periodic_on_lde(v, log_n, r) for v in air.periodic_values()],
                      PUB: [self.full(x) for x in pub], CHAL: [self.full(x) for x in chal], APUB: [self.full(x) for x in apub]}
        code = air.code
        self.vals, self.srcs, self.users, self.cons = [None] * len(code), [()] * len(code), defaultdict(list), {}
        cur = {}
        for k, w in enumerate(code):
            op, d, a, b = Z.decode(w)
            if op in (ADD, SUB, MUL):
                self.srcs[k] = (cur[a], cur[b])
                self.vals[k] = self.arith(op, self.vals[cur[a]], self.vals[cur[b]])
                cur[d] = k
            elif op in Z.ASSERTS:
                self.srcs[k] = (cur[a],)
                self.cons[k] = len(self.cons)
            else:
                self.vals[k] = self.load(op, a)
                cur[d] = k
            for s in set(self.srcs[k]):
                self.users[s].append(k)
        # the weight of constraint j in accumulator kk: alpha_kk^(K - 1 - j) times the selector of its kind (starky's ConstraintConsumer)
        w_N, last, ninv = O.root(log_n + r), pow(O.root(log_n), P - 2, P), pow(n, P - 2, P)
        xs = [S.G * pow(w_N, i, P) % P for i in range(N)]
        zh = [(pow(x, n, P) - 1) % P for x in xs]
        sel = {ASSERT: [1] * N, ASSERT_TRANSITION: [(x - last) % P for x in xs],
               ASSERT_FIRST: [z * ninv % P * pow((x - 1) % P, P - 2, P) % P for x, z in zip(xs, zh)],
               ASSERT_LAST: [z * ninv % P * last % P * pow((x - last) % P, P - 2, P) % P for x, z in zip(xs, zh)]}
        sel = {kind: np.array(v, dtype=np.uint64) for kind, v in sel.items()}
        K = len(self.cons)
        self.weight = [[O.batch_op("mul", self.full(pow(alphas[kk], K - 1 - j, P)), sel[Z.decode(code[k])[0]]) for k, j in self.cons.items()] for kk in range(2)]
        # the evaluator is faithful: its accumulators, divided by Z_H, are quotient_values' on the unmutated program
        self.base = self.quotient(air)
        zinv = np.array([pow(z, P - 2, P) for z in zh], dtype=np.uint64)
        for kk in range(2):
            acc = self.full(0)
            for k, j in self.cons.items():
                acc = O.batch_op("add", acc, O.batch_op("mul", self.weight[kk][j], self.vals[self.srcs[k][0]]))
            assert (O.batch_op("mul", acc, zinv) == self.base[kk]).all()

    def quotient(self, air):
        pub, alphas, log_n, r, chal, apub = self.args
        return S.quotient_values(air, self.lde, pub, alphas, log_n, r, chal, apub)

    @staticmethod
    def arith(op, x, y):
        return O.batch_op({ADD: "add", SUB: "sub", MUL: "mul"}[op], x, y)

    def load(self, op, a):
        return self.full(self.air.consts[a]) if op == CONST else self.loads[op][a]

    def survives(self, k, word):
        """whether the program with instruction k replaced by `word` has the original's quotient values"""
        op, _, a, _ = Z.decode(word)
        if op in (ADD, SUB):
            v = self.arith(op, self.vals[self.srcs[k][0]], self.vals[self.srcs[k][1]])
        else:
            v = self.full(self.air.consts[Z.decode(self.air.code[k])[2]] + 1) if op == CONST else self.loads[op][a]
        if np.array_equal(v, self.vals[k]):
            return True
        new, heap, queued = {k: v}, list(self.users[k]), set(self.users[k])
        heapq.heapify(heap)
        delta = [self.full(0), self.full(0)]
        while heap:
            u = heapq.heappop(heap)
            s = self.srcs[u]
            if u in self.cons:
                diff = O.batch_op("sub", new[s[0]], self.vals[s[0]])
                for kk in range(2):
                    delta[kk] = O.batch_op("add", delta[kk], O.batch_op("mul", self.weight[kk][self.cons[u]], diff))
                continue
            v = self.arith(Z.decode(self.air.code[u])[0], new.get(s[0], self.vals[s[0]]), new.get(s[1], self.vals[s[1]]))
            if not np.array_equal(v, self.vals[u]):
                new[u] = v
                for t in self.users[u]:
                    if t not in queued:
                        queued.add(t)
                        heapq.heappush(heap, t)
        return not delta[0].any() and not delta[1].any()

    def constant_zero(self, k, through_mul=True):
        """whether instruction k's value is 0 whatever the data: the constant 0, or (through_mul) a product with such a factor"""
        op, _, a, _ = Z.decode(self.air.code[k])
        if op == CONST:
            return self.air.consts[a] % P == 0
        return through_mul and op == MUL and any(self.constant_zero(s, False) for s in self.srcs[k])

    def survivors(self):
        """-> (number of mutants, [(kind, instruction index)] of the survivors); every CHECK_EVERY-th verdict and every survivor is
        checked against quotient_values on the mutated program"""
        ms = mutants(self.air)
        out = []
        for i, (kind, k, word) in enumerate(ms):
            alive = self.survives(k, word)
            if alive or i % CHECK_EVERY == 0:
                assert alive == bool((self.quotient(mutated(self.air, k, word)) == self.base).all()), (kind, k)
            if alive:
                out.append((kind, k))
        return len(ms), out


@pytest.mark.parametrize("name", QA.BUS_TABLES)
def test_arbitrary_data_kills_every_column_mutant(oracle, name):
    air, lde, pub, chal, apub, pairs = QA.arbitrary(name, LOG_N, RATE_BITS)
    run = Run(air, lde, pub, chal, apub, pairs[0][1])
    n, alive = run.survivors()
    print("%s: %d of %d mutants survive arbitrary data: %s" % (name, len(alive), n, alive))
    assert not [m for m in alive if m[0] in ("col+1", "loc<->nxt")], "the arbitrary data misses a wrong column or row"
    assert sorted(k for _, k in alive) == sorted(EQUIVALENT.get(name, {})), "survivors that are not listed as equivalent (or listed ones that died)"
    assert {kind for kind, _ in alive} <= {"add<->sub"}
    for _, k in alive:
        assert run.constant_zero(run.srcs[k][1]), "instruction %d: the operand that changes sign is not the constant 0" % k


def honest_transcript_lde():
    """the trace of the Transcript proof-parity test with its auxiliary columns, extended to the rate_bits 1 coset, natural order"""
    import transcript_ref as T

    trace, pub, _ = T.ref_table(T.synth_chains(["draw_17", "one_block", "interleaved"]))
    aux, apub = T.gen_aux(trace, T.CHAL, pub)
    rows = np.concatenate([trace, np.ascontiguousarray(aux, dtype=np.uint64)])
    log_n = rows.shape[1].bit_length() - 1
    leaves, _ = O.lde_from_values(rows, 1, S.G)
    return np.ascontiguousarray(leaves[S.bitrev_perm(log_n + 1)].T), pub, list(T.CHAL), apub, log_n


def test_an_honest_trace_leaves_column_mistakes_unseen(oracle):
    """the gap the arbitrary-data test closes: on a satisfying trace some col+1 mutants give the same quotient, hence the same proof"""
    air = QA.restatement("VX_AIR_TRANSCRIPT")
    lde, pub, chal, apub, log_n = honest_transcript_lde()
    assert lde.shape == (111, 1024)
    alphas = QA.alpha_pairs(np.random.default_rng(5))[0][1]
    n, alive = Run(air, lde, pub, chal, apub, alphas, log_n, 1).survivors()
    print("VX_AIR_TRANSCRIPT: %d of %d mutants survive the honest trace, %d of them col+1" % (len(alive), n, sum(kind == "col+1" for kind, _ in alive)))
    assert sum(kind == "col+1" for kind, _ in alive) >= 1
