"""Writes constraint programs for vx_air_register (include/vx.h `vx_air_program`): the host-side half of the run-time AIR
descriptor.  An AIR is stated as expressions over the local / next row, periodic columns, public inputs and constants --
what a starky `Stark::eval_packed_generic` body says (starky v0.2.0 stark.rs; the reference reaches it through curta's
AirParser) -- and lowered to the library's straight-line register code:

    b = AirBuilder(cols=2, n_public=3)
    b.assert_first(b.loc(0) - b.pub(0))
    b.assert_transition(b.nxt(1) - b.loc(0) - b.loc(1))
    air_id = b.register()            # -> lib.air_register

A table on a logUp bus DECLARES its messages instead of writing the bus block and a witness generator by hand:

    b.send(TAG, [b.loc(2), b.loc(3)], b.loc(0))          # slots t0, t1 (None leaves a slot out), multiplicity
    b.receive(TAG, [b.loc(2), None, b.loc(4)], b.loc(1))
    air_id = b.register()            # -> lib.air_register_bus: the library derives the constraints AND fills the auxiliary round

Constraints are consumed in the order they are asserted (the order is protocol).  Inside one constraint a shared
sub-expression (the same Python object used twice) is evaluated once; nothing is shared between constraints."""
import numpy as np

P = 2**64 - 2**32 + 1
OP = dict(loc=1, nxt=2, per=3, pub=4, const=5, add=6, sub=7, mul=8, assert_zero=9, assert_transition=10, assert_first=11, assert_last=12, chal=13, apub=14,
          bus_slot=64, bus_msg=65)
MAX_REGS = 32
BUS_MAX_REGS = 12  # include/vx.h VX_BUSP_MAX_REGS: what a message program may use (the lowering keeps the other 20)


def insn(op, d=0, a=0, b=0):
    return op | (d << 8) | (a << 16) | (b << 32)


class Expr:
    __slots__ = ("op", "a", "b")

    def __init__(self, op, a=0, b=0):
        self.op, self.a, self.b = op, a, b

    @staticmethod
    def of(x):
        return x if isinstance(x, Expr) else Expr("const", int(x) % P)

    def __add__(self, o):
        return Expr("add", self, Expr.of(o))

    def __radd__(self, o):
        return Expr("add", Expr.of(o), self)

    def __sub__(self, o):
        return Expr("sub", self, Expr.of(o))

    def __rsub__(self, o):
        return Expr("sub", Expr.of(o), self)

    def __mul__(self, o):
        return Expr("mul", self, Expr.of(o))

    def __rmul__(self, o):
        return Expr("mul", Expr.of(o), self)


class X2:
    """An element a + b X of the quadratic extension F[X]/(X^2 - 7) as a pair of expressions: lookup arguments (logUp) work there,
    and the library's instruction set is base-field only, so the products are written out here (csrc/air.cuh X2<F> does the same
    for the compiled AIRs, in the same order of operations)."""

    def __init__(self, a, b=0):
        self.a, self.b = Expr.of(a), Expr.of(b)

    def __add__(self, o):
        if isinstance(o, X2):
            return X2(self.a + o.a, self.b + o.b)
        return X2(self.a + o, self.b)

    def __sub__(self, o):
        if isinstance(o, X2):
            return X2(self.a - o.a, self.b - o.b)
        return X2(self.a - o, self.b)

    def __mul__(self, o):
        if isinstance(o, X2):
            bb = self.b * o.b
            b2 = bb + bb
            b4 = b2 + b2
            return X2(self.a * o.a + (b4 + b4 - bb), self.a * o.b + self.b * o.a)  # 7 x = 8 x - x
        return X2(self.a * o, self.b * o)


class AirBuilder:
    def __init__(self, cols, n_public=0, periodic=(), aux_cols=0, n_challenges=0, n_aux_public=0):
        self.cols, self.n_public = cols, n_public
        self.aux_cols, self.n_challenges, self.n_aux_public = aux_cols, n_challenges, n_aux_public
        self.periodic = [[int(v) % P for v in col] for col in periodic]
        self.constraints = []
        self.messages = []  # (tag, slots (Expr or None) x 4, signed multiplicity), in bus order: 2 e and 2 e + 1 share helper e
        self.bus_block_log, self.bus_step = 0, None

    def chal(self, i):
        return Expr("chal", i)

    def apub(self, i):
        return Expr("apub", i)

    def aux(self, j):
        """auxiliary column j of the local row (rows hold the main columns followed by the auxiliary ones)"""
        return Expr("loc", self.cols + j)

    def aux_nxt(self, j):
        return Expr("nxt", self.cols + j)

    def assert_zero_x2(self, e):
        self.assert_zero(e.a)
        self.assert_zero(e.b)

    def loc(self, col):
        return Expr("loc", col)

    def nxt(self, col):
        return Expr("nxt", col)

    def per(self, q):
        return Expr("per", q)

    def pub(self, i):
        return Expr("pub", i)

    def const(self, v):
        return Expr("const", int(v) % P)

    def assert_zero(self, e):
        self.constraints.append(("assert_zero", Expr.of(e)))

    def assert_transition(self, e):
        self.constraints.append(("assert_transition", Expr.of(e)))

    def assert_first(self, e):
        self.constraints.append(("assert_first", Expr.of(e)))

    def assert_last(self, e):
        self.constraints.append(("assert_last", Expr.of(e)))

    def send(self, tag, slots, mult):
        """a message (slots[0..3], tag) this row sends `mult` times; a slot that is None (or missing) is absent"""
        slots = list(slots) + [None] * (4 - len(slots))
        if len(slots) != 4 or not 0 <= int(tag) < 1 << 16:
            raise ValueError("a message has at most four slots and a tag below 2^16")
        self.messages.append((int(tag), [None if t is None else Expr.of(t) for t in slots], Expr.of(mult)))

    def receive(self, tag, slots, mult):
        self.send(tag, slots, Expr("sub", Expr("const", 0), Expr.of(mult)))

    def bus(self, block_log=0, step_periodic=None):
        """block_log 0: helpers per row, the sum advances on every row; 5: per 32-row block, the sum advances where periodic column
        step_periodic is 1"""
        self.bus_block_log, self.bus_step = block_log, step_periodic

    @staticmethod
    def _allocate(groups, max_regs):
        """The register allocator.  groups: (roots, close) -- the expressions of `roots` are evaluated (a shared sub-expression, the
        same Python object used twice, once; nothing is shared between groups) and close(registers of the roots) gives the
        instructions that consume them.  -> (code uint64[], consts uint64[], n_regs)"""
        code, consts, const_ix = [], [], {}
        n_regs = 0
        for roots, close in groups:
            uses, order, seen = {}, [], set()

            def visit(e):
                uses[id(e)] = uses.get(id(e), 0) + 1
                if id(e) in seen:
                    return
                seen.add(id(e))
                if e.op in ("add", "sub", "mul"):
                    visit(e.a), visit(e.b)
                order.append(e)

            for root in roots:
                visit(root)  # uses[e] = reads of e: one per parent reference, and the consumer's read of a root
            free, reg = list(range(max_regs - 1, -1, -1)), {}

            def release(e):
                uses[id(e)] -= 1
                if uses[id(e)] == 0:
                    free.append(reg[id(e)])

            for e in order:
                if e.op in ("add", "sub", "mul"):
                    ra, rb = reg[id(e.a)], reg[id(e.b)]
                    release(e.a), release(e.b)  # the destination may reuse an operand's register
                if not free:
                    raise ValueError("needs more than %d registers: split it or share less" % max_regs)
                d = free.pop()
                reg[id(e)] = d
                n_regs = max(n_regs, d + 1)
                if e.op == "const":
                    if e.a not in const_ix:
                        const_ix[e.a] = len(consts)
                        consts.append(e.a)
                    code.append(insn(OP["const"], d, const_ix[e.a]))
                elif e.op in ("loc", "nxt", "per", "pub", "chal", "apub"):
                    code.append(insn(OP[e.op], d, e.a))
                else:
                    code.append(insn(OP[e.op], d, ra, rb))
            code += close([reg[id(root)] for root in roots])
        return np.array(code, dtype=np.uint64), np.array(consts, dtype=np.uint64), n_regs

    def assemble(self):
        """-> (code uint64[], consts uint64[], n_regs)"""
        return self._allocate([([root], lambda r, kind=kind: [insn(OP[kind], 0, r[0])]) for kind, root in self.constraints], MAX_REGS)

    def assemble_bus(self):
        """the message program of include/vx.h vx_air_bus -> (code uint64[], consts uint64[], n_regs)"""
        groups = []
        for tag, slots, mult in self.messages:
            at = [j for j in range(4) if slots[j] is not None]

            def close(r, at=at, tag=tag):
                return [insn(OP["bus_slot"], j, r[k]) for k, j in enumerate(at)] + [insn(OP["bus_msg"], 0, r[-1], tag)]

            groups.append(([slots[j] for j in at] + [mult], close))
        return self._allocate(groups, BUS_MAX_REGS)

    def register(self, gen_aux=None):
        from . import lib

        code, consts, n_regs = self.assemble()
        if not self.messages:
            return lib.air_register(self.cols, self.n_public, code, consts, self.periodic, n_regs, self.aux_cols, self.n_challenges, self.n_aux_public, gen_aux)
        bcode, bconsts, bregs = self.assemble_bus()
        self.aux_cols, self.n_challenges, self.n_aux_public = 2 * ((len(self.messages) + 1) // 2) + 2, 4, 1
        return lib.air_register_bus(self.cols, self.n_public, code, bcode, consts, bconsts, self.periodic, n_regs, bregs, self.bus_block_log,
                                    -1 if self.bus_step is None else self.bus_step, self.aux_cols, self.n_challenges, self.n_aux_public, gen_aux)
