// Declared bus messages of a run-time AIR (include/vx.h vx_air_bus): the checks of vx_air_register_bus and the LOWERING of a message
// program into ordinary constraint instructions -- what bus_constraints<Air> (air.cuh) is for a compiled table.  Host-only standard
// C++ with no HIP dependency: the registry in vx_verify.hip includes it, and tests/host/bus_program_check.cpp compiles it alone.
// The witness side of the same declaration is k_bus_aux_prog (bus_aux_prog.cuh).
//
// The lowered code keeps the message program's registers 0 .. K-1 (K = vx_air_bus::n_regs) and works in the VX_BUSP_LOWER_REGS = 20
// registers behind them:
//   G2 G3 G4   gamma^2, gamma^3, gamma^4 (6)        HS   the sum of the helpers so far (2)
//   DA MA      denominator and multiplicity of the even message of the current pair (3: the message program may overwrite the
//              register the multiplicity came from before the odd message closes)
//   DB         denominator of the odd message (2)   NU   m_a D_b + m_b D_a (2)      PR   D_a D_b (2)      T0 T1 T2   scratch (3)
// A slot's term is added to the denominator AT the SLOT instruction and the multiplicity is read AT the MSG instruction, so a message
// means the register values of that moment -- the reading k_bus_aux_prog has.  Extension products are written out as air_program.X2
// and air.cuh X2<F> write them (X^2 = 7, 7 x = 8 x - x).  Emitted per helper, in helper order: the two halves of
// h D_a D_b - m_a D_b - m_b D_a (h D - m for the single message an odd count leaves); then the two halves of
// z' - z - sum h [* per[step]] + total.  The checks of the result (operands, def-before-use, degrees) are vx_air_register's own.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "air_program.h"

namespace busp {
constexpr uint64_t P = 0xFFFFFFFF00000001ULL;

struct Lowered {
    std::vector<uint64_t> code, consts;  // the program's own followed by the bus block
    uint32_t n_regs = 0, n_msgs = 0, n_help = 0;
};

static inline bool refuse(char* err, size_t errlen, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return false;
}
static inline uint64_t insn(int op, int d, int a, int b = 0) { return (uint64_t)op | ((uint64_t)d << 8) | ((uint64_t)a << 16) | ((uint64_t)b << 32); }

// Everything vx_air_register_bus refuses about the declaration itself.  `in` has passed the range checks of vx_air_register (columns,
// public inputs, periodic columns, the auxiliary round's ranges).  -> the message count
static bool validate(const vx_air_program& in, const vx_air_bus& bus, uint32_t* n_msgs_out, char* err, size_t errlen) {
#define BUSP_NEED(cond, ...) \
    do {                     \
        if (!(cond)) return refuse(err, errlen, __VA_ARGS__); \
    } while (0)
    BUSP_NEED(!in.gen_aux, "air bus: a gen_aux callback given together with a bus (the library fills the auxiliary round of declared messages)");
    BUSP_NEED(bus.n_regs >= 1 && bus.n_regs <= VX_BUSP_MAX_REGS, "air bus: %u registers (1..%d: the lowering keeps %d of the 32)", bus.n_regs, VX_BUSP_MAX_REGS, VX_BUSP_LOWER_REGS);
    BUSP_NEED(bus.code && bus.n_code >= 1 && bus.n_code <= VX_BUSP_MAX_CODE, "air bus: %u instructions (1..%d)", bus.n_code, VX_BUSP_MAX_CODE);
    BUSP_NEED(bus.n_consts <= 4096 && (bus.n_consts == 0 || bus.consts), "air bus: bad constant table");
    for (uint32_t k = 0; k < bus.n_consts; ++k) BUSP_NEED(bus.consts[k] < P, "air bus: non-canonical constant %u", k);
    if (bus.block_log == 0) {
        BUSP_NEED(bus.step_periodic < 0, "air bus: wrong step column: block_log 0 advances the sum on every row (step_periodic must be negative)");
    } else {
        BUSP_NEED(bus.block_log == 5, "air bus: block_log %u is not supported (0 or 5)", bus.block_log);
        BUSP_NEED(bus.step_periodic >= 0 && (uint32_t)bus.step_periodic < in.n_periodic && in.periodic_log && in.periodic_values, "air bus: wrong step column: %d is no periodic column", bus.step_periodic);
        size_t off = 0;
        for (int q = 0; q < bus.step_periodic; ++q) {
            BUSP_NEED(in.periodic_log[q] <= VX_AIRP_MAX_PERIOD_LOG, "air bus: periodic column %d out of range", q);
            off += (size_t)1 << in.periodic_log[q];
        }
        BUSP_NEED(in.periodic_log[bus.step_periodic] == bus.block_log, "air bus: wrong step column: periodic column %d has period 2^%u, the block 2^%u", bus.step_periodic,
                  in.periodic_log[bus.step_periodic], bus.block_log);
        for (size_t k = 0; k < ((size_t)1 << bus.block_log); ++k)
            BUSP_NEED(in.periodic_values[off + k] == (k == 0 ? 1u : 0u), "air bus: wrong step column: periodic column %d is not 1 at position 0 and 0 elsewhere", bus.step_periodic);
    }
    bool written[VX_BUSP_MAX_REGS] = {};
    bool slot_set[4] = {};
    bool open = false;
    uint32_t n_msgs = 0;
    for (uint32_t pc = 0; pc < bus.n_code; ++pc) {
        const uint64_t w = bus.code[pc];
        const AirpInsn i = airp_decode(w);
        BUSP_NEED((w >> 48) == 0, "air bus: instruction %u has reserved bits set", pc);
        auto reg_ok = [&](int r) { return r >= 0 && r < (int)bus.n_regs; };
        auto src = [&](int r) { return reg_ok(r) && written[r]; };
        switch (i.op) {
            case VX_AIRP_LOC:
                BUSP_NEED(i.a < (int)(in.cols + in.aux_cols), "air bus: instruction %u: bad column load", pc);
                BUSP_NEED(i.a < (int)in.cols, "air bus: instruction %u: LOC of an auxiliary column (a message is stated over the main columns)", pc);
                BUSP_NEED(reg_ok(i.d) && i.b == 0, "air bus: instruction %u: bad column load", pc);
                written[i.d] = true;
                break;
            case VX_AIRP_PER:
                BUSP_NEED(reg_ok(i.d) && i.a < (int)in.n_periodic && i.b == 0, "air bus: instruction %u: bad periodic load", pc);
                written[i.d] = true;
                break;
            case VX_AIRP_PUB:
                BUSP_NEED(reg_ok(i.d) && i.a < (int)in.n_public && i.b == 0, "air bus: instruction %u: bad public-input load", pc);
                written[i.d] = true;
                break;
            case VX_AIRP_CONST:
                BUSP_NEED(reg_ok(i.d) && i.a < (int)bus.n_consts && i.b == 0, "air bus: instruction %u: bad constant load", pc);
                written[i.d] = true;
                break;
            case VX_AIRP_ADD:
            case VX_AIRP_SUB:
            case VX_AIRP_MUL:
                BUSP_NEED(reg_ok(i.d) && src(i.a) && src(i.b), "air bus: instruction %u reads a register that was never written (or out of range)", pc);
                written[i.d] = true;
                break;
            case VX_BUSP_SLOT:
                BUSP_NEED(i.d <= 3, "air bus: instruction %u: slot index %d above 3", pc, i.d);
                BUSP_NEED(i.b == 0 && src(i.a), "air bus: instruction %u: SLOT reads a register that was never written (or out of range)", pc);
                BUSP_NEED(!slot_set[i.d], "air bus: instruction %u sets slot %d twice in one message", pc, i.d);
                slot_set[i.d] = open = true;
                break;
            case VX_BUSP_MSG:
                BUSP_NEED(i.d == 0 && src(i.a), "air bus: instruction %u: MSG reads a register that was never written (or out of range)", pc);
                ++n_msgs;
                BUSP_NEED((n_msgs + 1) / 2 <= VX_BUSP_MAX_HELPERS, "air bus: more than %d helpers (%d messages)", VX_BUSP_MAX_HELPERS, 2 * VX_BUSP_MAX_HELPERS);
                slot_set[0] = slot_set[1] = slot_set[2] = slot_set[3] = open = false;
                break;
            case VX_AIRP_NXT: BUSP_NEED(false, "air bus: instruction %u: NXT is not allowed in a message program (a message is stated over one row)", pc);
            case VX_AIRP_CHAL: BUSP_NEED(false, "air bus: instruction %u: CHAL is not allowed in a message program", pc);
            case VX_AIRP_APUB: BUSP_NEED(false, "air bus: instruction %u: APUB is not allowed in a message program", pc);
            case VX_AIRP_ASSERT:
            case VX_AIRP_ASSERT_TRANSITION:
            case VX_AIRP_ASSERT_FIRST:
            case VX_AIRP_ASSERT_LAST: BUSP_NEED(false, "air bus: instruction %u: an assert is not allowed in a message program", pc);
            default: BUSP_NEED(false, "air bus: instruction %u has unknown opcode %d", pc, i.op);
        }
    }
    BUSP_NEED(!open, "air bus: a SLOT not followed by a MSG");
    BUSP_NEED(n_msgs >= 1, "air bus: no message");
    const uint32_t n_help = (n_msgs + 1) / 2;
    BUSP_NEED(in.aux_cols == 2 * n_help + 2 && in.n_challenges == 4 && in.n_aux_public == 1,
              "air bus: %u messages need aux_cols %u, n_challenges 4, n_aux_public 1 (declared %u, %u, %u)", n_msgs, 2 * n_help + 2, in.aux_cols, in.n_challenges, in.n_aux_public);
    BUSP_NEED((size_t)in.n_consts + bus.n_consts + n_msgs + 1 <= 65536, "air bus: constant table too long");
    *n_msgs_out = n_msgs;
    return true;
#undef BUSP_NEED
}

// the program's code and constants followed by the bus block of a VALIDATED declaration
static void lower(const vx_air_program& in, const vx_air_bus& bus, uint32_t n_msgs, Lowered* out) {
    std::vector<uint64_t>& c = out->code;
    std::vector<uint64_t>& k = out->consts;
    c.assign(in.code, in.code + in.n_code);
    k.assign(in.consts, in.consts + in.n_consts);
    const int cbase = (int)in.n_consts;
    k.insert(k.end(), bus.consts, bus.consts + bus.n_consts);
    auto constant = [&](uint64_t v) {
        for (size_t j = (size_t)cbase + bus.n_consts; j < k.size(); ++j)
            if (k[j] == v) return (int)j;
        k.push_back(v);
        return (int)k.size() - 1;
    };
    const int zero = constant(0);
    const int B = (int)bus.n_regs, G2 = B, G3 = B + 2, G4 = B + 4, HS = B + 6, DA = B + 8, MA = B + 10, DB = B + 11, NU = B + 13, PR = B + 15, T0 = B + 17, T1 = B + 18, T2 = B + 19;
    static_assert(VX_BUSP_LOWER_REGS == 20 && VX_BUSP_MAX_REGS + VX_BUSP_LOWER_REGS == VX_AIRP_MAX_REGS, "bus_program.h: the register budget");
    auto op = [&](int o, int d, int a, int b = 0) { c.push_back(insn(o, d, a, b)); };
    auto xmul = [&](int o, int x, int y) {  // o = x y in F[X]/(X^2 - 7); o aliases neither
        op(VX_AIRP_MUL, T0, x + 1, y + 1);
        op(VX_AIRP_ADD, T1, T0, T0);
        op(VX_AIRP_ADD, T1, T1, T1);
        op(VX_AIRP_ADD, T1, T1, T1);
        op(VX_AIRP_SUB, T1, T1, T0);
        op(VX_AIRP_MUL, T0, x, y);
        op(VX_AIRP_ADD, o, T0, T1);
        op(VX_AIRP_MUL, T0, x, y + 1);
        op(VX_AIRP_MUL, T1, x + 1, y);
        op(VX_AIRP_ADD, o + 1, T0, T1);
    };
    const int H0 = (int)in.cols, Z = H0 + 2 * (int)((n_msgs + 1) / 2);
    // gamma's powers (gamma itself is loaded where it is used), the empty sum
    op(VX_AIRP_CHAL, DA, 2), op(VX_AIRP_CHAL, DA + 1, 3);
    xmul(G2, DA, DA), xmul(G3, G2, DA), xmul(G4, G2, G2);
    op(VX_AIRP_CONST, HS, zero), op(VX_AIRP_CONST, HS + 1, zero);
    uint32_t msg = 0;
    bool open = false;
    auto begin = [&](int D) {  // D = beta
        if (!open) op(VX_AIRP_CHAL, D, 0), op(VX_AIRP_CHAL, D + 1, 1);
        open = true;
    };
    auto term = [&](int D, int g, int t) {  // D += g t
        op(VX_AIRP_MUL, T0, g, t), op(VX_AIRP_ADD, D, D, T0);
        op(VX_AIRP_MUL, T0, g + 1, t), op(VX_AIRP_ADD, D + 1, D + 1, T0);
    };
    auto helper = [&](int h, uint32_t e) {  // h = helper e, added to the sum
        op(VX_AIRP_LOC, h, H0 + 2 * (int)e), op(VX_AIRP_LOC, h + 1, H0 + 2 * (int)e + 1);
        op(VX_AIRP_ADD, HS, HS, h), op(VX_AIRP_ADD, HS + 1, HS + 1, h + 1);
    };
    for (uint32_t pc = 0; pc < bus.n_code; ++pc) {
        const AirpInsn i = airp_decode(bus.code[pc]);
        const int D = (msg & 1) ? DB : DA;
        switch (i.op) {
            case VX_AIRP_CONST: op(i.op, i.d, cbase + i.a); break;
            case VX_BUSP_SLOT:
                begin(D);
                if (i.d == 0) op(VX_AIRP_ADD, D, D, i.a);
                else if (i.d == 1) op(VX_AIRP_CHAL, T1, 2), op(VX_AIRP_CHAL, T2, 3), op(VX_AIRP_MUL, T0, T1, i.a), op(VX_AIRP_ADD, D, D, T0), op(VX_AIRP_MUL, T0, T2, i.a), op(VX_AIRP_ADD, D + 1, D + 1, T0);
                else term(D, i.d == 2 ? G2 : G3, i.a);
                break;
            case VX_BUSP_MSG: {
                begin(D);
                if (i.b) op(VX_AIRP_CONST, T1, constant((uint64_t)i.b)), term(D, G4, T1);
                open = false;
                const uint32_t e = msg / 2;
                if (!(msg & 1) && msg + 1 < n_msgs) {  // the even message of a pair: keep the multiplicity
                    op(VX_AIRP_CONST, MA, zero), op(VX_AIRP_ADD, MA, i.a, MA);
                } else if (!(msg & 1)) {  // the single message of the last helper: h D - m
                    helper(PR, e);
                    xmul(NU, PR, DA);
                    op(VX_AIRP_SUB, NU, NU, i.a);
                    op(VX_AIRP_ASSERT, 0, NU), op(VX_AIRP_ASSERT, 0, NU + 1);
                } else {  // h D_a D_b - m_a D_b - m_b D_a
                    op(VX_AIRP_MUL, NU, MA, DB), op(VX_AIRP_MUL, T0, i.a, DA), op(VX_AIRP_ADD, NU, NU, T0);
                    op(VX_AIRP_MUL, NU + 1, MA, DB + 1), op(VX_AIRP_MUL, T0, i.a, DA + 1), op(VX_AIRP_ADD, NU + 1, NU + 1, T0);
                    xmul(PR, DA, DB);
                    helper(DA, e);
                    xmul(DB, DA, PR);
                    op(VX_AIRP_SUB, DB, DB, NU), op(VX_AIRP_SUB, DB + 1, DB + 1, NU + 1);
                    op(VX_AIRP_ASSERT, 0, DB), op(VX_AIRP_ASSERT, 0, DB + 1);
                }
                ++msg;
                break;
            }
            default: op(i.op, i.d, i.a, i.b); break;  // LOC PER PUB ADD SUB MUL: as stated
        }
    }
    for (int j = 0; j < 2; ++j) {  // z' - z - sum h [* per[step]] + total
        op(VX_AIRP_LOC, T0, Z + j), op(VX_AIRP_NXT, T1, Z + j), op(VX_AIRP_SUB, T1, T1, T0);
        if (bus.block_log) op(VX_AIRP_PER, T2, bus.step_periodic), op(VX_AIRP_MUL, T0, HS + j, T2), op(VX_AIRP_SUB, T1, T1, T0);
        else op(VX_AIRP_SUB, T1, T1, HS + j);
        op(VX_AIRP_APUB, T0, j), op(VX_AIRP_ADD, T1, T1, T0), op(VX_AIRP_ASSERT, 0, T1);
    }
    out->n_msgs = n_msgs, out->n_help = (n_msgs + 1) / 2;
    out->n_regs = in.n_regs > (uint32_t)(B + VX_BUSP_LOWER_REGS) ? in.n_regs : (uint32_t)(B + VX_BUSP_LOWER_REGS);
}
}  // namespace busp
