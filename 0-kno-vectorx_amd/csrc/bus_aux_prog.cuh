// The auxiliary round of a run-time AIR that declared its bus messages (include/vx.h vx_air_register_bus): what k_bus_aux<Air>
// (bus_aux.cuh) is for a compiled table, with the message list read from a program instead of from Air::messages.
//   k_bus_aux_prog  one lane per row, or per block of 2^block_log rows.  The message program is interpreted as k_quotient_prog
//                   interprets constraints: the register file in LDS (register r of lane t at lds[r * BUSP_BLOCK + t]: conflict-free),
//                   instruction words fetched wave-uniformly.  SLOT adds its term to the open denominator, MSG closes the message;
//                   every second MSG (and the last one of an odd count) closes a helper: num_e = m_a D_b + m_b D_a, den_e = D_a D_b
//                   and the running product den_0 .. den_e go to LDS beside the register file (the helper count is a run-time value,
//                   so they cannot sit in registers under constant indices).  A row or block whose multiplicities are all zero
//                   writes zero helpers and inverts nothing; otherwise ONE extension inversion yields all helpers (Montgomery's
//                   batch, walked back through LDS).  Output as k_bus_aux<Air>: helper e to columns [2 e, 2 e + 1] of all rows of the
//                   block, the helpers' sum to columns [2 N_HELP, 2 N_HELP + 1] of the block's first row, zero on the others
//   busp_walk       the interpreter's walk itself, stated once: the records kernel of the bus balance check (bus_balance.cuh) runs
//                   the same program and keeps (multiplicity, denominator) of every message instead of the helpers
//   bus_prog_gen_aux  uploads the program, launches, and closes the sum (vx_bus_close_dev)
// LDS per workgroup (one wave): (n_regs + 6 N_HELP) * 64 * 8 bytes, at most (12 + 6 * 19) * 512 = 64512 -- VX_BUSP_MAX_HELPERS is
// chosen so that this stays below 64 KiB.  profiles/README.md has the occupancy.
#pragma once
#include <vector>

#include "air_program.h"
#include "gl.cuh"
#include "vx_internal.h"

constexpr int BUSP_BLOCK = 64;
static_assert((VX_BUSP_MAX_REGS + 6 * VX_BUSP_MAX_HELPERS) * BUSP_BLOCK * sizeof(uint64_t) <= 65536, "bus_aux_prog.cuh: the LDS of one workgroup");
struct BusProgArgs {
    const uint64_t *code, *consts;  // device: the message program and its constants
    const uint64_t *per_tab;        // device: per periodic column (offset into periodic, period - 1)
    const uint64_t *periodic, *pub; // device: one period of every periodic column back to back; the public inputs
    int n_code, n_regs, n_msgs, block_log;
};

// The walk of a message program over one row, shared by the witness kernel below and the records kernel of the balance check
// (bus_balance.cuh): register code on the lane's LDS words R, SLOT adds its term to the open denominator, MSG closes the message and
// hands (ordinal, multiplicity, denominator) to on_msg.
template <class OnMsg>
__device__ __forceinline__ void busp_walk(const uint64_t* __restrict__ tr, size_t n, size_t row, uint64_t* R, gl2 beta, gl2 gamma, const BusProgArgs& p, OnMsg&& on_msg) {
    const gl2 g2 = gl2_mul(gamma, gamma), g3 = gl2_mul(g2, gamma), g4 = gl2_mul(g2, g2);
    gl2 D = beta;
    int msg = 0;
#pragma unroll 1
    for (int pc = 0; pc < p.n_code; ++pc) {
        const uint64_t w = p.code[pc];
        const int op = (int)(w & 0xFF), dn = (int)((w >> 8) & 0xFF), d = dn * BUSP_BLOCK, ra = (int)((w >> 16) & 0xFFFF), rb = (int)((w >> 32) & 0xFFFF);
        switch (op) {
            case VX_AIRP_LOC: R[d] = tr[(size_t)ra * n + row]; break;
            case VX_AIRP_PER: R[d] = p.periodic[p.per_tab[2 * ra] + (row & p.per_tab[2 * ra + 1])]; break;
            case VX_AIRP_PUB: R[d] = p.pub[ra]; break;
            case VX_AIRP_CONST: R[d] = p.consts[ra]; break;
            case VX_AIRP_ADD: R[d] = gl_add(R[ra * BUSP_BLOCK], R[rb * BUSP_BLOCK]); break;
            case VX_AIRP_SUB: R[d] = gl_sub(R[ra * BUSP_BLOCK], R[rb * BUSP_BLOCK]); break;
            case VX_AIRP_MUL: R[d] = gl_mul(R[ra * BUSP_BLOCK], R[rb * BUSP_BLOCK]); break;
            case VX_BUSP_SLOT: {
                const uint64_t t = R[ra * BUSP_BLOCK];
                if (dn == 0) D.a = gl_add(D.a, t);
                else D = gl2_add(D, gl2_scale(dn == 1 ? gamma : dn == 2 ? g2 : g3, t));
                break;
            }
            default: {  // VX_BUSP_MSG: registration admits nothing else
                const uint64_t m = R[ra * BUSP_BLOCK];
                if (rb) D = gl2_add(D, gl2_scale(g4, (uint64_t)rb));
                on_msg(msg, m, D);
                ++msg;
                D = beta;
                break;
            }
        }
    }
}

// (static: this header is part of two translation units, vx_stark.hip and -- through bus_balance.cuh -- vx_bus_group.hip)
static __global__ __launch_bounds__(BUSP_BLOCK) void k_bus_aux_prog(const uint64_t* __restrict__ tr, uint64_t* __restrict__ aux, size_t n, gl2 beta, gl2 gamma, BusProgArgs p) {
    extern __shared__ uint64_t busp_lds[];
    const size_t i = blockIdx.x * (size_t)BUSP_BLOCK + threadIdx.x;
    if (i >= (n >> p.block_log)) return;  // (no barrier below: a lane works on LDS words of its own)
    const size_t row = i << p.block_log;
    uint64_t* R = busp_lds + threadIdx.x;
    uint64_t* Q = R + p.n_regs * BUSP_BLOCK;  // helper e: num at Q[(6 e + 0 | 1) * BLOCK], den at + 2 | 3, den_0 .. den_e at + 4 | 5
    gl2 Da = beta, acc{1, 0};
    uint64_t ma = 0, any = 0;
    auto close = [&](int e, gl2 num, gl2 den) {
        acc = gl2_mul(acc, den);
        uint64_t* q = Q + 6 * e * BUSP_BLOCK;
        q[0] = num.a, q[BUSP_BLOCK] = num.b, q[2 * BUSP_BLOCK] = den.a, q[3 * BUSP_BLOCK] = den.b, q[4 * BUSP_BLOCK] = acc.a, q[5 * BUSP_BLOCK] = acc.b;
    };
    busp_walk(tr, n, row, R, beta, gamma, p, [&](int msg, uint64_t m, gl2 D) {
        any |= m;
        if (msg & 1) close(msg >> 1, gl2_add(gl2_scale(D, ma), gl2_scale(Da, m)), gl2_mul(Da, D));
        else if (msg + 1 == p.n_msgs) close(msg >> 1, gl2{m, 0}, D);  // an odd count: the last helper holds one message
        else Da = D, ma = m;
    });
    const int H = (p.n_msgs + 1) / 2, rows = 1 << p.block_log;
    gl2 sum{0, 0}, inv{0, 0};
    if (any) inv = gl2_inv(acc);
#pragma unroll 1
    for (int e = H - 1; e >= 0; --e) {
        gl2 h{0, 0};
        if (any) {
            const uint64_t* q = Q + 6 * e * BUSP_BLOCK;
            const gl2 num{q[0], q[BUSP_BLOCK]}, den{q[2 * BUSP_BLOCK], q[3 * BUSP_BLOCK]};
            h = gl2_mul(num, e ? gl2_mul(inv, gl2{q[-2 * BUSP_BLOCK], q[-BUSP_BLOCK]}) : inv);  // inv * (den_0 .. den_(e-1)) = 1 / den_e
            inv = gl2_mul(inv, den);
            sum = gl2_add(sum, h);
        }
        uint64_t *ca = aux + (size_t)(2 * e) * n + row, *cb = aux + (size_t)(2 * e + 1) * n + row;
#pragma unroll 8
        for (int r = 0; r < rows; ++r) ca[r] = h.a, cb[r] = h.b;
    }
    uint64_t *za = aux + (size_t)(2 * H) * n + row, *zb = aux + (size_t)(2 * H + 1) * n + row;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) za[r] = r == 0 ? sum.a : 0, zb[r] = r == 0 ? sum.b : 0;  // increments; the scan makes them the running sum
}

// what the interpreter reads, in one upload: code | constants | per_tab | periodic | public inputs
static void busp_blob(const AirProgram& pg, const uint64_t* pub, std::vector<uint64_t>& blob) {
    blob.insert(blob.end(), pg.bus_code.begin(), pg.bus_code.end());
    blob.insert(blob.end(), pg.bus_consts.begin(), pg.bus_consts.end());
    size_t off = 0;
    for (uint8_t pl : pg.plog) blob.push_back(off), blob.push_back(((uint64_t)1 << pl) - 1), off += (size_t)1 << pl;
    blob.insert(blob.end(), pg.periodic.begin(), pg.periodic.end());
    blob.insert(blob.end(), pub, pub + pg.pub);
}
static size_t busp_blob_words(const AirProgram& pg) { return pg.bus_code.size() + pg.bus_consts.size() + 2 * pg.plog.size() + pg.periodic.size() + pg.pub; }
// ... and the kernel's view of that blob once it is at `d` on the device
static BusProgArgs busp_args(const AirProgram& pg, const uint64_t* d) {
    BusProgArgs a{};
    a.code = d, a.consts = a.code + pg.bus_code.size(), a.per_tab = a.consts + pg.bus_consts.size(), a.periodic = a.per_tab + 2 * pg.plog.size(), a.pub = a.periodic + pg.periodic.size();
    a.n_code = (int)pg.bus_code.size(), a.n_regs = (int)pg.bus_regs, a.block_log = pg.bus_block_log;
    a.n_msgs = 0;
    for (uint64_t w : pg.bus_code) a.n_msgs += (int)(w & 0xFF) == VX_BUSP_MSG;
    return a;
}

// the generator of a program with declared messages: AirProgram::bus_help > 0
static int32_t bus_prog_gen_aux(vx_ctx* ctx, const AirProgram& pg, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    VX_CHECK(log_n >= pg.bus_block_log, "air program %d: 2^%d rows are less than one block of its bus", pg.id, log_n);
    const size_t n = (size_t)1 << log_n, lanes = n >> pg.bus_block_log;
    std::vector<uint64_t> blob;
    busp_blob(pg, pub, blob);
    Scratch mem;
    uint64_t* d = nullptr;
    mem.add(d, blob.size());
    mem.alloc(ctx);
    mem.up(d, blob.data(), blob.size() * 8);
    if (!mem.ok()) return mem.status("air program bus");
    const BusProgArgs a = busp_args(pg, d);
    const size_t lds = (size_t)(pg.bus_regs + 6 * pg.bus_help) * BUSP_BLOCK * sizeof(uint64_t);
    hipLaunchKernelGGL(k_bus_aux_prog, dim3((unsigned)((lanes + BUSP_BLOCK - 1) / BUSP_BLOCK)), dim3(BUSP_BLOCK), lds, ctx->stream, trace, aux, n, gl2{chal[0], chal[1]}, gl2{chal[2], chal[3]}, a);
    mem.launched();
    mem.sync();  // blob (a host vector) must outlive the copy, and the pool block the kernel
    if (!mem.ok()) return mem.status("air program bus");
    return vx_bus_close_dev(ctx, aux + (size_t)(2 * pg.bus_help) * n, log_n, aux_pub);
}
