// Host-side verifier for the STARK proofs vx_stark_prove emits: the `circuit.verify` half of
// the reference's library seam (/root/reference circuits/header_range.rs:170).  Mirrors starky
// v0.2.0 verify_stark_proof_with_challenges + plonky2 v0.2.0 verify_fri_proof
// (fri_combine_initial, compute_evaluation, verify_merkle_proof_to_cap); crates pinned at
// Cargo.lock:4848-4905, not vendored.  Verification is scalar work and stays on the host, as in the
// reference -- except, in the _dev forms, its Merkle openings (most of its Poseidon permutations),
// which one launch of k_merkle_check takes (vx_merkle_check.hip; this file still holds no GPU code).
// Every host verifier of a statement lives here too, and all of them end in ONE sequence, verify_bus_group: the tables of a logUp
// bus under their shared challenges, and the balance of the bus against the messages of a party outside the tables -- nobody (the
// circuit verifiers) or the verifier itself (the aggregation verifiers: argument checks, read_blob, their tables, their messages).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>

#include <array>

#include "air_list.h"
#include "air_program.h"
#include "bus_program.h"
#include "stark_proof.h"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

static_assert(VX_BLAKE_TABLE_LOG == blk::TABLE_LOG, "vx_table_shapes.h and air_blake.cuh disagree on the rows of the XOR lookup tables");

namespace {
struct AirV {
    int id, cols, pub, periodic, period_log, exact_log;
    void (*periodic_values)(std::vector<uint64_t>&);
    void (*eval)(const HostRow&, const HostRow&, const Fx*, const Fx*, const Fx*, const Fx*, Consumer<Fx>&);
    int aux, chal, auxpub;
    int (*plog)(int);
    const AirProgram* prog = nullptr;  // a registered constraint program instead of a compiled AIR
};
template <class Air>
void eval_host(const HostRow& l, const HostRow& n, const Fx* per, const Fx* pub, const Fx* chal, const Fx* apub, Consumer<Fx>& c) {
    Air::template eval<Fx>(l, n, per, pub, chal, apub, c);
}
template <class Air>
AirV vdesc() {
    return {Air::ID, Air::COLS, Air::PUB, Air::PERIODIC, Air::PERIOD_LOG, Air::EXACT_LOG, Air::periodic_values, eval_host<Air>, Air::AUX, Air::CHAL, Air::AUXPUB, Air::plog};
}
template <class... Airs>
std::array<AirV, sizeof...(Airs)> vdescs(AirList<Airs...>) { return {{vdesc<Airs>()...}}; }
const auto AIRS_V = vdescs(VxAirs{});
// coefficients of P(Y), deg < p, with P(w_p^k) = v[k]: in-place radix-2 inverse NTT on the host (a 2^16-entry lookup
// table is far too long for the O(p^2) sum the short selectors get away with)
void host_intt(std::vector<uint64_t>& a) {
    const size_t p = a.size();
    int lg = 0;
    while (((size_t)1 << lg) < p) ++lg;
    for (size_t i = 0; i < p; ++i) {
        const size_t j = stark_proof::brev(i, lg);
        if (j > i) std::swap(a[i], a[j]);
    }
    for (int st = 1; st <= lg; ++st) {
        const size_t half = (size_t)1 << (st - 1);
        const uint64_t wl = glh::inv(glh::root(st));
        for (size_t blk = 0; blk < p; blk += 2 * half) {
            uint64_t w = 1;
            for (size_t k = 0; k < half; ++k) {
                const uint64_t u = a[blk + k], t = glh::mul(a[blk + k + half], w);
                a[blk + k] = glh::add(u, t);
                a[blk + k + half] = glh::sub(u, t);
                w = glh::mul(w, wl);
            }
        }
    }
    const uint64_t pinv = glh::inv(p % glh::P);
    for (uint64_t& x : a) x = glh::mul(x, pinv);
}
// every refusal of this file: the reason into the caller's buffer, the code back
int32_t v_fail(int32_t code, char* err, size_t errlen, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return code;
}
#define NEED(cond, ...) \
    do {                \
        if (!(cond)) return v_fail(VX_ERR_STATEMENT, err, errlen, __VA_ARGS__); \
    } while (0)
}  // namespace


// ---- run-time AIR descriptors: the registry (process-wide; programs are immutable and never freed, ids never reused)
namespace {
std::mutex g_airp_mu;
std::map<int, std::shared_ptr<const AirProgram>> g_airp;       // live ids
std::vector<std::shared_ptr<const AirProgram>> g_airp_retired;  // kept alive: a prover may still hold the pointer
int g_airp_next = VX_AIR_USER_BASE;
#define AIRP_NEED(cond, ...) \
    do {                     \
        if (!(cond)) return v_fail(VX_ERR_ARG, err, errlen, __VA_ARGS__); \
    } while (0)
}  // namespace
const AirProgram* vx_air_program_find(int id) {
    std::lock_guard<std::mutex> lk(g_airp_mu);
    auto it = g_airp.find(id);
    return it == g_airp.end() ? nullptr : it->second.get();
}
namespace {
// the ranges of a descriptor's fields
int32_t airp_ranges_ok(const vx_air_program* in, char* err, size_t errlen) {
    AIRP_NEED(in->cols >= 1 && in->cols <= VX_AIRP_MAX_COLS, "air program: %u columns (1..%d)", in->cols, VX_AIRP_MAX_COLS);
    AIRP_NEED(in->n_public <= 64, "air program: %u public inputs (at most 64)", in->n_public);
    AIRP_NEED(in->n_periodic <= 256 && (in->n_periodic == 0 || (in->periodic_log && in->periodic_values)), "air program: bad periodic columns");
    AIRP_NEED(in->n_regs >= 1 && in->n_regs <= VX_AIRP_MAX_REGS, "air program: %u registers (1..%d)", in->n_regs, VX_AIRP_MAX_REGS);
    AIRP_NEED(in->n_consts <= 65536 && (in->n_consts == 0 || in->consts), "air program: bad constant table");
    AIRP_NEED(in->code && in->n_code >= 1 && in->n_code <= VX_AIRP_MAX_CODE, "air program: %u instructions (1..%d)", in->n_code, VX_AIRP_MAX_CODE);
    AIRP_NEED(in->aux_cols <= VX_AIRP_MAX_COLS && in->cols + in->aux_cols <= VX_AIRP_MAX_COLS && in->n_challenges <= 8 && in->n_aux_public <= 4,
              "air program: auxiliary round out of range (%u columns, %u challenges <= 8, %u published values <= 4)", in->aux_cols, in->n_challenges, in->n_aux_public);
    AIRP_NEED(in->aux_cols > 0 || (in->n_challenges == 0 && in->n_aux_public == 0 && !in->gen_aux), "air program: challenges / published values / a generator without auxiliary columns");
    AIRP_NEED(in->aux_cols == 0 || in->n_challenges > 0, "air program: an auxiliary round without a challenge is a second trace commitment, not a lookup round");
    return VX_OK;
}
// the checks of the code and the registration; `bus`: the declaration `in` was lowered from (bus_program.h), kept for the witness kernel
int32_t airp_register(const vx_air_program* in, const vx_air_bus* bus, uint32_t bus_help, int* air_id, char* err, size_t errlen) {
    if (const int32_t rc = airp_ranges_ok(in, err, errlen)) return rc;
    auto pg = std::make_shared<AirProgram>();
    if (bus) {
        pg->bus_code.assign(bus->code, bus->code + bus->n_code);
        pg->bus_consts.assign(bus->consts, bus->consts + bus->n_consts);
        pg->bus_regs = bus->n_regs, pg->bus_help = bus_help, pg->bus_block_log = (int)bus->block_log, pg->bus_step = bus->step_periodic;
    }
    pg->cols = in->cols, pg->pub = in->n_public, pg->n_regs = in->n_regs;
    pg->aux = in->aux_cols, pg->chal = in->n_challenges, pg->auxpub = in->n_aux_public, pg->gen_aux = in->gen_aux, pg->gen_aux_user = in->gen_aux_user;
    size_t n_per_values = 0;
    for (uint32_t q = 0; q < in->n_periodic; ++q) {
        AIRP_NEED(in->periodic_log[q] <= VX_AIRP_MAX_PERIOD_LOG, "air program: periodic column %u has period 2^%u (at most 2^%d)", q, in->periodic_log[q], VX_AIRP_MAX_PERIOD_LOG);
        pg->plog.push_back(in->periodic_log[q]);
        if (in->periodic_log[q] > pg->period_log) pg->period_log = in->periodic_log[q];
        n_per_values += (size_t)1 << in->periodic_log[q];
    }
    pg->periodic.assign(in->periodic_values, in->periodic_values + n_per_values);
    for (uint64_t v : pg->periodic) AIRP_NEED(v < glh::P, "air program: non-canonical periodic value");
    pg->consts.assign(in->consts, in->consts + in->n_consts);
    for (uint64_t v : pg->consts) AIRP_NEED(v < glh::P, "air program: non-canonical constant");
    pg->code.assign(in->code, in->code + in->n_code);
    // operands, def-before-use and degrees by abstract interpretation (degree of a register: columns and periodic columns 1)
    std::vector<int> deg(in->n_regs, -1);
    for (uint32_t pc = 0; pc < in->n_code; ++pc) {
        const uint64_t w = pg->code[pc];
        const AirpInsn i = airp_decode(w);
        AIRP_NEED((w >> 48) == 0, "air program: instruction %u has reserved bits set", pc);
        auto reg_ok = [&](int r) { return r >= 0 && r < (int)in->n_regs; };
        auto src = [&](int r) { return reg_ok(r) && deg[r] >= 0; };
        switch (i.op) {
            case VX_AIRP_LOC:
            case VX_AIRP_NXT:
                AIRP_NEED(reg_ok(i.d) && i.a < (int)(in->cols + in->aux_cols) && i.b == 0, "air program: instruction %u: bad column load", pc);
                deg[i.d] = 1;
                break;
            case VX_AIRP_PER:
                AIRP_NEED(reg_ok(i.d) && i.a < (int)in->n_periodic && i.b == 0, "air program: instruction %u: bad periodic load", pc);
                deg[i.d] = 1;
                break;
            case VX_AIRP_PUB:
                AIRP_NEED(reg_ok(i.d) && i.a < (int)in->n_public && i.b == 0, "air program: instruction %u: bad public-input load", pc);
                deg[i.d] = 0;
                break;
            case VX_AIRP_CONST:
                AIRP_NEED(reg_ok(i.d) && i.a < (int)in->n_consts && i.b == 0, "air program: instruction %u: bad constant load", pc);
                deg[i.d] = 0;
                break;
            case VX_AIRP_CHAL:
                AIRP_NEED(reg_ok(i.d) && i.a < (int)in->n_challenges && i.b == 0, "air program: instruction %u: bad challenge load", pc);
                deg[i.d] = 0;
                break;
            case VX_AIRP_APUB:
                AIRP_NEED(reg_ok(i.d) && i.a < (int)(2 * in->n_aux_public) && i.b == 0, "air program: instruction %u: bad published-value load", pc);
                deg[i.d] = 0;
                break;
            case VX_AIRP_ADD:
            case VX_AIRP_SUB:
            case VX_AIRP_MUL: {
                AIRP_NEED(reg_ok(i.d) && src(i.a) && src(i.b), "air program: instruction %u reads a register that was never written (or out of range)", pc);
                const int dg = i.op == VX_AIRP_MUL ? deg[i.a] + deg[i.b] : (deg[i.a] > deg[i.b] ? deg[i.a] : deg[i.b]);
                deg[i.d] = dg > 1000 ? 1000 : dg;
                break;
            }
            case VX_AIRP_ASSERT:
            case VX_AIRP_ASSERT_TRANSITION:
            case VX_AIRP_ASSERT_FIRST:
            case VX_AIRP_ASSERT_LAST: {
                AIRP_NEED(i.d == 0 && i.b == 0 && src(i.a), "air program: instruction %u asserts a register that was never written (or out of range)", pc);
                const int lim = i.op == VX_AIRP_ASSERT ? 3 : 2;
                AIRP_NEED(deg[i.a] <= lim, "air program: instruction %u asserts an expression of degree %d (limit %d: two quotient chunks per challenge)", pc, deg[i.a], lim);
                ++pg->n_constraints;
                break;
            }
            default: AIRP_NEED(false, "air program: instruction %u has unknown opcode %d", pc, i.op);
        }
    }
    AIRP_NEED(pg->n_constraints >= 1, "air program: no constraint");
    std::lock_guard<std::mutex> lk(g_airp_mu);
    AIRP_NEED(g_airp_next < 0x7FFFFFF0, "air program: id space exhausted");
    pg->id = g_airp_next++;
    *air_id = pg->id;
    g_airp[pg->id] = pg;
    return VX_OK;
}
}  // namespace
extern "C" {
int32_t vx_air_register(const vx_air_program* in, int* air_id, char* err, size_t errlen) {
    if (!in || !air_id) return VX_ERR_ARG;
    return airp_register(in, nullptr, 0, air_id, err, errlen);
}
int32_t vx_air_register_bus(const vx_air_program* in, const vx_air_bus* bus, int* air_id, char* err, size_t errlen) {
    if (!in || !bus || !air_id) return VX_ERR_ARG;
    if (const int32_t rc = airp_ranges_ok(in, err, errlen)) return rc;
    uint32_t n_msgs = 0;
    if (!busp::validate(*in, *bus, &n_msgs, err, errlen)) return VX_ERR_ARG;
    busp::Lowered lo;
    busp::lower(*in, *bus, n_msgs, &lo);
    vx_air_program all = *in;  // the program's own constraints, then the bus block
    all.code = lo.code.data(), all.n_code = (uint32_t)lo.code.size(), all.consts = lo.consts.data(), all.n_consts = (uint32_t)lo.consts.size(), all.n_regs = lo.n_regs;
    return airp_register(&all, bus, lo.n_help, air_id, err, errlen);
}
int32_t vx_air_unregister(int air_id) {
    std::lock_guard<std::mutex> lk(g_airp_mu);
    auto it = g_airp.find(air_id);
    if (it == g_airp.end()) return VX_ERR_ARG;
    g_airp_retired.push_back(it->second);
    g_airp.erase(it);
    return VX_OK;
}
}  // extern "C"

extern "C" {

int32_t vx_stark_verify(const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air,
                        const uint64_t* expect_public, size_t n_expect_public, char* err, size_t errlen) {
    return vx_stark_verify_ext(cfg, pr, len, expect_air, expect_public, n_expect_public, nullptr, nullptr, nullptr, err, errlen);
}
}  // extern "C"

// The verifier with its query phase in one of the three states of QueryPhase (vx_bus.h) and an optional sink: what the query
// phase saw, as the claims of the tables that prove it.
static int32_t stark_verify_impl(const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                 const uint64_t* ext_chal, const uint64_t** apub_out, int* log_n_out, QueryPhase mode, StarkQueries* sink, char* err, size_t errlen);
int32_t vx_stark_verify_ext(const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air, const uint64_t* expect_public,
                            size_t n_expect_public, const uint64_t* ext_chal, const uint64_t** apub_out, int* log_n_out, char* err, size_t errlen) {
    return stark_verify_impl(cfg, pr, len, expect_air, expect_public, n_expect_public, ext_chal, apub_out, log_n_out, QueryPhase::Walked, nullptr, err, errlen);
}
namespace sp = stark_proof;
static std::vector<Fx> fx_pairs(const uint64_t* w, size_t n) {
    std::vector<Fx> v(n);
    for (size_t j = 0; j < n; ++j) v[j] = {w[2 * j], w[2 * j + 1]};
    return v;
}
// The head of an untrusted proof: header -> the AIR it names -> the Shape that AIR, the degree bits and the configuration imply
// (config_ok(cfg) is the caller's).
struct ProofHead {
    AirV air{};
    std::optional<sp::Shape> shape;
};
static int32_t proof_head(const vx_stark_config& cfg, const uint64_t* pr, size_t len, int expect_air, ProofHead* head, char* err, size_t errlen) {
    AirV* const air = &head->air;
    NEED(len >= 10, "proof truncated (header)");
    NEED(pr[0] == sp::MAGIC, "bad magic");
    // (every narrow header field is compared as the 64-bit word it is: a proof has ONE encoding)
    NEED(((pr[1] | pr[2] | pr[5] | pr[6] | pr[7] | pr[8]) >> 31) == 0, "header word out of range");
    const int air_id = (int)pr[1];
    NEED(pr[2] >= 2 && pr[2] <= 26 && pr[9] <= 16, "bad shape");
    for (const AirV& a : AIRS_V)
        if (a.id == air_id) *air = a;
    if (!air->id && air_id >= VX_AIR_USER_BASE)
        if (const AirProgram* pg = vx_air_program_find(air_id))
            *air = {air_id, (int)pg->cols, (int)pg->pub, (int)pg->plog.size(), pg->period_log, 0, nullptr, nullptr, (int)pg->aux, (int)pg->chal, (int)pg->auxpub, nullptr, pg};
    NEED(air->id && (expect_air == 0 || expect_air == air_id), "unexpected AIR %d", air_id);
    head->shape.emplace(air->id, air->cols, air->aux, air->pub, air->auxpub, (int)pr[2], cfg);
    return VX_OK;
}
// The constraint identity at zeta: the AIR's constraints over the openings, combined under the two alphas, against Z_H(zeta) times
// the quotient assembled from its two chunks per challenge.
static int32_t constraints_at_zeta(const AirV& air, const sp::View& v, const uint64_t* chal, const uint64_t alphas[2], Fx zeta, char* err, size_t errlen) {
    const sp::Shape& s = *v.s;
    const size_t n = (size_t)1 << s.L;
    const uint64_t last = glh::inv(glh::root(s.L)), ninv = glh::inv(n % glh::P);
    const std::vector<Fx> o_local = fx_pairs(v.open_local(), s.c), o_next = fx_pairs(v.open_next(), s.c), o_quot = fx_pairs(v.open_quot(), sp::NQ);
    const Fx zn = fx_pow(zeta, n), one{1, 0};
    const Fx zh = zn - one;
    Consumer<Fx> cons;
    cons.acc[0] = cons.acc[1] = {0, 0};
    cons.alpha[0] = {alphas[0], 0};
    cons.alpha[1] = {alphas[1], 0};
    cons.z_last = zeta - Fx{last, 0};
    cons.l_first = zh * Fx{ninv, 0} * fx_inv(zeta - one);
    cons.l_last = zh * Fx{glh::mul(ninv, last), 0} * fx_inv(zeta - Fx{last, 0});
    std::vector<Fx> per(air.periodic ? air.periodic : 1), pubx(s.n_pub ? s.n_pub : 1), chalx(8), apubx(8);
    if (air.periodic) {
        std::vector<uint64_t> pv;
        if (air.prog) pv = air.prog->periodic;
        else air.periodic_values(pv);
        size_t in_off = 0;
        for (int j = 0; j < air.periodic; ++j) {
            const int pl = air.prog ? air.prog->plog[j] : air.plog(j);
            const size_t p = (size_t)1 << pl;
            NEED(in_off + p <= pv.size(), "periodic table of AIR %d is short", air.id);
            std::vector<uint64_t> coef(pv.begin() + in_off, pv.begin() + in_off + p);
            host_intt(coef);
            const Fx y = fx_pow(zeta, n >> pl);
            Fx a{0, 0};
            for (size_t k = p; k-- > 0;) a = a * y + Fx{coef[k], 0};
            per[j] = a;
            in_off += p;
        }
    }
    for (size_t i = 0; i < s.n_pub; ++i) pubx[i] = {v.pub()[i], 0};
    for (int q = 0; q < air.chal; ++q) chalx[q] = {chal[q], 0};
    for (size_t q = 0; s.ca && q < 2 * s.auxpub; ++q) apubx[q] = {v.apub()[q], 0};
    HostRow loc{o_local.data()}, nxt{o_next.data()};
    if (air.prog) air_program_eval<Fx>(*air.prog, loc, nxt, per.data(), pubx.data(), chalx.data(), apubx.data(), cons);
    else air.eval(loc, nxt, per.data(), pubx.data(), chalx.data(), apubx.data(), cons);
    for (int k = 0; k < 2; ++k) {
        const Fx q = o_quot[2 * k] + o_quot[2 * k + 1] * zn;
        NEED(fx_eq(cons.acc[k], zh * q), "constraint identity fails at zeta (challenge %d)", k);
    }
    return VX_OK;
}
// the refusal of an opening, for the walked check and the deferred one (kind: DeferredPaths::Opening, vx_bus.h)
static int32_t opening_invalid(int kind, size_t layer, size_t qi, char* err, size_t errlen) {
    if (kind == DeferredPaths::LAYER) return v_fail(VX_ERR_STATEMENT, err, errlen, "FRI layer %zu Merkle proof invalid (query %zu)", layer, qi);
    return v_fail(VX_ERR_STATEMENT, err, errlen, "%s Merkle proof invalid (query %zu)", kind == DeferredPaths::TRACE ? "trace" : kind == DeferredPaths::AUX ? "auxiliary" : "quotient", qi);
}
// The FRI query phase (verify_fri_proof): per query the three rows under their caps, the combination of their words
// (fri_combine_initial), and per layer the coset's leaf under its cap and its fold at beta (compute_evaluation), down to the
// final polynomial.  The arithmetic of a query is stated once; the modes differ in what happens to an OPENING: walked here,
// left to the tables of a bus group (with a sink it is recorded as their claim either way: of the path only its position in the
// proof is noted, no word of it is read), or -- query-free -- skipped with the whole record: the indices alone are derived.
template <class T>  // T: the transcript, over whichever challenger (stark_proof.h)
static int32_t fri_queries(const sp::View& v, T& ch, Fx alpha, Fx zeta, const std::vector<Fx>& betas, QueryPhase mode, StarkQueries* sink, char* err, size_t errlen) {
    const sp::Shape& s = *v.s;
    const size_t c = s.c, nq = sp::NQ, N = (size_t)1 << s.LN, n_layers = s.arities.size();
    const Fx zeta_next = fx_scale(zeta, glh::root(s.L));
    const sp::Reduced red = sp::reduce_openings(alpha, v.open_local(), v.open_next(), v.open_quot(), c, nq);
    auto opening = [&](uint64_t tree, size_t index, const uint64_t* leaf, size_t leaf_len, const uint64_t* sib, int depth, const uint64_t* cap) {
        if (sink) {
            StarkOpenings& so = sink->so;
            so.claims.push_back({tree, index, so.leaves.size(), leaf_len, (size_t)(sib - v.pr), depth});
            so.leaves.insert(so.leaves.end(), leaf, leaf + leaf_len);
        }
        return mode != QueryPhase::Walked || glh::merkle_path_ok(leaf, leaf_len, index, sib, depth, cap);
    };
    for (size_t qi = 0; qi < (size_t)s.num_queries; ++qi) {
        size_t x_index = ch.query_index(N);
        if (sink) sink->so.index.push_back(x_index);
        if (mode == QueryPhase::QueryFree) continue;  // every other step of a query is proven by the tables of vx_stark_queries_prove
        const sp::Query<const uint64_t> q = v.query(qi);
        if (!opening(VX_SOPEN_TREE0, x_index, q.row_t(), s.cm, q.sib_t(), s.depth0, v.cap_trace())) return opening_invalid(DeferredPaths::TRACE, 0, qi, err, errlen);
        if (s.ca && !opening(VX_SOPEN_TREE0 + 1, x_index, q.row_a(), s.ca, q.sib_a(), s.depth0, v.cap_aux())) return opening_invalid(DeferredPaths::AUX, 0, qi, err, errlen);
        if (!opening(VX_SOPEN_TREE0 + 2, x_index, q.row_q(), nq, q.sib_q(), s.depth0, v.cap_quot())) return opening_invalid(DeferredPaths::QUOT, 0, qi, err, errlen);
        uint64_t x = sp::query_point(x_index, s.LN);
        Fx s1{0, 0}, ap{1, 0};
        for (size_t j = 0; j < c; ++j) {
            s1 = s1 + ap * Fx{j < s.cm ? q.row_t()[j] : q.row_a()[j - s.cm], 0};
            ap = ap * alpha;
        }
        Fx s0 = s1;
        for (size_t j = 0; j < nq; ++j) {
            s0 = s0 + ap * Fx{q.row_q()[j], 0};
            ap = ap * alpha;
        }
        Fx ev = red.alpha_c * (s0 - red.y0) * fx_inv(Fx{x, 0} - zeta) + (s1 - red.y1) * fx_inv(Fx{x, 0} - zeta_next);
        if (sink) {
            sink->ev0.push_back(ev.a), sink->ev0.push_back(ev.b);
            sink->rows.insert(sink->rows.end(), q.row_t(), q.row_t() + s.cm);
            sink->rows.insert(sink->rows.end(), q.row_a(), q.row_a() + s.ca);
            sink->rows.insert(sink->rows.end(), q.row_q(), q.row_q() + nq);
        }
        for (size_t l = 0; l < n_layers; ++l) {
            const int a = s.arities[l];
            const size_t arity = (size_t)1 << a, within = x_index & (arity - 1);
            std::vector<uint64_t> leaf(2 * arity);
            for (size_t t = 0, src = 0; t < arity; ++t) {
                if (t == within) {
                    leaf[2 * t] = ev.a, leaf[2 * t + 1] = ev.b;
                } else {
                    leaf[2 * t] = q.evals(l)[2 * src], leaf[2 * t + 1] = q.evals(l)[2 * src + 1];
                    ++src;
                }
            }
            if (sink) sink->leaves.insert(sink->leaves.end(), leaf.begin(), leaf.end());
            if (!opening(l, x_index >> a, leaf.data(), 2 * arity, q.sibs(l), s.depth[l], v.layer_cap(l))) return opening_invalid(DeferredPaths::LAYER, l, qi, err, errlen);
            // compute_evaluation: interpolate the coset {x g^i} and evaluate at beta
            const uint64_t g = glh::root(a);
            std::vector<Fx> evn(arity);
            for (size_t t = 0; t < arity; ++t) evn[sp::brev(t, a)] = {leaf[2 * t], leaf[2 * t + 1]};
            const uint64_t start = glh::mul(x, glh::pow(g, arity - sp::brev(within, a)));
            std::vector<uint64_t> pts(arity);
            uint64_t gp = 1;
            for (size_t t = 0; t < arity; ++t) {
                pts[t] = glh::mul(start, gp);
                gp = glh::mul(gp, g);
            }
            Fx acc{0, 0};
            for (size_t i = 0; i < arity; ++i) {
                Fx num{1, 0};
                uint64_t den = 1;
                for (size_t j = 0; j < arity; ++j) {
                    if (j == i) continue;
                    num = num * (betas[l] - Fx{pts[j], 0});
                    den = glh::mul(den, glh::sub(pts[i], pts[j]));
                }
                acc = acc + evn[i] * num * Fx{glh::inv(den), 0};
            }
            ev = acc;
            x = glh::pow(x, arity);
            x_index >>= a;
        }
        NEED(fx_eq(sp::final_poly_at(v.final_poly(), s.final_len, x), ev), "final polynomial evaluation mismatch (query %zu)", qi);
        if (sink) sink->ev_last.push_back(ev.a), sink->ev_last.push_back(ev.b);
    }
    return VX_OK;
}
// The verifier, stated once over the transcript `ch` (sp::TranscriptOf<C>): C hashes (every verifier so far), hashes and records
// (the prover of TranscriptAir), or answers with claimed challenges and hashes nothing (vx_stark_transcripts_verify).  head_ok: a
// proof that ends at its head is accepted and read query-free whatever `mode` says (a whole proof is read in `mode`).
template <class T>
static int32_t stark_verify_over(T& ch, bool head_ok, const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                 const uint64_t* ext_chal, const uint64_t** apub_out, int* log_n_out, QueryPhase mode, StarkQueries* sink, char* err, size_t errlen) {
    if (!cfg || !pr) return VX_ERR_ARG;
    if (!sp::config_ok(*cfg)) return v_fail(VX_ERR_ARG, err, errlen, "stark verify: configuration out of range");
    ProofHead head;
    VX_TRY(proof_head(*cfg, pr, len, expect_air, &head, err, errlen));
    // the header is the one this AIR, these degree bits and the configuration imply, word for word
    const AirV& air = head.air;
    const sp::Shape& shape = *head.shape;
    const std::vector<uint64_t> hdr = shape.header_words();
    for (size_t i = 0; i < hdr.size(); ++i)
        NEED(i < len && pr[i] == hdr[i], "%s", i >= 5 && i <= 8 ? "config mismatch" : i >= 9 && i < hdr.size() - 2 ? "FRI plan mismatch" : "shape mismatch");
    // the proof is untrusted input: the shapes the prover refuses (vx_stark_prove_impl) are refused here too, so no Merkle depth
    // below can go negative (a crafted L = 2 proof used to reach the Merkle check with n_sib = SIZE_MAX)
    NEED(shape.LN >= shape.cap_h && shape.LN <= 27 && shape.L >= air.period_log, "degree bits %d out of range for this AIR / cap height", shape.L);
    NEED(!air.exact_log || shape.L == air.period_log, "this AIR has positional columns of period 2^%d: a trace of 2^%d rows is not acceptable", air.period_log, shape.L);
    // every word that is read is canonical -- the whole proof, everything but the siblings, or the head alone
    if (head_ok && len == shape.o_queries) mode = QueryPhase::QueryFree;
    const bool query_free = mode == QueryPhase::QueryFree;
    if (mode == QueryPhase::Walked || mode == QueryPhase::Deferred)
        for (size_t i = hdr.size(); i < len; ++i) NEED(pr[i] < glh::P, "non-canonical element at word %zu", i);
    sp::View v;
    const char* bad_length = query_free ? sp::View::parse_head(pr, len, shape, &v) : sp::View::parse(pr, len, shape, &v);
    if (query_free) NEED(!bad_length, "%s (%zu words, this shape has %zu and its head %zu)", bad_length, len, shape.words(), shape.o_queries);
    NEED(!bad_length, "%s (%zu words, this shape has %zu)", bad_length, len, shape.words());
    if (query_free) {  // the head alone is read
        for (size_t i = hdr.size(); i < shape.o_queries; ++i) NEED(pr[i] < glh::P, "non-canonical element at word %zu", i);
    } else if (mode == QueryPhase::Delegated) {  // everything but the siblings: in this mode none of their words is read
        auto canonical = [&](size_t from, size_t n) -> size_t {
            for (size_t i = from; i < from + n; ++i)
                if (pr[i] >= glh::P) return i;
            return 0;
        };
        size_t bad = canonical(hdr.size(), shape.o_queries - hdr.size());
        for (size_t k = 0; k < (size_t)shape.num_queries && !bad; ++k) {
            const size_t at = shape.o_queries + k * shape.q_words;
            bad = canonical(at, shape.cm);
            if (!bad) bad = canonical(at + shape.q_row_a, shape.ca);
            if (!bad) bad = canonical(at + shape.q_row_q, sp::NQ);
            for (size_t l = 0; l < shape.arities.size() && !bad; ++l) bad = canonical(at + shape.q_layer[l], 2 * (((size_t)1 << shape.arities[l]) - 1));
        }
        NEED(!bad, "non-canonical element at word %zu", bad);
    }
    if (expect_public) {
        NEED(n_expect_public == shape.n_pub, "public input count differs");
        for (size_t i = 0; i < shape.n_pub; ++i) NEED(v.pub()[i] == expect_public[i], "public input %zu differs", i);
    }
    ch.trace(v);
    uint64_t chal[8] = {0}, alphas[2];
    if (shape.ca) {  // auxiliary round: lookup challenges after the trace cap, then the published values and the second cap
        NEED(air.chal <= 8 && 2 * air.auxpub <= 8, "AIR %d auxiliary round is misconfigured", air.id);
        ch.lookup_challenges(chal, (size_t)air.chal, ext_chal);
        ch.aux(v);
    }
    ch.alphas(alphas);
    const Fx zeta = ch.zeta(v);
    VX_TRY(constraints_at_zeta(air, v, chal, alphas, zeta, err, errlen));
    const Fx alpha = ch.alpha(v);
    std::vector<Fx> betas;
    for (size_t l = 0; l < shape.arities.size(); ++l) betas.push_back(ch.beta(v, l));
    ch.final_poly(v);
    NEED(ch.pow_ok(*v.nonce(), shape.pow_bits), "proof of work invalid");
    if (sink) {
        *sink = StarkQueries();
        StarkOpenings& m = sink->so;
        m.LN = shape.LN, m.a = cfg->arity_bits, m.cap_h = shape.cap_h, m.cm = shape.cm, m.ca = shape.ca, m.NL = shape.arities.size(), m.n_queries = (size_t)shape.num_queries;
        auto tree = [&](uint64_t id, const uint64_t* cap) { m.tree.push_back(id), m.caps.insert(m.caps.end(), cap, cap + shape.cap_words); };
        tree(VX_SOPEN_TREE0, v.cap_trace());
        if (shape.ca) tree(VX_SOPEN_TREE0 + 1, v.cap_aux());
        tree(VX_SOPEN_TREE0 + 2, v.cap_quot());
        for (size_t l = 0; l < m.NL; ++l) tree(l, v.layer_cap(l));
        sink->rate_bits = cfg->rate_bits, sink->nq = sp::NQ, sink->alpha[0] = alpha.a, sink->alpha[1] = alpha.b, sink->zeta[0] = zeta.a, sink->zeta[1] = zeta.b;
        sink->openings.assign(v.open_local(), v.open_local() + 2 * shape.c);
        sink->openings.insert(sink->openings.end(), v.open_next(), v.open_next() + 2 * shape.c);
        sink->openings.insert(sink->openings.end(), v.open_quot(), v.open_quot() + 2 * sp::NQ);
        for (const Fx& b : betas) sink->betas.push_back(b.a), sink->betas.push_back(b.b);
        sink->final_poly.assign(v.final_poly(), v.final_poly() + 2 * shape.final_len);
    }
    VX_TRY(fri_queries(v, ch, alpha, zeta, betas, mode, sink, err, errlen));
    const uint64_t* apub = shape.ca ? v.apub() : nullptr;
    if (shape.ca && !ext_chal)  // a stand-alone proof has nobody to cancel a bus total against
        for (size_t q = 0; q < 2 * shape.auxpub; ++q) NEED(apub[q] == 0, "stand-alone proof publishes a non-zero bus total");
    if (apub_out) *apub_out = apub;
    if (log_n_out) *log_n_out = shape.L;
    return VX_OK;
}
static int32_t stark_verify_impl(const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                 const uint64_t* ext_chal, const uint64_t** apub_out, int* log_n_out, QueryPhase mode, StarkQueries* sink, char* err, size_t errlen) {
    sp::Transcript ch;
    return stark_verify_over(ch, false, cfg, pr, len, expect_air, expect_public, n_expect_public, ext_chal, apub_out, log_n_out, mode, sink, err, errlen);
}
// The deferred form (vx_bus.h): the pass of one proof keeps what its query phase recorded ...
int32_t DeferredPaths::pass(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public, const uint64_t* ext_chal,
                            const uint64_t** apub_out, int* log_n_out, char* err, size_t errlen) {
    StarkQueries sq;
    const int32_t rc = stark_verify_impl(cfg, proof, len, expect_air, expect_public, n_expect_public, ext_chal, apub_out, log_n_out, QueryPhase::Deferred, &sq, err, errlen);
    // a query records all its openings before its one check that can fail (the final polynomial): whole queries, in record order
    const StarkOpenings& so = sq.so;
    const size_t per_query = so.tree.size(), tree0 = batch.log_leaves.size();
    if (so.claims.empty()) return rc;
    const size_t first_layer = per_query - so.NL;
    batch.cap_height = so.cap_h;
    batch.caps.insert(batch.caps.end(), so.caps.begin(), so.caps.end());
    for (size_t pos = 0; pos < per_query; ++pos) batch.log_leaves.push_back(so.claims[pos].n_sib + so.cap_h);
    for (size_t k = 0; k < so.claims.size(); ++k) {
        const StarkOpenings::Claim& c = so.claims[k];
        const size_t pos = k % per_query;
        batch.tree_of.push_back(tree0 + pos), batch.leaf_idx.push_back(c.index), batch.leaf_len.push_back(c.leaf_len);
        batch.siblings.insert(batch.siblings.end(), proof + c.sib, proof + c.sib + 4 * (size_t)c.n_sib);
        opening.push_back({pos >= first_layer ? LAYER : pos == 0 ? TRACE : pos + 1 == first_layer ? QUOT : AUX, pos >= first_layer ? pos - first_layer : 0, k / per_query});
    }
    batch.leaves.insert(batch.leaves.end(), so.leaves.begin(), so.leaves.end());
    return rc;
}
// ... and the openings of every pass are checked together: the first that fails is what the walked verifier would have said
int32_t DeferredPaths::settle(int32_t verdict, char* err, size_t errlen) {
    if (opening.empty()) return verdict;
    size_t bad = SIZE_MAX;
    char own[256] = "";
    const int32_t rc = check(batch, &bad, own, sizeof own);
    if (rc != VX_OK) return v_fail(rc, err, errlen, "%s", own);
    if (bad == SIZE_MAX) return verdict;
    return opening_invalid(opening[bad].kind, opening[bad].layer, opening[bad].query, err, errlen);
}
// ... over the recording challenger (vx_bus.h): what the transcript of a valid proof did, as TranscriptAir's chain
int32_t vx_stark_transcript_record(const vx_stark_config* cfg, const uint64_t* proof, size_t len, const uint64_t* ext_chal, glh::TranscriptRecord* out, char* err, size_t errlen) {
    sp::TranscriptOf<glh::RecordingChallenger> ch;
    VX_TRY(stark_verify_over(ch, true, cfg, proof, len, 0, nullptr, 0, ext_chal, nullptr, nullptr, QueryPhase::Walked, nullptr, err, errlen));
    *out = static_cast<const glh::TranscriptRecord&>(ch);
    return VX_OK;
}
// ... and with the claims of the query phase from the same run (vx_bus.h): the one replay of vx_stark_inner_prove
int32_t vx_stark_inner_replay(const vx_stark_config* cfg, const uint64_t* proof, size_t len, const uint64_t* ext_chal, bool head_ok, StarkQueries* sq, glh::TranscriptRecord* rec, char* err,
                              size_t errlen) {
    sp::TranscriptOf<glh::RecordingChallenger> ch;
    VX_TRY(stark_verify_over(ch, head_ok, cfg, proof, len, 0, nullptr, 0, ext_chal, nullptr, nullptr, QueryPhase::Delegated, sq, err, errlen));
    *rec = static_cast<const glh::TranscriptRecord&>(ch);
    return VX_OK;
}

// One table of a bus group: its serialised proof, what peek_tables reads from it (public inputs, trace cap), and what the
// request implies for it (AIR id, public inputs).
struct BusTable {
    const uint64_t* proof;
    size_t len;
    const uint64_t *pub = nullptr, *cap = nullptr;
    size_t n_pub = 0;
    int air = 0;
    const uint64_t* want = nullptr;
    size_t n_want = 0;
    void expect(int air_id, const uint64_t* public_inputs, size_t n) { air = air_id, want = public_inputs, n_want = n; }
};
static bool peek_tables(const vx_stark_config* cfg, BusTable* t, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!stark_proof::peek(t[i].proof, t[i].len, cfg->cap_height, &t[i].pub, &t[i].n_pub, &t[i].cap)) return false;
    return true;
}
// The messages a party outside the tables puts on their bus -- the verifier itself, in an aggregation proof: the denominator of
// each, and whether the verifier receives it (+) or sends it (-).
using VBus = bus::Bus<X2<Fx>>;
struct BusMessages {
    std::vector<X2<Fx>> den;
    std::vector<uint64_t> mult;  // what the message adds to the right-hand side, in units of 1 / D: a canonical field word
    void reserve(size_t n) { den.reserve(n), mult.reserve(n); }
    void put(const X2<Fx>& d, uint64_t m) { den.push_back(d), mult.push_back(m); }
    void receive(const X2<Fx>& d) { put(d, 1); }
    void send(const X2<Fx>& d) { put(d, glh::P - 1); }
    // What the aggregation verifiers say about a query phase, each stated once.  The root a path ended in with the tree's depth,
    // in its two halves: the tables do not know which root belongs to which tree, the verifier does
    void receive_root(const VBus& bus, uint64_t tree, const uint64_t root[4], int depth) {
        const Fx t{tree, 0}, d{(uint64_t)depth, 0};
        receive(bus.root(t, Fx{root[0], 0}, Fx{root[1], 0}, bus::K<0>{}, d));
        receive(bus.root(t, Fx{root[2], 0}, Fx{root[3], 0}, bus::K<1>{}, d));
    }
    // the 32 words of the leaf a query opens in layer tree `layer` (arity 16)
    void send_layer_leaf(const VBus& bus, size_t layer, uint64_t index, const uint64_t leaf[32]) {
        for (size_t j = 0; j < 32; ++j) send(bus.row_of(Fx{(uint64_t)layer, 0}, Fx{index >> (4 * (layer + 1)), 0}, Fx{(uint64_t)j, 0}, Fx{leaf[j], 0}));
    }
    // the exit of a fold chain: the final polynomial at x_NL = x_0^(16^NL)
    void receive_exit(const VBus& bus, uint64_t index, int log_lde, size_t n_layers, const uint64_t* final_poly, size_t final_len) {
        const Fx fp = stark_proof::final_poly_at(final_poly, final_len, glh::pow(stark_proof::query_point(index, log_lde), (uint64_t)1 << (4 * n_layers)));
        receive(bus.fri(Fx{index, 0}, Fx{fp.a, 0}, Fx{fp.b, 0}, bus::K<1>{}));
    }
};
using BusOutside = std::function<void(const VBus&, BusMessages&)>;
// sum over the messages of mult / D (a received message counts + 1 / D, a sent one - 1 / D) with ONE inversion (Montgomery batch: prefix products, one inverse, walked back); false when
// the product of the denominators is zero
static bool bus_messages_sum(const BusMessages& m, X2<Fx>* sum) {
    const Fx zero{0, 0};
    *sum = X2<Fx>{zero, zero};
    const size_t n = m.den.size();
    if (!n) return true;
    std::vector<X2<Fx>> pre(n);
    for (size_t k = 0; k < n; ++k) pre[k] = k ? pre[k - 1] * m.den[k] : m.den[k];
    const X2<Fx>& prod = pre[n - 1];
    const Fx norm = prod.a * prod.a - f_mul7(prod.b * prod.b);
    if (norm.a == 0 && norm.b == 0) return false;
    const Fx ni = fx_inv(norm);
    X2<Fx> inv{prod.a * ni, (zero - prod.b) * ni};
    for (size_t k = n; k-- > 0;) {
        const X2<Fx> t = k ? inv * pre[k - 1] : inv;
        const uint64_t mu = m.mult[k];
        *sum = mu == 1 ? *sum + t : mu == glh::P - 1 ? *sum - t : *sum + t * Fx{mu, 0};
        inv = inv * m.den[k];
    }
    return true;
}
// The tables of one logUp bus, in bus order (the order of the shared-challenge transcript): the lookup challenges every proof must
// have used are a transcript of all (public inputs, trace cap) pairs; every table is verified under them against its expected
// AIR and public inputs; and the bus must close -- a table publishes its total / rows, and the sum of total x rows over the
// tables must be what the messages of the party `outside` them sum to: zero when the tables are a closed statement
// (vx_header_range_verify, vx_rotate_verify), the verifier's own claims when it is the last party of the bus (the aggregation
// verifiers vx_merkle_openings_verify, vx_merkle_rows_verify, vx_fri_fold_verify).
// With `paths` every table is read in the deferred form: its openings are kept for the caller's settle(), none is walked here.
static int32_t verify_bus_group(const vx_stark_config* cfg, const BusTable* t, size_t n, const char* unbalanced, char* err, size_t errlen, const BusOutside& outside = nullptr,
                                DeferredPaths* paths = nullptr) {
    std::vector<const uint64_t*> pubs(n), caps(n);
    std::vector<size_t> n_pubs(n);
    for (size_t i = 0; i < n; ++i) pubs[i] = t[i].pub, n_pubs[i] = t[i].n_pub, caps[i] = t[i].cap;
    uint64_t chal[4];
    stark_proof::shared_challenges_n(pubs.data(), n_pubs.data(), caps.data(), n, (size_t)4 << cfg->cap_height, chal, 4);
    uint64_t bus[2] = {0, 0};
    for (size_t i = 0; i < n; ++i) {
        const uint64_t* apub = nullptr;
        int L = 0;
        const int32_t rc = paths ? paths->pass(cfg, t[i].proof, t[i].len, t[i].air, t[i].want, t[i].n_want, chal, &apub, &L, err, errlen)
                                 : vx_stark_verify_ext(cfg, t[i].proof, t[i].len, t[i].air, t[i].want, t[i].n_want, chal, &apub, &L, err, errlen);
        if (rc != VX_OK) return rc;
        for (int q = 0; q < 2; ++q) bus[q] = glh::add(bus[q], glh::mul(apub[q], ((uint64_t)1 << L) % glh::P));
    }
    BusMessages msgs;
    if (outside) outside(VBus(Fx{chal[0], 0}, Fx{chal[1], 0}, Fx{chal[2], 0}, Fx{chal[3], 0}), msgs);
    X2<Fx> sum;
    NEED(bus_messages_sum(msgs, &sum), "a message of the verifier has a zero denominator under the challenges");
    NEED(sum.a.b == 0 && sum.b.b == 0 && bus[0] == sum.a.a && bus[1] == sum.b.a, "%s", unbalanced);
    return VX_OK;
}

// An aggregation blob (vx_bus.h: magic, the request words, one length per proof, the proofs) as the tables of its bus group: the
// blob must be for this request, every proof present and the lengths must add up to the blob.
static int32_t read_blob(const uint64_t* blob, size_t len, uint64_t magic, const char* what, const uint64_t* request, size_t n_request, BusTable* t, size_t n, char* err,
                         size_t errlen) {
    const size_t hdr = 1 + n_request + n;
    NEED(len > hdr && blob[0] == magic, "bad %s blob", what);
    NEED(std::equal(request, request + n_request, blob + 1), "blob is for a different request");
    size_t body = len - hdr;
    const uint64_t* p = blob + hdr;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t l = blob[hdr - n + i];
        NEED(l >= 1 && l <= body, "blob lengths are inconsistent");
        t[i].proof = p, t[i].len = l;
        p += l, body -= l;
    }
    NEED(body == 0, "blob lengths are inconsistent");
    return VX_OK;
}
static int32_t read_blob(const uint64_t* blob, size_t len, uint64_t magic, const char* what, std::initializer_list<uint64_t> request, BusTable* t, size_t n, char* err,
                         size_t errlen) {
    return read_blob(blob, len, magic, what, request.begin(), request.size(), t, n, err, errlen);
}
// the root of a tree known by its cap (a table proves paths to ONE root): the two-to-one fold of the cap
static int32_t cap_root(const uint64_t* cap, int cap_height, const char* what, uint64_t root[4], char* err, size_t errlen) {
    for (size_t i = 0; i < ((size_t)4 << cap_height); ++i) NEED(cap[i] < glh::P, "%s: non-canonical cap word", what);
    vx_cap_fold(cap, cap_height, root);
    return VX_OK;
}

// Expected public inputs and AIR ids of the three justification tables (vx_bus.h).
int32_t vx_justification_expect(const uint64_t* ppub_chain, size_t n_chain, const uint64_t* ppub_ed, size_t n_ed, size_t n_s512, const uint8_t authority_set_hash[32],
                                uint64_t authority_set_id, const uint8_t block_hash[32], uint32_t block_number, uint64_t round, uint64_t spub[10], uint64_t epub[2],
                                uint64_t hpub[15], int air[3], char* err, size_t errlen) {
    NEED(n_chain == 10 && n_ed == 2 && n_s512 == 15, "justification proofs have the wrong number of public inputs");
    // the request's authority_set_hash must be the proven commitment; the number of authorities it binds and the number of verified
    // signatures are read from the proofs: signed * 3 > authorities * 2 (justification.rs:164-186)
    be_limbs(authority_set_hash, spub);
    const uint64_t n_auth = ppub_chain[8], n_signed = ppub_ed[0];
    NEED(n_auth >= 1 && n_auth <= 512 && n_signed <= n_auth, "implausible authority counts");
    NEED(n_signed * 3 > n_auth * 2, "fewer than 2/3 of the authority set signed (%llu of %llu)", (unsigned long long)n_signed, (unsigned long long)n_auth);
    spub[8] = n_auth, spub[9] = 1;
    epub[0] = n_signed, epub[1] = 1;
    air[0] = VX_AIR_SHA_CHAIN;
    air[1] = ed_air_id(n_signed), air[2] = s512_air_id(n_signed);  // the tables are sized by the number of signatures they verify
    // the signed message: the precommit for (block hash, block number, round, set id) -- decoder.rs:159-200
    uint8_t msg[64];
    memset(msg, 0, sizeof msg);
    msg[0] = 1;
    memcpy(msg + 1, block_hash, 32);
    for (int b = 0; b < 4; ++b) msg[33 + b] = (uint8_t)(block_number >> (8 * b));
    for (int b = 0; b < 8; ++b) msg[37 + b] = (uint8_t)(round >> (8 * b)), msg[45 + b] = (uint8_t)(authority_set_id >> (8 * b));
    msg[53] = 0x80;
    for (int j = 0; j < 7; ++j) {
        uint64_t v = 0;
        for (int b = 0; b < 8; ++b) v = (v << 8) | msg[8 * j + b];
        hpub[2 * j] = v & 0xFFFFFFFFULL, hpub[2 * j + 1] = v >> 32;
    }
    hpub[14] = 1;
    return VX_OK;
}

// The two circuit verifiers, each stated once: walked (paths == nullptr) or in the deferred form, which the caller settles.
static int32_t header_range_verify_over(DeferredPaths* paths, const vx_stark_config* cfg, const uint64_t* blob, size_t len, uint32_t max_headers, uint32_t trusted_block,
                                        const uint8_t trusted_hash[32], uint64_t authority_set_id, const uint8_t* authority_set_hash, uint32_t target_block, const uint8_t out96[96],
                                        char* err, size_t errlen) {
    if (!cfg || !blob || !trusted_hash || !out96) return VX_ERR_ARG;
    NEED(len > VX_HR_BLOB_FIXED_WORDS + 1 && blob[0] == VX_HR_BLOB_MAGIC, "bad header_range blob");
    NEED(blob[1] == max_headers && blob[2] == trusted_block && blob[3] == target_block, "blob is for a different request");
    NEED(memcmp(blob + 4, out96, 96) == 0, "public outputs differ from the blob");
    NEED(target_block > trusted_block, "empty block range");
    const uint64_t S = blob[16];
    NEED(S >= 1 && S <= VX_HR_MAX_SEGMENTS && S <= (uint64_t)target_block - trusted_block, "bad number of map segments");
    const size_t HDR = VX_HR_BLOB_FIXED_WORDS + (size_t)S;
    NEED(len > HDR, "bad header_range blob");
    // proofs in blob order: the S hash-chain segments, authority-set commitment, Merkle, Ed25519, SHA-512
    const size_t NB = (size_t)S + 4;
    std::vector<size_t> plen(NB), off(NB);
    size_t tot = HDR;
    for (size_t t = 0; t < NB; ++t) {
        plen[t] = t < S ? blob[VX_HR_BLOB_FIXED_WORDS + t] : blob[17 + (t - S)];
        NEED(plen[t] <= len, "blob lengths are inconsistent");
        off[t] = tot, tot += plen[t];
    }
    NEED(tot == len, "blob lengths are inconsistent");
    for (size_t s = 0; s < S; ++s) NEED(plen[s] > 0, "a map segment of the hash-chain table is missing");
    NEED(plen[S + 1] > 0, "the Merkle table is missing");
    const bool justified = plen[S] > 0;
    NEED(justified ? (plen[S + 2] > 0 && plen[S + 3] > 0) : (plen[S + 2] == 0 && plen[S + 3] == 0), "blob carries part of a justification");
    NEED(!authority_set_hash || justified, "blob carries no authority-set commitment proof");
    NEED(!justified || authority_set_hash, "blob carries a justification: the request's authority_set_hash is needed to check it");
    const int tree_id = tree_air_id(max_headers);
    NEED(tree_id, "max_headers %u has no Merkle AIR", max_headers);
    // bus order (the order of the shared-challenge transcript): segments, Merkle, commitment, Ed25519, SHA-512
    const size_t n_tab = (size_t)S + (justified ? 4 : 1);
    std::vector<BusTable> tab(n_tab);
    for (size_t t = 0; t < n_tab; ++t) {
        const size_t b = t < S ? t : (t == S ? S + 1 : (t == S + 1 ? S : t));  // bus index -> blob index
        tab[t].proof = blob + off[b], tab[t].len = plen[b];
    }
    NEED(peek_tables(cfg, tab.data(), n_tab), "proofs are too short to hold a trace cap");
    // public inputs of every table, rebuilt from the request and the claimed outputs.  The hash a segment ends with is read from
    // its own proof and must be the hash the next segment starts from (the reference's reduce step, subchain_verification.rs:
    // 247-257): the first starts at trusted_header_hash / trusted_block + 1, the last ends at target_header_hash / target_block,
    // block numbers run on from segment to segment, and every segment counts its Merkle leaves from trusted_block + 1
    std::vector<uint64_t> spubs(20 * (size_t)S);
    uint64_t tpub[17], cpub[10], epub[2], hpub[15];
    uint64_t next_first = (uint64_t)trusted_block + 1;
    for (size_t s = 0; s < S; ++s) {
        uint64_t* pub = spubs.data() + 20 * s;
        NEED(tab[s].n_pub == 20, "a hash-chain segment has %zu public inputs", tab[s].n_pub);
        for (int j = 0; j < 8; ++j) {
            uint32_t a;
            memcpy(&a, trusted_hash + 4 * j, 4);
            pub[j] = s == 0 ? a : tab[s - 1].pub[8 + j];                      // starts where the previous segment ended
            uint32_t b;
            memcpy(&b, out96 + 4 * j, 4);                                     // target_header_hash = first 32 output bytes
            pub[8 + j] = s + 1 == S ? b : tab[s].pub[8 + j];                  // an inner boundary: the segment's own claim, bound by the next one
            NEED(pub[8 + j] >> 32 == 0, "a segment hash limb is out of range");
        }
        const uint64_t last = s + 1 == S ? target_block : tab[s].pub[17];
        NEED(last >= next_first && last <= target_block, "the block numbers of the map segments do not run on");
        pub[16] = next_first, pub[17] = last;
        pub[18] = (uint64_t)trusted_block + 1;  // the block of Merkle leaf 0
        pub[19] = 1;                            // bus on
        next_first = last + 1;
    }
    NEED(next_first == (uint64_t)target_block + 1, "the map segments do not cover the block range");
    be_limbs(out96 + 32, tpub), be_limbs(out96 + 64, tpub + 8);  // state_root_merkle_root || data_root_merkle_root as big-endian words
    tpub[16] = (uint64_t)target_block - trusted_block;  // the number of headers = of enabled leaves: the Merkle table MUST take every header's roots from the bus
    NEED(tpub[16] <= max_headers, "the block range exceeds max_headers");
    for (size_t s = 0; s < S; ++s) tab[s].expect(VX_AIR_BLAKE_CHAIN, spubs.data() + 20 * s, 20);
    tab[S].expect(tree_id, tpub, 17);
    if (justified) {
        int jair[3];
        const int32_t rc = vx_justification_expect(tab[S + 1].pub, tab[S + 1].n_pub, tab[S + 2].pub, tab[S + 2].n_pub, tab[S + 3].n_pub, authority_set_hash, authority_set_id, out96,
                                                   target_block, blob[21], cpub, epub, hpub, jair, err, errlen);
        if (rc != VX_OK) return rc;
        const uint64_t* jwant[3] = {cpub, epub, hpub};
        const size_t jn[3] = {10, 2, 15};
        for (int q = 0; q < 3; ++q) tab[S + 1 + q].expect(jair[q], jwant[q], jn[q]);
    }
    // the bus closes: state roots and data roots of the hashed headers = the leaves of the Merkle trees; the keys of the signed
    // authorities = the keys the signatures verify under; R || A and H between the curve table and the SHA-512 table
    return verify_bus_group(cfg, tab.data(), n_tab, "the lookup bus between the tables does not balance", err, errlen, nullptr, paths);
}

extern "C" {

int32_t vx_header_range_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, uint32_t max_headers,
                               uint32_t trusted_block, const uint8_t trusted_hash[32], uint64_t authority_set_id, const uint8_t* authority_set_hash,
                               uint32_t target_block, const uint8_t out96[96], char* err, size_t errlen) {
    return header_range_verify_over(nullptr, cfg, blob, len, max_headers, trusted_block, trusted_hash, authority_set_id, authority_set_hash, target_block, out96, err, errlen);
}

// The aggregation verifiers: the verifier holds claims and is the LAST PARTY of a logUp bus whose other parties are tables.  Each
// one below checks its arguments, reads its blob (read_blob), rebuilds the public inputs of its tables from its own arguments
// (the functions the provers call: vx_bus.h) and lists the messages it puts on the bus itself; verify_bus_group does the rest.
//
// Merkle openings (the prover is vx_merkle_open_air.hip): the claims are (index, leaf digest) pairs of a tree known by its cap.
// MerkleOpenAir sends every opened digest, the verifier receives every claim once:
//     published total x rows = sum over the claims of 1 / D_lo + 1 / D_hi.
// No Merkle path is walked here.
int32_t vx_merkle_openings_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* cap, int cap_height, int log_leaves, const uint64_t* leaf_idx,
                                  const uint64_t* leaf_digests, size_t n_idx, char* err, size_t errlen) {
    if (!cfg || !blob || !cap || !leaf_idx || !leaf_digests) return VX_ERR_ARG;
    NEED(log_leaves >= 1 && log_leaves <= 40 && cap_height >= 0 && cap_height <= 16 && cap_height <= log_leaves, "merkle openings: cap height %d / tree depth %d out of range", cap_height,
         log_leaves);
    NEED(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle openings: %zu openings (1..2^21)", n_idx);
    BusTable tab[1];
    VX_TRY(read_blob(blob, len, VX_MOPEN_MAGIC, "merkle-openings", {(uint64_t)log_leaves, n_idx}, tab, 1, err, errlen));
    NEED(peek_tables(cfg, tab, 1), "the proof is too short to hold a trace cap");
    uint64_t root[4], pub[mop::PUB];
    VX_TRY(cap_root(cap, cap_height, "merkle openings", root, err, errlen));
    std::vector<uint64_t> claims(5 * n_idx);
    for (size_t i = 0; i < n_idx; ++i) {
        NEED(leaf_idx[i] >> log_leaves == 0, "merkle openings: claim %zu names a leaf outside the tree", i);
        claims[5 * i] = leaf_idx[i];
        for (int j = 0; j < 4; ++j) {
            NEED(leaf_digests[4 * i + j] < glh::P, "merkle openings: claim %zu has a non-canonical digest word", i);
            claims[5 * i + 1 + j] = leaf_digests[4 * i + j];
        }
    }
    vx_merkle_open_public(root, log_leaves, claims.data(), n_idx, pub);
    tab[0].expect(VX_AIR_MERKLE_OPEN, pub, mop::PUB);
    return verify_bus_group(cfg, tab, 1, "the openings the table proves are not the claimed ones (the lookup bus does not balance)", err, errlen,
                            [&](const VBus& bus, BusMessages& m) {
                                m.reserve(2 * n_idx);
                                for (const uint64_t* c = claims.data(); c < claims.data() + 5 * n_idx; c += 5) {
                                    m.receive(bus.open(Fx{c[0], 0}, Fx{c[1], 0}, Fx{c[2], 0}, bus::K<0>{}));
                                    m.receive(bus.open(Fx{c[0], 0}, Fx{c[3], 0}, Fx{c[4], 0}, bus::K<1>{}));
                                }
                            });
}

// Merkle rows (the prover is vx_leaf_sponge_air.hip): two tables on one bus, openings first.  The claims are what a STARK verifier
// holds -- (index, opened ROW) pairs of a tree known by its cap.  LeafSpongeAir sends every word it absorbs, receives the leaf
// digests MerkleOpenAir sends (TAG_OPEN closes between the two tables), and MerkleOpenAir proves those digests lie under the root;
// the verifier receives every word of every claim once:
//     total_open x rows_open + total_sponge x rows_sponge = sum over the claims, j < leaf_len of 1 / D_row(index, j, row[j]).
// LeafSpongeAir's public inputs are rebuilt entirely from the arguments; of MerkleOpenAir's, root and depth are.  Its claims digest
// cannot be: the verifier never sees the leaf digests.  Those four words are taken from the proof's own public inputs (checked
// canonical); they ONLY feed the shared transcript -- the digests themselves are bound by the sponge table's committed trace, and
// the challenges depend on the rows through the sponge table's own claims digest.
// No Merkle path is walked and no leaf is hashed; the row-claims digest costs as many permutations as hashing the rows would.
int32_t vx_merkle_rows_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* cap, int cap_height, int log_leaves, size_t leaf_len,
                              const uint64_t* leaf_idx, const uint64_t* rows, size_t n_idx, char* err, size_t errlen) {
    if (!cfg || !blob || !cap || !leaf_idx || !rows) return VX_ERR_ARG;
    NEED(log_leaves >= 1 && log_leaves <= 32 && cap_height >= 0 && cap_height <= 16 && cap_height <= log_leaves, "merkle rows: cap height %d / tree depth %d out of range", cap_height,
         log_leaves);
    NEED(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle rows: %zu openings (1..2^21)", n_idx);
    NEED(leaf_len >= 5 && leaf_len <= ((size_t)1 << 20), "merkle rows: leaf_len %zu (5..2^20)", leaf_len);
    BusTable tab[2];
    VX_TRY(read_blob(blob, len, VX_MROWS_MAGIC, "merkle-rows", {(uint64_t)log_leaves, leaf_len, n_idx}, tab, 2, err, errlen));
    NEED(peek_tables(cfg, tab, 2), "a proof is too short to hold a trace cap");
    uint64_t root[4], opub[mop::PUB], spub[lsp::PUB];
    VX_TRY(cap_root(cap, cap_height, "merkle rows", root, err, errlen));
    vx_merkle_open_public(root, log_leaves, nullptr, 0, opub);
    NEED(tab[0].n_pub == (size_t)mop::PUB, "merkle rows: the openings table has %zu public inputs", tab[0].n_pub);
    for (int j = 5; j < mop::PUB; ++j) {
        NEED(tab[0].pub[j] < glh::P, "merkle rows: non-canonical claims digest in the openings table");
        opub[j] = tab[0].pub[j];
    }
    std::vector<uint64_t> claims(n_idx * (leaf_len + 1));
    for (size_t i = 0; i < n_idx; ++i) {
        NEED(leaf_idx[i] >> log_leaves == 0, "merkle rows: claim %zu names a leaf outside the tree", i);
        uint64_t* c = claims.data() + i * (leaf_len + 1);
        c[0] = leaf_idx[i];
        for (size_t j = 0; j < leaf_len; ++j) {
            NEED(rows[i * leaf_len + j] < glh::P, "merkle rows: claim %zu has a non-canonical word at %zu", i, j);
            c[1 + j] = rows[i * leaf_len + j];
        }
    }
    vx_leaf_sponge_public(leaf_len, claims.data(), n_idx, spub);
    tab[0].expect(VX_AIR_MERKLE_OPEN, opub, mop::PUB);
    tab[1].expect(VX_AIR_LEAF_SPONGE, spub, lsp::PUB);
    return verify_bus_group(cfg, tab, 2, "the rows the tables prove are not the claimed ones (the lookup bus does not balance)", err, errlen,
                            [&](const VBus& bus, BusMessages& m) {
                                m.reserve(n_idx * leaf_len);
                                for (size_t i = 0; i < n_idx; ++i)
                                    for (size_t j = 0; j < leaf_len; ++j) m.receive(bus.row(Fx{leaf_idx[i], 0}, Fx{(uint64_t)j, 0}, Fx{rows[i * leaf_len + j], 0}));
                            });
}

// RotateCircuit verify (the provers are vx_rotate.hip and, for the verifier above, vx_header_range.hip; every host verifier lives
// in this file, which holds no GPU code): the blob must be for this (authority_set_id, authority_set_hash) request and claim out32;
// then its six STARKs are verified in their two shared-challenge groups against the public inputs those values imply, and both
// buses must balance.
static int32_t rotate_verify_over(DeferredPaths* paths, const vx_stark_config* cfg, const uint64_t* blob, size_t len, uint64_t authority_set_id, const uint8_t authority_set_hash[32],
                                  const uint8_t out32[32], char* err, size_t errlen) {
    if (!cfg || !blob || !authority_set_hash || !out32) return VX_ERR_ARG;
    NEED(len > VX_ROT_HDR && blob[0] == VX_ROT_MAGIC, "bad rotate blob");
    NEED(blob[1] == authority_set_id && memcmp(blob + 8, authority_set_hash, 32) == 0, "blob is for a different request");
    NEED(memcmp(blob + 12, out32, 32) == 0, "public output differs from the blob");
    const size_t l0 = blob[16], l1 = blob[17], l2 = blob[18], l3 = blob[19], l4 = blob[24], l5 = blob[27];
    NEED(l0 <= len && l1 <= len && l2 <= len && l3 <= len && l4 <= len && l5 <= len && VX_ROT_HDR + l0 + l1 + l2 + l3 + l4 + l5 == len, "blob lengths are inconsistent");
    NEED(!(blob[2] >> 32) && blob[26] < VX_MAX_HEADER_SIZE && blob[3] != 0 && blob[3] <= 510, "block number, start position or authority count out of range");
    const uint64_t* p0 = blob + VX_ROT_HDR;
    // Bus B: the Blake2b table (a chain of exactly one header, numbered epoch_end_block, hashing to the blob's header hash; the anchor
    // is the parent hash the header itself carries -- free in this statement) sends the bytes from start_position + 1 on; the
    // epoch-end table reads the ScheduledChange log of blob[3] authorities there and sends its keys; the new set's commitment table
    // receives every key and hashes to out32.
    {
        uint64_t bpub[20], epub[10], spub[10];
        BusTable tab[3] = {{p0, l0}, {p0 + l0 + l1 + l2 + l3 + l4, l5}, {p0 + l0 + l1, l2}};
        tab[0].expect(VX_AIR_BLAKE_CHAIN, bpub, 20);
        tab[1].expect(VX_AIR_EPOCH_END, epub, 10);
        tab[2].expect(VX_AIR_SHA_CHAIN, spub, 10);
        NEED(peek_tables(cfg, tab, 3), "epoch-end proofs are too short to hold a trace cap");
        for (int j = 0; j < 8; ++j) {
            uint32_t a, b;
            memcpy(&a, (const uint8_t*)(blob + 20) + 4 * j, 4);
            memcpy(&b, (const uint8_t*)(blob + 4) + 4 * j, 4);
            bpub[j] = a;
            bpub[8 + j] = b;
        }
        bpub[16] = bpub[17] = blob[2];
        bpub[18] = blob[26] + 1, bpub[19] = 2;  // window mode: the bytes behind start_position
        // the byte lengths of the log's two compact ints are the prover's to state (one-hot); the table's constraints tie them to the bytes
        NEED(tab[1].n_pub == 10, "epoch-end proof is malformed");
        epub[0] = blob[3], epub[1] = 1;
        for (int g = 0; g < 2; ++g) {
            uint64_t sum = 0;
            for (int a = 0; a < 4; ++a) {
                const uint64_t f = tab[1].pub[2 + 4 * g + a];
                NEED(f <= 1, "epoch-end proof: length flags are not one-hot");
                epub[2 + 4 * g + a] = f, sum += f;
            }
            NEED(sum == 1, "epoch-end proof: length flags are not one-hot");
        }
        be_limbs(out32, spub);
        spub[8] = blob[3], spub[9] = 2;  // receives every key
        const int32_t rc = verify_bus_group(cfg, tab, 3, "the lookup bus between the header hash, the epoch-end table and the new set does not balance", err, errlen, nullptr, paths);
        if (rc != VX_OK) return rc;
    }
    // the justification by the current set: commitment, Ed25519 and SHA-512 tables under shared lookup challenges; the signed
    // message is the precommit for (the proven header hash, the block number, the round, the request's set id)
    uint64_t spub[10], epub[2], hpub[15];
    int air[3];
    BusTable tab[3] = {{p0 + l0, l1}, {p0 + l0 + l1 + l2, l3}, {p0 + l0 + l1 + l2 + l3, l4}};
    NEED(peek_tables(cfg, tab, 3), "justification proofs are too short to hold a trace cap");
    const int32_t rc = vx_justification_expect(tab[0].pub, tab[0].n_pub, tab[1].pub, tab[1].n_pub, tab[2].n_pub, authority_set_hash, authority_set_id, (const uint8_t*)(blob + 4),
                                               (uint32_t)blob[2], blob[25], spub, epub, hpub, air, err, errlen);
    if (rc != VX_OK) return rc;
    tab[0].expect(air[0], spub, 10);
    tab[1].expect(air[1], epub, 2);
    tab[2].expect(air[2], hpub, 15);
    return verify_bus_group(cfg, tab, 3, "the lookup bus between the justification tables does not balance", err, errlen, nullptr, paths);
}
int32_t vx_rotate_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, uint64_t authority_set_id,
                         const uint8_t authority_set_hash[32], const uint8_t out32[32], char* err, size_t errlen) {
    return rotate_verify_over(nullptr, cfg, blob, len, authority_set_id, authority_set_hash, out32, err, errlen);
}

// The deferred forms (include/vx.h).  On the device: the host pass of every proof, then ONE launch of k_merkle_check over the openings
// they recorded (vx_merkle_check.hip); vx_stark_verify_deferred runs the same code over glh::merkle_path_ok, one opening after
// the other, so that the order of the answers can be tested without a GPU.
static int32_t paths_on_host(const MerkleBatch& b, size_t* first_bad, char*, size_t) {
    const size_t cap_words = (size_t)4 << b.cap_height;
    const uint64_t *leaf = b.leaves.data(), *sib = b.siblings.data();
    for (size_t i = 0; i < b.tree_of.size() && *first_bad == SIZE_MAX; ++i) {
        const size_t t = b.tree_of[i], n_sib = (size_t)(b.log_leaves[t] - b.cap_height);
        if (!glh::merkle_path_ok(leaf, b.leaf_len[i], b.leaf_idx[i], sib, n_sib, b.caps.data() + t * cap_words)) *first_bad = i;
        leaf += b.leaf_len[i], sib += 4 * n_sib;
    }
    return VX_OK;
}
int32_t vx_stark_verify_deferred(const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public, char* err,
                                 size_t errlen) {
    DeferredPaths paths(paths_on_host);
    return paths.settle(paths.pass(cfg, pr, len, expect_air, expect_public, n_expect_public, nullptr, nullptr, nullptr, err, errlen), err, errlen);
}
int32_t vx_stark_verify_dev(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* pr, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public, char* err,
                            size_t errlen) {
    if (!ctx) return VX_ERR_ARG;
    DeferredPaths paths(vx_merkle_check_paths(ctx));
    return paths.settle(paths.pass(cfg, pr, len, expect_air, expect_public, n_expect_public, nullptr, nullptr, nullptr, err, errlen), err, errlen);
}
int32_t vx_header_range_verify_dev(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* blob, size_t len, uint32_t max_headers, uint32_t trusted_block,
                                   const uint8_t trusted_hash[32], uint64_t authority_set_id, const uint8_t* authority_set_hash, uint32_t target_block, const uint8_t out96[96],
                                   char* err, size_t errlen) {
    if (!ctx) return VX_ERR_ARG;
    DeferredPaths paths(vx_merkle_check_paths(ctx));
    return paths.settle(header_range_verify_over(&paths, cfg, blob, len, max_headers, trusted_block, trusted_hash, authority_set_id, authority_set_hash, target_block, out96, err, errlen),
                        err, errlen);
}
int32_t vx_rotate_verify_dev(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* blob, size_t len, uint64_t authority_set_id, const uint8_t authority_set_hash[32],
                             const uint8_t out32[32], char* err, size_t errlen) {
    if (!ctx) return VX_ERR_ARG;
    DeferredPaths paths(vx_merkle_check_paths(ctx));
    return paths.settle(rotate_verify_over(&paths, cfg, blob, len, authority_set_id, authority_set_hash, out32, err, errlen), err, errlen);
}

// FRI fold (the prover is vx_fri_fold_air.hip), the third aggregation verifier: the claims are what a STARK verifier holds when it
// enters the query phase's fold loop -- per query the index, ev_0 (its own FRI combination) and the opened leaves of every layer,
// and the betas and the final polynomial of the transcript.  FriFoldAir receives every leaf word and every entry, which the
// verifier sends, and sends every exit, which the verifier receives:
//     published total x rows = sum over the queries of  - sum over the layers l, j < 32 of 1 / D_row(tree l, index >> 4 (l + 1), j, leaf_l[j])
//                                                        - 1 / D_fri(index, ev_0, 0)  +  1 / D_fri(index, final_poly(x_NL), 1).
// NOTHING IS FOLDED here: per query one exponentiation for x_NL = x_0^(16^NL) and one Horner evaluation remain.
// The fold-side claims of an aggregation verifier, `what` its name in the messages: the ranges, then every word canonical and every
// index inside the LDE.  ev0 / leaves: nullptr where the verifier holds none.
static int32_t fold_claims_check(const char* what, int max_log_lde, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len,
                                 const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries, char* err, size_t errlen) {
    NEED(log_lde >= 5 && log_lde <= max_log_lde && n_layers >= 1 && n_layers <= (size_t)ffa::MAX_LAYERS && 4 * (int)n_layers < log_lde, "%s: log_lde %d / %zu layers out of range", what,
         log_lde, n_layers);
    NEED(n_queries >= 1 && n_queries <= ((size_t)1 << 20), "%s: %zu queries (1..2^20)", what, n_queries);
    NEED(final_len >= 1 && final_len <= ((size_t)1 << 27), "%s: a final polynomial of %zu coefficients", what, final_len);
    for (size_t i = 0; i < 2 * n_layers; ++i) NEED(betas[i] < glh::P, "%s: non-canonical beta word %zu", what, i);
    for (size_t i = 0; i < 2 * final_len; ++i) NEED(final_poly[i] < glh::P, "%s: non-canonical final-polynomial word %zu", what, i);
    for (size_t i = 0; i < n_queries; ++i) {
        NEED(index[i] >> log_lde == 0, "%s: claim %zu names an index outside the LDE", what, i);
        NEED(!ev0 || (ev0[2 * i] < glh::P && ev0[2 * i + 1] < glh::P), "%s: claim %zu has a non-canonical ev_0", what, i);
    }
    for (size_t i = 0; leaves && i < n_queries * n_layers * 32; ++i) NEED(leaves[i] < glh::P, "%s: claim %zu has a non-canonical leaf word", what, i / (32 * n_layers));
    return VX_OK;
}
int32_t vx_fri_fold_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly,
                           size_t final_len, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries, char* err, size_t errlen) {
    if (!cfg || !blob || !betas || !final_poly || !index || !ev0 || !leaves) return VX_ERR_ARG;
    if (cfg->arity_bits != 4) return v_fail(VX_ERR_ARG, err, errlen, "fri fold: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    VX_TRY(fold_claims_check("fri fold", 32, log_lde, betas, n_layers, final_poly, final_len, index, ev0, leaves, n_queries, err, errlen));
    BusTable tab[1];
    VX_TRY(read_blob(blob, len, VX_FFOLD_MAGIC, "fri-fold", {(uint64_t)log_lde, n_layers, n_queries}, tab, 1, err, errlen));
    NEED(peek_tables(cfg, tab, 1), "the proof is too short to hold a trace cap");
    uint64_t pub[ffa::PUB];
    vx_fri_fold_public(log_lde, betas, n_layers, 0, index, ev0, leaves, n_queries, pub);
    tab[0].expect(VX_AIR_FRI_FOLD, pub, ffa::PUB);
    return verify_bus_group(cfg, tab, 1, "the fold chains the table proves are not the claimed ones (the lookup bus does not balance)", err, errlen,
                            [&](const VBus& bus, BusMessages& m) {
                                m.reserve(n_queries * (32 * n_layers + 2));
                                for (size_t i = 0; i < n_queries; ++i) {
                                    for (size_t l = 0; l < n_layers; ++l) m.send_layer_leaf(bus, l, index[i], leaves + (i * n_layers + l) * 32);
                                    m.send(bus.fri(Fx{index[i], 0}, Fx{ev0[2 * i], 0}, Fx{ev0[2 * i + 1], 0}, bus::K<0>{}));
                                    m.receive_exit(bus, index[i], log_lde, n_layers, final_poly, final_len);
                                }
                            });
}

// FRI queries (the prover is vx_fri_queries.hip), the first aggregation verifier that holds NO leaves: three tables on one bus --
// MerkleOpenSetAir, LeafSpongeSetAir, FriFoldAir -- close TAG_OPEN and TAG_ROW among themselves in every layer tree.  The verifier
// holds what a succinct verifier holds: the layer caps, the betas, the final polynomial and (index, ev_0) per query.  It sends
// every entry, receives every exit, and receives the root and depth every path ended in -- the tables do not know which root
// belongs to which tree, the verifier does (cap_root of caps[l], depth log_lde - 4 (l + 1)):
//     sum over the tables of total x rows = sum over the queries of  - 1 / D_fri(index, ev_0, 0)  +  1 / D_fri(index, final_poly(x_NL), 1)
//                                                                     + sum over the layers l of 1 / D_root(l, lo) + 1 / D_root(l, hi).
// EVERY public input of all three tables is rebuilt from the arguments (their digest words are the statement digest, vx_bus.h).
// No path is walked, no leaf hashed, nothing folded.
int32_t vx_fri_queries_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly,
                              size_t final_len, const uint64_t* caps, int cap_height, const uint64_t* index, const uint64_t* ev0, size_t n_queries, char* err, size_t errlen) {
    if (!cfg || !blob || !betas || !final_poly || !caps || !index || !ev0) return VX_ERR_ARG;
    if (cfg->arity_bits != 4) return v_fail(VX_ERR_ARG, err, errlen, "fri queries: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    VX_TRY(fold_claims_check("fri queries", 30, log_lde, betas, n_layers, final_poly, final_len, index, ev0, nullptr, n_queries, err, errlen));
    NEED(cap_height >= 0 && cap_height <= 16 && cap_height <= log_lde - 4 * (int)n_layers, "fri queries: cap height %d out of range (at most log_lde - 4 layers)", cap_height);
    const int log_open = fri_queries_open_log_n(n_queries, log_lde, n_layers), log_sponge = fri_queries_sponge_log_n(n_queries, n_layers);
    NEED(log_open <= 26 && log_sponge <= 26, "fri queries: the request needs a table of more than 2^26 rows");
    BusTable tab[3];
    VX_TRY(read_blob(blob, len, VX_FQRY_MAGIC, "fri-queries", {(uint64_t)log_lde, n_layers, n_queries}, tab, 3, err, errlen));
    NEED(peek_tables(cfg, tab, 3), "a proof is too short to hold a trace cap");
    std::vector<uint64_t> roots(4 * n_layers);
    for (size_t l = 0; l < n_layers; ++l) VX_TRY(cap_root(caps + l * ((size_t)4 << cap_height), cap_height, "fri queries", roots.data() + 4 * l, err, errlen));
    uint64_t stmt[4], opub[mop::SET_PUB], spub[lsp::PUB], fpub[ffa::PUB];
    vx_fri_queries_statement(log_lde, betas, n_layers, final_poly, final_len, roots.data(), index, ev0, n_queries, stmt);
    vx_merkle_open_set_public(stmt, opub);
    vx_leaf_sponge_set_public(32, stmt, spub);
    vx_fri_fold_public_digest(log_lde, betas, n_layers, 0, stmt, fpub);
    tab[0].expect(VX_AIR_MERKLE_OPEN_SET, opub, mop::SET_PUB);
    tab[1].expect(VX_AIR_LEAF_SPONGE_SET, spub, lsp::PUB);
    tab[2].expect(VX_AIR_FRI_FOLD, fpub, ffa::PUB);
    return verify_bus_group(cfg, tab, 3, "the query phase the tables prove is not the claimed one (the lookup bus does not balance)", err, errlen,
                            [&](const VBus& bus, BusMessages& m) {
                                m.reserve(n_queries * (2 + 2 * n_layers));
                                for (size_t i = 0; i < n_queries; ++i) {
                                    m.send(bus.fri(Fx{index[i], 0}, Fx{ev0[2 * i], 0}, Fx{ev0[2 * i + 1], 0}, bus::K<0>{}));
                                    m.receive_exit(bus, index[i], log_lde, n_layers, final_poly, final_len);
                                    for (size_t l = 0; l < n_layers; ++l) m.receive_root(bus, l, roots.data() + 4 * l, log_lde - 4 * ((int)l + 1));
                                }
                            });
}

// The FRI side of a vx_stark_prove proof as FriFoldAir's claims (prover-side: it VERIFIES the proof on the way -- the transcript
// is replayed by the verifier's own code -- and hands out what its query phase saw).  The proof omits the `within` slot of every
// FRI leaf; here it is filled with the value the chain enters the layer with.
int32_t vx_stark_fri_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int* log_lde, size_t* n_layers, size_t* final_len, size_t* n_queries, uint64_t betas_out[16],
                            uint64_t* final_poly_out, size_t final_cap, uint64_t* index_out, uint64_t* ev0_out, uint64_t* ev_last_out, size_t query_cap, uint64_t* leaves_out,
                            size_t leaves_cap, char* err, size_t errlen) {
    if (!cfg || !proof || !log_lde || !n_layers || !final_len || !n_queries || !betas_out || !final_poly_out || !index_out || !ev0_out || !leaves_out) return VX_ERR_ARG;
    if (cfg->arity_bits != 4) return v_fail(VX_ERR_ARG, err, errlen, "fri claims: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    StarkQueries fc;
    VX_TRY(stark_verify_impl(cfg, proof, len, 0, nullptr, 0, nullptr, nullptr, nullptr, QueryPhase::Walked, &fc, err, errlen));
    const size_t nl = fc.so.NL, nq = fc.so.n_queries;
    if (nl < 1 || nl > (size_t)ffa::MAX_LAYERS || 4 * (int)nl >= fc.so.LN)
        return v_fail(VX_ERR_ARG, err, errlen, "fri claims: a proof with %zu fold layers over an LDE of 2^%d has no FriFoldAir statement (1..8 layers, one index bit left)", nl, fc.so.LN);
    *log_lde = fc.so.LN, *n_layers = nl, *final_len = fc.final_poly.size() / 2, *n_queries = nq;
    if (final_cap < fc.final_poly.size() || query_cap < nq || leaves_cap < fc.leaves.size())
        return v_fail(VX_ERR_BUFSZ, err, errlen, "fri claims: the buffers hold %zu / %zu / %zu words, %zu / %zu / %zu are needed", final_cap, query_cap, leaves_cap, fc.final_poly.size(), nq,
                      fc.leaves.size());
    memset(betas_out, 0, 16 * 8);
    memcpy(betas_out, fc.betas.data(), fc.betas.size() * 8);
    memcpy(final_poly_out, fc.final_poly.data(), fc.final_poly.size() * 8);
    memcpy(index_out, fc.so.index.data(), nq * 8);
    memcpy(ev0_out, fc.ev0.data(), 2 * nq * 8);
    if (ev_last_out) memcpy(ev_last_out, fc.ev_last.data(), 2 * nq * 8);
    memcpy(leaves_out, fc.leaves.data(), fc.leaves.size() * 8);
    return VX_OK;
}

}  // extern "C"

// The query phase of a vx_stark_prove proof as claims (vx_bus.h), from ONE run of the verifier's own code -- transcript, constraint
// identity at zeta, proof of work and, unless query-free, combination, folds and the final polynomial are all checked.
int32_t vx_stark_queries_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                const uint64_t* ext_chal, QueryPhase mode, StarkQueries* out, char* err, size_t errlen) {
    return stark_verify_impl(cfg, proof, len, expect_air, expect_public, n_expect_public, ext_chal, nullptr, nullptr, mode, out, err, errlen);
}
int32_t vx_stark_openings_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                 const uint64_t* ext_chal, StarkQueries* out, char* err, size_t errlen) {
    VX_TRY(vx_stark_queries_claims(cfg, proof, len, expect_air, expect_public, n_expect_public, ext_chal, QueryPhase::Delegated, out, err, errlen));
    if (out->so.NL > (size_t)ffa::MAX_LAYERS)
        return v_fail(VX_ERR_ARG, err, errlen, "stark openings: a proof with %zu fold layers (at most 8: the layer trees are ids 0..7, the commitment trees 8..10)", out->so.NL);
    return VX_OK;
}
void vx_cap_fold(const uint64_t* cap, int cap_height, uint64_t root[4]) {
    std::vector<uint64_t> fold(cap, cap + ((size_t)4 << cap_height));
    for (size_t nodes = (size_t)1 << cap_height; nodes > 1; nodes >>= 1)
        for (size_t i = 0; i < nodes / 2; ++i) glh::two_to_one(fold.data() + 8 * i, fold.data() + 8 * i + 4, fold.data() + 4 * i);
    memcpy(root, fold.data(), 32);
}
void vx_stark_openings_statement(const StarkOpenings& so, const uint64_t* roots, uint64_t digest[4]) {
    std::vector<uint64_t> w;
    w.reserve(7 + 4 * so.tree.size() + so.n_queries + so.leaves.size());
    for (uint64_t x : so.shape_words()) w.push_back(x);
    w.insert(w.end(), roots, roots + 4 * so.tree.size());
    const size_t per_query = so.tree.size();
    for (size_t i = 0; i < so.n_queries; ++i) {
        w.push_back(so.index[i]);
        for (size_t k = 0; k < per_query; ++k) {
            const StarkOpenings::Claim& c = so.claims[i * per_query + k];
            w.insert(w.end(), so.leaves.begin() + c.leaf, so.leaves.begin() + c.leaf + c.leaf_len);
        }
    }
    glh::hash_no_pad(w.data(), w.size(), digest);
}

extern "C" {
// The Merkle side of a vx_stark_prove proof (host only, prover-side): what vx_stark_openings_claims records, in caller-sized
// arrays.  Every other check of the proof has run; the paths are for the caller to prove (vx_stark_openings_prove).
int32_t vx_stark_merkle_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, const uint64_t* ext_chal, uint64_t shape_out[7], size_t* n_trees, uint64_t cap_tree_out[11],
                               uint64_t* caps_out, size_t caps_cap, size_t* n_claims, uint64_t* tree_out, uint64_t* index_out, uint64_t* leaf_len_out, size_t claims_cap, size_t* leaves_len,
                               uint64_t* leaves_out, size_t leaves_cap, size_t* siblings_len, uint64_t* siblings_out, size_t siblings_cap, char* err, size_t errlen) {
    if (!cfg || !proof || !shape_out || !n_trees || !cap_tree_out || !caps_out || !n_claims || !tree_out || !index_out || !leaf_len_out || !leaves_len || !leaves_out || !siblings_len ||
        !siblings_out)
        return VX_ERR_ARG;
    StarkQueries sq;
    VX_TRY(vx_stark_openings_claims(cfg, proof, len, 0, nullptr, 0, ext_chal, &sq, err, errlen));
    const StarkOpenings& so = sq.so;
    size_t sib_words = 0;
    for (const StarkOpenings::Claim& c : so.claims) sib_words += 4 * (size_t)(so.log_leaves(c.tree) - so.cap_h);
    const std::array<uint64_t, 7> sw = so.shape_words();
    memcpy(shape_out, sw.data(), sizeof sw);
    *n_trees = so.tree.size(), *n_claims = so.claims.size(), *leaves_len = so.leaves.size(), *siblings_len = sib_words;
    if (caps_cap < so.caps.size() || claims_cap < so.claims.size() || leaves_cap < so.leaves.size() || siblings_cap < sib_words)
        return v_fail(VX_ERR_BUFSZ, err, errlen, "merkle claims: the buffers hold %zu / %zu / %zu / %zu words, %zu / %zu / %zu / %zu are needed", caps_cap, claims_cap, leaves_cap, siblings_cap,
                      so.caps.size(), so.claims.size(), so.leaves.size(), sib_words);
    memset(cap_tree_out, 0, 11 * 8);
    memcpy(cap_tree_out, so.tree.data(), so.tree.size() * 8);
    memcpy(caps_out, so.caps.data(), so.caps.size() * 8);
    memcpy(leaves_out, so.leaves.data(), so.leaves.size() * 8);
    uint64_t* sib = siblings_out;
    for (size_t i = 0; i < so.claims.size(); ++i) {
        const StarkOpenings::Claim& c = so.claims[i];
        const size_t n = 4 * (size_t)(so.log_leaves(c.tree) - so.cap_h);
        tree_out[i] = c.tree, index_out[i] = c.index, leaf_len_out[i] = c.leaf_len;
        memcpy(sib, proof + c.sib, n * 8), sib += n;
    }
    return VX_OK;
}

// What the prover of a level (vx_stark_groups.hip) writes for this inner proof.  Openings and Queries: AT MOST -- read from the
// proof's head alone (AIR id and degree bits -> the columns of the three trees, the fold layers), nothing is verified, every table
// at its bound_words().  Inner: TO THE WORD -- the transcript table's rows and the claims need the block count, so the head is
// replayed (no query record is read), and a table's proof has the one length its AIR, its rows and the configuration imply
// (Shape::words()).  Callers see the difference (the `needed` of a refused buffer); the two numbers are not unified.
static int32_t stark_group_proof_bound(StarkLevel level, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, size_t* n_words) {
    if (!cfg || !proof || !n_words) return VX_ERR_ARG;
    const StarkLevelInfo& lv = stark_level(level);
    StarkGroupTables ts;
    if (level == StarkLevel::Inner) {
        size_t head = 0;
        if (vx_stark_proof_head_words(cfg, proof, proof_len, &head) != VX_OK || proof_len < head) return VX_ERR_ARG;
        StarkQueries sq;
        glh::TranscriptRecord rec;
        if (vx_stark_inner_replay(cfg, proof, head, ext_chal, true, &sq, &rec, nullptr, 0) != VX_OK) return VX_ERR_ARG;
        const StarkOpenings& so = sq.so;
        if (so.cap_h > 16 || !stark_level_tables(level, so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, rec.n_blocks(), *cfg, &ts)) return VX_ERR_ARG;
        size_t total = lv.hdr + rec.chal.size() + (size_t)ts.n;
        for (int k = 0; k < ts.n; ++k) {
            BusAirShape a;
            if (!vx_air_bus_shape(ts.air[k], &a)) return VX_ERR_ARG;
            total += sp::Shape(ts.air[k], a.cols, a.aux, a.pub, a.auxpub, ts.log_n[k], *cfg).words();
        }
        *n_words = total;
        return VX_OK;
    }
    if (!sp::config_ok(*cfg)) return VX_ERR_ARG;
    ProofHead head;
    if (proof_head(*cfg, proof, proof_len, 0, &head, nullptr, 0) != VX_OK) return VX_ERR_ARG;
    const sp::Shape& shape = *head.shape;
    if (shape.LN < shape.cap_h || shape.cap_h > 16) return VX_ERR_ARG;
    if (!stark_level_tables(level, shape.LN, shape.cm, shape.ca, cfg->arity_bits, shape.arities.size(), (size_t)shape.num_queries, 0, *cfg, &ts)) return VX_ERR_ARG;
    TableShape sh[StarkGroupTables::MAX];
    for (int k = 0; k < ts.n; ++k) sh[k] = {ts.air[k], ts.log_n[k]};
    return vx_tables_proof_bound(cfg, lv.hdr + (size_t)ts.n, sh, (size_t)ts.n, n_words);
}
int32_t vx_stark_openings_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, size_t* n_words) {
    return stark_group_proof_bound(StarkLevel::Openings, cfg, proof, proof_len, nullptr, n_words);
}
int32_t vx_stark_queries_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, size_t* n_words) {
    return stark_group_proof_bound(StarkLevel::Queries, cfg, proof, proof_len, nullptr, n_words);
}
int32_t vx_stark_inner_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, size_t* n_words) {
    return stark_group_proof_bound(StarkLevel::Inner, cfg, proof, proof_len, ext_chal, n_words);
}

// FRI combine (the prover is vx_fri_combine_air.hip), the fourth aggregation verifier: the claims are what a STARK verifier holds
// when it enters the query phase -- alpha, zeta, the openings at zeta and, per query, the index, the opened trace / auxiliary /
// quotient row and ev_0.  FriCombineAir receives every row word, which the verifier sends, and sends every (index, ev_0, 0),
// which the verifier receives:
//     published total x rows = sum over the queries of  - sum over j < cm + ca + nq of 1 / D_row(tree 8 + t_j, index, position_j, w_j)
//                                                        + 1 / D_fri(index, ev_0, 0).
// NOTHING IS COMBINED per query: y0, y1, alpha^c and zeta' are computed once.
static int32_t fc_stmt_check(const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, size_t n_queries, const char* what, char* err, size_t errlen) {
    NEED(st.log_lde >= 5 && st.log_lde <= 32 && st.rate_bits >= 1 && st.rate_bits < st.log_lde, "%s: log_lde %d / rate_bits %d out of range", what, st.log_lde, st.rate_bits);
    const size_t M = (size_t)1 << 20;
    NEED(st.cm >= 1 && st.cm <= M && st.ca <= M && st.nq >= 1 && st.nq <= M, "%s: %zu / %zu / %zu columns out of range", what, st.cm, st.ca, st.nq);
    NEED(n_queries >= 1 && n_queries <= M, "%s: %zu queries (1..2^20)", what, n_queries);
    const size_t c = st.cm + st.ca, absn = c + st.nq;
    for (int i = 0; i < 2; ++i) NEED(st.alpha[i] < glh::P && st.zeta[i] < glh::P, "%s: non-canonical alpha or zeta", what);
    for (size_t i = 0; i < 2 * c; ++i) NEED(st.open_local[i] < glh::P && st.open_next[i] < glh::P, "%s: non-canonical opening word %zu", what, i);
    for (size_t i = 0; i < 2 * st.nq; ++i) NEED(st.open_quot[i] < glh::P, "%s: non-canonical quotient opening word %zu", what, i);
    for (size_t i = 0; i < n_queries; ++i) NEED(index[i] >> st.log_lde == 0, "%s: claim %zu names an index outside the LDE", what, i);
    for (size_t i = 0; i < n_queries * absn; ++i) NEED(rows[i] < glh::P, "%s: claim %zu has a non-canonical row word", what, i / absn);
    return VX_OK;
}
// the row words of one query as the verifier sends them: tree TREE0 + t, position within the tree's row
static void fc_send_rows(const VBus& bus, BusMessages& m, const FriCombineStmt& st, uint64_t index, const uint64_t* row) {
    const size_t c = st.cm + st.ca, absn = c + st.nq;
    for (size_t j = 0; j < absn; ++j) {
        const uint64_t t = j < st.cm ? 0 : j < c ? 1 : 2, pos = j < st.cm ? j : j < c ? j - st.cm : j - c;
        m.send(bus.row_of(Fx{fca::TREE0 + t, 0}, Fx{index, 0}, Fx{pos, 0}, Fx{row[j], 0}));
    }
}
int32_t vx_fri_combine_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2],
                              const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0,
                              size_t n_queries, char* err, size_t errlen) {
    if (!cfg || !blob || !alpha || !zeta || !open_local || !open_next || !open_quot || !index || !rows || !ev0) return VX_ERR_ARG;
    const FriCombineStmt st{log_lde, cfg->rate_bits, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot};
    VX_TRY(fc_stmt_check(st, index, rows, n_queries, "fri combine", err, errlen));
    for (size_t i = 0; i < n_queries; ++i) NEED(ev0[2 * i] < glh::P && ev0[2 * i + 1] < glh::P, "fri combine: claim %zu has a non-canonical ev_0", i);
    NEED(fri_combine_log_n(n_queries, log_lde, cm, ca, nq) <= 26, "fri combine: the request needs a table of more than 2^26 rows");
    BusTable tab[1];
    VX_TRY(read_blob(blob, len, VX_FCOMB_MAGIC, "fri-combine", {(uint64_t)log_lde, cm, ca, nq, n_queries}, tab, 1, err, errlen));
    NEED(peek_tables(cfg, tab, 1), "the proof is too short to hold a trace cap");
    uint64_t pub[fca::PUB];
    vx_fri_combine_public(st, fca::TREE0, index, rows, ev0, n_queries, pub);
    tab[0].expect(VX_AIR_FRI_COMBINE, pub, fca::PUB);
    const size_t absn = cm + ca + nq;
    return verify_bus_group(cfg, tab, 1, "the combinations the table proves are not the claimed ones (the lookup bus does not balance)", err, errlen,
                            [&](const VBus& bus, BusMessages& m) {
                                m.reserve(n_queries * (absn + 1));
                                for (size_t i = 0; i < n_queries; ++i) {
                                    fc_send_rows(bus, m, st, index[i], rows + i * absn);
                                    m.receive(bus.fri(Fx{index[i], 0}, Fx{ev0[2 * i], 0}, Fx{ev0[2 * i + 1], 0}, bus::K<0>{}));
                                }
                            });
}

// FRI combine + fold (the prover is vx_fri_combine_fold_prove): two tables on one bus, combine first.  TAG_FRI end 0 closes BETWEEN
// the tables, so the verifier holds NO ev_0: it sends every row word and every leaf word and receives the exit of every chain:
//     sum over the tables of total x rows = sum over the queries of  - the row words  - the leaf words  + 1 / D_fri(index, final_poly(x_NL), 1).
// Every public input of both tables is rebuilt from the arguments; their digest words are one statement digest over all of them.
int32_t vx_fri_combine_fold_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2],
                                   const uint64_t zeta[2], const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* betas, size_t n_layers,
                                   const uint64_t* final_poly, size_t final_len, const uint64_t* index, const uint64_t* rows, const uint64_t* leaves, size_t n_queries, char* err,
                                   size_t errlen) {
    if (!cfg || !blob || !alpha || !zeta || !open_local || !open_next || !open_quot || !betas || !final_poly || !index || !rows || !leaves) return VX_ERR_ARG;
    if (cfg->arity_bits != 4) return v_fail(VX_ERR_ARG, err, errlen, "fri combine-fold: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    const FriCombineStmt st{log_lde, cfg->rate_bits, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot};
    VX_TRY(fc_stmt_check(st, index, rows, n_queries, "fri combine-fold", err, errlen));
    VX_TRY(fold_claims_check("fri combine-fold", 32, log_lde, betas, n_layers, final_poly, final_len, index, nullptr, leaves, n_queries, err, errlen));
    NEED(fri_combine_log_n(n_queries, log_lde, cm, ca, nq) <= 26 && fri_fold_log_n(n_queries, log_lde, n_layers) <= 26, "fri combine-fold: the request needs a table of more than 2^26 rows");
    BusTable tab[2];
    VX_TRY(read_blob(blob, len, VX_FCFLD_MAGIC, "fri-combine-fold", {(uint64_t)log_lde, cm, ca, nq, n_layers, n_queries}, tab, 2, err, errlen));
    NEED(peek_tables(cfg, tab, 2), "a proof is too short to hold a trace cap");
    uint64_t stmt[4], cpub[fca::PUB], fpub[ffa::PUB];
    vx_fri_combine_fold_statement(st, betas, n_layers, final_poly, final_len, index, rows, leaves, n_queries, stmt);
    vx_fri_combine_public_digest(st, fca::TREE0, stmt, cpub);
    vx_fri_fold_public_digest(log_lde, betas, n_layers, 0, stmt, fpub);
    tab[0].expect(VX_AIR_FRI_COMBINE, cpub, fca::PUB);
    tab[1].expect(VX_AIR_FRI_FOLD, fpub, ffa::PUB);
    const size_t absn = cm + ca + nq;
    return verify_bus_group(cfg, tab, 2, "the query-phase arithmetic the tables prove is not the claimed one (the lookup bus does not balance)", err, errlen,
                            [&](const VBus& bus, BusMessages& m) {
                                m.reserve(n_queries * (absn + 32 * n_layers + 1));
                                for (size_t i = 0; i < n_queries; ++i) {
                                    fc_send_rows(bus, m, st, index[i], rows + i * absn);
                                    for (size_t l = 0; l < n_layers; ++l) m.send_layer_leaf(bus, l, index[i], leaves + (i * n_layers + l) * 32);
                                    m.receive_exit(bus, index[i], log_lde, n_layers, final_poly, final_len);
                                }
                            });
}

// The combination side of a vx_stark_prove proof as FriCombineAir's claims (prover-side: the proof is VERIFIED on the way, by the
// verifier's own code with a sink in its query loop): the shape, alpha, zeta, the openings at zeta (local [c][2], next [c][2],
// quotient [nq][2], back to back) and per query the index, the c + nq opened row words and ev_0.
int32_t vx_stark_combine_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int* log_lde, size_t* cm, size_t* ca, size_t* nq, size_t* n_queries, uint64_t alpha_out[2],
                                uint64_t zeta_out[2], uint64_t* openings_out, size_t openings_cap, uint64_t* index_out, uint64_t* ev0_out, size_t query_cap, uint64_t* rows_out,
                                size_t rows_cap, char* err, size_t errlen) {
    if (!cfg || !proof || !log_lde || !cm || !ca || !nq || !n_queries || !alpha_out || !zeta_out || !openings_out || !index_out || !ev0_out || !rows_out) return VX_ERR_ARG;
    StarkQueries fc;
    VX_TRY(stark_verify_impl(cfg, proof, len, 0, nullptr, 0, nullptr, nullptr, nullptr, QueryPhase::Walked, &fc, err, errlen));
    const size_t n = fc.so.n_queries;
    *log_lde = fc.so.LN, *cm = fc.so.cm, *ca = fc.so.ca, *nq = fc.nq, *n_queries = n;
    if (openings_cap < fc.openings.size() || query_cap < n || rows_cap < fc.rows.size())
        return v_fail(VX_ERR_BUFSZ, err, errlen, "combine claims: the buffers hold %zu / %zu / %zu words, %zu / %zu / %zu are needed", openings_cap, query_cap, rows_cap, fc.openings.size(), n,
                      fc.rows.size());
    memcpy(alpha_out, fc.alpha, 16), memcpy(zeta_out, fc.zeta, 16);
    memcpy(openings_out, fc.openings.data(), fc.openings.size() * 8);
    memcpy(index_out, fc.so.index.data(), n * 8);
    memcpy(ev0_out, fc.ev0.data(), 2 * n * 8);
    memcpy(rows_out, fc.rows.data(), fc.rows.size() * 8);
    return VX_OK;
}

}

void vx_stark_queries_statement(const StarkQueries& sq, const uint64_t* roots, uint64_t digest[4]) {
    const StarkOpenings& so = sq.so;
    std::vector<uint64_t> w;
    w.reserve(11 + sq.openings.size() + sq.betas.size() + sq.final_poly.size() + 4 * so.tree.size() + so.n_queries);
    for (uint64_t x : so.shape_words()) w.push_back(x);
    w.insert(w.end(), sq.alpha, sq.alpha + 2), w.insert(w.end(), sq.zeta, sq.zeta + 2);
    w.insert(w.end(), sq.openings.begin(), sq.openings.end());
    w.insert(w.end(), sq.betas.begin(), sq.betas.end());
    w.insert(w.end(), sq.final_poly.begin(), sq.final_poly.end());
    w.insert(w.end(), roots, roots + 4 * so.tree.size());
    w.insert(w.end(), so.index.begin(), so.index.end());
    glh::hash_no_pad(w.data(), w.size(), digest);
}

// ---- a proof under a CLAIMED transcript, for the verifiers of TranscriptAir's chains (vx_stark_transcripts_verify: one per proof;
// stark_group_verify at Inner: the one chain 0).  `prefix` opens every message ("chain 3: " or "").
using ClaimedTranscript = sp::TranscriptOf<glh::ClaimedChallenger>;
static std::string chain_prefix(size_t c) { return "chain " + std::to_string(c) + ": "; }
// the claims of a chain as the blob states them: canonical values, each drawn after at most n_obs words
static int32_t transcript_claims_ok(const TranscriptClaim& claim, const char* prefix, char* err, size_t errlen) {
    for (size_t j = 0; j < claim.n_chal; ++j) {
        NEED(claim.chal[2 * j + 1] < glh::P, "%sclaimed challenge %zu is not canonical", prefix, j);
        NEED(claim.chal[2 * j] <= claim.n_obs, "%schallenge %zu claims %llu absorbed words of %zu", prefix, j, (unsigned long long)claim.chal[2 * j], claim.n_obs);
    }
    return VX_OK;
}
// The verifier's own code over the claimed challenger `ch`, which hashes nothing: every challenge is the blob's claim, every absorbed
// word is noted.  Then the claims against what the run did: as many as the shape draws, each drawn after as many words as the blob
// says.  Leaves claim->words at the absorbed words (they live in `ch`).  A head alone is read query-free whatever `mode` says.
static int32_t claimed_transcript_check(TranscriptClaim* claim, const char* prefix, ClaimedTranscript& ch, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int expect_air,
                                        const uint64_t* expect_public, size_t n_expect_public, const uint64_t* ext_chal, QueryPhase mode, StarkQueries* sink, char* err, size_t errlen) {
    ch.claims = claim->chal, ch.n_claims = claim->n_chal;
    char inner[200] = "";
    const int32_t rc = stark_verify_over(ch, true, cfg, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, nullptr, nullptr, mode, sink, inner, sizeof inner);
    // what the claims got wrong comes first: a run on too few claims was answered with zeros
    NEED(!ch.short_of, "%sthe blob claims %zu challenges, the proof's shape draws more", prefix, claim->n_chal);
    if (rc != VX_OK) return v_fail(rc, err, errlen, "%s%s", prefix, inner);
    NEED(ch.next == claim->n_chal, "%sthe blob claims %zu challenges, the proof's shape draws %zu", prefix, claim->n_chal, ch.next);
    NEED(ch.words.size() == claim->n_obs, "%sthe blob claims %zu absorbed words, the proof's shape absorbs %zu", prefix, claim->n_obs, ch.words.size());
    for (size_t j = 0; j < claim->n_chal; ++j)
        NEED(claim->chal[2 * j] == ch.absorbed[j], "%schallenge %zu is claimed after %llu absorbed words, the proof's shape draws it after %llu", prefix, j,
             (unsigned long long)claim->chal[2 * j], (unsigned long long)ch.absorbed[j]);
    claim->words = ch.words.data();
    return VX_OK;
}
// what the outside party says about chain `c`: it SENDS obs(c, i, w_i) for every observed word and RECEIVES chal(c, j, A_j, v_j)
static void transcript_messages(const VBus& bus, BusMessages& m, size_t c, const TranscriptClaim& claim) {
    const Fx chain{(uint64_t)c, 0};
    for (size_t i = 0; i < claim.n_obs; ++i) m.send(bus.obs(chain, Fx{(uint64_t)i, 0}, Fx{claim.words[i], 0}));
    for (size_t j = 0; j < claim.n_chal; ++j) m.receive(bus.chal(chain, Fx{(uint64_t)j, 0}, Fx{claim.chal[2 * j], 0}, Fx{claim.chal[2 * j + 1], 0}));
}

extern "C" {
// Where the query records of a vx_stark_prove proof start: the length of its head, all vx_stark_queries_verify reads.  Read from the
// proof's header alone (AIR id, degree bits) and the configuration; nothing is verified.
int32_t vx_stark_proof_head_words(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, size_t* head_words) {
    if (!cfg || !proof || !head_words || !sp::config_ok(*cfg)) return VX_ERR_ARG;
    ProofHead head;
    if (proof_head(*cfg, proof, proof_len, 0, &head, nullptr, 0) != VX_OK) return VX_ERR_ARG;
    *head_words = head.shape->o_queries;
    return VX_OK;
}
}

extern "C" {
// The transcript of one proof as TranscriptAir's claims (include/vx.h): one replay of the verifier's code over the recording challenger.
int32_t vx_stark_transcript_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, size_t* n_obs, uint64_t* obs_out, size_t obs_cap,
                                   size_t* n_chal, uint64_t* chal_out, size_t chal_cap, char* err, size_t errlen) {
    if (!cfg || !proof || !n_obs || !n_chal) return VX_ERR_ARG;
    glh::TranscriptRecord r;
    VX_TRY(vx_stark_transcript_record(cfg, proof, proof_len, ext_chal, &r, err, errlen));
    *n_obs = r.words.size(), *n_chal = r.n_chal();
    if (!obs_out || !chal_out || obs_cap < r.words.size() || chal_cap < r.chal.size())
        return v_fail(VX_ERR_BUFSZ, err, errlen, "transcript claims: the buffers hold %zu / %zu words, %zu / %zu are needed", obs_out ? obs_cap : (size_t)0, chal_out ? chal_cap : (size_t)0,
                      r.words.size(), r.chal.size());
    memcpy(obs_out, r.words.data(), r.words.size() * 8);
    memcpy(chal_out, r.chal.data(), r.chal.size() * 8);
    return VX_OK;
}

// The transcripts of n inner proofs (the prover is vx_transcript_air.hip): ONE TranscriptAir table, alone on its bus.  Every inner proof
// is verified in the TRANSCRIPT-FREE state: the verifier's own code over the claimed challenger, which hashes nothing -- every
// challenge is the blob's claim, every absorbed word is noted.  Proof of work (the response has pow_bits leading zero bits), query
// indices (value mod N), the constraint identity at zeta and, for a whole proof, the walked query phase use the claimed values; a
// head alone is read query-free.  The claims must be canonical, as many as the shape draws, each drawn after as many words as the
// blob says.  The verifier is the outside party: per chain it SENDS obs(c, i, w_i) and RECEIVES chal(c, j, A_j, v_j):
//     total x rows of the table = sum over the chains of  sum_j 1 / D_chal(c, j, A_j, v_j)  -  sum_i 1 / D_obs(c, i, w_i).
// What forces what: DESIGN.md 5m.  Stand-alone the statement digest hashes the words the transcripts would have hashed.
int32_t vx_stark_transcripts_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* const* proofs, const size_t* lens, size_t n,
                                    const uint64_t* const* ext_chals, char* err, size_t errlen) {
    if (!cfg || !blob || !proofs || !lens) return VX_ERR_ARG;
    if (n < 1 || n > (size_t)tsc::MAX_CHAINS) return v_fail(VX_ERR_ARG, err, errlen, "stark transcripts: %zu proofs (1..%d)", n, tsc::MAX_CHAINS);
    // ---- the request inside the blob: n, then per chain n_obs, n_chal and the claims
    NEED(len >= 2 && blob[0] == VX_STRN_MAGIC, "bad stark-transcripts blob");
    NEED(blob[1] == n, "blob is for a different request (%llu chains, %zu proofs)", (unsigned long long)blob[1], n);
    std::vector<TranscriptClaim> claims(n);
    size_t at = 2;
    for (size_t c = 0; c < n; ++c) {
        NEED(len - at >= 2 && blob[at + 1] <= (len - at - 2) / 2, "blob truncated (the claims of chain %zu)", c);
        claims[c] = {nullptr, (size_t)blob[at], blob + at + 2, (size_t)blob[at + 1]};
        at += 2 + 2 * claims[c].n_chal;
        VX_TRY(transcript_claims_ok(claims[c], chain_prefix(c).c_str(), err, errlen));
    }
    const size_t n_request = at - 1;
    // ---- every inner proof under its claimed transcript (the claims of EVERY chain were read first: a bad claim of a later chain
    // is reported before an earlier proof's own failure)
    std::vector<ClaimedTranscript> ch(n);
    for (size_t c = 0; c < n; ++c) {
        if (!proofs[c]) return VX_ERR_ARG;
        VX_TRY(claimed_transcript_check(&claims[c], chain_prefix(c).c_str(), ch[c], cfg, proofs[c], lens[c], 0, nullptr, 0, ext_chals ? ext_chals[c] : nullptr, QueryPhase::Walked, nullptr, err,
                                        errlen));
    }
    // ---- the table, and the verifier as the outside party of its bus
    BusTable tab[1];
    VX_TRY(read_blob(blob, len, VX_STRN_MAGIC, "stark-transcripts", blob + 1, n_request, tab, 1, err, errlen));
    NEED(peek_tables(cfg, tab, 1), "the proof is too short to hold a trace cap");
    uint64_t stmt[4], pub[tsc::PUB];
    vx_stark_transcripts_statement(claims.data(), n, stmt);
    vx_transcript_public(stmt, pub);
    tab[0].expect(VX_AIR_TRANSCRIPT, pub, tsc::PUB);
    return verify_bus_group(cfg, tab, 1, "the transcripts the table proves are not the claimed ones (the lookup bus does not balance)", err, errlen, [&](const VBus& bus, BusMessages& m) {
        for (size_t c = 0; c < n; ++c) transcript_messages(bus, m, c, claims[c]);
    });
}
}

void vx_stark_inner_statement(const std::array<uint64_t, 7>& shape, const TranscriptClaim& chain, uint64_t digest[4]) {
    std::vector<uint64_t> w(shape.begin(), shape.end());
    w.reserve(9 + chain.n_obs + 2 * chain.n_chal);
    w.push_back(chain.n_obs), w.push_back(chain.n_chal);
    w.insert(w.end(), chain.words, chain.words + chain.n_obs);
    w.insert(w.end(), chain.chal, chain.chal + 2 * chain.n_chal);
    glh::hash_no_pad(w.data(), w.size(), digest);
}

// ---- the three proof-sourced groups (the prover is vx_stark_groups.hip), levels of ONE group: statement digest, public inputs and
// verifier body are stated once, for every level
void stark_group_statement(StarkLevel level, const StarkQueries& sq, const uint64_t* roots, const TranscriptClaim& chain, uint64_t digest[4]) {
    if (level == StarkLevel::Openings) vx_stark_openings_statement(sq.so, roots, digest);
    else if (level == StarkLevel::Queries) vx_stark_queries_statement(sq, roots, digest);
    else vx_stark_inner_statement(sq.so.shape_words(), chain, digest);
}
static_assert(mop::SET_PUB <= VX_STARK_TABLE_MAX_PUB && lsp::PUB <= VX_STARK_TABLE_MAX_PUB && lnp::PUB <= VX_STARK_TABLE_MAX_PUB && fca::PUB <= VX_STARK_TABLE_MAX_PUB &&
                  ffa::PUB <= VX_STARK_TABLE_MAX_PUB && tsc::PUB <= VX_STARK_TABLE_MAX_PUB,
              "vx_bus.h: VX_STARK_TABLE_MAX_PUB is smaller than a table's public inputs");
size_t stark_table_public(const StarkGroupTables& ts, int k, const StarkQueries& sq, const uint64_t stmt[4], uint64_t* pub) {
    const StarkOpenings& so = sq.so;
    switch (ts.air[k]) {
        case VX_AIR_MERKLE_OPEN_SET: vx_merkle_open_set_public(stmt, pub); return mop::SET_PUB;
        case VX_AIR_LEAF_SPONGE_SET: vx_leaf_sponge_set_public(ts.leaf_len[k], stmt, pub); return lsp::PUB;
        case VX_AIR_LEAF_NOOP: vx_leaf_noop_public(stmt, pub); return lnp::PUB;
        case VX_AIR_FRI_COMBINE: vx_fri_combine_public_digest(sq.stmt(), fca::TREE0, stmt, pub); return fca::PUB;
        case VX_AIR_FRI_FOLD: vx_fri_fold_public_digest(so.LN, sq.betas.data(), so.NL, 0, stmt, pub); return ffa::PUB;
        default: vx_transcript_public(stmt, pub); return tsc::PUB;  // VX_AIR_TRANSCRIPT: the table lists hold no other AIR
    }
}

// The ONE verifier body.  What a level's tables are: vx_table_shapes.h.  How the inner proof is replayed:
//   Openings  delegated: every check except the paths (no path is walked, no leaf hashed, no sibling read);
//   Queries   QUERY-FREE: transcript, proof of work, the constraint identity at zeta, reduce_openings and the query indices, from the
//             head of the proof alone -- it may be handed over whole or without its query records;
//   Inner     query-free over the CLAIMED challenger (claimed_transcript_check): no Poseidon permutation runs for the inner transcript.
// The verifier is the party outside the tables.  Openings: per claim (query, tree) it receives the root the path ended in with the
// tree's depth -- the tables do not know which root belongs to which tree, the verifier does --, every word of a row longer than 4
// words, and the opening itself of a row that is its own digest:
//     sum over the tables of total x rows = sum over the claims of 1 / D_root(tree, lo) + 1 / D_root(tree, hi)
//         + [leaf_len > 4] sum over j of 1 / D_row(tree, index, j, word_j)  +  [leaf_len <= 4] (1 / D_open(lo) + 1 / D_open(hi)).
// Queries and Inner: per query the roots of every tree of the record and the exit of the fold chain, fri(index, final_poly(x_NL), 1);
// Inner adds the messages of chain 0 (transcript_messages):
//     sum over the tables of total x rows = sum over the queries of sum over the trees (1 / D_root(lo) + 1 / D_root(hi)) + 1 / D_fri(exit)
//                                           [+ sum_j 1 / D_chal(0, j, A_j, v_j) - sum_i 1 / D_obs(0, i, w_i)].
// EVERY public input of every table is rebuilt from the inner proof (stark_table_public over the level's statement digest).  What
// forces what: DESIGN.md 5k / 5l / 5o.
static int32_t stark_group_verify(StarkLevel level, const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* proof, size_t proof_len, int expect_air,
                                  const uint64_t* expect_public, size_t n_expect_public, const uint64_t* ext_chal, char* err, size_t errlen) {
    if (!cfg || !blob || !proof) return VX_ERR_ARG;
    const StarkLevelInfo& lv = stark_level(level);
    if (level != StarkLevel::Openings && sp::config_ok(*cfg) && cfg->arity_bits != 4)
        return v_fail(VX_ERR_ARG, err, errlen, "%s: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", lv.name, cfg->arity_bits);
    // ---- the inner proof, replayed as the level says; Inner reads its claims from the blob first, bounds before values
    StarkQueries sq;
    TranscriptClaim claim{nullptr, 0, nullptr, 0};
    ClaimedTranscript ch;
    if (level == StarkLevel::Inner) {
        NEED(len >= lv.hdr && blob[0] == lv.magic, "bad %s blob", lv.blob_name);
        NEED(blob[10] <= (len - lv.hdr) / 2, "blob truncated (the claims)");
        claim = {nullptr, (size_t)blob[9], blob + lv.hdr, (size_t)blob[10]};
        VX_TRY(transcript_claims_ok(claim, "", err, errlen));
        VX_TRY(claimed_transcript_check(&claim, "", ch, cfg, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, QueryPhase::QueryFree, &sq, err, errlen));
    } else if (level == StarkLevel::Queries) {
        VX_TRY(vx_stark_queries_claims(cfg, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, QueryPhase::QueryFree, &sq, err, errlen));
    } else {
        VX_TRY(vx_stark_openings_claims(cfg, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, &sq, err, errlen));
    }
    // ---- the tables: the blob must be for this shape (and these claims).  The table list gives the count and the leaf lengths; every
    // table's rows are read from its proof, so no block count is stated here
    const StarkOpenings& so = sq.so;
    StarkGroupTables ts;
    const bool has_group = stark_level_tables(level, so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, 0, *cfg, &ts);
    if (level == StarkLevel::Openings) {  // this level's verifier words the two refusals apart, as statement errors
        NEED(has_group, "stark openings: the proof's shape has no openings group (a tree without a level, or a table of more than 2^26 rows)");
        NEED(so.cap_h <= 16, "stark openings: cap height %d (at most 16)", so.cap_h);
    } else if (so.cap_h > 16 || !has_group) {
        return v_fail(VX_ERR_ARG, err, errlen, "%s", lv.no_group);
    }
    BusTable tab[StarkGroupTables::MAX];
    const std::vector<uint64_t> request = stark_group_request(level, so, ts.n, claim);
    VX_TRY(read_blob(blob, len, lv.magic, lv.blob_name, request.data(), request.size(), tab, (size_t)ts.n, err, errlen));
    NEED(peek_tables(cfg, tab, (size_t)ts.n), "a proof is too short to hold a trace cap");
    const std::vector<uint64_t> roots = so.roots();
    uint64_t stmt[4], pub[StarkGroupTables::MAX][VX_STARK_TABLE_MAX_PUB];
    stark_group_statement(level, sq, roots.data(), claim, stmt);
    for (int k = 0; k < ts.n; ++k) tab[k].expect(ts.air[k], pub[k], stark_table_public(ts, k, sq, stmt, pub[k]));
    const size_t n_trees = so.tree.size();
    return verify_bus_group(cfg, tab, (size_t)ts.n, lv.unbalanced, err, errlen, [&](const VBus& bus, BusMessages& m) {
        if (level == StarkLevel::Openings) {
            m.reserve(2 * so.claims.size() + so.leaves.size());
            for (size_t i = 0; i < so.claims.size(); ++i) {
                const StarkOpenings::Claim& c = so.claims[i];
                const uint64_t* leaf = so.leaves.data() + c.leaf;
                const Fx tree{c.tree, 0}, idx{c.index, 0};
                m.receive_root(bus, c.tree, roots.data() + 4 * (i % n_trees), so.log_leaves(c.tree));
                if (c.leaf_len > 4) {
                    for (size_t j = 0; j < c.leaf_len; ++j) m.receive(bus.row_of(tree, idx, Fx{(uint64_t)j, 0}, Fx{leaf[j], 0}));
                } else {
                    uint64_t d[4] = {0, 0, 0, 0};
                    memcpy(d, leaf, c.leaf_len * 8);
                    m.receive(bus.open_of(tree, idx, Fx{d[0], 0}, Fx{d[1], 0}, bus::K<0>{}));
                    m.receive(bus.open_of(tree, idx, Fx{d[2], 0}, Fx{d[3], 0}, bus::K<1>{}));
                }
            }
            return;
        }
        m.reserve(so.n_queries * (2 * n_trees + 1) + claim.n_obs + claim.n_chal);
        for (size_t i = 0; i < so.n_queries; ++i) {
            for (size_t t = 0; t < n_trees; ++t) m.receive_root(bus, so.tree[t], roots.data() + 4 * t, so.log_leaves(so.tree[t]));
            m.receive_exit(bus, so.index[i], so.LN, so.NL, sq.final_poly.data(), sq.final_poly.size() / 2);
        }
        if (level == StarkLevel::Inner) transcript_messages(bus, m, 0, claim);
    });
}
extern "C" {
int32_t vx_stark_openings_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* proof, size_t proof_len, int expect_air, const uint64_t* expect_public,
                                 size_t n_expect_public, const uint64_t* ext_chal, char* err, size_t errlen) {
    return stark_group_verify(StarkLevel::Openings, cfg, blob, len, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, err, errlen);
}
int32_t vx_stark_queries_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* proof, size_t proof_len, int expect_air, const uint64_t* expect_public,
                                size_t n_expect_public, const uint64_t* ext_chal, char* err, size_t errlen) {
    return stark_group_verify(StarkLevel::Queries, cfg, blob, len, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, err, errlen);
}
int32_t vx_stark_inner_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const uint64_t* proof, size_t proof_len, int expect_air, const uint64_t* expect_public,
                              size_t n_expect_public, const uint64_t* ext_chal, char* err, size_t errlen) {
    return stark_group_verify(StarkLevel::Inner, cfg, blob, len, proof, proof_len, expect_air, expect_public, n_expect_public, ext_chal, err, errlen);
}
}

// ---- the generic bus group (include/vx.h "A generic bus group"; the prover is vx_bus_group.hip).  The verifier states its own AIR
// ids and public inputs -- the blob carries neither -- and the outside party's messages as words (t0, t1, t2, t3, tag, m): m is the
// party's own signed multiplicity (sent m, received 0 - m), so the right-hand side of verify_bus_group gets 0 - m per message.
bool vx_air_bus_shape(int air_id, BusAirShape* out) {
    for (const AirV& a : AIRS_V)
        if (a.id == air_id) {
            *out = {a.cols, a.pub, a.aux, a.chal, a.auxpub, nullptr};
            return true;
        }
    if (air_id >= VX_AIR_USER_BASE)
        if (const AirProgram* pg = vx_air_program_find(air_id)) {
            *out = {(int)pg->cols, (int)pg->pub, (int)pg->aux, (int)pg->chal, (int)pg->auxpub, pg};
            return true;
        }
    return false;
}
int32_t vx_bus_group_admit(const int32_t* air_ids, const size_t* n_public, size_t n, BusAirShape* shapes, char* err, size_t errlen) {
    AIRP_NEED(n >= 1 && n <= (size_t)VX_BUS_GROUP_MAX_TABLES, "bus group: %zu tables (1..%d)", n, (int)VX_BUS_GROUP_MAX_TABLES);
    for (size_t k = 0; k < n; ++k) {
        BusAirShape sh;
        AIRP_NEED(vx_air_bus_shape(air_ids[k], &sh), "bus group: table %zu names no AIR (%d)", k, air_ids[k]);
        AIRP_NEED(sh.aux > 0 && sh.chal == 4 && sh.auxpub == 1, "bus group: table %zu (air %d) has no logUp round of 4 challenges and one total", k, air_ids[k]);
        if (n_public) AIRP_NEED(n_public[k] <= (size_t)BusMeet::MAX_PUB, "bus group: table %zu has %zu public inputs (at most %d)", k, n_public[k], BusMeet::MAX_PUB);
        if (shapes) shapes[k] = sh;
    }
    return VX_OK;
}
int32_t vx_bus_outside_ok(const uint64_t* outside, size_t n_outside, int32_t code, char* err, size_t errlen) {
    if (n_outside && !outside) return v_fail(code, err, errlen, "bus group: %zu outside messages and no words", n_outside);
    for (size_t i = 0; i < n_outside; ++i) {
        const uint64_t* w = outside + i * VX_BUS_MSG_WORDS;
        for (int j = 0; j < VX_BUS_MSG_WORDS; ++j)
            if (w[j] >= glh::P) return v_fail(code, err, errlen, "bus group: outside message %zu has a non-canonical word at %d", i, j);
        if (w[4] >> 16) return v_fail(code, err, errlen, "bus group: outside message %zu has a tag of 2^16 or more", i);
    }
    return VX_OK;
}
// the outside party of a generic group from its words
static BusOutside bus_outside_words(const uint64_t* outside, size_t n_outside) {
    return [=](const VBus& bus, BusMessages& m) {
        m.reserve(n_outside);
        for (size_t i = 0; i < n_outside; ++i) {
            const uint64_t* w = outside + i * VX_BUS_MSG_WORDS;
            if (w[5]) m.put(bus.denom(bus.beta, Fx{w[0], 0}, Fx{w[1], 0}, Fx{w[2], 0}, Fx{w[3], 0}, Fx{w[4], 0}), glh::sub(0, w[5]));
        }
    };
}
int32_t vx_bus_group_closes(const vx_stark_config* cfg, const uint64_t* const* proofs, const size_t* lens, size_t n, const uint64_t* outside, size_t n_outside, char* err, size_t errlen) {
    std::vector<BusTable> tab(n);
    for (size_t k = 0; k < n; ++k) tab[k].proof = proofs[k], tab[k].len = lens[k];
    NEED(peek_tables(cfg, tab.data(), n), "bus group: a proof is too short to hold a trace cap");
    std::vector<const uint64_t*> pubs(n), caps(n);
    std::vector<size_t> n_pubs(n);
    for (size_t k = 0; k < n; ++k) pubs[k] = tab[k].pub, n_pubs[k] = tab[k].n_pub, caps[k] = tab[k].cap;
    const size_t cw = (size_t)4 << cfg->cap_height;
    uint64_t chal[4], bus[2] = {0, 0};
    stark_proof::shared_challenges_n(pubs.data(), n_pubs.data(), caps.data(), n, cw, chal, 4);
    for (size_t k = 0; k < n; ++k) {  // (an admitted table has an auxiliary round: its total follows the trace cap)
        NEED(tab[k].len >= (size_t)(tab[k].cap - tab[k].proof) + cw + 2 && tab[k].proof[2] < 64, "bus group: a proof is too short to hold its total");
        for (int q = 0; q < 2; ++q) bus[q] = glh::add(bus[q], glh::mul(tab[k].cap[cw + q] % glh::P, ((uint64_t)1 << tab[k].proof[2]) % glh::P));
    }
    BusMessages msgs;
    bus_outside_words(outside, n_outside)(VBus(Fx{chal[0], 0}, Fx{chal[1], 0}, Fx{chal[2], 0}, Fx{chal[3], 0}), msgs);
    X2<Fx> sum;
    NEED(bus_messages_sum(msgs, &sum), "bus group: an outside message has a zero denominator under the challenges");
    NEED(sum.a.b == 0 && sum.b.b == 0 && bus[0] == sum.a.a && bus[1] == sum.b.a, "bus group: the bus does not close (the tables' totals and the outside messages do not cancel)");
    return VX_OK;
}
extern "C" int32_t vx_bus_group_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t len, const vx_bus_expect* expect, size_t n, const uint64_t* outside, size_t n_outside,
                                       char* err, size_t errlen) {
    if (!cfg || !blob || !expect) return VX_ERR_ARG;
    int32_t ids[VX_BUS_GROUP_MAX_TABLES];
    size_t n_pub[VX_BUS_GROUP_MAX_TABLES];
    for (size_t k = 0; k < n && k < (size_t)VX_BUS_GROUP_MAX_TABLES; ++k) ids[k] = expect[k].air_id, n_pub[k] = expect[k].n_public;
    BusAirShape shape[VX_BUS_GROUP_MAX_TABLES];
    VX_TRY(vx_bus_group_admit(ids, n_pub, n, shape, err, errlen));
    static const uint64_t no_words[1] = {0};
    for (size_t k = 0; k < n; ++k) {  // (the public inputs are always compared: an AIR without any is compared with none)
        if (expect[k].n_public && !expect[k].public_inputs) return VX_ERR_ARG;
        NEED(expect[k].n_public == (size_t)shape[k].pub, "bus group: table %zu (air %d) takes %d public inputs, %zu expected", k, ids[k], shape[k].pub, expect[k].n_public);
    }
    VX_TRY(vx_bus_outside_ok(outside, n_outside, VX_ERR_STATEMENT, err, errlen));
    NEED(len >= VX_BGRP_HDR && blob[0] == VX_BGRP_MAGIC, "bad bus-group blob");
    NEED(blob[1] == n, "blob is for a different request (%llu tables, %zu expected)", (unsigned long long)blob[1], n);
    BusTable tab[VX_BUS_GROUP_MAX_TABLES];
    VX_TRY(read_blob(blob, len, VX_BGRP_MAGIC, "bus-group", {(uint64_t)n}, tab, n, err, errlen));
    NEED(peek_tables(cfg, tab, n), "a proof is too short to hold a trace cap");
    for (size_t k = 0; k < n; ++k) tab[k].expect(expect[k].air_id, expect[k].n_public ? expect[k].public_inputs : no_words, expect[k].n_public);
    return verify_bus_group(cfg, tab, n, "the lookup bus does not balance", err, errlen, bus_outside_words(outside, n_outside));
}
