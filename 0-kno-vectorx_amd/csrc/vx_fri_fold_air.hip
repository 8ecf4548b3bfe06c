// Witness and prover of FriFoldAir (air_fri_fold.cuh): the FRI fold chain of every query of one inner proof in one table.
//   k_fri_fold_trace  one lane per ROW.  The rows of a query are a chain only through ev_l, and the prover holds every leaf (slot
//                     `within` of leaf l IS ev_l), so every row is independent: a lane recomputes its row from (index, layer,
//                     leaf, beta_l) -- the digits, 1 / x_l by a small power, the one-hots, the four fold levels, the prefix of
//                     the square-and-multiply accumulator -- and stores its cells itself (adjacent lanes = adjacent rows of a
//                     column).  A bit row refolds the last leaf: it carries ev_NL.  Fold rows and bit rows run the same code;
//                     the table is a few hundred rows and latency-bound, so nothing here is tuned
// The auxiliary columns are bus_aux.cuh's, from the AIR's own message list: one lane per row, 17 helpers.
// vx_fri_fold_prove folds every query natively on the host first (the same level algebra in Fx) and refuses a chain that does
// not hold, or does not end in the final polynomial, with VX_ERR_STATEMENT before anything is proven.
// Parity: tests/test_gpu_fri_fold.py compares trace, auxiliary columns and proof with tests/fri_fold_ref.py and the reference prover.
#include <string.h>

#include "air_fri_fold.cuh"
#include "bus_aux.cuh"
#include "glh_poseidon.h"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace ffa;

struct FoldArgs {
    const uint64_t* index;   // [n_queries], < 2^LN (checked by the host)
    const uint64_t* leaves;  // [n_queries][NL][32], canonical (checked by the host)
    uint64_t beta[2 * MAX_LAYERS];
    size_t n_queries, n;
    int LN, NL, rpq;         // rpq = NL + FB rows per query
    uint64_t winv;           // 1 / w, w the 2^LN-th root of unity
    uint64_t* tr;            // [COLS][n]
};

__device__ __forceinline__ uint64_t brev64(uint64_t x, int bits) { return bits ? __brevll(x) >> (64 - bits) : 0; }

__global__ __launch_bounds__(64) void k_fri_fold_trace(FoldArgs a) {
    constexpr Tab T = make_tab();
    const size_t i = blockIdx.x * (size_t)64 + threadIdx.x;
    if (i >= a.n) return;
    uint64_t* out = a.tr + i;
    auto put = [&](int col, uint64_t v) { out[(size_t)col * a.n] = v; };
    const size_t qi = i / (size_t)a.rpq;
    if (qi >= a.n_queries) {  // an idle row
#pragma unroll 8
        for (int j = 0; j < COLS; ++j) put(j, 0);
        return;
    }
    const int k = (int)(i - qi * (size_t)a.rpq);
    const bool is_fold = k < a.NL;
    const uint64_t fo = is_fold ? ~(uint64_t)0 : 0;  // the mask of a fold row's cells
    const uint64_t index = a.index[qi];
    const int l = is_fold ? k : a.NL - 1;                     // the layer whose leaf this row folds
    const int pos = is_fold ? 4 * k : 4 * a.NL + (k - a.NL);  // index bits consumed before this row
    const uint64_t rr = index >> pos, within = is_fold ? rr & 15 : rr & 1;
    put(ACT, 1), put(FOLD, is_fold), put(FIRST, k == 0), put(LAST, k == a.rpq - 1), put(FBIT, k == a.NL);
    put(CNT, (uint64_t)k), put(R, rr), put(Q, is_fold ? rr >> 4 : rr >> 1), put(IDX, index);
#pragma unroll
    for (int t = 0; t < 4; ++t) put(B + t, (within >> t) & 1);
#pragma unroll
    for (int t = 0; t < 16; ++t) put(OH + t, is_fold && (uint64_t)t == within);
#pragma unroll
    for (int t = 0; t < MAX_LAYERS; ++t) put(LSEL + t, is_fold && t == k);
    {  // the accumulator: w^-bitrev(the bits consumed so far), then this row's own steps
        uint64_t acc = gl_pow(a.winv, brev64(index & (((uint64_t)1 << pos) - 1), pos));
        put(A, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc = gl_sqr(acc);
            if ((within >> t) & 1) acc = gl_mul(acc, a.winv);
            put(A + 1 + t, acc);
        }
    }
    const uint64_t y0 = gl_mul(INV7, gl_pow(a.winv, brev64(index, a.LN)));
    uint64_t yl = y0;  // 1 / x_l = (1 / x_0)^(16^l)
    for (int t = 0; t < 4 * l; ++t) yl = gl_sqr(yl);
    put(Y0, y0);
    const uint64_t wl = (index >> (4 * l)) & 15;
    const uint64_t* leaf = a.leaves + (qi * (size_t)a.NL + (size_t)l) * 32;
    gl2 v[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        v[t] = gl2{leaf[2 * t], leaf[2 * t + 1]};
        put(LEAF + 2 * t, v[t].a & fo), put(LEAF + 2 * t + 1, v[t].b & fo);
    }
    const gl2 ev_in{leaf[2 * wl], leaf[2 * wl + 1]};
    uint64_t s = gl_mul(yl, T.gp[wl]);
    gl2 be{a.beta[2 * l], a.beta[2 * l + 1]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        put(SI + j, s & fo), put(BE + 2 * j, be.a & fo), put(BE + 2 * j + 1, be.b & fo);
#pragma unroll
        for (int p = 0; p < (8 >> j); ++p) {
            const gl2 u = v[2 * p], w = v[2 * p + 1];
            v[p] = gl2_add(gl2_scale(gl2_add(u, w), HALF), gl2_scale(gl2_mul(be, gl2_sub(u, w)), gl_mul(s, T.fc[j][p])));
            put(vlev(j + 1) + 2 * p, v[p].a & fo), put(vlev(j + 1) + 2 * p + 1, v[p].b & fo);
        }
        s = gl_sqr(s), be = gl2_mul(be, be);
    }
    // a fold row: the value entering the layer and 1 / x_l; a bit row: ev_NL and 1 / x_NL (s is (1 / x_l)^16 by now: g^16 = 1)
    const gl2 ev = is_fold ? ev_in : v[0];
    put(EV, ev.a), put(EV + 1, ev.b), put(Y, is_fold ? yl : s);
}

constexpr size_t MAX_QUERIES = (size_t)1 << 20;
bool shape_ok(int log_lde, size_t n_layers, size_t n_queries) {
    return log_lde >= 5 && log_lde <= 32 && n_layers >= 1 && n_layers <= (size_t)MAX_LAYERS && 4 * (int)n_layers < log_lde && n_queries >= 1 && n_queries <= MAX_QUERIES;
}
#define FF_SHAPE_MSG "fri fold: log_lde %d (5..32), %zu layers (1..8, 4 bits each, at least one index bit left), %zu queries (1..2^20)"

// the claims as the host gets them: ranges and canonical words
int32_t check_claims(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries) {
    VX_CHECK(shape_ok(log_lde, n_layers, n_queries), FF_SHAPE_MSG, log_lde, n_layers, n_queries);
    for (size_t i = 0; i < 2 * n_layers; ++i) VX_CHECK(betas[i] < glh::P, "fri fold: non-canonical beta word %zu", i);
    for (size_t i = 0; i < n_queries; ++i) {
        VX_CHECK(index[i] >> log_lde == 0, "fri fold: query %zu has an index outside the LDE", i);
        VX_CHECK(ev0[2 * i] < glh::P && ev0[2 * i + 1] < glh::P, "fri fold: query %zu has a non-canonical ev_0", i);
    }
    for (size_t i = 0; i < n_queries * n_layers * 32; ++i) VX_CHECK(leaves[i] < glh::P, "fri fold: non-canonical leaf word (query %zu, layer %zu)", i / (32 * n_layers), i / 32 % n_layers);
    return VX_OK;
}

}  // namespace

// The witness of FriFoldAir on the device, and the public inputs (vx_bus.h).  The claims have passed check_claims.
int32_t vx_fri_fold_trace_dev(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves,
                           size_t n_queries, int log_n, uint64_t* trace_d, uint64_t pub_out[PUB]) {
    const int rpq = log_lde - 3 * (int)n_layers;
    VX_CHECK(log_n >= 5 && log_n <= 26 && n_queries * (size_t)rpq <= ((size_t)1 << log_n), "fri fold: %zu queries of %d rows do not fit 2^%d rows", n_queries, rpq, log_n);
    VX_CHECK(tree0 < ((uint64_t)1 << 32), "fri fold: TREE0 out of range");
    const size_t w_leaves = n_queries * n_layers * 32;
    Scratch sc;
    uint64_t *index_d, *leaves_d;
    sc.add(index_d, n_queries), sc.add(leaves_d, w_leaves);
    sc.alloc(ctx);
    FoldArgs a{};
    a.index = index_d, a.leaves = leaves_d, a.n_queries = n_queries, a.n = (size_t)1 << log_n, a.LN = log_lde, a.NL = (int)n_layers, a.rpq = rpq;
    a.winv = glh::inv(glh::root(log_lde)), a.tr = trace_d;
    memcpy(a.beta, betas, 2 * n_layers * 8);
    sc.up(index_d, index, n_queries * 8), sc.up(leaves_d, leaves, w_leaves * 8);
    if (sc.ok()) {
        hipLaunchKernelGGL(k_fri_fold_trace, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, ctx->stream, a);
        sc.launched();
    }
    VX_TRY(sc.status("fri fold"));
    vx_fri_fold_public(log_lde, betas, n_layers, tree0, index, ev0, leaves, n_queries, pub_out);
    return VX_OK;
}

namespace {
// ---- the fold on the host (Fx): what the table proves, checked natively before anything is proven
Fx fold16_host(const uint64_t* leaf, uint64_t within, Fx beta, uint64_t x_inv) {
    constexpr Tab T = make_tab();
    Fx v[16];
    for (int t = 0; t < 16; ++t) v[t] = Fx{leaf[2 * t], leaf[2 * t + 1]};
    uint64_t s = glh::mul(x_inv, T.gp[within]);
    for (int j = 0; j < 4; ++j) {
        for (int p = 0; p < (8 >> j); ++p) {
            const Fx u = v[2 * p], w = v[2 * p + 1];
            v[p] = (u + w) * Fx{HALF, 0} + beta * (u - w) * Fx{glh::mul(s, T.fc[j][p]), 0};
        }
        s = glh::mul(s, s), beta = beta * beta;
    }
    return v[0];
}
}  // namespace

// NL, NL + FB, 1 / w, TREE0, the betas (zero behind NL), the claims digest: shared with the verifier (vx_verify.hip)
void vx_fri_fold_public_digest(int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t digest[4], uint64_t pub[24]) {
    pub[PUB_NL] = n_layers, pub[PUB_ROWS] = (uint64_t)log_lde - 3 * n_layers, pub[PUB_WINV] = glh::inv(glh::root(log_lde)), pub[PUB_TREE0] = tree0;
    for (size_t i = 0; i < 2 * (size_t)MAX_LAYERS; ++i) pub[PUB_BETA + i] = i < 2 * n_layers ? betas[i] : 0;
    memcpy(pub + PUB_DIGEST, digest, 32);
}
void vx_fri_fold_public(int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries,
                        uint64_t pub[24]) {
    const size_t per = 3 + 32 * n_layers;
    std::vector<uint64_t> claims(n_queries * per);
    for (size_t i = 0; i < n_queries; ++i) {
        uint64_t* c = claims.data() + i * per;
        c[0] = index[i], c[1] = ev0[2 * i], c[2] = ev0[2 * i + 1];
        memcpy(c + 3, leaves + i * 32 * n_layers, 32 * n_layers * 8);
    }
    uint64_t digest[4];
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_fri_fold_public_digest(log_lde, betas, n_layers, tree0, digest, pub);
}

// ranges, then the statement natively (vx_bus.h): every chain holds and ends in the final polynomial
int32_t vx_fri_fold_check_dev(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len, const uint64_t* index, const uint64_t* ev0,
                              const uint64_t* leaves, size_t n_queries) {
    VX_TRY(check_claims(ctx, log_lde, betas, n_layers, index, ev0, leaves, n_queries));
    VX_CHECK(final_len >= 1 && final_len <= ((size_t)1 << 27), "fri fold: a final polynomial of %zu coefficients", final_len);
    for (size_t i = 0; i < 2 * final_len; ++i) VX_CHECK(final_poly[i] < glh::P, "fri fold: non-canonical final-polynomial word %zu", i);
    // the statement, natively: leaf_l[within_l] = ev_l, ev_(l+1) = the fold, final_poly(x_NL) = ev_NL
    for (size_t i = 0; i < n_queries; ++i) {
        uint64_t x = stark_proof::query_point(index[i], log_lde), xi = glh::inv(x);
        Fx ev{ev0[2 * i], ev0[2 * i + 1]};
        for (size_t l = 0; l < n_layers; ++l) {
            const uint64_t* leaf = leaves + (i * n_layers + l) * 32;
            const uint64_t within = (index[i] >> (4 * l)) & 15;
            if (leaf[2 * within] != ev.a || leaf[2 * within + 1] != ev.b)
                return vx_fail(ctx, VX_ERR_STATEMENT, "fri fold: query %zu, layer %zu: the leaf's slot %llu is not the value the chain enters the layer with", i, l, (unsigned long long)within);
            ev = fold16_host(leaf, within, Fx{betas[2 * l], betas[2 * l + 1]}, xi);
            x = glh::pow(x, 16), xi = glh::pow(xi, 16);
        }
        const Fx fp = stark_proof::final_poly_at(final_poly, final_len, x);
        if (fp.a != ev.a || fp.b != ev.b)
            return vx_fail(ctx, VX_ERR_STATEMENT, "fri fold: query %zu, layer %zu: the folded value is not the final polynomial's at x^(16^%zu)", i, n_layers, n_layers);
    }
    return VX_OK;
}

int32_t FriFoldAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<FriFoldAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

extern "C" {
int32_t vx_fri_fold_air_trace(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves,
                              size_t n_queries, int log_n, vx_buf* trace_out, uint64_t public_out[24]) {
    if (!ctx || !betas || !index || !ev0 || !leaves || !trace_out || !public_out) return VX_ERR_ARG;
    VX_TRY(check_claims(ctx, log_lde, betas, n_layers, index, ev0, leaves, n_queries));
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)COLS << log_n), "fri fold: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, COLS, log_n);
    return vx_fri_fold_trace_dev(ctx, log_lde, betas, n_layers, tree0, index, ev0, leaves, n_queries, log_n, trace_out->d, public_out);
}

int32_t vx_fri_fold_proof_bound(const vx_stark_config* cfg, int log_lde, size_t n_layers, size_t n_queries, size_t* n_words) {
    if (!cfg || !n_words || cfg->arity_bits != 4 || !shape_ok(log_lde, n_layers, n_queries)) return VX_ERR_ARG;
    const int log_n = fri_fold_log_n(n_queries, log_lde, n_layers);
    if (log_n > 26) return VX_ERR_ARG;
    size_t w = 0;
    const int32_t rc = vx_stark_proof_bound(VX_AIR_FRI_FOLD, cfg, log_n, &w);
    if (rc != VX_OK) return rc;
    *n_words = VX_FFOLD_HDR + w;
    return VX_OK;
}

int32_t vx_fri_fold_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len,
                          const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries, uint64_t* blob_out, size_t blob_cap, size_t* blob_len) {
    if (!ctx || !cfg || !betas || !final_poly || !index || !ev0 || !leaves || !blob_len) return VX_ERR_ARG;
    VX_CHECK(cfg->arity_bits == 4, "fri fold: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    VX_TRY(vx_fri_fold_check_dev(ctx, log_lde, betas, n_layers, final_poly, final_len, index, ev0, leaves, n_queries));
    const int log_n = fri_fold_log_n(n_queries, log_lde, n_layers);
    VX_CHECK(log_n <= 26, "fri fold: %zu queries of %d rows need more than 2^26 rows", n_queries, log_lde - 3 * (int)n_layers);
    TableJob job;
    const vx_chal_hook hook{vx_one_table_hook, nullptr};
    VX_TRY(run_table(ctx, job, VX_AIR_FRI_FOLD, log_n, COLS, PUB, cfg, &hook, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
        return vx_fri_fold_trace_dev(c, log_lde, betas, n_layers, 0, index, ev0, leaves, n_queries, log_n, trace->d, pub);
    }));
    return pack_blob(ctx, "fri fold", VX_FFOLD_MAGIC, {(uint64_t)log_lde, n_layers, n_queries}, {&job}, blob_out, blob_cap, blob_len);
}
}  // extern "C"
