// Witness and prover of FriCombineAir (air_fri_combine.cuh): the FRI combination of every query of one inner proof in one table.
//   k_fri_combine_trace  one lane per ROW, one block of 256 lanes per QUERY, which strides over the query's c + nq + LN rows in
//                        tiles of 256 (adjacent lanes = adjacent rows of a column: every store is coalesced).  The running sum S
//                        is an inclusive prefix scan of alpha^j w_j over the query's absorb rows: a wave scan by cross-lane
//                        shuffles (6 steps), the four wave totals through LDS, and the block's carry from tile to tile in a
//                        register -- no lane walks a query's rows.  A block holds one query, so the scan needs no segment flags; a
//                        bit row adds a zero term and so gets the full sum.  alpha^j comes from a table of c + nq powers built
//                        once per call.  S1 (the sum at row c - 1) is known only after its tile: a second pass over the tiles
//                        stores it, and the last row's lane computes D0, D1 and EV.  A bit row recomputes its accumulator from
//                        (index, bit position).  Blocks behind the queries zero the idle rows.  The table is store-bound (28
//                        columns) and small; nothing else is tuned
// The auxiliary columns are bus_aux.cuh's, from the AIR's own message list: one lane per row; the one helper is also the row's
// running-sum increment.
// vx_fri_combine_prove combines every query natively on the host first and refuses a claimed ev_0 that differs, or x = zeta, with
// VX_ERR_STATEMENT before anything is proven.
// vx_fri_combine_fold_prove: FriCombineAir + FriFoldAir on one bus, TAG_FRI end 0 closing between them.
// Parity: tests/test_gpu_fri_combine.py compares trace, auxiliary columns and proof with tests/fri_combine_ref.py and the reference prover.
#include <string.h>

#include "air_fri_combine.cuh"
#include "air_fri_fold.cuh"
#include "bus_aux.cuh"
#include "stark_proof.h"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace fca;
constexpr int BLOCK = 256, WAVES = BLOCK / 64;

struct CombArgs {
    const uint64_t* index;  // [n_queries], < 2^LN (checked by the host)
    const uint64_t* rows;   // [n_queries][c + nq], canonical (checked by the host)
    const gl2* apow;        // [c + nq]: alpha^j
    size_t n_queries, n;
    int LN, cm, c, absn, rpq;  // c = cm + ca, absn = c + nq absorb rows, rpq = absn + LN rows per query
    uint64_t w;                // the 2^LN-th root of unity
    gl2 alphac, zeta, zetan, y0, y1;
    uint64_t* tr;  // [COLS][n]
};

__device__ __forceinline__ uint64_t brev64(uint64_t x, int bits) { return bits ? __brevll(x) >> (64 - bits) : 0; }
__device__ __forceinline__ gl2 shfl_up2(gl2 v, int d) { return gl2{(uint64_t)__shfl_up((unsigned long long)v.a, d, 64), (uint64_t)__shfl_up((unsigned long long)v.b, d, 64)}; }

__global__ __launch_bounds__(BLOCK) void k_fri_combine_trace(CombArgs a) {
    __shared__ gl2 wave_tot[WAVES];
    __shared__ gl2 s1_sh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (blockIdx.x >= a.n_queries) {  // the idle rows: all zero
        const size_t nb = gridDim.x - a.n_queries;
        for (size_t i = a.n_queries * (size_t)a.rpq + (blockIdx.x - a.n_queries) * (size_t)BLOCK + tid; i < a.n; i += nb * BLOCK)
#pragma unroll 4
            for (int j = 0; j < COLS; ++j) a.tr[(size_t)j * a.n + i] = 0;
        return;
    }
    const size_t qi = blockIdx.x;
    uint64_t* out = a.tr + qi * (size_t)a.rpq;
    const uint64_t index = a.index[qi];
    const uint64_t* words = a.rows + qi * (size_t)a.absn;
    gl2 carry{0, 0};  // the sum of the tiles before this one: the same in every lane
    for (int t0 = 0; t0 < a.rpq; t0 += BLOCK) {  // the trip count is the block's: every lane reaches every barrier and shuffle
        const int k = t0 + tid;
        const bool live = k < a.rpq, is_abs = k < a.absn;
        const uint64_t word = is_abs ? words[k] : 0;
        const gl2 ap = is_abs ? a.apow[k] : gl2{0, 0};
        gl2 v = gl2_scale(ap, word);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const gl2 u = shfl_up2(v, d);
            if (lane >= d) v = gl2_add(v, u);
        }
        if (lane == 63) wave_tot[wid] = v;
        __syncthreads();
        gl2 pre = carry, tot = carry;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) {
            const gl2 t = wave_tot[q];
            tot = gl2_add(tot, t);
            if (q < wid) pre = gl2_add(pre, t);
        }
        const gl2 s = gl2_add(pre, v);
        carry = tot;
        if (live) {
            auto put = [&](int col, uint64_t x) { out[(size_t)col * a.n + k] = x; };
            const int tree = !is_abs ? 3 : k < a.cm ? 0 : k < a.c ? 1 : 2;
            const int pos = tree == 0 ? k : tree == 1 ? k - a.cm : tree == 2 ? k - a.c : 0;
            put(ACT, 1), put(TM, tree == 0), put(TA, tree == 1), put(TQ, tree == 2), put(FIRST, k == 0), put(LAST, k == a.rpq - 1), put(FBIT, k == a.absn);
            put(CNT, (uint64_t)k), put(POS, (uint64_t)pos), put(W, word), put(IDX, index);
            put(AP, ap.a), put(AP + 1, ap.b), put(S, s.a), put(S + 1, s.b);
            uint64_t rr = 0, bit = 0, acc = 0, acc1 = 0;
            if (!is_abs) {  // a bit row: w^bitrev(the bits consumed so far), then this row's own step
                const int j = k - a.absn;
                rr = index >> j, bit = rr & 1;
                acc = gl_pow(a.w, brev64(index & (((uint64_t)1 << j) - 1), j));
                acc1 = gl_sqr(acc);
                if (bit) acc1 = gl_mul(acc1, a.w);
            }
            put(R, rr), put(Q, rr >> 1), put(B, bit), put(A, acc), put(A1, acc1);
            if (k == a.c - 1) s1_sh = s;
        }
        __syncthreads();  // the wave totals are read; the next tile may overwrite them
    }
    const gl2 s1 = s1_sh, s0 = carry;
    for (int t0 = 0; t0 < a.rpq; t0 += BLOCK) {
        const int k = t0 + tid;
        if (k >= a.rpq) break;
        auto put = [&](int col, uint64_t x) { out[(size_t)col * a.n + k] = x; };
        gl2 d0{0, 0}, d1{0, 0}, ev{0, 0};
        if (k == a.rpq - 1) {  // the query's last row: x = 7 w^bitrev(index), the two inverses, ev_0 (the host has refused x = zeta)
            const uint64_t x = gl_mul(7, gl_pow(a.w, brev64(index, a.LN)));
            d0 = gl2_inv(gl2{gl_sub(x, a.zeta.a), gl_neg(a.zeta.b)});
            d1 = gl2_inv(gl2{gl_sub(x, a.zetan.a), gl_neg(a.zetan.b)});
            ev = gl2_add(gl2_mul(gl2_mul(a.alphac, gl2_sub(s0, a.y0)), d0), gl2_mul(gl2_sub(s1, a.y1), d1));
        }
        put(S1, s1.a), put(S1 + 1, s1.b), put(D0, d0.a), put(D0 + 1, d0.b), put(D1, d1.a), put(D1 + 1, d1.b), put(EV, ev.a), put(EV + 1, ev.b);
    }
}

constexpr size_t MAX_QUERIES = (size_t)1 << 20, MAX_ROW = (size_t)1 << 20;
bool shape_ok(int log_lde, int rate_bits, size_t cm, size_t ca, size_t nq, size_t n_queries) {
    return log_lde >= 5 && log_lde <= 32 && rate_bits >= 1 && rate_bits < log_lde && cm >= 1 && nq >= 1 && cm <= MAX_ROW && ca <= MAX_ROW && nq <= MAX_ROW && n_queries >= 1 &&
           n_queries <= MAX_QUERIES;
}
#define FC_SHAPE_MSG "fri combine: log_lde %d (5..32), rate_bits %d (1..log_lde - 1), %zu main (1..2^20), %zu auxiliary (0..2^20), %zu quotient columns (1..2^20), %zu queries (1..2^20)"
}  // namespace

int32_t vx_fri_combine_check_claims(vx_ctx* ctx, const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries) {
    VX_CHECK(shape_ok(st.log_lde, st.rate_bits, st.cm, st.ca, st.nq, n_queries), FC_SHAPE_MSG, st.log_lde, st.rate_bits, st.cm, st.ca, st.nq, n_queries);
    const size_t c = st.cm + st.ca, absn = c + st.nq;
    for (int i = 0; i < 2; ++i) VX_CHECK(st.alpha[i] < glh::P && st.zeta[i] < glh::P, "fri combine: non-canonical alpha or zeta");
    for (size_t i = 0; i < 2 * c; ++i) VX_CHECK(st.open_local[i] < glh::P && st.open_next[i] < glh::P, "fri combine: non-canonical opening word %zu", i);
    for (size_t i = 0; i < 2 * st.nq; ++i) VX_CHECK(st.open_quot[i] < glh::P, "fri combine: non-canonical quotient opening word %zu", i);
    for (size_t i = 0; i < n_queries; ++i) {
        VX_CHECK(index[i] >> st.log_lde == 0, "fri combine: query %zu has an index outside the LDE", i);
        VX_CHECK(ev0[2 * i] < glh::P && ev0[2 * i + 1] < glh::P, "fri combine: query %zu has a non-canonical ev_0", i);
    }
    for (size_t i = 0; i < n_queries * absn; ++i) VX_CHECK(rows[i] < glh::P, "fri combine: non-canonical row word (query %zu, word %zu)", i / absn, i % absn);
    return VX_OK;
}

// what prover and verifier compute ONCE per proof: alpha^c, zeta' = zeta w_n and the reduced openings
void vx_fri_combine_reduced(const FriCombineStmt& st, uint64_t alphac[2], uint64_t zetan[2], uint64_t y0[2], uint64_t y1[2]) {
    const stark_proof::Reduced red = stark_proof::reduce_openings(Fx{st.alpha[0], st.alpha[1]}, st.open_local, st.open_next, st.open_quot, st.cm + st.ca, st.nq);
    const Fx ap = red.alpha_c, a0 = red.y0, a1 = red.y1;
    alphac[0] = ap.a, alphac[1] = ap.b;
    const Fx zn = Fx{st.zeta[0], st.zeta[1]} * Fx{glh::root(st.log_lde - st.rate_bits), 0};
    zetan[0] = zn.a, zetan[1] = zn.b, y0[0] = a0.a, y0[1] = a0.b, y1[0] = a1.a, y1[1] = a1.b;
}

void vx_fri_combine_public_digest(const FriCombineStmt& st, uint64_t tree0, const uint64_t digest[4], uint64_t pub[22]) {
    pub[PUB_ROWS] = st.cm + st.ca + st.nq + (uint64_t)st.log_lde, pub[PUB_CM] = st.cm, pub[PUB_CA] = st.ca, pub[PUB_NQ] = st.nq, pub[PUB_TREE0] = tree0, pub[PUB_W] = glh::root(st.log_lde);
    memcpy(pub + PUB_ALPHA, st.alpha, 16), memcpy(pub + PUB_ZETA, st.zeta, 16);
    vx_fri_combine_reduced(st, pub + PUB_ALPHAC, pub + PUB_ZETAN, pub + PUB_Y0, pub + PUB_Y1);
    memcpy(pub + PUB_DIGEST, digest, 32);
}
// the shape, alpha, zeta and the openings: the head of the claims digest and of the group's statement digest
void vx_fri_combine_statement_words(const FriCombineStmt& st, size_t n_queries, std::vector<uint64_t>& w) {
    const size_t c = st.cm + st.ca;
    for (uint64_t v : {(uint64_t)st.log_lde, (uint64_t)st.rate_bits, (uint64_t)st.cm, (uint64_t)st.ca, (uint64_t)st.nq, (uint64_t)n_queries, st.alpha[0], st.alpha[1], st.zeta[0], st.zeta[1]})
        w.push_back(v);
    w.insert(w.end(), st.open_local, st.open_local + 2 * c);
    w.insert(w.end(), st.open_next, st.open_next + 2 * c);
    w.insert(w.end(), st.open_quot, st.open_quot + 2 * st.nq);
}
void vx_fri_combine_public(const FriCombineStmt& st, uint64_t tree0, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries, uint64_t pub[22]) {
    const size_t absn = st.cm + st.ca + st.nq;
    std::vector<uint64_t> w;
    w.reserve(10 + 4 * absn + n_queries * (absn + 3));
    vx_fri_combine_statement_words(st, n_queries, w);
    for (size_t i = 0; i < n_queries; ++i) {
        w.push_back(index[i]);
        w.insert(w.end(), rows + i * absn, rows + (i + 1) * absn);
        w.push_back(ev0[2 * i]), w.push_back(ev0[2 * i + 1]);
    }
    uint64_t digest[4];
    glh::hash_no_pad(w.data(), w.size(), digest);
    vx_fri_combine_public_digest(st, tree0, digest, pub);
}

// The witness of FriCombineAir on the device, and the public inputs (vx_bus.h).  The claims have passed vx_fri_combine_check_claims.
int32_t vx_fri_combine_trace_dev(vx_ctx* ctx, const FriCombineStmt& st, uint64_t tree0, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries, int log_n,
                                 uint64_t* trace_d, uint64_t pub_out[22]) {
    const size_t c = st.cm + st.ca, absn = c + st.nq, rpq = absn + (size_t)st.log_lde;
    VX_CHECK(log_n >= 5 && log_n <= 26 && n_queries * rpq <= ((size_t)1 << log_n), "fri combine: %zu queries of %zu rows do not fit 2^%d rows", n_queries, rpq, log_n);
    VX_CHECK(tree0 < ((uint64_t)1 << 32), "fri combine: TREE0 out of range");
    vx_fri_combine_public(st, tree0, index, rows, ev0, n_queries, pub_out);
    std::vector<uint64_t> apow(2 * absn);  // alpha^j, once per call
    {
        const Fx alpha{st.alpha[0], st.alpha[1]};
        Fx ap{1, 0};
        for (size_t j = 0; j < absn; ++j, ap = ap * alpha) apow[2 * j] = ap.a, apow[2 * j + 1] = ap.b;
    }
    const size_t w_rows = n_queries * absn;
    Scratch sc;
    uint64_t *index_d, *rows_d, *apow_d;
    sc.add(index_d, n_queries), sc.add(rows_d, w_rows), sc.add(apow_d, 2 * absn);
    sc.alloc(ctx);
    CombArgs a{};
    a.index = index_d, a.rows = rows_d, a.apow = (const gl2*)apow_d, a.n_queries = n_queries, a.n = (size_t)1 << log_n;
    a.LN = st.log_lde, a.cm = (int)st.cm, a.c = (int)c, a.absn = (int)absn, a.rpq = (int)rpq, a.w = pub_out[PUB_W], a.tr = trace_d;
    a.alphac = gl2{pub_out[PUB_ALPHAC], pub_out[PUB_ALPHAC + 1]}, a.zeta = gl2{st.zeta[0], st.zeta[1]}, a.zetan = gl2{pub_out[PUB_ZETAN], pub_out[PUB_ZETAN + 1]};
    a.y0 = gl2{pub_out[PUB_Y0], pub_out[PUB_Y0 + 1]}, a.y1 = gl2{pub_out[PUB_Y1], pub_out[PUB_Y1 + 1]};
    const size_t idle = a.n - n_queries * rpq, idle_blocks = idle ? ((idle + BLOCK - 1) / BLOCK < 1024 ? (idle + BLOCK - 1) / BLOCK : 1024) : 0;
    sc.up(index_d, index, n_queries * 8), sc.up(rows_d, rows, w_rows * 8), sc.up(apow_d, apow.data(), 2 * absn * 8);
    if (sc.ok()) {
        hipLaunchKernelGGL(k_fri_combine_trace, dim3((unsigned)(n_queries + idle_blocks)), dim3(BLOCK), 0, ctx->stream, a);
        sc.launched();
    }
    return sc.status("fri combine");
}

// the combination on the host (Fx), what the table proves: ev0_out [n_queries][2]; VX_ERR_STATEMENT when x = zeta or zeta w_n
int32_t vx_fri_combine_host(vx_ctx* ctx, const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, size_t n_queries, uint64_t* ev0_out) {
    const size_t c = st.cm + st.ca, absn = c + st.nq;
    uint64_t ac[2], zn[2], y0[2], y1[2];
    vx_fri_combine_reduced(st, ac, zn, y0, y1);
    const Fx alpha{st.alpha[0], st.alpha[1]}, zeta{st.zeta[0], st.zeta[1]};
    for (size_t i = 0; i < n_queries; ++i) {
        const Fx x{stark_proof::query_point(index[i], st.log_lde), 0}, e0 = x - zeta, e1 = x - Fx{zn[0], zn[1]};
        if ((e0.a | e0.b) == 0 || (e1.a | e1.b) == 0) return vx_fail(ctx, VX_ERR_STATEMENT, "fri combine: query %zu: the point of the index is zeta or zeta w_n", i);
        Fx s1{0, 0}, s0{0, 0}, ap{1, 0};
        for (size_t j = 0; j < absn; ++j) {
            s0 = s0 + ap * Fx{rows[i * absn + j], 0};
            if (j + 1 == c) s1 = s0;
            ap = ap * alpha;
        }
        const Fx ev = Fx{ac[0], ac[1]} * (s0 - Fx{y0[0], y0[1]}) * fx_inv(e0) + (s1 - Fx{y1[0], y1[1]}) * fx_inv(e1);
        ev0_out[2 * i] = ev.a, ev0_out[2 * i + 1] = ev.b;
    }
    return VX_OK;
}

// ranges, then the statement natively (vx_bus.h): every claimed ev_0 is the combination of its rows
int32_t vx_fri_combine_check_dev(vx_ctx* ctx, const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries) {
    VX_TRY(vx_fri_combine_check_claims(ctx, st, index, rows, ev0, n_queries));
    std::vector<uint64_t> ev(2 * n_queries);
    VX_TRY(vx_fri_combine_host(ctx, st, index, rows, n_queries, ev.data()));
    for (size_t i = 0; i < n_queries; ++i)
        if (ev[2 * i] != ev0[2 * i] || ev[2 * i + 1] != ev0[2 * i + 1])
            return vx_fail(ctx, VX_ERR_STATEMENT, "fri combine: query %zu: the claimed ev_0 is not the combination of the opened rows", i);
    return VX_OK;
}

// the statement of FriCombineAir + FriFoldAir on one bus: hash_n_to_hash_no_pad(the combine statement's head, n_layers, betas,
// final_poly, (index, rows, leaves) of every query) -- everything the verifier puts on the bus is a function of it
void vx_fri_combine_fold_statement(const FriCombineStmt& st, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len, const uint64_t* index,
                                   const uint64_t* rows, const uint64_t* leaves, size_t n_queries, uint64_t digest[4]) {
    const size_t absn = st.cm + st.ca + st.nq;
    std::vector<uint64_t> w;
    w.reserve(11 + 4 * absn + 2 * n_layers + 2 * final_len + n_queries * (1 + absn + 32 * n_layers));
    vx_fri_combine_statement_words(st, n_queries, w);
    w.push_back(n_layers);
    w.insert(w.end(), betas, betas + 2 * n_layers);
    w.insert(w.end(), final_poly, final_poly + 2 * final_len);
    for (size_t i = 0; i < n_queries; ++i) {
        w.push_back(index[i]);
        w.insert(w.end(), rows + i * absn, rows + (i + 1) * absn);
        w.insert(w.end(), leaves + i * 32 * n_layers, leaves + (i + 1) * 32 * n_layers);
    }
    glh::hash_no_pad(w.data(), w.size(), digest);
}

int32_t FriCombineAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<FriCombineAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

extern "C" {
int32_t vx_fri_combine_air_trace(vx_ctx* ctx, int log_lde, int rate_bits, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2], const uint64_t* open_local,
                                 const uint64_t* open_next, const uint64_t* open_quot, uint64_t tree0, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries,
                                 int log_n, vx_buf* trace_out, uint64_t public_out[22]) {
    if (!ctx || !alpha || !zeta || !open_local || !open_next || !open_quot || !index || !rows || !ev0 || !trace_out || !public_out) return VX_ERR_ARG;
    const FriCombineStmt st{log_lde, rate_bits, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot};
    VX_TRY(vx_fri_combine_check_claims(ctx, st, index, rows, ev0, n_queries));
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)COLS << log_n), "fri combine: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, COLS, log_n);
    return vx_fri_combine_trace_dev(ctx, st, tree0, index, rows, ev0, n_queries, log_n, trace_out->d, public_out);
}

int32_t vx_fri_combine_proof_bound(const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, size_t n_queries, size_t* n_words) {
    if (!cfg || !n_words || !shape_ok(log_lde, cfg->rate_bits, cm, ca, nq, n_queries)) return VX_ERR_ARG;
    const int log_n = fri_combine_log_n(n_queries, log_lde, cm, ca, nq);
    if (log_n > 26) return VX_ERR_ARG;
    size_t w = 0;
    const int32_t rc = vx_stark_proof_bound(VX_AIR_FRI_COMBINE, cfg, log_n, &w);
    if (rc != VX_OK) return rc;
    *n_words = VX_FCOMB_HDR + w;
    return VX_OK;
}

int32_t vx_fri_combine_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2],
                             const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0,
                             size_t n_queries, uint64_t* blob_out, size_t blob_cap, size_t* blob_len) {
    if (!ctx || !cfg || !alpha || !zeta || !open_local || !open_next || !open_quot || !index || !rows || !ev0 || !blob_len) return VX_ERR_ARG;
    const FriCombineStmt st{log_lde, cfg->rate_bits, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot};
    VX_TRY(vx_fri_combine_check_dev(ctx, st, index, rows, ev0, n_queries));
    const int log_n = fri_combine_log_n(n_queries, log_lde, cm, ca, nq);
    VX_CHECK(log_n <= 26, "fri combine: %zu queries of %zu rows need more than 2^26 rows", n_queries, cm + ca + nq + (size_t)log_lde);
    TableJob job;
    const vx_chal_hook hook{vx_one_table_hook, nullptr};
    VX_TRY(run_table(ctx, job, VX_AIR_FRI_COMBINE, log_n, COLS, PUB, cfg, &hook, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
        return vx_fri_combine_trace_dev(c, st, TREE0, index, rows, ev0, n_queries, log_n, trace->d, pub);
    }));
    return pack_blob(ctx, "fri combine", VX_FCOMB_MAGIC, {(uint64_t)log_lde, cm, ca, nq, n_queries}, {&job}, blob_out, blob_cap, blob_len);
}

int32_t vx_fri_combine_fold_proof_bound(const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, size_t n_layers, size_t n_queries, size_t* n_words) {
    size_t one = 0;  // (the bounds of the tables alone check the request)
    VX_TRY(vx_fri_combine_proof_bound(cfg, log_lde, cm, ca, nq, n_queries, &one));
    VX_TRY(vx_fri_fold_proof_bound(cfg, log_lde, n_layers, n_queries, &one));
    return vx_tables_proof_bound(cfg, VX_FCFLD_HDR, {{VX_AIR_FRI_COMBINE, fri_combine_log_n(n_queries, log_lde, cm, ca, nq)}, {VX_AIR_FRI_FOLD, fri_fold_log_n(n_queries, log_lde, n_layers)}}, n_words);
}

int32_t vx_fri_combine_fold_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2],
                                  const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly,
                                  size_t final_len, const uint64_t* index, const uint64_t* rows, const uint64_t* leaves, size_t n_queries, uint64_t* blob_out, size_t blob_cap,
                                  size_t* blob_len) {
    if (!ctx || !cfg || !alpha || !zeta || !open_local || !open_next || !open_quot || !betas || !final_poly || !index || !rows || !leaves || !blob_len) return VX_ERR_ARG;
    VX_CHECK(cfg->arity_bits == 4, "fri combine-fold: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    const FriCombineStmt st{log_lde, cfg->rate_bits, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot};
    // ---- the statement, natively: stage 1 the combination (it yields ev_0), stage 2 the fold chains from that ev_0
    VX_CHECK(n_queries >= 1 && n_queries <= MAX_QUERIES, "fri combine-fold: %zu queries (1..2^20)", n_queries);
    std::vector<uint64_t> ev0(2 * n_queries, 0);
    VX_TRY(vx_fri_combine_check_claims(ctx, st, index, rows, ev0.data(), n_queries));
    VX_TRY(vx_fri_combine_host(ctx, st, index, rows, n_queries, ev0.data()));
    VX_TRY(vx_fri_fold_check_dev(ctx, log_lde, betas, n_layers, final_poly, final_len, index, ev0.data(), leaves, n_queries));
    const int log_c = fri_combine_log_n(n_queries, log_lde, cm, ca, nq), log_f = fri_fold_log_n(n_queries, log_lde, n_layers);
    VX_CHECK(log_c <= 26 && log_f <= 26, "fri combine-fold: %zu queries need a table of more than 2^26 rows", n_queries);
    uint64_t stmt[4];
    vx_fri_combine_fold_statement(st, betas, n_layers, final_poly, final_len, index, rows, leaves, n_queries, stmt);
    // two tables on one bus, in transcript order: the combination on a side context and a host thread of its own, the fold here
    TableGroup g(ctx, cfg, "fri combine-fold");
    g.add({"combination", VX_AIR_FRI_COMBINE, log_c, COLS, PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_fri_combine_trace_dev(c, st, TREE0, index, rows, ev0.data(), n_queries, log_c, trace->d, pub));
               vx_fri_combine_public_digest(st, TREE0, stmt, pub);
               return (int32_t)VX_OK;
           }});
    const int fold = g.add({"fold", VX_AIR_FRI_FOLD, log_f, ffa::COLS, ffa::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                VX_TRY(vx_fri_fold_trace_dev(c, log_lde, betas, n_layers, 0, index, ev0.data(), leaves, n_queries, log_f, trace->d, pub));
                                vx_fri_fold_public_digest(log_lde, betas, n_layers, 0, stmt, pub);
                                return (int32_t)VX_OK;
                            }});
    VX_TRY(g.prove(fold));
    return pack_blob(ctx, "fri combine-fold", VX_FCFLD_MAGIC, {(uint64_t)log_lde, cm, ca, nq, n_layers, n_queries}, {&g.job[0], &g.job[1]}, blob_out, blob_cap, blob_len);
}
}  // extern "C"
