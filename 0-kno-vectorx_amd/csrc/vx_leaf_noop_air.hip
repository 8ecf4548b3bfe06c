// Witness of LeafNoopAir (air_leaf_noop.cuh): the openings of leaves that are their own digest, one row per opening.
//   k_leaf_noop_trace  one lane per ROW: the lane reads its opening (tree, index, length, the four zero-padded words -- two 16-byte
//                      loads) and stores its eleven cells; rows behind the openings are zero.  Column-major stores: a wave writes
//                      one run of 64 words of a column, every store is coalesced.  The table is small (one row per opening of a
//                      commitment tree of at most 4 columns) and store-bound; nothing else is tuned
//   k_leaf_noop_aux    one lane per row: ONE extension inversion for the row's three helpers (Montgomery batch over the products
//                      of its denominator pairs) and the row's running-sum increment (vx_bus_close_dev scans it)
// Parity: tests/test_gpu_leaf_noop.py compares trace, auxiliary columns and public inputs with tests/leaf_noop_ref.py.
#include <string.h>

#include "air_leaf_noop.cuh"
#include "glh_poseidon.h"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace lnp;
constexpr int BLOCK = 256;

__global__ __launch_bounds__(BLOCK) void k_leaf_noop_trace(const ulonglong2* __restrict__ rows, const uint64_t* __restrict__ tree_of, const uint64_t* __restrict__ idx,
                                                           const uint64_t* __restrict__ len, size_t n_idx, size_t n, uint64_t* __restrict__ tr) {
    const size_t i = blockIdx.x * (size_t)BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t cell[COLS];
#pragma unroll
    for (int j = 0; j < COLS; ++j) cell[j] = 0;
    if (i < n_idx) {
        const ulonglong2 lo = rows[2 * i], hi = rows[2 * i + 1];
        const uint64_t l = len[i];
        cell[ACT] = 1, cell[TREE] = tree_of[i], cell[IDX] = idx[i];
        cell[W] = lo.x, cell[W + 1] = lo.y, cell[W + 2] = hi.x, cell[W + 3] = hi.y;  // zero behind the length (checked by the host)
#pragma unroll
        for (int j = 0; j < 4; ++j) cell[E + j] = (uint64_t)j < l;
    }
#pragma unroll
    for (int j = 0; j < COLS; ++j) tr[(size_t)j * n + i] = cell[j];
}

__global__ __launch_bounds__(BLOCK) void k_leaf_noop_aux(const uint64_t* __restrict__ tr, uint64_t* __restrict__ aux, size_t n, gl2 beta, gl2 gamma) {
    const size_t i = blockIdx.x * (size_t)BLOCK + threadIdx.x;
    if (i >= n) return;
    auto cell = [&](int j) -> uint64_t { return tr[(size_t)j * n + i]; };
    gl2 h[N_HELP];
#pragma unroll
    for (int e = 0; e < N_HELP; ++e) h[e] = gl2{0, 0};
    if (cell(ACT)) {  // h_e = (m_a D_b + m_b D_a) / (D_a D_b) for the three message pairs, with one inversion
        const bus::Bus<gl2> bus(beta.a, beta.b, gamma.a, gamma.b);
        const uint64_t tree = cell(TREE), idx = cell(IDX);
        uint64_t w[4], e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = cell(W + j), e[j] = cell(E + j);
        gl2 num[N_HELP], den[N_HELP];
        {
            const gl2 dlo = bus.open_of(tree, idx, w[0], w[1], bus::K<0>{}), dhi = bus.open_of(tree, idx, w[2], w[3], bus::K<1>{});
            num[0] = gl2_scale(gl2_add(dlo, dhi), GL_P - 1), den[0] = gl2_mul(dlo, dhi);  // received: multiplicity -ACT
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const gl2 da = bus.row_of(tree, idx, (uint64_t)(2 * k), w[2 * k]), db = bus.row_of(tree, idx, (uint64_t)(2 * k + 1), w[2 * k + 1]);
            num[1 + k] = gl2_add(gl2_scale(db, e[2 * k]), gl2_scale(da, e[2 * k + 1])), den[1 + k] = gl2_mul(da, db);
        }
        gl2_batch_div(num, den, h);
    }
    gl2 sum = h[0];
#pragma unroll
    for (int e = 1; e < N_HELP; ++e) sum = gl2_add(sum, h[e]);
#pragma unroll
    for (int e = 0; e < N_HELP; ++e) aux[(size_t)(2 * e) * n + i] = h[e].a, aux[(size_t)(2 * e + 1) * n + i] = h[e].b;
    aux[(size_t)(2 * N_HELP) * n + i] = sum.a, aux[(size_t)(2 * N_HELP + 1) * n + i] = sum.b;  // the increment; the scan makes it the running sum
}
}  // namespace

void vx_leaf_noop_public(const uint64_t digest[4], uint64_t pub[4]) { memcpy(pub + PUB_DIGEST, digest, 32); }

// ranges of the openings (vx_bus.h): a length outside 1..4, a non-canonical word, a word behind its length that is not zero
int32_t vx_leaf_noop_check(vx_ctx* ctx, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* leaf_len, const uint64_t* rows, size_t n_idx) {
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 26), "leaf noop: %zu openings (1..2^26)", n_idx);
    for (size_t i = 0; i < n_idx; ++i) {
        VX_CHECK(tree_of[i] >> 32 == 0 && leaf_idx[i] >> 40 == 0, "leaf noop: opening %zu names leaf %llu of tree %llu (below 2^40 / 2^32)", i, (unsigned long long)leaf_idx[i],
                 (unsigned long long)tree_of[i]);
        VX_CHECK(leaf_len[i] >= 1 && leaf_len[i] <= (uint64_t)MAX_LEN, "leaf noop: opening %zu has a leaf of %llu words (1..4; a longer row is hashed: LeafSpongeSetAir)", i,
                 (unsigned long long)leaf_len[i]);
        for (size_t j = 0; j < 4; ++j) {
            VX_CHECK(rows[4 * i + j] < glh::P, "leaf noop: opening %zu has a non-canonical word", i);
            VX_CHECK(j < leaf_len[i] || rows[4 * i + j] == 0, "leaf noop: opening %zu has a word behind its length that is not zero", i);
        }
    }
    return VX_OK;
}

// The witness of LeafNoopAir on the device (vx_bus.h).  The openings have passed vx_leaf_noop_check.
int32_t vx_leaf_noop_trace_dev(vx_ctx* ctx, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* leaf_len, const uint64_t* rows, size_t n_idx, int log_n, uint64_t* trace_d) {
    VX_CHECK(log_n >= 5 && log_n <= 26 && n_idx <= ((size_t)1 << log_n), "leaf noop: %zu openings do not fit 2^%d rows", n_idx, log_n);
    const size_t n = (size_t)1 << log_n;
    Scratch sc;
    uint64_t *rows_d, *tree_d, *idx_d, *len_d;
    sc.add(rows_d, 4 * n_idx), sc.add(tree_d, n_idx), sc.add(idx_d, n_idx), sc.add(len_d, n_idx);  // the rows first: read as 16-byte pairs
    sc.alloc(ctx);
    sc.up(rows_d, rows, 4 * n_idx * 8), sc.up(tree_d, tree_of, n_idx * 8), sc.up(idx_d, leaf_idx, n_idx * 8), sc.up(len_d, leaf_len, n_idx * 8);
    if (sc.ok()) {
        hipLaunchKernelGGL(k_leaf_noop_trace, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ctx->stream, (const ulonglong2*)rows_d, tree_d, idx_d, len_d, n_idx, n, trace_d);
        sc.launched();
    }
    return sc.status("leaf noop");
}

int32_t LeafNoopAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t*, uint64_t* aux, uint64_t* aux_pub) {
    const size_t n = (size_t)1 << log_n;
    hipLaunchKernelGGL(k_leaf_noop_aux, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, ctx->stream, trace, aux, n, gl2{chal[0], chal[1]}, gl2{chal[2], chal[3]});
    VX_HIP(hipGetLastError());
    return vx_bus_close_dev(ctx, aux + (size_t)(2 * N_HELP) * n, log_n, aux_pub);
}

extern "C" {
int32_t vx_leaf_noop_air_trace(vx_ctx* ctx, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* leaf_len, const uint64_t* rows, size_t n_idx, int log_n, vx_buf* trace_out,
                               uint64_t public_out[4]) {
    if (!ctx || !tree_of || !leaf_idx || !leaf_len || !rows || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)COLS << log_n), "leaf noop: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, COLS, log_n);
    VX_TRY(vx_leaf_noop_check(ctx, tree_of, leaf_idx, leaf_len, rows, n_idx));
    VX_TRY(vx_leaf_noop_trace_dev(ctx, tree_of, leaf_idx, leaf_len, rows, n_idx, log_n, trace_out->d));
    std::vector<uint64_t> claims;  // (tree, index, length, the four words) of every opening: the claims digest
    claims.reserve(7 * n_idx);
    for (size_t i = 0; i < n_idx; ++i) {
        claims.push_back(tree_of[i]), claims.push_back(leaf_idx[i]), claims.push_back(leaf_len[i]);
        claims.insert(claims.end(), rows + 4 * i, rows + 4 * i + 4);
    }
    uint64_t digest[4];
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_leaf_noop_public(digest, public_out);
    return VX_OK;
}
}  // extern "C"
