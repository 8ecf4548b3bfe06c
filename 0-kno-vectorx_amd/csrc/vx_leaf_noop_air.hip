// Witness of LeafNoopAir (air_leaf_noop.cuh): the openings of leaves that are their own digest, one row per opening.
//   k_leaf_noop_trace  one lane per ROW: the lane reads its opening (tree, index, length, the four zero-padded words -- two 16-byte
//                      loads) and stores its eleven cells; rows behind the openings are zero.  Column-major stores: a wave writes
//                      one run of 64 words of a column, every store is coalesced.  The table is small (one row per opening of a
//                      commitment tree of at most 4 columns) and store-bound; nothing else is tuned
// The auxiliary columns are bus_aux.cuh's, from the AIR's own message list: one lane per row.
// Parity: tests/test_gpu_leaf_noop.py compares trace, auxiliary columns and public inputs with tests/leaf_noop_ref.py.
#include <string.h>

#include "air_leaf_noop.cuh"
#include "bus_aux.cuh"
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

int32_t LeafNoopAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<LeafNoopAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
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
