// Witness and prover of MerkleOpenAir (air_merkle_open.cuh): a batch of openings of one vx_tree proven in one table.
//   k_merkle_open_trace  one lane per block (path p, level l): the tree in HBM already holds every node of every path, so the
//                        levels of a path are independent -- the lane gathers the node entering its level and the sibling,
//                        orders them by the index bit, walks the 30 rounds (poseidon_air.cuh) and writes its 32 rows
//   k_merkle_open_aux    one lane per block: one extension inversion for the helper of the block's two TAG_OPEN messages, written
//                        to its 32 rows, and the block's running-sum increment on its first row (vx_bus_close_dev scans it)
// The levels above the tree's cap (the table proves paths to ONE root: the two-to-one fold of the cap) are folded here with the
// tree builder's own level kernel.  Parity: tests/test_gpu_merkle_open.py compares trace, auxiliary columns and proof with
// tests/merkle_open_ref.py and the reference prover.
// MerkleOpenSetAir (paths into several trees, the openings table of vx_fri_queries_prove):
//   k_merkle_open_set_trace  as k_merkle_open_trace, one lane per block; the path of a block and the first block of a path are
//                            tables the host precomputes (the paths have different depths), the tree of a path one entry of a small
//                            device table (node storage, the fold of its cap, depth, root): three dependent loads, no search
//   k_merkle_open_set_aux    one lane per block: one extension inversion for both helpers (the opening, the root)
// Parity: tests/test_gpu_fri_queries.py against tests/fri_queries_ref.py.
// The same table from AUTHENTICATION PATHS (vx_merkle_paths_air_trace, the openings table of vx_stark_openings_prove): no tree is in HBM,
// a path is what a proof carries -- the leaf digest and one sibling per level up to the cap -- so its levels are a chain:
//   k_merkle_path_states     16 lanes per path run the tree builder's cooperative permutation (poseidon.cuh) up the path, siblings
//                            below the cap from the proof, above it from the fold of the tree's cap, store the node and the sibling
//                            ENTERING every level and compare the end with the folded root
//   k_merkle_open_set_trace<true>  the same kernel with those stored pairs as its source instead of the tree's node storage
// Parity: tests/test_gpu_stark_openings.py against tests/stark_openings_ref.py.
#include <string.h>

#include "air_merkle_open.cuh"
#include "glh_poseidon.h"
#include "poseidon.cuh"
#include "poseidon_air.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace mop;

struct OpenArgs {
    const uint64_t* levels;  // the tree: level l (n_leaves >> l nodes) at 8 (n_leaves - (n_leaves >> l)), l <= low
    const uint64_t* upper;   // the fold of the cap: its level j (n_cap >> j nodes) at 8 (n_cap - (n_cap >> j)); level 0 = the cap
    const uint64_t* idx;     // [n_idx] leaf indices (< n_leaves: checked by the host)
    size_t n_leaves, n_cap, n_idx, n;
    int depth, low;          // depth = log2(n_leaves) levels per path; levels below `low` = depth - cap_height are read from the tree
    uint64_t* tr;            // [COLS][n]
    uint64_t* claims;        // [n_idx][5]: (index, leaf digest), written by the lane of each path's first level
};

__global__ __launch_bounds__(64) void k_merkle_open_trace(OpenArgs a) {
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= a.n / 32) return;
    uint64_t s[12], shape[COLS - BIT];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 0;
#pragma unroll
    for (int j = 0; j < COLS - BIT; ++j) shape[j] = 0;
    shape[LVL - BIT] = 1;  // an idle block is the zero state at level 1
    if (b < a.n_idx * (size_t)a.depth) {
        const size_t p = b / (size_t)a.depth;
        const int l = (int)(b - p * (size_t)a.depth);
        const uint64_t idx = a.idx[p], node = idx >> l, bit = node & 1;
        const uint64_t* lv = l < a.low ? a.levels + 8 * (a.n_leaves - (a.n_leaves >> l)) : a.upper + 8 * (a.n_cap - (a.n_cap >> (l - a.low)));
        const uint64_t *cur = lv + 4 * node, *sib = lv + 4 * (node ^ 1), *leaf = a.levels + 4 * idx;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t c = gl_canon(cur[i]), sb = gl_canon(sib[i]), lf = gl_canon(leaf[i]);
            s[i] = bit ? sb : c, s[4 + i] = bit ? c : sb;
            shape[SIB - BIT + i] = sb, shape[CUR - BIT + i] = c, shape[LEAF - BIT + i] = lf;
            if (l == 0) a.claims[5 * p + 1 + i] = lf;
        }
        if (l == 0) a.claims[5 * p] = idx;
        shape[BIT - BIT] = bit, shape[R - BIT] = node, shape[LVL - BIT] = (uint64_t)l + 1, shape[ACT - BIT] = 1;
        shape[END - BIT] = l == a.depth - 1, shape[FIRSTB - BIT] = l == 0;
    }
    poseidon_air_walk(s, a.tr, a.n, 32 * b);
    poseidon_air_block_cols(shape, a.tr, a.n, BIT, 32 * b);
}

__global__ __launch_bounds__(64) void k_merkle_open_aux(const uint64_t* __restrict__ tr, uint64_t* __restrict__ aux, size_t n, gl2 beta, gl2 gamma) {
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= n / 32) return;
    const size_t row = 32 * b;
    auto cell = [&](int j) -> uint64_t { return tr[(size_t)j * n + row]; };
    gl2 h{0, 0};
    const uint64_t firstb = cell(FIRSTB);
    if (firstb) {  // h = FIRSTB (1 / D_lo + 1 / D_hi) with one inversion
        const bus::Bus<gl2> bus(beta.a, beta.b, gamma.a, gamma.b);
        const gl2 dlo = bus.open(cell(R), cell(LEAF), cell(LEAF + 1), bus::K<0>{}), dhi = bus.open(cell(R), cell(LEAF + 2), cell(LEAF + 3), bus::K<1>{});
        h = gl2_scale(gl2_mul(gl2_add(dlo, dhi), gl2_inv(gl2_mul(dlo, dhi))), firstb);
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        aux[row + r] = h.a, aux[n + row + r] = h.b;
        aux[2 * n + row + r] = r == 0 ? h.a : 0, aux[3 * n + row + r] = r == 0 ? h.b : 0;  // increments; the scan makes them the running sum
    }
}

// ---- MerkleOpenSetAir
struct SetTree {             // one tree of the set
    const uint64_t* levels;  // as OpenArgs
    const uint64_t* upper;
    const uint64_t* root;    // the last node of `upper`
    size_t n_leaves, n_cap;
    int depth, low;
};
struct OpenSetArgs {
    const SetTree* trees;
    const uint64_t* path;      // [n_idx][3]: tree, leaf index, first block (all checked by the host)
    const uint32_t* blk_path;  // [n_active]: the path of every active block
    size_t n_active, n;
    uint64_t* tr;              // [SET_COLS][n]
    uint64_t* claims;          // [n_idx][6]: (tree, index, leaf digest), written by the lane of each path's first level
    // the second source (PATHS): what k_merkle_path_states stored; SetTree::levels is unused then
    const uint64_t* nodes;     // [n_active][8]: the node and the sibling entering every block
    const uint64_t* leaf;      // [n_idx]: where the 4 words of every path's leaf digest lie (device addresses)
};

template <bool PATHS>
__global__ __launch_bounds__(64) void k_merkle_open_set_trace(OpenSetArgs a) {
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= a.n / 32) return;
    uint64_t s[12], shape[SET_COLS - BIT];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 0;
#pragma unroll
    for (int j = 0; j < SET_COLS - BIT; ++j) shape[j] = 0;
    shape[LVL - BIT] = 1;  // an idle block is the zero state at level 1 (tree 0, root 0, depth 0: nothing reads them)
    if (b < a.n_active) {
        const size_t p = a.blk_path[b];
        const uint64_t* pe = a.path + 3 * p;
        const SetTree t = a.trees[pe[0]];
        const int l = (int)(b - pe[2]);
        const uint64_t idx = pe[1], node = idx >> l, bit = node & 1;
        const uint64_t *cur, *sib, *leaf;
        if constexpr (PATHS) {
            cur = a.nodes + 8 * b, sib = cur + 4, leaf = (const uint64_t*)a.leaf[p];
        } else {
            const uint64_t* lv = l < t.low ? t.levels + 8 * (t.n_leaves - (t.n_leaves >> l)) : t.upper + 8 * (t.n_cap - (t.n_cap >> (l - t.low)));
            cur = lv + 4 * node, sib = lv + 4 * (node ^ 1), leaf = t.levels + 4 * idx;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint64_t c = gl_canon(cur[i]), sb = gl_canon(sib[i]), lf = gl_canon(leaf[i]);
            s[i] = bit ? sb : c, s[4 + i] = bit ? c : sb;
            shape[SIB - BIT + i] = sb, shape[CUR - BIT + i] = c, shape[LEAF - BIT + i] = lf, shape[ROOT - BIT + i] = gl_canon(t.root[i]);
            if (l == 0) a.claims[6 * p + 2 + i] = lf;
        }
        if (l == 0) a.claims[6 * p] = pe[0], a.claims[6 * p + 1] = idx;
        shape[BIT - BIT] = bit, shape[R - BIT] = node, shape[LVL - BIT] = (uint64_t)l + 1, shape[ACT - BIT] = 1;
        shape[END - BIT] = l == t.depth - 1, shape[FIRSTB - BIT] = l == 0;
        shape[TREE - BIT] = pe[0], shape[DEPTH - BIT] = (uint64_t)t.depth;
    }
    poseidon_air_walk(s, a.tr, a.n, 32 * b);
    poseidon_air_block_cols(shape, a.tr, a.n, BIT, 32 * b);
}

// The chain of every path.  Lanes 0..3 of a group hold the node the path has reached; every level the group loads the sibling
// (lanes 0..7, word l & 3), stores the pair, orders it by the index bit and permutes.  Every group of a launch runs max_depth
// levels -- the DPP exchange of the permutation wants whole waves in step -- and a path shorter than that keeps its node from its
// last level on; surplus groups redo the last path and do not write.  (16 lanes per path as in k_leaf_sponge_states, whose
// measurement of the analogous chain -- 6.23 ms one lane per leaf, 2.30 ms cooperative -- this grouping rests on; this kernel
// itself has not been measured against a one-lane form.)
struct PathArgs {
    const SetTree* trees;
    const uint64_t* path;  // [n_idx][3]: tree, leaf index, first block
    const uint64_t* leaf;  // [n_idx]: device addresses of the leaf digests
    const uint64_t* sib;   // [n_idx]: device addresses of the siblings below the cap, 4 words per level
    size_t n_idx;
    int max_depth;
    uint64_t* nodes;            // [n_active][8]
    unsigned long long* bad;    // 1 + the first opening that does not reach its root (~0: none)
};
__global__ __launch_bounds__(256) void k_merkle_path_states(PathArgs a) {
    __shared__ uint64_t lds[16 * 12];
    const int l = threadIdx.x & 15, grp = threadIdx.x >> 4, lane0 = threadIdx.x & 48;
    const size_t t = blockIdx.x * (size_t)16 + grp;
    const bool live = t < a.n_idx;
    const size_t p = live ? t : a.n_idx - 1;
    const uint64_t* pe = a.path + 3 * p;
    const SetTree tr = a.trees[pe[0]];
    const uint64_t idx = pe[1], first = pe[2];
    const uint64_t *leaf = (const uint64_t*)a.leaf[p], *sibs = (const uint64_t*)a.sib[p];
    uint64_t cur = l < 4 ? gl_canon(leaf[l]) : 0;
    for (int lv = 0; lv < a.max_depth; ++lv) {
        const bool on = lv < tr.depth;
        const uint64_t node = idx >> lv, bit = node & 1;
        uint64_t sb = 0;
        if (on && l < 8) {
            const uint64_t* sp = lv < tr.low ? sibs + 4 * lv : tr.upper + 8 * (tr.n_cap - (tr.n_cap >> (lv - tr.low))) + 4 * (node ^ 1);
            sb = gl_canon(sp[l & 3]);
        }
        const uint64_t c = (uint64_t)__shfl((unsigned long long)cur, lane0 | (l & 3), 64);
        if (live && on && l < 8) a.nodes[8 * (first + lv) + l] = l < 4 ? c : sb;
        uint64_t s = 0;
        if (l < 8) s = ((l >= 4) == (bit != 0)) ? c : sb;  // (node, sibling) when the bit is 0, (sibling, node) otherwise
        s = poseidon_permute_coop(s, l, lds + 12 * grp);
        if (on) cur = s;
    }
    if (live && l < 4 && cur != gl_canon(tr.root[l])) atomicMin(a.bad, (unsigned long long)(p + 1));
}

__global__ __launch_bounds__(64) void k_merkle_open_set_aux(const uint64_t* __restrict__ tr, uint64_t* __restrict__ aux, size_t n, gl2 beta, gl2 gamma) {
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= n / 32) return;
    const size_t row = 32 * b;
    auto cell = [&](int j) -> uint64_t { return tr[(size_t)j * n + row]; };
    gl2 h[2] = {gl2{0, 0}, gl2{0, 0}};
    const uint64_t firstb = cell(FIRSTB), end = cell(END);
    if (firstb | end) {  // h = FIRSTB (1 / D_lo + 1 / D_hi) of the opening, h2 = END (...) of the root, with one inversion
        const bus::Bus<gl2> bus(beta.a, beta.b, gamma.a, gamma.b);
        const uint64_t tree = cell(TREE), r = cell(R), depth = cell(DEPTH);
        const gl2 dlo = bus.open_of(tree, r, cell(LEAF), cell(LEAF + 1), bus::K<0>{}), dhi = bus.open_of(tree, r, cell(LEAF + 2), cell(LEAF + 3), bus::K<1>{});
        const gl2 rlo = bus.root(tree, cell(ROOT), cell(ROOT + 1), bus::K<0>{}, depth), rhi = bus.root(tree, cell(ROOT + 2), cell(ROOT + 3), bus::K<1>{}, depth);
        const gl2 num[2] = {gl2_scale(gl2_add(dlo, dhi), firstb), gl2_scale(gl2_add(rlo, rhi), end)}, den[2] = {gl2_mul(dlo, dhi), gl2_mul(rlo, rhi)};
        gl2_batch_div(num, den, h);
    }
    const gl2 sum = gl2_add(h[0], h[1]);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        uint64_t *ca = aux + (size_t)(2 * e) * n + row, *cb = aux + (size_t)(2 * e + 1) * n + row;
        const gl2 v = h[e];
#pragma unroll 8
        for (int r = 0; r < 32; ++r) ca[r] = v.a, cb[r] = v.b;
    }
    uint64_t *za = aux + 4 * n + row, *zb = aux + 5 * n + row;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) za[r] = r == 0 ? sum.a : 0, zb[r] = r == 0 ? sum.b : 0;  // increments; the scan makes them the running sum
}

}  // namespace

int32_t MerkleOpenSetAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    (void)pub;
    const size_t n = (size_t)1 << log_n, blocks = n / 32;
    hipLaunchKernelGGL(k_merkle_open_set_aux, dim3((unsigned)((blocks + 63) / 64)), dim3(64), 0, ctx->stream, trace, aux, n, gl2{chal[0], chal[1]}, gl2{chal[2], chal[3]});
    VX_HIP(hipGetLastError());
    return vx_bus_close_dev(ctx, aux + 4 * n, log_n, aux_pub);
}

// The witness of MerkleOpenSetAir on the device: path i opens leaf leaf_idx[i] of trees[tree_of[i]].  pub_out: the digest of the
// claims (tree, index, leaf digest).
int32_t vx_merkle_open_set_trace_dev(vx_ctx* ctx, const vx_tree* const* trees, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx, int log_n,
                                     uint64_t* trace_d, uint64_t pub_out[4]) {
    VX_CHECK(n_trees >= 1 && n_trees <= VX_OPEN_SET_MAX_TREES, "merkle openings: %zu trees (1..%d)", n_trees, VX_OPEN_SET_MAX_TREES);
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle openings: %zu openings (1..2^21)", n_idx);
    VX_CHECK(log_n >= 5 && log_n <= 26, "merkle openings: 2^%d rows (5 <= log_n <= 26)", log_n);
    const size_t n = (size_t)1 << log_n;
    std::vector<SetTree> tab(n_trees);
    size_t up_words = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        VX_CHECK(trees[t], "merkle openings: tree %zu is missing", t);
        const int depth = ceil_log2(trees[t]->n_leaves);
        VX_CHECK(depth >= 1 && depth <= 40 && trees[t]->cap_height >= 0 && trees[t]->cap_height <= depth, "merkle openings: tree %zu of %zu leaves has no path to prove", t,
                 trees[t]->n_leaves);
        up_words += 4 * (((size_t)2 << trees[t]->cap_height) - 1);
    }
    // the first block of every path, the path of every block
    std::vector<uint64_t> path(3 * n_idx);
    std::vector<uint32_t> blk_path;
    for (size_t i = 0; i < n_idx; ++i) {
        VX_CHECK(tree_of[i] < n_trees, "merkle openings: opening %zu names tree %llu of %zu", i, (unsigned long long)tree_of[i], n_trees);
        const vx_tree* t = trees[tree_of[i]];
        VX_CHECK(leaf_idx[i] < t->n_leaves, "merkle openings: index %zu (%llu) is not a leaf of tree %llu", i, (unsigned long long)leaf_idx[i], (unsigned long long)tree_of[i]);
        path[3 * i] = tree_of[i], path[3 * i + 1] = leaf_idx[i], path[3 * i + 2] = blk_path.size();
        VX_CHECK(blk_path.size() + (size_t)ceil_log2(t->n_leaves) <= n / 32, "merkle openings: the paths do not fit 2^%d rows", log_n);
        blk_path.insert(blk_path.end(), (size_t)ceil_log2(t->n_leaves), (uint32_t)i);
    }
    const size_t n_active = blk_path.size(), w_tab = (n_trees * sizeof(SetTree) + 7) / 8, w_blk = (n_active + 1) / 2;
    // scratch: the folds of the caps, the tree table, the paths, the block map, the claims
    uint64_t* sc = (uint64_t*)vx_pool_alloc(ctx, (up_words + w_tab + 3 * n_idx + w_blk + 6 * n_idx) * 8);
    VX_CHECK(sc, "merkle openings: out of device memory");
    uint64_t *upper = sc, *tab_d = upper + up_words, *path_d = tab_d + w_tab, *blk_d = path_d + 3 * n_idx, *claims_d = blk_d + w_blk;
    std::vector<uint64_t> claims(6 * n_idx);
    int32_t rc = VX_OK;
    do {
        hipError_t e = hipSuccess;
        uint64_t* up = upper;
        for (size_t t = 0; t < n_trees && e == hipSuccess; ++t) {
            const vx_tree* tr = trees[t];
            const size_t n_cap = (size_t)1 << tr->cap_height;
            const int depth = ceil_log2(tr->n_leaves);
            e = hipMemcpyAsync(up, tr->levels + tr->total - 4 * n_cap, 4 * n_cap * 8, hipMemcpyDeviceToDevice, ctx->stream);
            vx_merkle_levels_launch(ctx, up, n_cap, 1);
            tab[t] = SetTree{tr->levels, up, up + 8 * n_cap - 8, tr->n_leaves, n_cap, depth, depth - tr->cap_height};
            up += 4 * (2 * n_cap - 1);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(tab_d, tab.data(), n_trees * sizeof(SetTree), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(path_d, path.data(), path.size() * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(blk_d, blk_path.data(), n_active * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle openings: %s", hipGetErrorString(e));
            break;
        }
        const OpenSetArgs a{(const SetTree*)tab_d, path_d, (const uint32_t*)blk_d, n_active, n, trace_d, claims_d, nullptr, nullptr};
        hipLaunchKernelGGL(k_merkle_open_set_trace<false>, dim3((unsigned)((n / 32 + 63) / 64)), dim3(64), 0, ctx->stream, a);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(claims.data(), claims_d, claims.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle openings: %s", hipGetErrorString(e));
    } while (0);
    vx_pool_free(ctx, sc);
    VX_TRY(rc);
    uint64_t digest[4];
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_merkle_open_set_public(digest, pub_out);
    return VX_OK;
}

// ---- the same witness from authentication paths (vx_bus.h)
int32_t vx_merkle_paths_states_dev(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                                   const uint64_t* leaf_digests, const uint64_t* const* leaf_dev, const uint64_t* siblings, size_t n_idx, MerklePathsWitness* w, size_t* bad_out) {
    VX_CHECK(n_trees >= 1 && n_trees <= VX_OPEN_SET_MAX_TREES, "merkle paths: %zu trees (1..%d)", n_trees, VX_OPEN_SET_MAX_TREES);
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle paths: %zu openings (1..2^21)", n_idx);
    VX_CHECK(cap_height >= 0 && cap_height <= 16, "merkle paths: cap height %d (0..16)", cap_height);
    const size_t n_cap = (size_t)1 << cap_height, up_tree = 4 * (2 * n_cap - 1);
    int max_depth = 0;
    for (size_t t = 0; t < n_trees; ++t)
        VX_CHECK(log_leaves[t] == 0 || (log_leaves[t] >= 1 && log_leaves[t] <= 40 && cap_height <= log_leaves[t]), "merkle paths: tree %zu of 2^%d leaves under a cap of height %d", t,
                 log_leaves[t], cap_height);
    // the first block of every path, the path of every block, where its siblings start
    std::vector<uint64_t> path(3 * n_idx), sib_at(n_idx);
    std::vector<uint32_t> blk_path;
    size_t sib_words = 0;
    for (size_t i = 0; i < n_idx; ++i) {
        VX_CHECK(tree_of[i] < n_trees && log_leaves[tree_of[i]] > 0, "merkle paths: opening %zu names tree %llu, which is not one of the trees", i, (unsigned long long)tree_of[i]);
        const int depth = log_leaves[tree_of[i]];
        VX_CHECK(leaf_idx[i] >> depth == 0, "merkle paths: index %zu (%llu) is not a leaf of tree %llu", i, (unsigned long long)leaf_idx[i], (unsigned long long)tree_of[i]);
        VX_CHECK(blk_path.size() + (size_t)depth <= ((size_t)1 << 21), "merkle paths: the paths have more than 2^21 levels");
        path[3 * i] = tree_of[i], path[3 * i + 1] = leaf_idx[i], path[3 * i + 2] = blk_path.size();
        blk_path.insert(blk_path.end(), (size_t)depth, (uint32_t)i);
        sib_at[i] = sib_words, sib_words += 4 * (size_t)(depth - cap_height);
        if (depth > max_depth) max_depth = depth;
    }
    std::vector<SetTree> tab(n_trees);
    const size_t n_active = blk_path.size(), w_tab = (n_trees * sizeof(SetTree) + 7) / 8, w_blk = (n_active + 1) / 2;
    // scratch: the folds of the caps, the tree table, the paths, the block map, the leaf and sibling addresses, the leaf digests, the
    // siblings, the stored pairs, the claims, the mismatch word
    uint64_t* sc = (uint64_t*)vx_pool_alloc(ctx, (n_trees * up_tree + w_tab + 3 * n_idx + w_blk + 2 * n_idx + 4 * n_idx + sib_words + 8 * n_active + 6 * n_idx + 1) * 8);
    if (!sc) return vx_fail(ctx, VX_ERR_OOM, "merkle paths: out of device memory");
    uint64_t *upper = sc, *tab_d = upper + n_trees * up_tree, *path_d = tab_d + w_tab, *blk_d = path_d + 3 * n_idx, *leaf_d = blk_d + w_blk, *sibp_d = leaf_d + n_idx,
             *dig_d = sibp_d + n_idx, *sib_d = dig_d + 4 * n_idx, *nodes_d = sib_d + sib_words, *claims_d = nodes_d + 8 * n_active, *bad_d = claims_d + 6 * n_idx;
    std::vector<uint64_t> leaf_at(n_idx), sibp(n_idx);
    for (size_t i = 0; i < n_idx; ++i) {
        leaf_at[i] = leaf_dev && leaf_dev[i] ? (uint64_t)(uintptr_t)leaf_dev[i] : (uint64_t)(uintptr_t)(dig_d + 4 * i);
        sibp[i] = (uint64_t)(uintptr_t)(sib_d + sib_at[i]);
    }
    unsigned long long bad = ~0ULL;
    int32_t rc = VX_OK;
    do {
        hipError_t e = hipSuccess;
        for (size_t t = 0; t < n_trees && e == hipSuccess; ++t) {
            uint64_t* up = upper + t * up_tree;
            tab[t] = SetTree{nullptr, up, up + up_tree - 4, (size_t)1 << log_leaves[t], n_cap, log_leaves[t], log_leaves[t] - cap_height};
            if (!log_leaves[t]) continue;
            e = hipMemcpyAsync(up, caps + t * 4 * n_cap, 4 * n_cap * 8, hipMemcpyHostToDevice, ctx->stream);
            vx_merkle_levels_launch(ctx, up, n_cap, 1);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(tab_d, tab.data(), n_trees * sizeof(SetTree), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(path_d, path.data(), path.size() * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(blk_d, blk_path.data(), n_active * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(leaf_d, leaf_at.data(), n_idx * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(sibp_d, sibp.data(), n_idx * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && leaf_digests) e = hipMemcpyAsync(dig_d, leaf_digests, 4 * n_idx * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && !leaf_digests) e = hipMemsetAsync(dig_d, 0, 4 * n_idx * 8, ctx->stream);
        if (e == hipSuccess && sib_words) e = hipMemcpyAsync(sib_d, siblings, sib_words * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(bad_d, &bad, 8, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle paths: %s", hipGetErrorString(e));
            break;
        }
        const PathArgs a{(const SetTree*)tab_d, path_d, leaf_d, sibp_d, n_idx, max_depth, nodes_d, (unsigned long long*)bad_d};
        hipLaunchKernelGGL(k_merkle_path_states, dim3((unsigned)((n_idx + 15) / 16)), dim3(256), 0, ctx->stream, a);  // 16 lanes per path
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, bad_d, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle paths: %s", hipGetErrorString(e));
    } while (0);
    if (rc != VX_OK) {
        vx_pool_free(ctx, sc);
        return rc;
    }
    *w = MerklePathsWitness{sc, tab_d, path_d, nodes_d, leaf_d, (const uint32_t*)blk_d, claims_d, n_idx, n_active};
    *bad_out = bad == ~0ULL ? n_idx : (size_t)(bad - 1);
    if (bad != ~0ULL)
        return vx_fail(ctx, VX_ERR_STATEMENT, "merkle paths: opening %llu (leaf %llu of tree %llu) does not reach the root of its tree", bad - 1, (unsigned long long)leaf_idx[bad - 1],
                       (unsigned long long)tree_of[bad - 1]);
    return VX_OK;
}

int32_t vx_merkle_paths_trace_dev(vx_ctx* ctx, const MerklePathsWitness& w, int log_n, uint64_t* trace_d) {
    VX_CHECK(log_n >= 5 && log_n <= 26 && w.n_active <= ((size_t)1 << log_n) / 32, "merkle paths: %zu levels do not fit 2^%d rows (5 <= log_n <= 26)", w.n_active, log_n);
    const size_t n = (size_t)1 << log_n;
    const OpenSetArgs a{(const SetTree*)w.trees_d, w.path_d, w.blk_d, w.n_active, n, trace_d, w.claims_d, w.nodes_d, w.leaf_d};
    hipLaunchKernelGGL(k_merkle_open_set_trace<true>, dim3((unsigned)((n / 32 + 63) / 64)), dim3(64), 0, ctx->stream, a);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

void vx_merkle_paths_free(vx_ctx* ctx, MerklePathsWitness* w) {
    if (w->sc) vx_pool_free(ctx, w->sc);
    *w = MerklePathsWitness();
}

// MerkleOpenSetAir's public inputs: the digest the table does not constrain (prover and verifier alike: vx_bus.h)
void vx_merkle_open_set_public(const uint64_t digest[4], uint64_t pub[4]) { memcpy(pub, digest, 32); }

int32_t MerkleOpenAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    (void)pub;
    const size_t n = (size_t)1 << log_n, blocks = n / 32;
    hipLaunchKernelGGL(k_merkle_open_aux, dim3((unsigned)((blocks + 63) / 64)), dim3(64), 0, ctx->stream, trace, aux, n, gl2{chal[0], chal[1]}, gl2{chal[2], chal[3]});
    VX_HIP(hipGetLastError());
    return vx_bus_close_dev(ctx, aux + 2 * n, log_n, aux_pub);
}

// root, depth, the digest of the (index, leaf digest) claims: shared with the verifier (vx_verify.hip)
void vx_merkle_open_public(const uint64_t root[4], int depth, const uint64_t* claims, size_t n_idx, uint64_t pub[9]) {
    memcpy(pub, root, 32);
    pub[4] = (uint64_t)depth;
    if (claims) glh::hash_no_pad(claims, 5 * n_idx, pub + 5);
}

int32_t vx_merkle_open_trace_dev(vx_ctx* ctx, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, uint64_t pub_out[9]) {
    const int depth = ceil_log2(tree->n_leaves);
    VX_CHECK(depth >= 1 && depth <= 40, "merkle openings: a tree of %zu leaves has no path to prove", tree->n_leaves);
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle openings: %zu openings (1..2^21)", n_idx);
    VX_CHECK(log_n >= 5 && log_n <= 26 && 32 * n_idx * (size_t)depth <= ((size_t)1 << log_n), "merkle openings: %zu paths of %d levels do not fit 2^%d rows", n_idx, depth, log_n);
    for (size_t i = 0; i < n_idx; ++i) VX_CHECK(leaf_idx[i] < tree->n_leaves, "merkle openings: index %zu (%llu) is not a leaf of the tree", i, (unsigned long long)leaf_idx[i]);
    const size_t n = (size_t)1 << log_n, n_cap = (size_t)1 << tree->cap_height, up_words = 4 * (2 * n_cap - 1);
    // scratch: the fold of the cap, the indices, the claims
    uint64_t* sc = (uint64_t*)vx_pool_alloc(ctx, (up_words + 6 * n_idx) * 8);
    VX_CHECK(sc, "merkle openings: out of device memory");
    uint64_t *upper = sc, *idx_d = sc + up_words, *claims_d = idx_d + n_idx;
    std::vector<uint64_t> claims(5 * n_idx);
    uint64_t root[4];
    int32_t rc = VX_OK;
    do {
        hipError_t e = hipMemcpyAsync(upper, tree->levels + tree->total - 4 * n_cap, 4 * n_cap * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(idx_d, leaf_idx, n_idx * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle openings: %s", hipGetErrorString(e));
            break;
        }
        vx_merkle_levels_launch(ctx, upper, n_cap, 1);
        OpenArgs a{tree->levels, upper, idx_d, tree->n_leaves, n_cap, n_idx, n, depth, depth - tree->cap_height, trace_d, claims_d};
        hipLaunchKernelGGL(k_merkle_open_trace, dim3((unsigned)((n / 32 + 63) / 64)), dim3(64), 0, ctx->stream, a);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(claims.data(), claims_d, claims.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(root, upper + up_words - 4, 32, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle openings: %s", hipGetErrorString(e));
    } while (0);
    vx_pool_free(ctx, sc);
    VX_TRY(rc);
    vx_merkle_open_public(root, depth, claims.data(), n_idx, pub_out);
    return VX_OK;
}

extern "C" {
int32_t vx_merkle_open_air_trace(vx_ctx* ctx, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx, int log_n, vx_buf* trace_out, uint64_t public_out[9]) {
    if (!ctx || !tree || !leaf_idx || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)COLS << log_n), "merkle openings: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, COLS, log_n);
    return vx_merkle_open_trace_dev(ctx, tree, leaf_idx, n_idx, log_n, trace_out->d, public_out);
}

int32_t vx_merkle_open_set_air_trace(vx_ctx* ctx, const vx_tree* const* trees, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx, int log_n,
                                     vx_buf* trace_out, uint64_t public_out[4]) {
    if (!ctx || !trees || !tree_of || !leaf_idx || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)SET_COLS << log_n), "merkle openings: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, SET_COLS, log_n);
    return vx_merkle_open_set_trace_dev(ctx, trees, n_trees, tree_of, leaf_idx, n_idx, log_n, trace_out->d, public_out);
}

int32_t vx_merkle_paths_air_trace(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                                  const uint64_t* leaf_digests, const uint64_t* siblings, size_t n_idx, int log_n, vx_buf* trace_out, uint64_t public_out[4]) {
    if (!ctx || !caps || !log_leaves || !tree_of || !leaf_idx || !leaf_digests || !siblings || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)SET_COLS << log_n), "merkle paths: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, SET_COLS, log_n);
    MerklePathsWitness w;
    size_t bad = 0;
    int32_t rc = vx_merkle_paths_states_dev(ctx, caps, cap_height, log_leaves, n_trees, tree_of, leaf_idx, leaf_digests, nullptr, siblings, n_idx, &w, &bad);
    std::vector<uint64_t> claims(6 * n_idx);
    if (rc == VX_OK) rc = vx_merkle_paths_trace_dev(ctx, w, log_n, trace_out->d);
    if (rc == VX_OK) {
        hipError_t e = hipMemcpyAsync(claims.data(), w.claims_d, claims.size() * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = vx_fail(ctx, VX_ERR_DEVICE, "merkle paths: %s", hipGetErrorString(e));
    }
    vx_merkle_paths_free(ctx, &w);
    VX_TRY(rc);
    uint64_t digest[4];
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_merkle_open_set_public(digest, public_out);
    return VX_OK;
}

int32_t vx_merkle_openings_proof_bound(const vx_stark_config* cfg, size_t n_leaves, size_t n_idx, size_t* n_words) {
    if (!cfg || !n_words || n_leaves < 2 || (n_leaves & (n_leaves - 1)) || n_idx < 1 || n_idx > ((size_t)1 << 21)) return VX_ERR_ARG;
    const int log_n = vx_merkle_open_log_n(n_idx, ceil_log2(n_leaves));
    if (log_n > 26) return VX_ERR_ARG;
    size_t w = 0;
    const int32_t rc = vx_stark_proof_bound(VX_AIR_MERKLE_OPEN, cfg, log_n, &w);
    if (rc != VX_OK) return rc;
    *n_words = VX_MOPEN_HDR + w;
    return VX_OK;
}

int32_t vx_merkle_openings_prove(vx_ctx* ctx, const vx_stark_config* cfg, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx, uint64_t* blob_out, size_t blob_cap,
                                 size_t* blob_len) {
    if (!ctx || !cfg || !tree || !leaf_idx || !blob_len) return VX_ERR_ARG;
    const int depth = ceil_log2(tree->n_leaves);
    VX_CHECK(depth >= 1 && n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle openings: %zu openings of a tree of %zu leaves", n_idx, tree->n_leaves);
    const int log_n = vx_merkle_open_log_n(n_idx, depth);
    VX_CHECK(log_n <= 26, "merkle openings: %zu paths of %d levels need more than 2^26 rows", n_idx, depth);
    TableJob job;
    const vx_chal_hook hook{vx_one_table_hook, nullptr};
    VX_TRY(run_table(ctx, job, VX_AIR_MERKLE_OPEN, log_n, COLS, PUB, cfg, &hook, 0,
                     [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) { return vx_merkle_open_trace_dev(c, tree, leaf_idx, n_idx, log_n, trace->d, pub); }));
    return pack_blob(ctx, "merkle openings", VX_MOPEN_MAGIC, {(uint64_t)depth, n_idx}, {&job}, blob_out, blob_cap, blob_len);
}
}  // extern "C"
