// Witness and prover of the openings tables (air_merkle_open.cuh): MerkleOpenAir, a batch of openings of one vx_tree proven in one
// table, and MerkleOpenSetAir, paths into several trees (the openings table of vx_fri_queries_prove and vx_stark_openings_prove).
// One witness (MerkleOpenWitness, vx_bus.h) for three sources, all stated as one OpenRequest:
//   open_layout                  checks a request and lays out the first block of every path and the path of every block
//   open_witness                 folds the caps -- the tables prove paths to ONE root per tree: the two-to-one fold of its cap -- with
//                                the tree builder's own level kernel and uploads the tables
//   k_merkle_open_trace<SET, PATHS>  one lane per block (path p, level l): the lane gathers the node entering its level and the
//                                sibling, orders them by the index bit, walks the 30 rounds (poseidon_air.cuh) and writes its 32
//                                rows.  The path of a block and the first block of a path are the host's tables (the paths have
//                                different depths), the tree of a path one entry of a small device table (node storage, the fold of
//                                its cap, depth, root): three dependent loads, no search.  MerkleOpenAir (SET = false) is the set
//                                of one tree without the trailing TREE, ROOT and DEPTH columns: root and depth are public inputs
// The auxiliary columns of both tables are bus_aux.cuh's, from the AIRs' own message list: one lane per block, one helper for the
// opening and, in the set, one for the root.
// The sources: one tree or several trees in HBM (PATHS = false) -- the node storage already holds every node of every path, so the
// levels of a path are independent -- and AUTHENTICATION PATHS (vx_merkle_paths_air_trace, PATHS = true): no tree is in HBM, a path is
// what a proof carries -- the leaf digest and one sibling per level up to the cap -- so its levels are a chain:
//   k_merkle_path_states         16 lanes per path run the tree builder's cooperative permutation (poseidon.cuh) up the path, siblings
//                                below the cap from the proof, above it from the fold of the tree's cap, store the node and the sibling
//                                ENTERING every level and compare the end with the folded root
// Parity: tests/test_gpu_merkle_open.py compares trace, auxiliary columns and proof with tests/merkle_open_ref.py and the reference
// prover, tests/test_gpu_fri_queries.py with tests/fri_queries_ref.py, tests/test_gpu_stark_openings.py with tests/stark_openings_ref.py.
#include <string.h>

#include "air_merkle_open.cuh"
#include "bus_aux.cuh"
#include "glh_poseidon.h"
#include "poseidon.cuh"
#include "poseidon_air.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace mop;

struct SetTree {             // one tree of the request on the device
    const uint64_t* levels;  // the tree: level l (n_leaves >> l nodes) at 8 (n_leaves - (n_leaves >> l)), l <= low; nullptr without node storage
    const uint64_t* upper;   // the fold of the cap: its level j (n_cap >> j nodes) at 8 (n_cap - (n_cap >> j)); level 0 = the cap
    const uint64_t* root;    // the last node of `upper`
    size_t n_leaves, n_cap;
    int depth, low;          // depth = log2(n_leaves) levels per path; levels below `low` = depth - cap_height are read from the tree
};
struct OpenArgs {
    const SetTree* trees;
    const uint64_t* path;      // [n_idx][3]: tree, leaf index, first block (all checked by the host)
    const uint32_t* blk_path;  // [n_active]: the path of every active block
    size_t n_active, n;
    uint64_t* tr;              // [SET ? SET_COLS : COLS][n]
    uint64_t* claims;          // SET: [n_idx][6] = (tree, index, leaf digest), else [n_idx][5] = (index, leaf digest); written by the lane of each path's first level
    // PATHS: what k_merkle_path_states stored; SetTree::levels is unused then
    const uint64_t* nodes;     // [n_active][8]: the node and the sibling entering every block
    const uint64_t* leaf;      // [n_idx]: where the 4 words of every path's leaf digest lie (device addresses)
};

template <bool SET, bool PATHS>
__global__ __launch_bounds__(64) void k_merkle_open_trace(OpenArgs a) {
    constexpr int NC = SET ? SET_COLS : COLS, CL = SET ? 6 : 5;
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= a.n / 32) return;
    uint64_t s[12], shape[NC - BIT];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 0;
#pragma unroll
    for (int j = 0; j < NC - BIT; ++j) shape[j] = 0;
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
            shape[SIB - BIT + i] = sb, shape[CUR - BIT + i] = c, shape[LEAF - BIT + i] = lf;
            if constexpr (SET) shape[ROOT - BIT + i] = gl_canon(t.root[i]);
            if (l == 0) a.claims[CL * p + CL - 4 + i] = lf;
        }
        if (l == 0) a.claims[CL * p + CL - 5] = idx;
        shape[BIT - BIT] = bit, shape[R - BIT] = node, shape[LVL - BIT] = (uint64_t)l + 1, shape[ACT - BIT] = 1;
        shape[END - BIT] = l == t.depth - 1, shape[FIRSTB - BIT] = l == 0;
        if constexpr (SET) {
            shape[TREE - BIT] = pe[0], shape[DEPTH - BIT] = (uint64_t)t.depth;
            if (l == 0) a.claims[CL * p] = pe[0];
        }
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

// ---- a request, as every source states it
struct OpenTree {
    int depth = 0;                     // log2 of its leaves; 0: no such tree (the tree ids of a proof have gaps)
    int cap_height = 0;
    const uint64_t* cap = nullptr;     // its 4 << cap_height words: the end of a vx_tree's node storage, or host words
    bool cap_on_device = false;
    const uint64_t* levels = nullptr;  // the node storage of a vx_tree, or nullptr: the pairs come from paths
};
struct OpenRequest {
    const char* what;  // the prefix of every message
    const OpenTree* trees;
    size_t n_trees;
    const uint64_t* tree_of;  // [n_idx], or nullptr: every opening is of tree 0
    const uint64_t* leaf_idx;
    size_t n_idx;
    int log_n;  // the rows of the table the paths must fit, or 0: no table yet, at most 2^21 levels in all
};
struct OpenLayout {
    std::vector<uint64_t> path;      // [n_idx][3]: tree, leaf index, first block
    std::vector<uint32_t> blk_path;  // the path of every block
    std::vector<uint64_t> sib_at;    // [n_idx]: where the siblings of a path below its cap start, 4 words per level
    size_t sib_words = 0;
    int max_depth = 0;
};
OpenTree open_tree(const vx_tree* t) { return OpenTree{ceil_log2(t->n_leaves), t->cap_height, t->levels + t->total - ((size_t)4 << t->cap_height), true, t->levels}; }

// checks a request and lays it out (host-pure)
int32_t open_layout(vx_ctx* ctx, const OpenRequest& rq, OpenLayout* lo) {
    VX_CHECK(rq.n_idx >= 1 && rq.n_idx <= ((size_t)1 << 21), "%s: %zu openings (1..2^21)", rq.what, rq.n_idx);
    for (size_t t = 0; t < rq.n_trees; ++t) {
        const OpenTree& tr = rq.trees[t];
        VX_CHECK(tr.depth == 0 || (tr.depth >= 1 && tr.depth <= 40 && tr.cap_height >= 0 && tr.cap_height <= tr.depth), "%s: tree %zu of 2^%d leaves under a cap of height %d", rq.what, t,
                 tr.depth, tr.cap_height);
    }
    const size_t max_blocks = (size_t)1 << (rq.log_n ? rq.log_n - 5 : 21);
    lo->path.resize(3 * rq.n_idx), lo->sib_at.resize(rq.n_idx);
    for (size_t i = 0; i < rq.n_idx; ++i) {
        const uint64_t t = rq.tree_of ? rq.tree_of[i] : 0, idx = rq.leaf_idx[i];
        VX_CHECK(t < rq.n_trees, "%s: opening %zu names tree %llu of %zu", rq.what, i, (unsigned long long)t, rq.n_trees);
        VX_CHECK(rq.trees[t].depth > 0, "%s: opening %zu names tree %llu, which is not one of the trees", rq.what, i, (unsigned long long)t);
        const int depth = rq.trees[t].depth;
        if (rq.tree_of) VX_CHECK(idx >> depth == 0, "%s: index %zu (%llu) is not a leaf of tree %llu", rq.what, i, (unsigned long long)idx, (unsigned long long)t);
        else VX_CHECK(idx >> depth == 0, "%s: index %zu (%llu) is not a leaf of the tree", rq.what, i, (unsigned long long)idx);
        if (lo->blk_path.size() + (size_t)depth > max_blocks)
            return rq.log_n ? vx_fail(ctx, VX_ERR_ARG, "%s: the paths do not fit 2^%d rows", rq.what, rq.log_n) : vx_fail(ctx, VX_ERR_ARG, "%s: the paths have more than 2^21 levels", rq.what);
        lo->path[3 * i] = t, lo->path[3 * i + 1] = idx, lo->path[3 * i + 2] = lo->blk_path.size();
        lo->blk_path.insert(lo->blk_path.end(), (size_t)depth, (uint32_t)i);
        lo->sib_at[i] = lo->sib_words, lo->sib_words += 4 * (size_t)(depth - rq.trees[t].cap_height);
        if (depth > lo->max_depth) lo->max_depth = depth;
    }
    return VX_OK;
}

struct PathSource {  // what the paths of a proof add to a request (vx_bus.h)
    const uint64_t* leaf_digests;
    const uint64_t* const* leaf_dev;
    const uint64_t* siblings;
};

// The witness of a request on ctx->stream: folds the caps, uploads the tables.  With `ps` it then walks every path, waits -- side
// contexts read the buffers -- and reports the first opening that misses its root; without, nothing is waited for.
int32_t open_witness(vx_ctx* ctx, const OpenRequest& rq, const PathSource* ps, MerkleOpenWitness* w, size_t* bad_out) {
    OpenLayout lo;
    VX_TRY(open_layout(ctx, rq, &lo));
    const size_t n_idx = rq.n_idx, n_active = lo.blk_path.size();
    size_t up_words = 0;
    for (size_t t = 0; t < rq.n_trees; ++t) up_words += rq.trees[t].depth ? ((size_t)8 << rq.trees[t].cap_height) - 4 : 0;
    Scratch& sc = w->sc;
    sc.add(w->upper_d, up_words);
    // what the host makes lies together and goes up in one copy
    sc.add(w->trees_d, (rq.n_trees * sizeof(SetTree) + 7) / 8), sc.add(w->path_d, 3 * n_idx), sc.add(w->blk_d, (n_active + 1) / 2);
    if (ps) sc.add(w->leaf_d, n_idx), sc.add(w->sibp_d, n_idx), sc.add(w->bad_d, 1);
    w->tables.assign(sc.words - up_words, 0);
    sc.add(w->claims_d, 6 * n_idx);
    if (ps) sc.add(w->dig_d, 4 * n_idx), sc.add(w->sib_d, lo.sib_words), sc.add(w->nodes_d, 8 * n_active);
    sc.alloc(ctx);
    VX_TRY(sc.status(rq.what));
    w->n_idx = n_idx, w->n_active = n_active;
    auto host = [&](uint64_t* d) { return w->tables.data() + (d - w->trees_d); };
    std::vector<SetTree> tab(rq.n_trees, SetTree{});
    uint64_t* up = w->upper_d;
    for (size_t t = 0; t < rq.n_trees; ++t) {
        const OpenTree& tr = rq.trees[t];
        if (!tr.depth) continue;
        const size_t n_cap = (size_t)1 << tr.cap_height;
        sc.copy(up, tr.cap, 4 * n_cap * 8, tr.cap_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
        vx_merkle_levels_launch(ctx, up, n_cap, 1);
        tab[t] = SetTree{tr.levels, up, up + 8 * n_cap - 8, (size_t)1 << tr.depth, n_cap, tr.depth, tr.depth - tr.cap_height};
        up += 8 * n_cap - 4;
    }
    memcpy(host(w->trees_d), tab.data(), rq.n_trees * sizeof(SetTree));
    memcpy(host(w->path_d), lo.path.data(), 3 * n_idx * 8);
    memcpy(host(w->blk_d), lo.blk_path.data(), n_active * 4);
    if (ps) {
        for (size_t i = 0; i < n_idx; ++i) {
            host(w->leaf_d)[i] = (uint64_t)(uintptr_t)(ps->leaf_dev && ps->leaf_dev[i] ? ps->leaf_dev[i] : w->dig_d + 4 * i);
            host(w->sibp_d)[i] = (uint64_t)(uintptr_t)(w->sib_d + lo.sib_at[i]);
        }
        *host(w->bad_d) = ~0ULL;
    }
    sc.up(w->trees_d, w->tables.data(), w->tables.size() * 8);
    if (!ps) return sc.status(rq.what);
    if (ps->leaf_digests) sc.up(w->dig_d, ps->leaf_digests, 4 * n_idx * 8);
    else sc.fill(w->dig_d, 0, 4 * n_idx * 8);
    if (lo.sib_words) sc.up(w->sib_d, ps->siblings, lo.sib_words * 8);
    if (sc.ok()) {
        const PathArgs a{(const SetTree*)w->trees_d, w->path_d, w->leaf_d, w->sibp_d, n_idx, lo.max_depth, w->nodes_d, (unsigned long long*)w->bad_d};
        hipLaunchKernelGGL(k_merkle_path_states, dim3((unsigned)((n_idx + 15) / 16)), dim3(256), 0, ctx->stream, a);  // 16 lanes per path
        sc.launched();
    }
    unsigned long long bad = ~0ULL;
    sc.down(&bad, w->bad_d, 8), sc.sync();
    VX_TRY(sc.status(rq.what));
    *bad_out = bad == ~0ULL ? n_idx : (size_t)(bad - 1);
    if (bad != ~0ULL)
        return vx_fail(ctx, VX_ERR_STATEMENT, "%s: opening %llu (leaf %llu of tree %llu) does not reach the root of its tree", rq.what, bad - 1, (unsigned long long)rq.leaf_idx[bad - 1],
                       (unsigned long long)(rq.tree_of ? rq.tree_of[bad - 1] : 0));
    return VX_OK;
}

// the trace kernel over a witness, on any context of the device
template <bool SET>
int32_t open_trace(vx_ctx* ctx, const MerkleOpenWitness& w, const char* what, int log_n, uint64_t* trace_d) {
    VX_CHECK(log_n >= 5 && log_n <= 26 && w.n_active <= ((size_t)1 << log_n) / 32, "%s: %zu levels do not fit 2^%d rows (5 <= log_n <= 26)", what, w.n_active, log_n);
    const size_t n = (size_t)1 << log_n;
    const OpenArgs a{(const SetTree*)w.trees_d, w.path_d, (const uint32_t*)w.blk_d, w.n_active, n, trace_d, w.claims_d, w.nodes_d, w.leaf_d};
    const dim3 grid((unsigned)((n / 32 + 63) / 64)), block(64);
    if (!SET) hipLaunchKernelGGL((k_merkle_open_trace<false, false>), grid, block, 0, ctx->stream, a);
    else if (w.nodes_d) hipLaunchKernelGGL((k_merkle_open_trace<true, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_merkle_open_trace<true, false>), grid, block, 0, ctx->stream, a);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// The tail of a table made alone: the claims back -- here the one-shot forms wait --, their digest, the public inputs.  `single`: the
// tree of MerkleOpenAir, whose root and depth are public inputs.
int32_t open_public(vx_ctx* ctx, MerkleOpenWitness& w, const char* what, const OpenTree* single, uint64_t* pub_out) {
    std::vector<uint64_t> claims((single ? 5 : 6) * w.n_idx);
    uint64_t root[4], digest[4];
    w.sc.down(claims.data(), w.claims_d, claims.size() * 8);
    if (single) w.sc.down(root, w.upper_d + ((size_t)8 << single->cap_height) - 8, 32);
    w.sc.sync();
    VX_TRY(w.sc.status(what));
    if (single) {
        vx_merkle_open_public(root, single->depth, claims.data(), w.n_idx, pub_out);
        return VX_OK;
    }
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_merkle_open_set_public(digest, pub_out);
    return VX_OK;
}

// a table of trees in HBM, made alone: witness, trace, public inputs
template <bool SET>
int32_t open_trees_trace(vx_ctx* ctx, const OpenTree* trees, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, uint64_t* pub_out) {
    VX_CHECK(log_n >= 5 && log_n <= 26, "merkle openings: 2^%d rows (5 <= log_n <= 26)", log_n);
    const OpenRequest rq{"merkle openings", trees, n_trees, tree_of, leaf_idx, n_idx, log_n};
    MerkleOpenWitness w;
    VX_TRY(open_witness(ctx, rq, nullptr, &w, nullptr));
    VX_TRY(open_trace<SET>(ctx, w, rq.what, log_n, trace_d));
    return open_public(ctx, w, rq.what, SET ? nullptr : trees, pub_out);
}

}  // namespace

int32_t MerkleOpenSetAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<MerkleOpenSetAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

// MerkleOpenSetAir's public inputs: the digest the table does not constrain (prover and verifier alike: vx_bus.h)
void vx_merkle_open_set_public(const uint64_t digest[4], uint64_t pub[4]) { memcpy(pub, digest, 32); }

int32_t MerkleOpenAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<MerkleOpenAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

// root, depth, the digest of the (index, leaf digest) claims: shared with the verifier (vx_verify.hip)
void vx_merkle_open_public(const uint64_t root[4], int depth, const uint64_t* claims, size_t n_idx, uint64_t pub[9]) {
    memcpy(pub, root, 32);
    pub[4] = (uint64_t)depth;
    if (claims) glh::hash_no_pad(claims, 5 * n_idx, pub + 5);
}

// The witness of MerkleOpenSetAir on the device: path i opens leaf leaf_idx[i] of trees[tree_of[i]].  pub_out: the digest of the
// claims (tree, index, leaf digest).
int32_t vx_merkle_open_set_trace_dev(vx_ctx* ctx, const vx_tree* const* trees, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx, int log_n,
                                     uint64_t* trace_d, uint64_t pub_out[4]) {
    VX_CHECK(n_trees >= 1 && n_trees <= VX_OPEN_SET_MAX_TREES, "merkle openings: %zu trees (1..%d)", n_trees, VX_OPEN_SET_MAX_TREES);
    OpenTree ot[VX_OPEN_SET_MAX_TREES];
    for (size_t t = 0; t < n_trees; ++t) {
        VX_CHECK(trees[t], "merkle openings: tree %zu is missing", t);
        VX_CHECK(trees[t]->n_leaves > 1, "merkle openings: tree %zu of %zu leaves has no path to prove", t, trees[t]->n_leaves);
        ot[t] = open_tree(trees[t]);
    }
    return open_trees_trace<true>(ctx, ot, n_trees, tree_of, leaf_idx, n_idx, log_n, trace_d, pub_out);
}

// ... of MerkleOpenAir: the set of the one tree.  pub_out: root, depth, the digest of the claims (index, leaf digest).
int32_t vx_merkle_open_trace_dev(vx_ctx* ctx, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, uint64_t pub_out[9]) {
    VX_CHECK(tree->n_leaves > 1, "merkle openings: a tree of %zu leaves has no path to prove", tree->n_leaves);
    const OpenTree ot = open_tree(tree);
    return open_trees_trace<false>(ctx, &ot, 1, nullptr, leaf_idx, n_idx, log_n, trace_d, pub_out);
}

// ---- the same witness from authentication paths (vx_bus.h)
int32_t vx_merkle_paths_states_dev(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                                   const uint64_t* leaf_digests, const uint64_t* const* leaf_dev, const uint64_t* siblings, size_t n_idx, MerkleOpenWitness* w, size_t* bad_out) {
    VX_CHECK(n_trees >= 1 && n_trees <= VX_OPEN_SET_MAX_TREES, "merkle paths: %zu trees (1..%d)", n_trees, VX_OPEN_SET_MAX_TREES);
    VX_CHECK(cap_height >= 0 && cap_height <= 16, "merkle paths: cap height %d (0..16)", cap_height);
    OpenTree ot[VX_OPEN_SET_MAX_TREES];
    for (size_t t = 0; t < n_trees; ++t) ot[t] = OpenTree{log_leaves[t], cap_height, caps + t * ((size_t)4 << cap_height), false, nullptr};
    const PathSource ps{leaf_digests, leaf_dev, siblings};
    return open_witness(ctx, OpenRequest{"merkle paths", ot, n_trees, tree_of, leaf_idx, n_idx, 0}, &ps, w, bad_out);
}

int32_t vx_merkle_paths_trace_dev(vx_ctx* ctx, const MerkleOpenWitness& w, int log_n, uint64_t* trace_d) { return open_trace<true>(ctx, w, "merkle paths", log_n, trace_d); }

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
    MerkleOpenWitness w;
    size_t bad = 0;
    VX_TRY(vx_merkle_paths_states_dev(ctx, caps, cap_height, log_leaves, n_trees, tree_of, leaf_idx, leaf_digests, nullptr, siblings, n_idx, &w, &bad));
    VX_TRY(vx_merkle_paths_trace_dev(ctx, w, log_n, trace_out->d));
    return open_public(ctx, w, "merkle paths", nullptr, public_out);
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
