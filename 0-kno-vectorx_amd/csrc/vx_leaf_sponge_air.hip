// Witness and prover of the sponge tables (air_leaf_sponge.cuh): LeafSpongeAir, the opened leaf rows of one tree hashed in one
// table, LeafSpongeSetAir, rows of several trees (the sponge tables of vx_fri_queries_prove and vx_stark_openings_prove), and the
// two-table proof vx_merkle_rows_prove (MerkleOpenAir + LeafSpongeAir on one logUp bus).  One witness (LeafSpongeWitness, vx_bus.h),
// made by sponge_states from any source and read by sponge_trace:
//   k_leaf_sponge_states  the blocks of one leaf are a CHAIN (block k needs the output of block k - 1), and the workload has few
//                         leaves and long chains (84 leaves x 128 permutations at leaf_len 1018): latency-bound.  16 lanes per
//                         leaf run the cooperative permutation of the tree builder (poseidon.cuh), gather the row from its
//                         source, and store the state ENTERING every block, the row (the claims the public inputs digest) and the
//                         digest, which is compared with the tree's leaf digest: the first opening that differs is reported
//   k_leaf_sponge_trace   one lane per block: the blocks are independent once their entering states exist -- the lane writes
//                         the shape columns and walks the 30 rounds (poseidon_air.cuh) over its 32 rows; SET: with the TREE column
// The auxiliary columns of both tables are bus_aux.cuh's, from the AIRs' own message list: one lane per block.
// The sources of the states kernel: one tree's leaf data in any of the three vx_merkle_build layouts; the leaves of FRI layers -- 16
// extension values at natural positions bitrev(16 j + t), what vx_fri_layer_tree hashes -- with a per-leaf entry (tree, layer
// values, the tree's leaf digests, log2 of its leaves); and the rows themselves, handed over one per opening (their rows come out of
// a proof: no tree exists to compare a digest with -- the path the digest enters is the check); any leaf length, one per table.
// Parity: tests/test_gpu_leaf_sponge.py compares trace, auxiliary columns and both proofs with tests/leaf_sponge_ref.py and the
// reference prover.
#include <string.h>

#include "air_leaf_sponge.cuh"
#include "air_merkle_open.cuh"
#include "bus_aux.cuh"
#include "glh_poseidon.h"
#include "poseidon.cuh"
#include "poseidon_air.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace lsp;

constexpr int LAYOUT_FRI_LAYER = 3;  // behind the three vx_merkle_build layouts: the leaves of FRI layers, one entry per leaf
constexpr int LAYOUT_ROWS = 4;       // ... and rows handed over directly, one entry per leaf: `data` is the row itself
struct SetLeaf {
    const uint64_t* data;         // the layer: 2^(log_leaves + 4) extension values (a, b) in natural order; LAYOUT_ROWS: the row
    const uint64_t* tree_leaves;  // its tree's leaf digests, or nullptr
    uint64_t tree;
    int log_leaves;
};

struct SpongeArgs {
    const uint64_t* data;         // the leaves, as vx_merkle_build reads them
    const uint64_t* idx;          // [n_idx] leaf indices (< n_leaves: checked by the host)
    const uint64_t* tree_leaves;  // the tree's leaf digests [n_leaves][4], or nullptr (the witness alone: nothing to compare with)
    size_t n_leaves, leaf_len, n_idx, n_blk;  // n_blk = ceil(leaf_len / 8) blocks per leaf
    int log_leaves;
    uint64_t* states;   // [n_idx n_blk][12]: the state entering every block
    uint64_t* claims;   // [n_idx][1 + leaf_len]: (index, row)
    uint64_t* digests;  // [n_idx][4]
    unsigned long long* bad;  // LeafSpongeWitness::bad_d
    const SetLeaf* set;  // LAYOUT_FRI_LAYER / LAYOUT_ROWS: [n_idx]; data, tree_leaves, n_leaves, log_leaves above are unused, leaf_len is 32 / the rows'
};

// (Tried: one lane per leaf with the tree builder's poseidon_permute -- 6.23 ms against 2.30 ms for 84 leaves x 128 blocks,
// profiles/README.md "LeafSpongeAir": 84 chains cannot fill the chip, so the shorter chain per permutation wins.)
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_leaf_sponge_states(SpongeArgs a) {
    __shared__ uint64_t lds[16 * 12];
    const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const size_t t = blockIdx.x * (size_t)16 + grp;
    const bool live = t < a.n_idx;
    const size_t p = live ? t : a.n_idx - 1;  // surplus groups redo the last leaf and do not write
    const uint64_t j = a.idx[p];
    constexpr bool FRI = LAYOUT == LAYOUT_FRI_LAYER, ROWS = LAYOUT == LAYOUT_ROWS;
    constexpr size_t CLAIM_HDR = FRI || ROWS ? 2 : 1;  // the set's claims name the tree: (tree, index, row)
    int log_leaves = a.log_leaves;
    const uint64_t *data = a.data, *tree_leaves = a.tree_leaves;
    uint64_t* claim = a.claims + p * (a.leaf_len + CLAIM_HDR);
    if constexpr (FRI || ROWS) {
        const SetLeaf sl = a.set[p];
        log_leaves = sl.log_leaves, data = sl.data, tree_leaves = sl.tree_leaves;
        if (live && l == 0) claim[0] = sl.tree;
    }
    const size_t r = ROWS ? 0 : (LAYOUT == VX_LEAVES_COLS_BITREV || FRI) ? brev32((uint32_t)j, log_leaves) : j;
    const size_t estride = LAYOUT == VX_LEAVES_ROW_MAJOR || ROWS ? 1 : a.n_leaves;
    const uint64_t* src = ROWS ? data : LAYOUT == VX_LEAVES_ROW_MAJOR ? data + r * a.leaf_len : FRI ? data + 2 * r : data + r;
    if (live && l == 0) claim[CLAIM_HDR - 1] = j;
    uint64_t s = 0;
    for (size_t k = 0; k < a.n_blk; ++k) {
        const size_t e = 8 * k + l;
        if (l < 8 && e < a.leaf_len) {  // overwrite mode: a word behind the tail keeps the previous output
            if constexpr (FRI) s = gl_canon(src[((size_t)brev32((uint32_t)(e >> 1), 4) << (log_leaves + 1)) + (e & 1)]);  // word e: half e & 1 of value e / 2
            else s = gl_canon(src[e * estride]);
            if (live) claim[CLAIM_HDR + e] = s;
        }
        if (live && l < 12) a.states[(p * a.n_blk + k) * 12 + l] = s;
        s = poseidon_permute_coop(s, l, lds + 12 * grp);
    }
    if (live && l < 4) {
        a.digests[4 * p + l] = s;
        if (tree_leaves && gl_canon(tree_leaves[4 * j + l]) != s) atomicMin(a.bad, (unsigned long long)(p + 1));
    }
}

template <bool SET>  // SET: LeafSpongeSetAir, the leaf's tree from `set`
__global__ __launch_bounds__(64) void k_leaf_sponge_trace(const uint64_t* __restrict__ states, const uint64_t* __restrict__ idx, size_t n_idx, size_t n_blk, size_t n,
                                                          uint64_t* __restrict__ tr, const SetLeaf* __restrict__ set) {
    constexpr int NC = SET ? SET_COLS : COLS;
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= n / 32) return;
    uint64_t s[12], shape[NC - MSG];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 0;
#pragma unroll
    for (int j = 0; j < NC - MSG; ++j) shape[j] = 0;
    if (b < n_idx * n_blk) {
        const size_t p = b / n_blk, k = b - p * n_blk;
#pragma unroll
        for (int i = 0; i < 12; ++i) s[i] = states[12 * b + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) shape[i] = s[i];
        shape[IDX - MSG] = idx[p], shape[POS - MSG] = k, shape[ACT - MSG] = 1;
        shape[FIRSTB - MSG] = k == 0, shape[LASTB - MSG] = k + 1 == n_blk, shape[NXL - MSG] = k + 2 == n_blk;
        if constexpr (SET) shape[TREE - MSG] = set[p].tree;
    }
    poseidon_air_walk(s, tr, n, 32 * b);
#pragma unroll
    for (int i = 0; i < 4; ++i) shape[DIG - MSG + i] = s[i];
    poseidon_air_block_cols(shape, tr, n, MSG, 32 * b);
}

constexpr size_t MAX_LEAF_LEN = (size_t)1 << 20;

// where the rows of a witness come from: what SpongeArgs distinguishes
struct SpongeSource {
    int layout;  // a vx_merkle_build layout: the data of one tree; LAYOUT_FRI_LAYER, LAYOUT_ROWS: one `set` entry per opening
    size_t leaf_len;
    const uint64_t *data = nullptr, *tree_leaves = nullptr;  // one tree (SpongeArgs)
    size_t n_leaves = 0;
    int log_leaves = 0;
    const SetLeaf* set = nullptr;    // [n_idx]
    const uint64_t* rows = nullptr;  // LAYOUT_ROWS: [n_idx][leaf_len] on the host; uploaded here, and the entries go up with `data` = their row
};

// The states of every opening's chain, enqueued on ctx->stream.  The requests' ranges are the caller's to check.
int32_t sponge_states(vx_ctx* ctx, const SpongeSource& src, const uint64_t* leaf_idx, size_t n_idx, LeafSpongeWitness* w) {
    const size_t leaf_len = src.leaf_len, n_blk = sponge_blocks(leaf_len), w_set = src.set ? n_idx * sizeof(SetLeaf) / 8 : 0;
    static_assert(sizeof(SetLeaf) % 8 == 0, "SetLeaf is a whole number of words");
    Scratch& sc = w->sc;
    sc.add(w->states_d, 12 * n_idx * n_blk), sc.add(w->idx_d, n_idx), sc.add(w->claims_d, n_idx * (leaf_len + (src.set ? 2 : 1))), sc.add(w->digests_d, 4 * n_idx), sc.add(w->bad_d, 1);
    sc.add(w->set_d, w_set), sc.add(w->rows_d, src.rows ? n_idx * leaf_len : 0);
    sc.alloc(ctx);
    VX_TRY(sc.status("leaf sponge"));
    w->n_idx = n_idx, w->n_blk = n_blk, w->leaf_len = leaf_len;
    sc.up(w->idx_d, leaf_idx, n_idx * 8), sc.fill(w->bad_d, 0xff, 8);
    const SetLeaf* set = src.set;
    std::vector<SetLeaf> row_set;
    if (src.rows) {
        row_set.assign(set, set + n_idx);
        for (size_t i = 0; i < n_idx; ++i) row_set[i].data = w->rows_d + i * leaf_len;
        set = row_set.data();
        sc.up(w->rows_d, src.rows, n_idx * leaf_len * 8);
    }
    if (set) sc.up(w->set_d, set, w_set * 8);
    if (src.rows) sc.sync();  // (`row_set` is pageable host memory of this frame)
    if (sc.ok()) {
        const SpongeArgs a{src.data,    w->idx_d,    src.tree_leaves, src.n_leaves, leaf_len, n_idx, n_blk, src.log_leaves,
                           w->states_d, w->claims_d, w->digests_d, (unsigned long long*)w->bad_d, (const SetLeaf*)w->set_d};
        const dim3 grid((unsigned)((n_idx + 15) / 16)), block(256);  // 16 lanes per leaf
        if (src.layout == VX_LEAVES_ROW_MAJOR) hipLaunchKernelGGL(k_leaf_sponge_states<VX_LEAVES_ROW_MAJOR>, grid, block, 0, ctx->stream, a);
        else if (src.layout == VX_LEAVES_COLS_BITREV) hipLaunchKernelGGL(k_leaf_sponge_states<VX_LEAVES_COLS_BITREV>, grid, block, 0, ctx->stream, a);
        else if (src.layout == VX_LEAVES_COLS) hipLaunchKernelGGL(k_leaf_sponge_states<VX_LEAVES_COLS>, grid, block, 0, ctx->stream, a);
        else if (src.layout == LAYOUT_FRI_LAYER) hipLaunchKernelGGL(k_leaf_sponge_states<LAYOUT_FRI_LAYER>, grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_leaf_sponge_states<LAYOUT_ROWS>, grid, block, 0, ctx->stream, a);
        sc.launched();
    }
    return sc.status("leaf sponge");
}

// the trace kernel over a witness, on any context of the device
template <bool SET>
int32_t sponge_trace(vx_ctx* ctx, const LeafSpongeWitness& w, int log_n, uint64_t* trace_d) {
    VX_CHECK(log_n >= 5 && log_n <= 26 && 32 * w.n_idx * w.n_blk <= ((size_t)1 << log_n), "leaf sponge: %zu leaves of %zu blocks do not fit 2^%d rows", w.n_idx, w.n_blk, log_n);
    const size_t n = (size_t)1 << log_n;
    hipLaunchKernelGGL(k_leaf_sponge_trace<SET>, dim3((unsigned)((n / 32 + 63) / 64)), dim3(64), 0, ctx->stream, w.states_d, w.idx_d, w.n_idx, w.n_blk, n, trace_d, (const SetLeaf*)w.set_d);
    VX_HIP(hipGetLastError());
    return VX_OK;
}

// A table made in one go: states, trace, then the claims and the mismatch word back -- the one wait.  *bad: the first opening that
// does not hash to its tree's leaf digest, n_idx when all do (the caller words the refusal).
template <bool SET>
int32_t sponge_table(vx_ctx* ctx, const SpongeSource& src, const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, std::vector<uint64_t>* claims, size_t* bad) {
    LeafSpongeWitness w;
    VX_TRY(sponge_states(ctx, src, leaf_idx, n_idx, &w));
    VX_TRY(sponge_trace<SET>(ctx, w, log_n, trace_d));
    claims->resize(n_idx * (src.leaf_len + (SET ? 2 : 1)));
    uint64_t word = 0;
    w.sc.down(claims->data(), w.claims_d, claims->size() * 8), w.sc.down(&word, w.bad_d, 8), w.sc.sync();
    VX_TRY(w.sc.status("leaf sponge"));
    *bad = word == ~0ULL ? n_idx : (size_t)(word - 1);
    return VX_OK;
}

}  // namespace

int32_t LeafSpongeAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<LeafSpongeAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}
int32_t LeafSpongeSetAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<LeafSpongeSetAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

// L, B, the tail flags, the digest of the (index, row) claims: shared with the verifier (vx_verify.hip)
void vx_leaf_sponge_public(size_t leaf_len, const uint64_t* claims, size_t n_idx, uint64_t pub[14]) {
    const size_t t = leaf_len % 8;
    pub[PUB_L] = leaf_len, pub[PUB_B] = sponge_blocks(leaf_len);
    for (size_t i = 0; i < 8; ++i) pub[PUB_W + i] = i < (t ? t : 8);
    glh::hash_no_pad(claims, n_idx * (leaf_len + 1), pub + PUB_DIGEST);
}

// LeafSpongeSetAir's public inputs: L, B, the tail flags, a digest the table does not constrain (prover and verifier alike: vx_bus.h)
void vx_leaf_sponge_set_public(size_t leaf_len, const uint64_t digest[4], uint64_t pub[14]) {
    const size_t t = leaf_len % 8;
    pub[PUB_L] = leaf_len, pub[PUB_B] = sponge_blocks(leaf_len);
    for (size_t i = 0; i < 8; ++i) pub[PUB_W + i] = i < (t ? t : 8);
    memcpy(pub + PUB_DIGEST, digest, 32);
}

// The witness of LeafSpongeSetAir on the device for leaves of FRI layers (vx_bus.h): leaf i is leaf leaf_idx[i] of layer
// tree_of[i].  pub_out: L = 32, B = 4, the tail flags, the digest of the claims (tree, index, row).
int32_t vx_leaf_sponge_set_trace_dev(vx_ctx* ctx, const uint64_t* const* evals_d, const int* log_leaves, const uint64_t* const* tree_leaves, size_t n_trees, const uint64_t* tree_of,
                                     const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, uint64_t pub_out[PUB]) {
    constexpr size_t leaf_len = 32, n_blk = 4;
    VX_CHECK(n_trees >= 1 && n_trees <= VX_OPEN_SET_MAX_TREES, "leaf sponge: %zu trees (1..%d)", n_trees, VX_OPEN_SET_MAX_TREES);
    for (size_t t = 0; t < n_trees; ++t) VX_CHECK(evals_d[t] && log_leaves[t] >= 0 && log_leaves[t] <= 26, "leaf sponge: layer %zu of 2^%d leaves (0..26)", t, log_leaves[t]);
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 19), "leaf sponge: %zu openings (1..2^19)", n_idx);
    VX_CHECK(log_n >= 5 && log_n <= 26 && 32 * n_idx * n_blk <= ((size_t)1 << log_n), "leaf sponge: %zu leaves of %zu blocks do not fit 2^%d rows", n_idx, n_blk, log_n);
    std::vector<SetLeaf> set(n_idx);
    for (size_t i = 0; i < n_idx; ++i) {
        VX_CHECK(tree_of[i] < n_trees, "leaf sponge: opening %zu names tree %llu of %zu", i, (unsigned long long)tree_of[i], n_trees);
        const size_t t = tree_of[i];
        VX_CHECK(leaf_idx[i] >> log_leaves[t] == 0, "leaf sponge: index %zu (%llu) is not a leaf of tree %zu", i, (unsigned long long)leaf_idx[i], t);
        set[i] = SetLeaf{evals_d[t], tree_leaves ? tree_leaves[t] : nullptr, tree_of[i], log_leaves[t]};
    }
    SpongeSource src{LAYOUT_FRI_LAYER, leaf_len};
    src.set = set.data();
    std::vector<uint64_t> claims;
    size_t bad = 0;
    VX_TRY(sponge_table<true>(ctx, src, leaf_idx, n_idx, log_n, trace_d, &claims, &bad));
    if (bad < n_idx)
        return vx_fail(ctx, VX_ERR_STATEMENT, "leaf sponge: opening %llu (leaf %llu of tree %llu) does not hash to the tree's leaf digest -- the layer is not what the tree was built from",
                       (unsigned long long)bad, (unsigned long long)leaf_idx[bad], (unsigned long long)tree_of[bad]);
    uint64_t digest[4];
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_leaf_sponge_set_public(leaf_len, digest, pub_out);
    return VX_OK;
}

// ---- the witness of LeafSpongeSetAir from rows handed over directly (vx_bus.h)
int32_t vx_leaf_sponge_rows_states_dev(vx_ctx* ctx, size_t leaf_len, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* rows, size_t n_idx, LeafSpongeWitness* w) {
    VX_CHECK(leaf_len >= 5 && leaf_len <= MAX_LEAF_LEN, "leaf sponge: leaf_len %zu (5..2^20; a row of at most 4 words is its own digest and has no sponge)", leaf_len);
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "leaf sponge: %zu openings (1..2^21)", n_idx);
    const size_t n_blk = sponge_blocks(leaf_len);
    VX_CHECK(n_idx * n_blk <= ((size_t)1 << 21), "leaf sponge: %zu leaves of %zu blocks need more than 2^26 rows", n_idx, n_blk);
    for (size_t i = 0; i < n_idx; ++i)
        VX_CHECK(tree_of[i] >> 32 == 0 && leaf_idx[i] >> 40 == 0, "leaf sponge: opening %zu names leaf %llu of tree %llu (below 2^40 / 2^32)", i, (unsigned long long)leaf_idx[i],
                 (unsigned long long)tree_of[i]);
    for (size_t i = 0; i < n_idx * leaf_len; ++i) VX_CHECK(rows[i] < glh::P, "leaf sponge: opening %zu has a non-canonical word", i / leaf_len);
    std::vector<SetLeaf> set(n_idx);
    for (size_t i = 0; i < n_idx; ++i) set[i] = SetLeaf{nullptr, nullptr, tree_of[i], 0};
    SpongeSource src{LAYOUT_ROWS, leaf_len};
    src.set = set.data(), src.rows = rows;
    return sponge_states(ctx, src, leaf_idx, n_idx, w);
}

int32_t vx_leaf_sponge_rows_trace_dev(vx_ctx* ctx, const LeafSpongeWitness& w, int log_n, uint64_t* trace_d) { return sponge_trace<true>(ctx, w, log_n, trace_d); }

// The witness of LeafSpongeAir on the device.  data_d: the leaves of the whole tree ([n_leaves x leaf_len] words in `layout`; the
// caller has checked that the buffer holds them).  tree_leaves (device, may be nullptr): the leaf digests of the tree the openings
// are proven against -- a row that does not hash to its leaf digest is refused with VX_ERR_STATEMENT before anything is proven.
static int32_t leaf_sponge_trace_dev(vx_ctx* ctx, const uint64_t* data_d, size_t n_leaves, size_t leaf_len, int layout, const uint64_t* tree_leaves, const uint64_t* leaf_idx,
                                     size_t n_idx, int log_n, uint64_t* trace_d, uint64_t pub_out[PUB]) {
    const int log_leaves = ceil_log2(n_leaves);
    VX_CHECK(n_leaves >= 1 && ((size_t)1 << log_leaves) == n_leaves && log_leaves <= 32, "leaf sponge: %zu leaves (a power of two, at most 2^32)", n_leaves);
    VX_CHECK(layout >= 0 && layout <= 2, "leaf sponge: bad layout %d", layout);
    VX_CHECK(leaf_len >= 5 && leaf_len <= MAX_LEAF_LEN, "leaf sponge: leaf_len %zu (5..2^20; a row of at most 4 words is its own digest and has no sponge)", leaf_len);
    VX_CHECK(n_idx >= 1 && n_idx <= ((size_t)1 << 21), "leaf sponge: %zu openings (1..2^21)", n_idx);
    const size_t n_blk = sponge_blocks(leaf_len);
    VX_CHECK(log_n >= 5 && log_n <= 26 && 32 * n_idx * n_blk <= ((size_t)1 << log_n), "leaf sponge: %zu leaves of %zu blocks do not fit 2^%d rows", n_idx, n_blk, log_n);
    for (size_t i = 0; i < n_idx; ++i) VX_CHECK(leaf_idx[i] < n_leaves, "leaf sponge: index %zu (%llu) is not a leaf of the tree", i, (unsigned long long)leaf_idx[i]);
    SpongeSource src{layout, leaf_len, data_d, tree_leaves, n_leaves, log_leaves};
    std::vector<uint64_t> claims;
    size_t bad = 0;
    VX_TRY(sponge_table<false>(ctx, src, leaf_idx, n_idx, log_n, trace_d, &claims, &bad));
    if (bad < n_idx)
        return vx_fail(ctx, VX_ERR_STATEMENT, "merkle rows: opening %llu (leaf %llu) does not hash to the tree's leaf digest -- the leaf data is not what the tree was built from",
                       (unsigned long long)bad, (unsigned long long)leaf_idx[bad]);
    vx_leaf_sponge_public(leaf_len, claims.data(), n_idx, pub_out);
    return VX_OK;
}

extern "C" {
int32_t vx_leaf_sponge_air_trace(vx_ctx* ctx, const vx_buf* data, size_t off, size_t n_leaves, size_t leaf_len, int layout, const uint64_t* leaf_idx, size_t n_idx, int log_n,
                                 vx_buf* trace_out, uint64_t public_out[14]) {
    if (!ctx || !data || !leaf_idx || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(leaf_len >= 5 && leaf_len <= MAX_LEAF_LEN && n_leaves <= ((size_t)1 << 32) && off <= data->n && n_leaves * leaf_len <= data->n - off,
             "leaf sponge: %zu leaves x %zu words (leaf_len 5..2^20) exceed the buffer", n_leaves, leaf_len);
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)COLS << log_n), "leaf sponge: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, COLS, log_n);
    return leaf_sponge_trace_dev(ctx, data->d + off, n_leaves, leaf_len, layout, nullptr, leaf_idx, n_idx, log_n, trace_out->d, public_out);
}

int32_t vx_leaf_sponge_set_air_trace(vx_ctx* ctx, const vx_buf* const* evals, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx,
                                     int log_n, vx_buf* trace_out, uint64_t public_out[14]) {
    if (!ctx || !evals || !log_leaves || !tree_of || !leaf_idx || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(n_trees >= 1 && n_trees <= VX_OPEN_SET_MAX_TREES, "leaf sponge: %zu trees (1..%d)", n_trees, VX_OPEN_SET_MAX_TREES);
    const uint64_t* ev[VX_OPEN_SET_MAX_TREES];
    for (size_t t = 0; t < n_trees; ++t) {
        VX_CHECK(evals[t] && log_leaves[t] >= 0 && log_leaves[t] <= 26 && evals[t]->n >= ((size_t)32 << log_leaves[t]), "leaf sponge: layer %zu does not hold 2^%d leaves of 32 words", t,
                 log_leaves[t]);
        ev[t] = evals[t]->d;
    }
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)SET_COLS << log_n), "leaf sponge: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, SET_COLS, log_n);
    return vx_leaf_sponge_set_trace_dev(ctx, ev, log_leaves, nullptr, n_trees, tree_of, leaf_idx, n_idx, log_n, trace_out->d, public_out);
}

int32_t vx_leaf_sponge_rows_air_trace(vx_ctx* ctx, size_t leaf_len, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* rows, size_t n_idx, int log_n, vx_buf* trace_out,
                                      uint64_t public_out[14]) {
    if (!ctx || !tree_of || !leaf_idx || !rows || !trace_out || !public_out) return VX_ERR_ARG;
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)SET_COLS << log_n), "leaf sponge: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, SET_COLS, log_n);
    LeafSpongeWitness w;
    VX_TRY(vx_leaf_sponge_rows_states_dev(ctx, leaf_len, tree_of, leaf_idx, rows, n_idx, &w));
    VX_TRY(vx_leaf_sponge_rows_trace_dev(ctx, w, log_n, trace_out->d));
    w.sc.sync();
    VX_TRY(w.sc.status("leaf sponge"));
    std::vector<uint64_t> claims;  // (tree, index, row) of every opening: the set's claims digest
    claims.reserve(n_idx * (leaf_len + 2));
    for (size_t i = 0; i < n_idx; ++i) {
        claims.push_back(tree_of[i]), claims.push_back(leaf_idx[i]);
        claims.insert(claims.end(), rows + i * leaf_len, rows + (i + 1) * leaf_len);
    }
    uint64_t digest[4];
    glh::hash_no_pad(claims.data(), claims.size(), digest);
    vx_leaf_sponge_set_public(leaf_len, digest, public_out);
    return VX_OK;
}

int32_t vx_merkle_rows_proof_bound(const vx_stark_config* cfg, size_t n_leaves, size_t leaf_len, size_t n_idx, size_t* n_words) {
    if (!cfg || !n_words || n_leaves < 2 || (n_leaves & (n_leaves - 1)) || n_idx < 1 || n_idx > ((size_t)1 << 21) || leaf_len < 5 || leaf_len > MAX_LEAF_LEN) return VX_ERR_ARG;
    const int log_open = vx_merkle_open_log_n(n_idx, ceil_log2(n_leaves)), log_sponge = leaf_sponge_log_n(n_idx, leaf_len);
    if (log_open > 26 || log_sponge > 26) return VX_ERR_ARG;
    return vx_tables_proof_bound(cfg, VX_MROWS_HDR, {{VX_AIR_MERKLE_OPEN, log_open}, {VX_AIR_LEAF_SPONGE, log_sponge}}, n_words);
}

int32_t vx_merkle_rows_prove(vx_ctx* ctx, const vx_stark_config* cfg, const vx_tree* tree, const vx_buf* data, size_t off, size_t leaf_len, int layout, const uint64_t* leaf_idx,
                             size_t n_idx, uint64_t* blob_out, size_t blob_cap, size_t* blob_len) {
    if (!ctx || !cfg || !tree || !data || !leaf_idx || !blob_len) return VX_ERR_ARG;
    const size_t n_leaves = tree->n_leaves;
    const int depth = ceil_log2(n_leaves);
    VX_CHECK(depth >= 1 && depth <= 32 && n_idx >= 1 && n_idx <= ((size_t)1 << 21), "merkle rows: %zu openings of a tree of %zu leaves", n_idx, n_leaves);
    VX_CHECK(leaf_len >= 5 && leaf_len <= MAX_LEAF_LEN, "merkle rows: leaf_len %zu (5..2^20; a row of at most 4 words is its own digest: vx_merkle_openings_prove covers it)", leaf_len);
    VX_CHECK(layout >= 0 && layout <= 2, "merkle rows: bad layout %d", layout);
    VX_CHECK(off <= data->n && n_leaves * leaf_len <= data->n - off, "merkle rows: %zu leaves x %zu words exceed the buffer", n_leaves, leaf_len);
    for (size_t i = 0; i < n_idx; ++i) VX_CHECK(leaf_idx[i] < n_leaves, "merkle rows: index %zu (%llu) is not a leaf of the tree", i, (unsigned long long)leaf_idx[i]);
    const int log_open = vx_merkle_open_log_n(n_idx, depth), log_sponge = leaf_sponge_log_n(n_idx, leaf_len);
    VX_CHECK(log_open <= 26 && log_sponge <= 26, "merkle rows: %zu openings of %zu words in a tree of depth %d need more than 2^26 rows", n_idx, leaf_len, depth);
    // two tables on one bus, in transcript order: the openings (a side context, its own host thread), the sponge (this context)
    TableGroup g(ctx, cfg, "merkle rows");
    g.add({"openings", VX_AIR_MERKLE_OPEN, log_open, mop::COLS, mop::PUB, 0,
           [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) { return vx_merkle_open_trace_dev(c, tree, leaf_idx, n_idx, log_open, trace->d, pub); }});
    const int sponge = g.add({"sponge", VX_AIR_LEAF_SPONGE, log_sponge, COLS, PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                  return leaf_sponge_trace_dev(c, data->d + off, n_leaves, leaf_len, layout, tree->levels, leaf_idx, n_idx, log_sponge, trace->d, pub);
                              }});
    // the tree and the leaf data are the work of this context's stream; the openings table reads the tree from another one
    VX_HIP(vx_wait(ctx));
    VX_TRY(g.prove(sponge));
    return pack_blob(ctx, "merkle rows", VX_MROWS_MAGIC, {(uint64_t)depth, leaf_len, n_idx}, {&g.job[0], &g.job[1]}, blob_out, blob_cap, blob_len);
}
}  // extern "C"
