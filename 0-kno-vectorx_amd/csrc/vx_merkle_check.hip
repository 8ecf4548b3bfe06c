// Merkle openings CHECKED on the device (vx_merkle_check, include/vx.h): what glh::merkle_path_ok does for one opening on the host --
// hash_or_noop of the leaf row, two_to_one up the path, the cap entry compared -- for a whole batch in one launch.  No witness is
// built and no level is stored (k_leaf_sponge_states and k_merkle_path_states do that for the AIR tables): the one word the kernel
// writes is the first opening that fails.  The verifiers that end here are in vx_verify.hip (the _dev forms).
#include <stdio.h>

#include <algorithm>

#include "poseidon.cuh"
#include "vx_bus.h"
#include "vx_internal.h"

namespace {
// One opening, as the kernel reads it: where its words lie in the staged arrays (word offsets) and which claim of the caller it is.
struct CheckClaim {
    uint64_t index, leaf, sib, cap, id;
    uint32_t leaf_len, n_sib;
};
struct CheckArgs {
    const CheckClaim* claims;  // [n], ordered so that the openings of one tree are adjacent
    const uint64_t *leaves, *sibs, *caps;
    size_t n;
    unsigned long long* bad;  // 1 + the smallest id whose opening misses its cap (~0: none)
};

// A group of 16 lanes per opening, 16 groups per block.  The group absorbs the row as hash_or_noop does -- a row of at most 4 words is
// its own zero-padded digest, a longer one takes one overwrite-mode permutation per 8 words, a word behind the tail keeps the previous
// output -- and walks the path: lanes 0..3 hold the node, lanes 0..7 load the sibling, the pair is ordered by the index bit.  The DPP
// exchange of poseidon_permute_coop wants whole waves in step: the four groups of a wave all run the steps of the longest of them
// (openings of one tree are adjacent, so mostly their own), a shorter chain keeps its state and idles.  Surplus groups of the last
// block redo the last opening and do not write.  Words are canonical: the callers have checked.
__global__ __launch_bounds__(256) void k_merkle_check(CheckArgs a) {
    __shared__ uint64_t lds[16 * 12];
    const int l = threadIdx.x & 15, grp = threadIdx.x >> 4, lane0 = threadIdx.x & 48;
    const size_t t = blockIdx.x * (size_t)16 + grp;
    const bool live = t < a.n;
    const CheckClaim c = a.claims[live ? t : a.n - 1];
    const uint64_t *leaf = a.leaves + c.leaf, *sibs = a.sibs + c.sib;
    const int n_blk = c.leaf_len > 4 ? (int)((c.leaf_len + 7) / 8) : 0, n_sib = (int)c.n_sib;
    int w_blk = n_blk, w_sib = n_sib;
    for (int o = 16; o < 64; o <<= 1) {
        w_blk = max(w_blk, __shfl_xor(w_blk, o, 64));
        w_sib = max(w_sib, __shfl_xor(w_sib, o, 64));
    }
    uint64_t s = 0;
    if (n_blk == 0 && l < (int)c.leaf_len) s = leaf[l];
    for (int k = 0; k < w_blk; ++k) {
        const bool on = k < n_blk;
        const size_t e = 8 * (size_t)k + l;
        uint64_t in = s;
        if (on && l < 8 && e < c.leaf_len) in = leaf[e];
        const uint64_t out = poseidon_permute_coop(in, l, lds + 12 * grp);
        if (on) s = out;
    }
    uint64_t cur = s;
    for (int lv = 0; lv < w_sib; ++lv) {
        const bool on = lv < n_sib;
        const uint64_t bit = (c.index >> lv) & 1;
        uint64_t sb = 0;
        if (on && l < 8) sb = sibs[4 * lv + (l & 3)];
        const uint64_t node = (uint64_t)__shfl((unsigned long long)cur, lane0 | (l & 3), 64);
        uint64_t in = 0;
        if (l < 8) in = ((l >= 4) == (bit != 0)) ? node : sb;  // (node, sibling) when the bit is 0, (sibling, node) otherwise
        const uint64_t out = poseidon_permute_coop(in, l, lds + 12 * grp);
        if (on) cur = out;
    }
    if (live && l < 4 && cur != a.caps[c.cap + 4 * (c.index >> n_sib) + l]) atomicMin(a.bad, (unsigned long long)(c.id + 1));
}
}  // namespace

extern "C" int32_t vx_merkle_check(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                                   const uint64_t* leaf_len, const uint64_t* leaves, size_t leaves_len, const uint64_t* siblings, size_t siblings_len, size_t n_claims,
                                   size_t* first_bad) {
    if (!ctx || !first_bad) return VX_ERR_ARG;
    *first_bad = SIZE_MAX;
    if (n_claims == 0) {
        VX_CHECK(leaves_len == 0 && siblings_len == 0, "merkle check: no claim, but %zu leaf words and %zu sibling words", leaves_len, siblings_len);
        return VX_OK;
    }
    VX_CHECK(caps && log_leaves && tree_of && leaf_idx && leaf_len && (leaves || !leaves_len) && (siblings || !siblings_len), "merkle check: a null argument");
    VX_CHECK(cap_height >= 0 && cap_height <= 16 && n_trees >= 1 && n_trees <= ((size_t)1 << 16) && n_claims <= ((size_t)1 << 24), "merkle check: cap height %d (0..16), %zu trees (1..2^16), %zu claims (at most 2^24)",
             cap_height, n_trees, n_claims);
    const size_t cap_words = (size_t)4 << cap_height;
    for (size_t t = 0; t < n_trees; ++t)
        VX_CHECK(log_leaves[t] >= cap_height && log_leaves[t] <= 40, "merkle check: tree %zu of 2^%d leaves under a cap of height %d", t, log_leaves[t], cap_height);
    std::vector<CheckClaim> cl(n_claims);
    size_t leaf_at = 0, sib_at = 0;
    for (size_t i = 0; i < n_claims; ++i) {
        const uint64_t t = tree_of[i];
        VX_CHECK(t < n_trees, "merkle check: claim %zu names tree %llu of %zu", i, (unsigned long long)t, n_trees);
        VX_CHECK(leaf_idx[i] >> log_leaves[t] == 0, "merkle check: claim %zu names leaf %llu, outside tree %llu", i, (unsigned long long)leaf_idx[i], (unsigned long long)t);
        const size_t n_sib = (size_t)(log_leaves[t] - cap_height);
        VX_CHECK(leaf_len[i] >> 31 == 0, "merkle check: claim %zu has a leaf of %llu words", i, (unsigned long long)leaf_len[i]);
        VX_CHECK(leaf_len[i] >= 1 && leaf_len[i] <= leaves_len - leaf_at && 4 * n_sib <= siblings_len - sib_at, "merkle check: the leaf or sibling words end before claim %zu does", i);
        cl[i] = CheckClaim{leaf_idx[i], leaf_at, sib_at, t * cap_words, i, (uint32_t)leaf_len[i], (uint32_t)n_sib};
        leaf_at += leaf_len[i], sib_at += 4 * n_sib;
    }
    VX_CHECK(leaf_at == leaves_len && sib_at == siblings_len, "merkle check: %zu leaf words and %zu sibling words, the claims have %zu and %zu", leaves_len, siblings_len, leaf_at, sib_at);
    for (size_t i = 0; i < n_trees * cap_words; ++i) VX_CHECK(caps[i] < glh::P, "merkle check: non-canonical cap word %zu", i);
    for (size_t i = 0; i < leaves_len; ++i) VX_CHECK(leaves[i] < glh::P, "merkle check: non-canonical leaf word %zu", i);
    for (size_t i = 0; i < siblings_len; ++i) VX_CHECK(siblings[i] < glh::P, "merkle check: non-canonical sibling word %zu", i);
    // the openings of one tree share leaf length and depth: adjacent, the groups of a wave run the same steps
    std::stable_sort(cl.begin(), cl.end(), [](const CheckClaim& x, const CheckClaim& y) { return x.cap < y.cap; });
    static_assert(sizeof(CheckClaim) % 8 == 0, "claims are staged as words");
    Scratch sc;
    uint64_t *claims_d, *leaves_d, *sibs_d, *caps_d, *bad_d;
    sc.add(claims_d, n_claims * (sizeof(CheckClaim) / 8)), sc.add(leaves_d, leaves_len), sc.add(sibs_d, siblings_len), sc.add(caps_d, n_trees * cap_words), sc.add(bad_d, 1);
    sc.alloc(ctx);
    VX_TRY(sc.status("merkle check"));
    sc.up(claims_d, cl.data(), n_claims * sizeof(CheckClaim)), sc.up(leaves_d, leaves, leaves_len * 8), sc.up(caps_d, caps, n_trees * cap_words * 8);
    if (siblings_len) sc.up(sibs_d, siblings, siblings_len * 8);
    sc.fill(bad_d, 0xFF, 8);
    if (sc.ok()) {
        const CheckArgs a{(const CheckClaim*)claims_d, leaves_d, sibs_d, caps_d, n_claims, (unsigned long long*)bad_d};
        hipLaunchKernelGGL(k_merkle_check, dim3((unsigned)((n_claims + 15) / 16)), dim3(256), 0, ctx->stream, a);
        sc.launched();
    }
    unsigned long long bad = ~0ULL;
    sc.down(&bad, bad_d, 8), sc.sync();  // the caller's arrays may go once this returns
    VX_TRY(sc.status("merkle check"));
    if (bad == ~0ULL) return VX_OK;
    *first_bad = (size_t)(bad - 1);
    return vx_fail(ctx, VX_ERR_STATEMENT, "merkle check: claim %zu does not reach the cap of its tree", *first_bad);
}

// the path checker of the _dev verifiers (vx_bus.h): the batch in one launch on `ctx`
PathChecker vx_merkle_check_paths(vx_ctx* ctx) {
    return [ctx](const MerkleBatch& b, size_t* first_bad, char* err, size_t errlen) -> int32_t {
        const int32_t rc = vx_merkle_check(ctx, b.caps.data(), b.cap_height, b.log_leaves.data(), b.log_leaves.size(), b.tree_of.data(), b.leaf_idx.data(), b.leaf_len.data(),
                                           b.leaves.data(), b.leaves.size(), b.siblings.data(), b.siblings.size(), b.tree_of.size(), first_bad);
        if (rc == VX_OK || rc == VX_ERR_STATEMENT) return VX_OK;
        if (err && errlen) snprintf(err, errlen, "%s", vx_last_error(ctx));
        return rc;
    };
}
