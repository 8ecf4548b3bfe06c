// vx_stark_openings_prove: the Merkle side of one inner vx_stark_prove proof on ONE logUp bus, sourced from the proof itself -- per
// query the opened rows, the FRI leaves and every sibling up to the cap are all in it, so no vx_tree and no LDE is needed (an
// aggregator holds proof bytes, not trees).  The openings table (MerkleOpenSetAir: one path per (query, tree), tree ids as in
// vx_bus.h) and one LeafSpongeSetAir table per leaf length above 4 among {cm, ca, 2 2^a}, in that bus order (vx_table_shapes.h);
// TAG_OPEN closes between them for every tree whose rows are hashed.  What is left for the party outside -- the verifier,
// vx_stark_openings_verify in vx_verify.hip -- is the root and depth every path ended in (TAG_ROOT), every word of the hashed
// rows (TAG_ROW) and the opening of a row that is its own digest (TAG_OPEN).  The claims come from the verifier's own query phase in
// its delegated mode (vx_stark_openings_claims); the four digest words of every table are the STATEMENT digest (vx_bus.h).
// No kernels here: the witnesses are vx_leaf_sponge_air.hip (rows -> states, digests) and vx_merkle_open_air.hip (paths -> states).
#include <string.h>

#include "air_leaf_sponge.cuh"
#include "air_merkle_open.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
constexpr int N_TREE_IDS = (int)VX_SOPEN_TREE0 + 3;
const char* tree_name(uint64_t t) { return t == VX_SOPEN_TREE0 ? "trace" : t == VX_SOPEN_TREE0 + 1 ? "auxiliary" : t == VX_SOPEN_TREE0 + 2 ? "quotient" : "FRI layer"; }
}  // namespace

extern "C" {
int32_t vx_stark_openings_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                                size_t* blob_len) {
    if (!ctx || !cfg || !proof || !blob_len) return VX_ERR_ARG;
    // ---- the claims: the proof is verified on the way, every check except the paths
    StarkOpenings so;
    char err[256] = "";
    const int32_t vrc = vx_stark_openings_claims(cfg, proof, proof_len, 0, nullptr, 0, ext_chal, true, &so, err, sizeof err);
    if (vrc != VX_OK) return vx_fail(ctx, vrc, "stark openings: %s", err[0] ? err : "the inner proof or the configuration is not acceptable");
    StarkOpeningsTables ts;
    VX_CHECK(so.cap_h <= 16 && stark_openings_tables(so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, &ts),
             "stark openings: the proof's shape has no openings group (cap height above 16, a tree without a level, or a table of more than 2^26 rows)");
    const size_t n_claims = so.claims.size(), n_trees = so.tree.size(), cap_words = (size_t)4 << so.cap_h;
    // the witnesses hold pool blocks of this context until the group has proven (declared before it: vx_bus.h)
    MerkleOpenWitness paths;
    LeafSpongeWitness sponge[3];
    // ---- the sponge chains of every leaf longer than 4 words, one launch per length; their digests enter the paths on the device
    std::vector<const uint64_t*> leaf_dev(n_claims, nullptr);
    std::vector<uint64_t> leaf_dig(4 * n_claims, 0);
    std::vector<uint64_t> s_tree[3], s_idx[3], s_rows[3];
    for (int k = 1; k < ts.n; ++k) {
        const size_t L = ts.leaf_len[k];
        std::vector<size_t> who;
        for (size_t i = 0; i < n_claims; ++i) {
            const StarkOpenings::Claim& c = so.claims[i];
            if (c.leaf_len != L) continue;
            who.push_back(i), s_tree[k - 1].push_back(c.tree), s_idx[k - 1].push_back(c.index);
            s_rows[k - 1].insert(s_rows[k - 1].end(), so.leaves.begin() + c.leaf, so.leaves.begin() + c.leaf + L);
        }
        VX_TRY(vx_leaf_sponge_rows_states_dev(ctx, L, s_tree[k - 1].data(), s_idx[k - 1].data(), s_rows[k - 1].data(), who.size(), &sponge[k - 1]));
        for (size_t j = 0; j < who.size(); ++j) leaf_dev[who[j]] = sponge[k - 1].digests_d + 4 * j;
    }
    // ---- the paths: a row of at most 4 words is its own digest, zero-padded; the siblings are read where the claims say they lie
    int log_leaves[N_TREE_IDS] = {0};
    std::vector<uint64_t> caps((size_t)N_TREE_IDS * cap_words, 0), roots(4 * n_trees), tree_of(n_claims), leaf_idx(n_claims), sibs;
    for (size_t k = 0; k < n_trees; ++k) {
        const uint64_t t = so.tree[k];
        log_leaves[t] = so.log_leaves(t);
        memcpy(caps.data() + t * cap_words, so.caps.data() + k * cap_words, cap_words * 8);
        vx_cap_fold(so.caps.data() + k * cap_words, so.cap_h, roots.data() + 4 * k);
    }
    for (size_t i = 0; i < n_claims; ++i) {
        const StarkOpenings::Claim& c = so.claims[i];
        tree_of[i] = c.tree, leaf_idx[i] = c.index;
        if (c.leaf_len <= 4) memcpy(leaf_dig.data() + 4 * i, so.leaves.data() + c.leaf, c.leaf_len * 8);
        sibs.insert(sibs.end(), proof + c.sib, proof + c.sib + 4 * (size_t)(so.log_leaves(c.tree) - so.cap_h));
    }
    // the native statement check: every path reaches the root of its tree (this also waits for the sponge chains)
    size_t bad = 0;
    const int32_t prc = vx_merkle_paths_states_dev(ctx, caps.data(), so.cap_h, log_leaves, (size_t)N_TREE_IDS, tree_of.data(), leaf_idx.data(), leaf_dig.data(), leaf_dev.data(), sibs.data(),
                                                   n_claims, &paths, &bad);
    if (prc == VX_ERR_STATEMENT && bad < n_claims) {
        const uint64_t t = so.claims[bad].tree;
        if (t < VX_SOPEN_TREE0)
            return vx_fail(ctx, VX_ERR_STATEMENT, "stark openings: query %zu: the path of FRI layer %llu (leaf %llu) does not reach the root of its tree", bad / n_trees, (unsigned long long)t,
                           (unsigned long long)so.claims[bad].index);
        return vx_fail(ctx, VX_ERR_STATEMENT, "stark openings: query %zu: the path of the %s tree (leaf %llu) does not reach the root of its tree", bad / n_trees, tree_name(t),
                       (unsigned long long)so.claims[bad].index);
    }
    VX_TRY(prc);
    uint64_t stmt[4];
    vx_stark_openings_statement(so, roots.data(), stmt);
    // ---- the tables of one bus, in transcript order: the openings on this context, every sponge table on a side context and a
    // host thread of its own; their gens only launch trace kernels over the buffers above, which nothing writes any more
    TableGroup g(ctx, cfg, "stark openings");
    const int open = g.add({"openings", VX_AIR_MERKLE_OPEN_SET, ts.log_n[0], mop::SET_COLS, mop::SET_PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                VX_TRY(vx_merkle_paths_trace_dev(c, paths, ts.log_n[0], trace->d));
                                vx_merkle_open_set_public(stmt, pub);
                                return (int32_t)VX_OK;
                            }});
    for (int k = 1; k < ts.n; ++k)
        g.add({"sponge", VX_AIR_LEAF_SPONGE_SET, ts.log_n[k], lsp::SET_COLS, lsp::PUB, 0, [&, k](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                   VX_TRY(vx_leaf_sponge_rows_trace_dev(c, sponge[k - 1], ts.log_n[k], trace->d));
                   vx_leaf_sponge_set_public(ts.leaf_len[k], stmt, pub);
                   return (int32_t)VX_OK;
               }});
    VX_TRY(g.prove(open));
    const std::array<uint64_t, 7> sw = so.shape_words();
    uint64_t request[8];
    memcpy(request, sw.data(), sizeof sw);
    request[7] = (uint64_t)ts.n;
    const TableJob* jobs[4];
    for (int k = 0; k < ts.n; ++k) jobs[k] = &g.job[k];
    return pack_blob(ctx, "stark openings", VX_SOPEN_MAGIC, request, 8, jobs, (size_t)ts.n, blob_out, blob_cap, blob_len);
}
}  // extern "C"
