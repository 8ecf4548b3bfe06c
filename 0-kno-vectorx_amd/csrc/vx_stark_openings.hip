// vx_stark_openings_prove: the Merkle side of one inner vx_stark_prove proof on ONE logUp bus, sourced from the proof itself -- per
// query the opened rows, the FRI leaves and every sibling up to the cap are all in it, so no vx_tree and no LDE is needed (an
// aggregator holds proof bytes, not trees).  The openings table (MerkleOpenSetAir: one path per (query, tree), tree ids as in
// vx_bus.h) and one LeafSpongeSetAir table per leaf length above 4 among {cm, ca, 2 2^a}, in that bus order (vx_table_shapes.h);
// TAG_OPEN closes between them for every tree whose rows are hashed.  What is left for the party outside -- the verifier,
// vx_stark_openings_verify in vx_verify.hip -- is the root and depth every path ended in (TAG_ROOT), every word of the hashed
// rows (TAG_ROW) and the opening of a row that is its own digest (TAG_OPEN).  The claims come from the verifier's own query phase with
// the paths delegated (vx_stark_openings_claims); the four digest words of every table are the STATEMENT digest (vx_bus.h).
// No kernels here: the witnesses are vx_leaf_sponge_air.hip (rows -> states, digests) and vx_merkle_open_air.hip (paths -> states).
#include <string.h>

#include "air_leaf_sponge.cuh"
#include "air_merkle_open.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
const char* tree_name(uint64_t t) { return t == VX_SOPEN_TREE0 ? "trace" : t == VX_SOPEN_TREE0 + 1 ? "auxiliary" : t == VX_SOPEN_TREE0 + 2 ? "quotient" : "FRI layer"; }
}  // namespace

// ---- the Merkle side of a proof-sourced group (vx_bus.h), for vx_stark_queries_prove as well.  Gathered on the host: per sponge
// table its openings as rows; per tree id its cap, depth and folded root; per claim tree, index and siblings (read where the claims
// say they lie) and, for a row of at most 4 words, the row as its own digest, zero-padded, and as an opening of LeafNoopAir.
StarkMerkleSide::StarkMerkleSide(vx_ctx* ctx, const char* prefix, const StarkOpenings& so, const uint64_t* proof, const size_t* lens, int n_sponge)
    : ctx(ctx), prefix(prefix), so(so), n_sponge(n_sponge) {
    const size_t n_claims = so.claims.size(), n_trees = so.tree.size(), cap_words = (size_t)4 << so.cap_h;
    leaf_dev.assign(n_claims, nullptr), leaf_dig.assign(4 * n_claims, 0), tree_of.resize(n_claims), leaf_idx.resize(n_claims);
    caps.assign((size_t)N_TREE_IDS * cap_words, 0), roots.resize(4 * n_trees);
    for (int k = 0; k < n_sponge; ++k) {
        sponge_len[k] = lens[k];
        for (size_t i = 0; i < n_claims; ++i) {
            const StarkOpenings::Claim& c = so.claims[i];
            if (c.leaf_len != lens[k]) continue;
            s_who[k].push_back(i), s_tree[k].push_back(c.tree), s_idx[k].push_back(c.index);
            s_rows[k].insert(s_rows[k].end(), so.leaves.begin() + c.leaf, so.leaves.begin() + c.leaf + c.leaf_len);
        }
    }
    for (size_t k = 0; k < n_trees; ++k) {
        const uint64_t t = so.tree[k];
        log_leaves[t] = so.log_leaves(t);
        memcpy(caps.data() + t * cap_words, so.caps.data() + k * cap_words, cap_words * 8);
        vx_cap_fold(so.caps.data() + k * cap_words, so.cap_h, roots.data() + 4 * k);
    }
    for (size_t i = 0; i < n_claims; ++i) {
        const StarkOpenings::Claim& c = so.claims[i];
        tree_of[i] = c.tree, leaf_idx[i] = c.index;
        if (c.leaf_len <= 4) {
            memcpy(leaf_dig.data() + 4 * i, so.leaves.data() + c.leaf, c.leaf_len * 8);
            n_tree.push_back(c.tree), n_idx.push_back(c.index), n_len.push_back(c.leaf_len);
            n_rows.insert(n_rows.end(), leaf_dig.begin() + 4 * i, leaf_dig.begin() + 4 * i + 4);
        }
        sibs.insert(sibs.end(), proof + c.sib, proof + c.sib + 4 * (size_t)(so.log_leaves(c.tree) - so.cap_h));
    }
}
int32_t StarkMerkleSide::launch() {
    for (int k = 0; k < n_sponge; ++k) {
        VX_TRY(vx_leaf_sponge_rows_states_dev(ctx, sponge_len[k], s_tree[k].data(), s_idx[k].data(), s_rows[k].data(), s_who[k].size(), &sponge[k]));
        for (size_t j = 0; j < s_who[k].size(); ++j) leaf_dev[s_who[k][j]] = sponge[k].digests_d + 4 * j;
    }
    // the native statement check: every path reaches the root of its tree (this also waits for the sponge chains)
    const size_t n_claims = so.claims.size();
    size_t bad = 0;
    const int32_t rc = vx_merkle_paths_states_dev(ctx, caps.data(), so.cap_h, log_leaves, (size_t)N_TREE_IDS, tree_of.data(), leaf_idx.data(), leaf_dig.data(), leaf_dev.data(), sibs.data(),
                                                  n_claims, &paths, &bad);
    if (rc == VX_ERR_STATEMENT && bad < n_claims) {
        const StarkOpenings::Claim& c = so.claims[bad];
        if (c.tree < VX_SOPEN_TREE0)
            return vx_fail(ctx, VX_ERR_STATEMENT, "%s query %zu: the path of FRI layer %llu (leaf %llu) does not reach the root of its tree", prefix, bad / so.tree.size(),
                           (unsigned long long)c.tree, (unsigned long long)c.index);
        return vx_fail(ctx, VX_ERR_STATEMENT, "%s query %zu: the path of the %s tree (leaf %llu) does not reach the root of its tree", prefix, bad / so.tree.size(), tree_name(c.tree),
                       (unsigned long long)c.index);
    }
    return rc;
}
// the gens only launch trace kernels over the witnesses, which nothing writes any more
int StarkMerkleSide::add_tables(TableGroup& g, const int* log_n, const uint64_t* stmt) {
    const int open = g.add({"openings", VX_AIR_MERKLE_OPEN_SET, log_n[0], mop::SET_COLS, mop::SET_PUB, 0, [this, stmt, ln = log_n[0]](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                VX_TRY(vx_merkle_paths_trace_dev(c, paths, ln, trace->d));
                                vx_merkle_open_set_public(stmt, pub);
                                return (int32_t)VX_OK;
                            }});
    for (int k = 0; k < n_sponge; ++k)
        g.add({"sponge", VX_AIR_LEAF_SPONGE_SET, log_n[1 + k], lsp::SET_COLS, lsp::PUB, 0, [this, stmt, k, ln = log_n[1 + k]](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                   VX_TRY(vx_leaf_sponge_rows_trace_dev(c, sponge[k], ln, trace->d));
                   vx_leaf_sponge_set_public(sponge_len[k], stmt, pub);
                   return (int32_t)VX_OK;
               }});
    return open;
}
int32_t vx_stark_group_blob(TableGroup& g, int n_tables, uint64_t magic, const StarkOpenings& so, uint64_t* blob_out, size_t blob_cap, size_t* blob_len) {
    const std::array<uint64_t, 7> sw = so.shape_words();
    uint64_t request[8];
    memcpy(request, sw.data(), sizeof sw);
    request[7] = (uint64_t)n_tables;
    const TableJob* jobs[BusGroup::MAX];
    for (int k = 0; k < n_tables; ++k) jobs[k] = &g.job[k];
    return pack_blob(g.ctx, g.what, magic, request, 8, jobs, (size_t)n_tables, blob_out, blob_cap, blob_len);
}

extern "C" {
int32_t vx_stark_openings_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                                size_t* blob_len) {
    if (!ctx || !cfg || !proof || !blob_len) return VX_ERR_ARG;
    // ---- the claims: the proof is verified on the way, every check except the paths
    StarkQueries sq;
    char err[256] = "";
    const int32_t vrc = vx_stark_openings_claims(cfg, proof, proof_len, 0, nullptr, 0, ext_chal, &sq, err, sizeof err);
    if (vrc != VX_OK) return vx_fail(ctx, vrc, "stark openings: %s", err[0] ? err : "the inner proof or the configuration is not acceptable");
    const StarkOpenings& so = sq.so;
    StarkGroupTables ts;
    VX_CHECK(so.cap_h <= 16 && stark_openings_tables(so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, &ts),
             "stark openings: the proof's shape has no openings group (cap height above 16, a tree without a level, or a table of more than 2^26 rows)");
    // ---- the Merkle side, with its native statement check: every path reaches the root of its tree
    StarkMerkleSide ms(ctx, "stark openings:", so, proof, ts.leaf_len + 1, ts.n_sponge);
    VX_TRY(ms.launch());
    uint64_t stmt[4];
    vx_stark_openings_statement(so, ms.roots.data(), stmt);
    // ---- the tables of one bus, in transcript order: the openings on this context, every sponge table on a side context and a
    // host thread of its own
    TableGroup g(ctx, cfg, "stark openings");
    VX_TRY(g.prove(ms.add_tables(g, ts.log_n, stmt)));
    return vx_stark_group_blob(g, ts.n, VX_SOPEN_MAGIC, so, blob_out, blob_cap, blob_len);
}
}  // extern "C"
