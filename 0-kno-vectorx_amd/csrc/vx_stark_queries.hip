// vx_stark_queries_prove: the WHOLE query phase of one inner vx_stark_prove proof on ONE logUp bus -- the group of
// vx_stark_openings_prove (MerkleOpenSetAir: one path per (query, tree); one LeafSpongeSetAir table per leaf length above 4) with
// LeafNoopAir (the openings of leaves of at most 4 words, which are their own digest), FriCombineAir (TREE0 = 8) and FriFoldAir
// (TREE0 = 0) in the verifier's place on the row bus.  TAG_OPEN closes between the openings and the leaf tables, TAG_ROW between
// the leaf tables and the arithmetic -- for every tree of the proof --, TAG_FRI end 0 between combination and fold.  What is left
// for the party outside -- vx_stark_queries_verify in vx_verify.hip -- is the root and depth every path ended in (TAG_ROOT) and the
// exit of every fold chain (TAG_FRI end 1): it reads no query record.  The claims come from ONE replay of the verifier's code
// (vx_stark_queries_claims); the four digest words of every table are the statement digest (vx_bus.h), which holds no row word and
// no leaf word.  No kernels here: the witnesses are vx_merkle_open_air.hip, vx_leaf_sponge_air.hip, vx_leaf_noop_air.hip,
// vx_fri_combine_air.hip and vx_fri_fold_air.hip.
#include <string.h>

#include "air_fri_combine.cuh"
#include "air_fri_fold.cuh"
#include "air_leaf_noop.cuh"
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
int32_t vx_stark_queries_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                               size_t* blob_len) {
    if (!ctx || !cfg || !proof || !blob_len) return VX_ERR_ARG;
    VX_CHECK(cfg->arity_bits == 4, "stark queries: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    // ---- the claims, from one replay: the proof is verified on the way, every check except the paths
    StarkQueries sq;
    char err[256] = "";
    const int32_t vrc = vx_stark_queries_claims(cfg, proof, proof_len, 0, nullptr, 0, ext_chal, false, &sq, err, sizeof err);
    if (vrc != VX_OK) return vx_fail(ctx, vrc, "stark queries: %s", err[0] ? err : "the inner proof or the configuration is not acceptable");
    const StarkOpenings& so = sq.so;
    StarkQueriesTables ts;
    VX_CHECK(so.cap_h <= 16 && stark_queries_tables(so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, *cfg, &ts),
             "stark queries: the proof's shape has no query-phase group (no fold layer or more than 8, no index bit left, cap height above 16, or a table of more than 2^26 rows)");
    const size_t n_claims = so.claims.size(), n_trees = so.tree.size(), cap_words = (size_t)4 << so.cap_h, n_q = so.n_queries;
    const FriCombineStmt st = sq.stmt();
    MerkleOpenWitness paths;
    LeafSpongeWitness sponge[3];
    // ---- the sponge chains of every leaf longer than 4 words, one launch per length; their digests enter the paths on the device
    std::vector<const uint64_t*> leaf_dev(n_claims, nullptr);
    std::vector<uint64_t> leaf_dig(4 * n_claims, 0);
    std::vector<uint64_t> s_tree[3], s_idx[3], s_rows[3];
    for (int k = 1; k <= ts.n_sponge; ++k) {
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
    // ---- the paths, and the openings of the leaves that are their own digest
    int log_leaves[N_TREE_IDS] = {0};
    std::vector<uint64_t> caps((size_t)N_TREE_IDS * cap_words, 0), roots(4 * n_trees), tree_of(n_claims), leaf_idx(n_claims), sibs;
    std::vector<uint64_t> n_tree, n_idx, n_len, n_rows;
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
    VX_CHECK(n_tree.size() == n_q * ts.noop_per_query, "stark queries: %zu openings of leaves of at most 4 words, the shape says %zu", n_tree.size(), n_q * ts.noop_per_query);
    VX_TRY(vx_leaf_noop_check(ctx, n_tree.data(), n_idx.data(), n_len.data(), n_rows.data(), n_tree.size()));
    // ---- the native statement checks: every path reaches the root of its tree (this also waits for the sponge chains) ...
    size_t bad = 0;
    const int32_t prc = vx_merkle_paths_states_dev(ctx, caps.data(), so.cap_h, log_leaves, (size_t)N_TREE_IDS, tree_of.data(), leaf_idx.data(), leaf_dig.data(), leaf_dev.data(), sibs.data(),
                                                   n_claims, &paths, &bad);
    if (prc == VX_ERR_STATEMENT && bad < n_claims) {
        const uint64_t t = so.claims[bad].tree;
        if (t < VX_SOPEN_TREE0)
            return vx_fail(ctx, VX_ERR_STATEMENT, "stark queries: query %zu: the path of FRI layer %llu (leaf %llu) does not reach the root of its tree", bad / n_trees, (unsigned long long)t,
                           (unsigned long long)so.claims[bad].index);
        return vx_fail(ctx, VX_ERR_STATEMENT, "stark queries: query %zu: the path of the %s tree (leaf %llu) does not reach the root of its tree", bad / n_trees, tree_name(t),
                       (unsigned long long)so.claims[bad].index);
    }
    VX_TRY(prc);
    // ... every ev_0 is the combination of its rows, and every fold chain holds and ends in the final polynomial
    VX_TRY(vx_fri_combine_check_dev(ctx, st, so.index.data(), sq.rows.data(), sq.ev0.data(), n_q));
    VX_TRY(vx_fri_fold_check_dev(ctx, so.LN, sq.betas.data(), so.NL, sq.final_poly.data(), sq.final_poly.size() / 2, so.index.data(), sq.ev0.data(), sq.leaves.data(), n_q));
    uint64_t stmt[4];
    vx_stark_queries_statement(sq, roots.data(), stmt);
    // ---- the tables of one bus, in transcript order: the openings on this context, every other table on a side context and a host
    // thread of its own; their gens read the buffers above, which nothing writes any more
    const int k_noop = 1 + ts.n_sponge, k_comb = k_noop + 1, k_fold = k_noop + 2;
    TableGroup g(ctx, cfg, "stark queries");
    const int open = g.add({"openings", VX_AIR_MERKLE_OPEN_SET, ts.log_n[0], mop::SET_COLS, mop::SET_PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                VX_TRY(vx_merkle_paths_trace_dev(c, paths, ts.log_n[0], trace->d));
                                vx_merkle_open_set_public(stmt, pub);
                                return (int32_t)VX_OK;
                            }});
    for (int k = 1; k <= ts.n_sponge; ++k)
        g.add({"sponge", VX_AIR_LEAF_SPONGE_SET, ts.log_n[k], lsp::SET_COLS, lsp::PUB, 0, [&, k](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                   VX_TRY(vx_leaf_sponge_rows_trace_dev(c, sponge[k - 1], ts.log_n[k], trace->d));
                   vx_leaf_sponge_set_public(ts.leaf_len[k], stmt, pub);
                   return (int32_t)VX_OK;
               }});
    g.add({"noop leaves", VX_AIR_LEAF_NOOP, ts.log_n[k_noop], lnp::COLS, lnp::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_leaf_noop_trace_dev(c, n_tree.data(), n_idx.data(), n_len.data(), n_rows.data(), n_tree.size(), ts.log_n[k_noop], trace->d));
               vx_leaf_noop_public(stmt, pub);
               return (int32_t)VX_OK;
           }});
    g.add({"combination", VX_AIR_FRI_COMBINE, ts.log_n[k_comb], fca::COLS, fca::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_fri_combine_trace_dev(c, st, fca::TREE0, so.index.data(), sq.rows.data(), sq.ev0.data(), n_q, ts.log_n[k_comb], trace->d, pub));
               vx_fri_combine_public_digest(st, fca::TREE0, stmt, pub);
               return (int32_t)VX_OK;
           }});
    g.add({"fold", VX_AIR_FRI_FOLD, ts.log_n[k_fold], ffa::COLS, ffa::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_fri_fold_trace_dev(c, so.LN, sq.betas.data(), so.NL, 0, so.index.data(), sq.ev0.data(), sq.leaves.data(), n_q, ts.log_n[k_fold], trace->d, pub));
               vx_fri_fold_public_digest(so.LN, sq.betas.data(), so.NL, 0, stmt, pub);
               return (int32_t)VX_OK;
           }});
    VX_TRY(g.prove(open));
    const std::array<uint64_t, 7> sw = so.shape_words();
    uint64_t request[8];
    memcpy(request, sw.data(), sizeof sw);
    request[7] = (uint64_t)ts.n;
    const TableJob* jobs[7];
    for (int k = 0; k < ts.n; ++k) jobs[k] = &g.job[k];
    return pack_blob(ctx, "stark queries", VX_SQRY_MAGIC, request, 8, jobs, (size_t)ts.n, blob_out, blob_cap, blob_len);
}
}  // extern "C"
