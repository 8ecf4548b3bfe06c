// vx_stark_openings_prove / vx_stark_queries_prove / vx_stark_inner_prove: parts of one inner vx_stark_prove proof on ONE logUp bus,
// sourced from the proof itself -- per query the opened rows, the FRI leaves and every sibling up to the cap are all in it, so no
// vx_tree and no LDE is needed (an aggregator holds proof bytes, not trees).  The three are LEVELS of one group and ONE prover body,
// stark_group_prove: which tables a level has, in bus order, is vx_table_shapes.h; its magic, names and refusal texts are
// stark_level, its request words, statement digest and every table's public inputs the functions beside it (vx_bus.h); what is left
// for the party outside is said where that party is, at stark_group_verify in vx_verify.hip.  The claims come from ONE replay of the
// verifier's code with the paths delegated.  No kernels here: the witnesses are vx_merkle_open_air.hip, vx_leaf_sponge_air.hip,
// vx_leaf_noop_air.hip, vx_fri_combine_air.hip, vx_fri_fold_air.hip and vx_transcript_air.hip.
#include <string.h>

#include "air_fri_combine.cuh"
#include "air_fri_fold.cuh"
#include "air_leaf_noop.cuh"
#include "air_leaf_sponge.cuh"
#include "air_merkle_open.cuh"
#include "air_transcript.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
const char* tree_name(uint64_t t) { return t == VX_SOPEN_TREE0 ? "trace" : t == VX_SOPEN_TREE0 + 1 ? "auxiliary" : t == VX_SOPEN_TREE0 + 2 ? "quotient" : "FRI layer"; }
}  // namespace

// ---- the Merkle side of a proof-sourced group (vx_bus.h), at every level.  Gathered on the host: per sponge
// table its openings as rows; per tree id its cap, depth and folded root; per claim tree, index and siblings (read where the claims
// say they lie) and, for a row of at most 4 words, the row as its own digest, zero-padded, and as an opening of LeafNoopAir.
StarkMerkleSide::StarkMerkleSide(vx_ctx* ctx, const char* what, const StarkOpenings& so, const uint64_t* proof, const size_t* lens, int n_sponge)
    : ctx(ctx), what(what), so(so), n_sponge(n_sponge), roots(so.roots()) {
    const size_t n_claims = so.claims.size(), n_trees = so.tree.size(), cap_words = (size_t)4 << so.cap_h;
    leaf_dev.assign(n_claims, nullptr), leaf_dig.assign(4 * n_claims, 0), tree_of.resize(n_claims), leaf_idx.resize(n_claims);
    caps.assign((size_t)N_TREE_IDS * cap_words, 0);
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
            return vx_fail(ctx, VX_ERR_STATEMENT, "%s: query %zu: the path of FRI layer %llu (leaf %llu) does not reach the root of its tree", what, bad / so.tree.size(),
                           (unsigned long long)c.tree, (unsigned long long)c.index);
        return vx_fail(ctx, VX_ERR_STATEMENT, "%s: query %zu: the path of the %s tree (leaf %llu) does not reach the root of its tree", what, bad / so.tree.size(), tree_name(c.tree),
                       (unsigned long long)c.index);
    }
    return rc;
}
// the gens only launch trace kernels over the witnesses, which nothing writes any more
int StarkMerkleSide::add_tables(TableGroup& g, const StarkGroupTables& ts, const StarkQueries& sq, const uint64_t* stmt) {
    const int open = g.add({"openings", VX_AIR_MERKLE_OPEN_SET, ts.log_n[0], mop::SET_COLS, mop::SET_PUB, 0, [this, &ts, &sq, stmt](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                VX_TRY(vx_merkle_paths_trace_dev(c, paths, ts.log_n[0], trace->d));
                                stark_table_public(ts, 0, sq, stmt, pub);
                                return (int32_t)VX_OK;
                            }});
    for (int k = 1; k <= n_sponge; ++k)
        g.add({"sponge", VX_AIR_LEAF_SPONGE_SET, ts.log_n[k], lsp::SET_COLS, lsp::PUB, 0, [this, &ts, &sq, stmt, k](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                   VX_TRY(vx_leaf_sponge_rows_trace_dev(c, sponge[k - 1], ts.log_n[k], trace->d));
                   stark_table_public(ts, k, sq, stmt, pub);
                   return (int32_t)VX_OK;
               }});
    return open;
}

namespace {
// ---- the arithmetic side of a group from Queries up, beside the Merkle side: LeafNoopAir over the short leaves `ms` gathered,
// FriCombineAir (TREE0 = 8) and FriFoldAir (TREE0 = 0) over the claims of the replay.  The native statement checks first -- every ev_0
// is the combination of its rows, every fold chain holds and ends in the final polynomial --, then the three tables behind the sponges.
int32_t arith_check(vx_ctx* ctx, const StarkQueries& sq) {
    const StarkOpenings& so = sq.so;
    VX_TRY(vx_fri_combine_check_dev(ctx, sq.stmt(), so.index.data(), sq.rows.data(), sq.ev0.data(), so.n_queries));
    return vx_fri_fold_check_dev(ctx, so.LN, sq.betas.data(), so.NL, sq.final_poly.data(), sq.final_poly.size() / 2, so.index.data(), sq.ev0.data(), sq.leaves.data(), so.n_queries);
}
void arith_add_tables(TableGroup& g, const StarkMerkleSide& ms, const StarkGroupTables& ts, const StarkQueries& sq, const uint64_t* stmt) {
    const StarkOpenings& so = sq.so;
    const int k_noop = 1 + ts.n_sponge, k_comb = k_noop + 1, k_fold = k_noop + 2;
    g.add({"noop leaves", VX_AIR_LEAF_NOOP, ts.log_n[k_noop], lnp::COLS, lnp::PUB, 0, [&ms, &ts, &sq, stmt, k_noop](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_leaf_noop_trace_dev(c, ms.n_tree.data(), ms.n_idx.data(), ms.n_len.data(), ms.n_rows.data(), ms.n_tree.size(), ts.log_n[k_noop], trace->d));
               stark_table_public(ts, k_noop, sq, stmt, pub);
               return (int32_t)VX_OK;
           }});
    g.add({"combination", VX_AIR_FRI_COMBINE, ts.log_n[k_comb], fca::COLS, fca::PUB, 0, [&so, &ts, &sq, stmt, k_comb](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_fri_combine_trace_dev(c, sq.stmt(), fca::TREE0, so.index.data(), sq.rows.data(), sq.ev0.data(), so.n_queries, ts.log_n[k_comb], trace->d, pub));
               stark_table_public(ts, k_comb, sq, stmt, pub);
               return (int32_t)VX_OK;
           }});
    g.add({"fold", VX_AIR_FRI_FOLD, ts.log_n[k_fold], ffa::COLS, ffa::PUB, 0, [&so, &ts, &sq, stmt, k_fold](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_fri_fold_trace_dev(c, so.LN, sq.betas.data(), so.NL, 0, so.index.data(), sq.ev0.data(), sq.leaves.data(), so.n_queries, ts.log_n[k_fold], trace->d, pub));
               stark_table_public(ts, k_fold, sq, stmt, pub);
               return (int32_t)VX_OK;
           }});
}

// ---- the ONE prover body.  A level differs in its replay, its statement digest (both chosen below) and its tables.
int32_t stark_group_prove(StarkLevel level, vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                          size_t* blob_len) {
    if (!ctx || !cfg || !proof || !blob_len) return VX_ERR_ARG;
    const StarkLevelInfo& lv = stark_level(level);
    const bool arith = level >= StarkLevel::Queries, inner = level == StarkLevel::Inner;
    if (arith) VX_CHECK(cfg->arity_bits == 4, "%s: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", lv.name, cfg->arity_bits);
    // ---- the claims, from ONE replay of the verifier's code: the proof is verified on the way, every check except the paths.  Inner:
    // over the recording challenger, so what the transcript did comes from the same run
    StarkQueries sq;
    glh::TranscriptRecord rec;
    char err[256] = "";
    const int32_t vrc = inner   ? vx_stark_inner_replay(cfg, proof, proof_len, ext_chal, false, &sq, &rec, err, sizeof err)
                        : arith ? vx_stark_queries_claims(cfg, proof, proof_len, 0, nullptr, 0, ext_chal, QueryPhase::Delegated, &sq, err, sizeof err)
                                : vx_stark_openings_claims(cfg, proof, proof_len, 0, nullptr, 0, ext_chal, &sq, err, sizeof err);
    if (vrc != VX_OK) return vx_fail(ctx, vrc, "%s: %s", lv.name, err[0] ? err : "the inner proof or the configuration is not acceptable");
    const StarkOpenings& so = sq.so;
    const TranscriptClaim claim{rec.words.data(), rec.words.size(), rec.chal.data(), rec.n_chal()};  // empty below Inner
    StarkGroupTables ts;
    VX_CHECK(so.cap_h <= 16 && stark_level_tables(level, so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, rec.n_blocks(), *cfg, &ts), "%s", lv.no_group);
    // ---- the Merkle side, and the openings of the leaves that are their own digest
    StarkMerkleSide ms(ctx, lv.name, so, proof, ts.leaf_len + 1, ts.n_sponge);
    if (arith) {
        VX_CHECK(ms.n_tree.size() == so.n_queries * ts.noop_per_query, "%s: %zu openings of leaves of at most 4 words, the shape says %zu", lv.name, ms.n_tree.size(),
                 so.n_queries * ts.noop_per_query);
        VX_TRY(vx_leaf_noop_check(ctx, ms.n_tree.data(), ms.n_idx.data(), ms.n_len.data(), ms.n_rows.data(), ms.n_tree.size()));
    }
    // ---- the native statement checks: every path reaches the root of its tree, then the arithmetic
    VX_TRY(ms.launch());
    if (arith) VX_TRY(arith_check(ctx, sq));
    // ---- the statement digest: at Inner the claims are in it, so they are fixed before the group's lookup challenges are drawn
    uint64_t stmt[4];
    stark_group_statement(level, sq, ms.roots.data(), claim, stmt);
    // ---- the tables of one bus, in bus order: the openings on this context, every other table on a side context and a host thread
    // of its own; their gens read the buffers above, which nothing writes any more
    TableGroup g(ctx, cfg, lv.name);
    const int open = ms.add_tables(g, ts, sq, stmt);
    if (arith) arith_add_tables(g, ms, ts, sq, stmt);
    if (inner)
        g.add({"transcript", VX_AIR_TRANSCRIPT, ts.log_n[ts.n - 1], tsc::COLS, tsc::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                   VX_TRY(vx_transcript_trace_dev(c, &rec, 1, ts.log_n[ts.n - 1], trace->d, nullptr));
                   stark_table_public(ts, ts.n - 1, sq, stmt, pub);
                   return (int32_t)VX_OK;
               }});
    VX_TRY(g.prove(open));
    const std::vector<uint64_t> request = stark_group_request(level, so, ts.n, claim);
    const TableJob* jobs[BusGroup::MAX];
    for (int k = 0; k < ts.n; ++k) jobs[k] = &g.job[k];
    return pack_blob(ctx, lv.name, lv.magic, request.data(), request.size(), jobs, (size_t)ts.n, blob_out, blob_cap, blob_len);
}
}  // namespace

extern "C" {
int32_t vx_stark_openings_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                                size_t* blob_len) {
    return stark_group_prove(StarkLevel::Openings, ctx, cfg, proof, proof_len, ext_chal, blob_out, blob_cap, blob_len);
}
int32_t vx_stark_queries_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                               size_t* blob_len) {
    return stark_group_prove(StarkLevel::Queries, ctx, cfg, proof, proof_len, ext_chal, blob_out, blob_cap, blob_len);
}
int32_t vx_stark_inner_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                             size_t* blob_len) {
    return stark_group_prove(StarkLevel::Inner, ctx, cfg, proof, proof_len, ext_chal, blob_out, blob_cap, blob_len);
}
}  // extern "C"
