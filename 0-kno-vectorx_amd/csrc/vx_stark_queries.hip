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

extern "C" {
int32_t vx_stark_queries_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                               size_t* blob_len) {
    if (!ctx || !cfg || !proof || !blob_len) return VX_ERR_ARG;
    VX_CHECK(cfg->arity_bits == 4, "stark queries: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    // ---- the claims, from one replay: the proof is verified on the way, every check except the paths
    StarkQueries sq;
    char err[256] = "";
    const int32_t vrc = vx_stark_queries_claims(cfg, proof, proof_len, 0, nullptr, 0, ext_chal, QueryPhase::Delegated, &sq, err, sizeof err);
    if (vrc != VX_OK) return vx_fail(ctx, vrc, "stark queries: %s", err[0] ? err : "the inner proof or the configuration is not acceptable");
    const StarkOpenings& so = sq.so;
    StarkGroupTables ts;
    VX_CHECK(so.cap_h <= 16 && stark_queries_tables(so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, *cfg, &ts),
             "stark queries: the proof's shape has no query-phase group (no fold layer or more than 8, no index bit left, cap height above 16, or a table of more than 2^26 rows)");
    const size_t n_q = so.n_queries;
    const FriCombineStmt st = sq.stmt();
    // ---- the Merkle side, and the openings of the leaves that are their own digest
    StarkMerkleSide ms(ctx, "stark queries:", so, proof, ts.leaf_len + 1, ts.n_sponge);
    VX_CHECK(ms.n_tree.size() == n_q * ts.noop_per_query, "stark queries: %zu openings of leaves of at most 4 words, the shape says %zu", ms.n_tree.size(), n_q * ts.noop_per_query);
    VX_TRY(vx_leaf_noop_check(ctx, ms.n_tree.data(), ms.n_idx.data(), ms.n_len.data(), ms.n_rows.data(), ms.n_tree.size()));
    // ---- the native statement checks: every path reaches the root of its tree ...
    VX_TRY(ms.launch());
    // ... every ev_0 is the combination of its rows, and every fold chain holds and ends in the final polynomial
    VX_TRY(vx_fri_combine_check_dev(ctx, st, so.index.data(), sq.rows.data(), sq.ev0.data(), n_q));
    VX_TRY(vx_fri_fold_check_dev(ctx, so.LN, sq.betas.data(), so.NL, sq.final_poly.data(), sq.final_poly.size() / 2, so.index.data(), sq.ev0.data(), sq.leaves.data(), n_q));
    uint64_t stmt[4];
    vx_stark_queries_statement(sq, ms.roots.data(), stmt);
    // ---- the tables of one bus, in transcript order: the openings on this context, every other table on a side context and a host
    // thread of its own; their gens read the buffers above, which nothing writes any more
    const int k_noop = 1 + ts.n_sponge, k_comb = k_noop + 1, k_fold = k_noop + 2;
    TableGroup g(ctx, cfg, "stark queries");
    const int open = ms.add_tables(g, ts.log_n, stmt);
    g.add({"noop leaves", VX_AIR_LEAF_NOOP, ts.log_n[k_noop], lnp::COLS, lnp::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_leaf_noop_trace_dev(c, ms.n_tree.data(), ms.n_idx.data(), ms.n_len.data(), ms.n_rows.data(), ms.n_tree.size(), ts.log_n[k_noop], trace->d));
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
    return vx_stark_group_blob(g, ts.n, VX_SQRY_MAGIC, so, blob_out, blob_cap, blob_len);
}
}  // extern "C"
