// vx_stark_inner_prove: the query phase AND the Fiat-Shamir transcript of one inner vx_stark_prove proof on ONE logUp bus -- the tables
// of vx_stark_queries_prove in their order, then TranscriptAir with one chain (id 0).  TAG_OBS / TAG_CHAL live beside TAG_OPEN / TAG_ROW /
// TAG_ROOT / TAG_FRI: the tags do not meet.  The party outside -- vx_stark_inner_verify in vx_verify.hip -- receives the roots and the
// fold exits, sends the words the transcript absorbs and receives its challenges: it reads no query record and replays no transcript.
// Claims and chain come from ONE replay of the verifier's code (vx_stark_inner_replay); the four digest words of every table are the
// ONE statement digest (vx_stark_inner_statement, vx_bus.h).  No kernels here: the witnesses are vx_merkle_open_air.hip,
// vx_leaf_sponge_air.hip, vx_leaf_noop_air.hip, vx_fri_combine_air.hip, vx_fri_fold_air.hip and vx_transcript_air.hip.
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

static const char* const NO_GROUP =
    "stark inner: the proof's shape has no query-phase group (no fold layer or more than 8, no index bit left, cap height above 16, or a table of more than 2^26 rows)";

extern "C" {
// What vx_stark_inner_prove writes for this inner proof, to the word: a table's proof has the one length its AIR, its rows and the
// configuration imply (stark_proof::Shape::words).  Shape and block count follow from the head alone: no query record is read.
int32_t vx_stark_inner_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, size_t* n_words) {
    if (!cfg || !proof || !n_words) return VX_ERR_ARG;
    size_t head = 0;
    if (vx_stark_proof_head_words(cfg, proof, proof_len, &head) != VX_OK || proof_len < head) return VX_ERR_ARG;
    StarkQueries sq;
    glh::TranscriptRecord rec;
    if (vx_stark_inner_replay(cfg, proof, head, ext_chal, true, &sq, &rec, nullptr, 0) != VX_OK) return VX_ERR_ARG;
    const StarkOpenings& so = sq.so;
    StarkGroupTables ts;
    if (so.cap_h > 16 || !stark_inner_tables(so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, rec.n_blocks(), *cfg, &ts)) return VX_ERR_ARG;
    size_t total = VX_SINR_HDR + rec.chal.size() + (size_t)ts.n;
    for (int k = 0; k < ts.n; ++k) {
        BusAirShape a;
        if (!vx_air_bus_shape(ts.air[k], &a)) return VX_ERR_ARG;
        total += stark_proof::Shape(ts.air[k], a.cols, a.aux, a.pub, a.auxpub, ts.log_n[k], *cfg).words();
    }
    *n_words = total;
    return VX_OK;
}

int32_t vx_stark_inner_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                             size_t* blob_len) {
    if (!ctx || !cfg || !proof || !blob_len) return VX_ERR_ARG;
    VX_CHECK(cfg->arity_bits == 4, "stark inner: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    // ---- the claims of both halves, from ONE replay: the proof is verified on the way, every check except the paths
    StarkQueries sq;
    glh::TranscriptRecord rec;
    char err[256] = "";
    const int32_t vrc = vx_stark_inner_replay(cfg, proof, proof_len, ext_chal, false, &sq, &rec, err, sizeof err);
    if (vrc != VX_OK) return vx_fail(ctx, vrc, "stark inner: %s", err[0] ? err : "the inner proof or the configuration is not acceptable");
    const StarkOpenings& so = sq.so;
    StarkGroupTables ts;
    VX_CHECK(so.cap_h <= 16 && stark_inner_tables(so.LN, so.cm, so.ca, so.a, so.NL, so.n_queries, rec.n_blocks(), *cfg, &ts), "%s", NO_GROUP);
    const size_t n_q = so.n_queries;
    const FriCombineStmt st = sq.stmt();
    // ---- the Merkle side, and the openings of the leaves that are their own digest
    StarkMerkleSide ms(ctx, "stark inner:", so, proof, ts.leaf_len + 1, ts.n_sponge);
    VX_CHECK(ms.n_tree.size() == n_q * ts.noop_per_query, "stark inner: %zu openings of leaves of at most 4 words, the shape says %zu", ms.n_tree.size(), n_q * ts.noop_per_query);
    VX_TRY(vx_leaf_noop_check(ctx, ms.n_tree.data(), ms.n_idx.data(), ms.n_len.data(), ms.n_rows.data(), ms.n_tree.size()));
    // ---- the native statement checks: every path reaches the root of its tree, every ev_0 is the combination of its rows, every fold
    // chain holds and ends in the final polynomial
    VX_TRY(ms.launch());
    VX_TRY(vx_fri_combine_check_dev(ctx, st, so.index.data(), sq.rows.data(), sq.ev0.data(), n_q));
    VX_TRY(vx_fri_fold_check_dev(ctx, so.LN, sq.betas.data(), so.NL, sq.final_poly.data(), sq.final_poly.size() / 2, so.index.data(), sq.ev0.data(), sq.leaves.data(), n_q));
    // ---- the one statement digest: the claims are in it, so they are fixed before the group's lookup challenges are drawn
    const TranscriptClaim claim{rec.words.data(), rec.words.size(), rec.chal.data(), rec.n_chal()};
    uint64_t stmt[4];
    vx_stark_inner_statement(so.shape_words(), claim, stmt);
    // ---- the tables of one bus, in bus order; their gens read the buffers above, which nothing writes any more
    const int k_noop = 1 + ts.n_sponge, k_comb = k_noop + 1, k_fold = k_noop + 2, k_tran = k_noop + 3;
    TableGroup g(ctx, cfg, "stark inner");
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
    g.add({"transcript", VX_AIR_TRANSCRIPT, ts.log_n[k_tran], tsc::COLS, tsc::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_transcript_trace_dev(c, &rec, 1, ts.log_n[k_tran], trace->d, nullptr));
               vx_transcript_public(stmt, pub);
               return (int32_t)VX_OK;
           }});
    VX_TRY(g.prove(open));
    // ---- the blob: magic, the shape words, the table count, n_obs, n_chal, the claims, one length per table, the proofs
    const std::array<uint64_t, 7> sw = so.shape_words();
    std::vector<uint64_t> request(sw.begin(), sw.end());
    request.push_back((uint64_t)ts.n), request.push_back(claim.n_obs), request.push_back(claim.n_chal);
    request.insert(request.end(), rec.chal.begin(), rec.chal.end());
    const TableJob* jobs[BusGroup::MAX];
    for (int k = 0; k < ts.n; ++k) jobs[k] = &g.job[k];
    return pack_blob(ctx, "stark inner", VX_SINR_MAGIC, request.data(), request.size(), jobs, (size_t)ts.n, blob_out, blob_cap, blob_len);
}
}  // extern "C"
