// vx_fri_queries_prove: the query phase of one inner proof's FRI on ONE logUp bus -- the layer leaves opened (MerkleOpenSetAir),
// hashed (LeafSpongeSetAir) and folded (FriFoldAir), three tables of one group (vx_bus.h) in that bus order.  TAG_OPEN closes between the
// first two, TAG_ROW between the last two, in every one of the NL layer trees (tree id = layer); what is left for the party
// outside -- the verifier, vx_fri_queries_verify in vx_verify.hip -- is the entry and the exit of every chain (TAG_FRI) and the
// root and depth every path ended in (TAG_ROOT).  The four digest words among the public inputs of all three tables are the
// STATEMENT digest (vx_bus.h), which the verifier rebuilds from its own arguments: nothing is taken from a proof.
// No kernels here: the witnesses are vx_merkle_open_air.hip, vx_leaf_sponge_air.hip and vx_fri_fold_air.hip.
#include <string.h>

#include "air_fri_fold.cuh"
#include "air_leaf_sponge.cuh"
#include "air_merkle_open.cuh"
#include "glh_poseidon.h"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
constexpr size_t MAX_QUERIES = (size_t)1 << 20;
// the request as both entry points see it: arity 4, 1..8 layers with an index bit left, tables of at most 2^26 rows
bool shape_ok(const vx_stark_config* cfg, int log_lde, size_t n_layers, size_t n_queries) {
    if (cfg->arity_bits != 4 || log_lde < 5 || log_lde > 30 || n_layers < 1 || n_layers > (size_t)ffa::MAX_LAYERS || 4 * (int)n_layers >= log_lde) return false;
    if (n_queries < 1 || n_queries > MAX_QUERIES) return false;
    return fri_queries_open_log_n(n_queries, log_lde, n_layers) <= 26 && fri_queries_sponge_log_n(n_queries, n_layers) <= 26 && fri_fold_log_n(n_queries, log_lde, n_layers) <= 26;
}
}  // namespace

void vx_fri_queries_statement(int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len, const uint64_t* roots, const uint64_t* index,
                              const uint64_t* ev0, size_t n_queries, uint64_t digest[4]) {
    std::vector<uint64_t> w;
    w.reserve(3 + 6 * n_layers + 2 * final_len + 3 * n_queries);
    w.push_back((uint64_t)log_lde), w.push_back(n_layers), w.push_back(n_queries);
    w.insert(w.end(), betas, betas + 2 * n_layers);
    w.insert(w.end(), final_poly, final_poly + 2 * final_len);
    w.insert(w.end(), roots, roots + 4 * n_layers);
    for (size_t i = 0; i < n_queries; ++i) w.push_back(index[i]), w.push_back(ev0[2 * i]), w.push_back(ev0[2 * i + 1]);
    glh::hash_no_pad(w.data(), w.size(), digest);
}

extern "C" {
int32_t vx_fri_queries_proof_bound(const vx_stark_config* cfg, int log_lde, size_t n_layers, size_t n_queries, size_t* n_words) {
    if (!cfg || !n_words || !shape_ok(cfg, log_lde, n_layers, n_queries)) return VX_ERR_ARG;
    return vx_tables_proof_bound(cfg, VX_FQRY_HDR,
                                 {{VX_AIR_MERKLE_OPEN_SET, fri_queries_open_log_n(n_queries, log_lde, n_layers)},
                                  {VX_AIR_LEAF_SPONGE_SET, fri_queries_sponge_log_n(n_queries, n_layers)},
                                  {VX_AIR_FRI_FOLD, fri_fold_log_n(n_queries, log_lde, n_layers)}},
                                 n_words);
}

int32_t vx_fri_queries_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len,
                             const vx_tree* const* trees, const vx_buf* const* evals, const uint64_t* index, size_t n_queries, uint64_t* blob_out, size_t blob_cap, size_t* blob_len) {
    if (!ctx || !cfg || !betas || !final_poly || !trees || !evals || !index || !blob_len) return VX_ERR_ARG;
    VX_CHECK(cfg->arity_bits == 4, "fri queries: FriFoldAir is compiled for arity_bits 4 (16 values per leaf), the configuration says %d", cfg->arity_bits);
    VX_CHECK(log_lde >= 5 && log_lde <= 30 && n_layers >= 1 && n_layers <= (size_t)ffa::MAX_LAYERS && 4 * (int)n_layers < log_lde && n_queries >= 1 && n_queries <= MAX_QUERIES,
             "fri queries: log_lde %d (5..30), %zu layers (1..8, 4 bits each, at least one index bit left), %zu queries (1..2^20)", log_lde, n_layers, n_queries);
    VX_CHECK(shape_ok(cfg, log_lde, n_layers, n_queries), "fri queries: %zu queries of %zu layers over an LDE of 2^%d need a table of more than 2^26 rows", n_queries, n_layers, log_lde);
    const size_t NL = n_layers;
    int log_leaves[ffa::MAX_LAYERS];
    const uint64_t *evals_d[ffa::MAX_LAYERS], *tree_leaves[ffa::MAX_LAYERS];
    for (size_t l = 0; l < NL; ++l) {
        log_leaves[l] = log_lde - 4 * ((int)l + 1);
        VX_CHECK(trees[l] && evals[l], "fri queries: layer %zu is missing", l);
        VX_CHECK(trees[l]->n_leaves == (size_t)1 << log_leaves[l], "fri queries: the tree of layer %zu has %zu leaves, not 2^%d", l, trees[l]->n_leaves, log_leaves[l]);
        VX_CHECK(trees[l]->cap_height == trees[0]->cap_height && trees[l]->cap_height >= 0 && trees[l]->cap_height <= 16 && trees[l]->cap_height <= log_lde - 4 * (int)NL,
                 "fri queries: cap height %d of layer %zu (one height for all layers, at most log_lde - 4 layers = %d and 16)", trees[l]->cap_height, l, log_lde - 4 * (int)NL);
        VX_CHECK(evals[l]->n >= ((size_t)32 << log_leaves[l]), "fri queries: the values of layer %zu hold %zu words, fewer than 2^%d extension values", l, evals[l]->n, log_leaves[l] + 4);
        evals_d[l] = evals[l]->d, tree_leaves[l] = trees[l]->levels;
    }
    for (size_t i = 0; i < n_queries; ++i) VX_CHECK(index[i] >> log_lde == 0, "fri queries: query %zu has an index outside the LDE", i);
    for (size_t i = 0; i < 2 * NL; ++i) VX_CHECK(betas[i] < glh::P, "fri queries: non-canonical beta word %zu", i);
    // ---- the leaves of every query in every layer and ev_0, gathered on the device; the roots, folded from the caps
    std::vector<uint64_t> leaves(n_queries * NL * 32), ev0(2 * n_queries), roots(4 * NL), lidx(n_queries), got(n_queries * 32);
    for (size_t l = 0; l < NL; ++l) {
        for (size_t i = 0; i < n_queries; ++i) lidx[i] = index[i] >> (4 * (l + 1));
        VX_TRY(vx_fri_leaves_dev(ctx, evals_d[l], log_leaves[l] + 4, 4, lidx.data(), n_queries, got.data()));
        for (size_t i = 0; i < n_queries; ++i) {
            uint64_t* leaf = leaves.data() + (i * NL + l) * 32;
            for (int j = 0; j < 32; ++j) leaf[j] = got[32 * i + j] >= glh::P ? got[32 * i + j] - glh::P : got[32 * i + j];
        }
        const size_t n_cap = (size_t)1 << trees[l]->cap_height;
        std::vector<uint64_t> cap(4 * n_cap);
        VX_HIP(hipMemcpyAsync(cap.data(), trees[l]->levels + trees[l]->total - 4 * n_cap, 4 * n_cap * 8, hipMemcpyDeviceToHost, ctx->stream));
        VX_HIP(vx_wait(ctx));  // also: the trees and the layers are this stream's work, the side contexts read them
        for (uint64_t& w : cap) w = w >= glh::P ? w - glh::P : w;
        vx_cap_fold(cap.data(), trees[l]->cap_height, roots.data() + 4 * l);
    }
    for (size_t i = 0; i < n_queries; ++i) memcpy(ev0.data() + 2 * i, leaves.data() + i * NL * 32 + 2 * (index[i] & 15), 16);
    // ---- the statement, natively: every chain holds and ends in the final polynomial (VX_ERR_STATEMENT names query and layer)
    VX_TRY(vx_fri_fold_check_dev(ctx, log_lde, betas, NL, final_poly, final_len, index, ev0.data(), leaves.data(), n_queries));
    uint64_t stmt[4];
    vx_fri_queries_statement(log_lde, betas, NL, final_poly, final_len, roots.data(), index, ev0.data(), n_queries, stmt);
    // ---- one path and one leaf per (query, layer), duplicates included
    std::vector<uint64_t> tree_of(n_queries * NL), leaf_of(n_queries * NL);
    for (size_t i = 0; i < n_queries; ++i)
        for (size_t l = 0; l < NL; ++l) tree_of[i * NL + l] = l, leaf_of[i * NL + l] = index[i] >> (4 * (l + 1));
    const int log_open = fri_queries_open_log_n(n_queries, log_lde, NL), log_sponge = fri_queries_sponge_log_n(n_queries, NL), log_fold = fri_fold_log_n(n_queries, log_lde, NL);
    // three tables on one bus, in transcript order: the openings and the sponge on side contexts and host threads of their own,
    // the fold on this context
    TableGroup g(ctx, cfg, "fri queries");
    g.add({"openings", VX_AIR_MERKLE_OPEN_SET, log_open, mop::SET_COLS, mop::SET_PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_merkle_open_set_trace_dev(c, trees, NL, tree_of.data(), leaf_of.data(), tree_of.size(), log_open, trace->d, pub));
               vx_merkle_open_set_public(stmt, pub);
               return (int32_t)VX_OK;
           }});
    // (a layer that is not what its tree was built from is refused here: VX_ERR_STATEMENT, "does not hash")
    g.add({"sponge", VX_AIR_LEAF_SPONGE_SET, log_sponge, lsp::SET_COLS, lsp::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
               VX_TRY(vx_leaf_sponge_set_trace_dev(c, evals_d, log_leaves, tree_leaves, NL, tree_of.data(), leaf_of.data(), tree_of.size(), log_sponge, trace->d, pub));
               vx_leaf_sponge_set_public(32, stmt, pub);
               return (int32_t)VX_OK;
           }});
    const int fold = g.add({"fold", VX_AIR_FRI_FOLD, log_fold, ffa::COLS, ffa::PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                                VX_TRY(vx_fri_fold_trace_dev(c, log_lde, betas, NL, 0, index, ev0.data(), leaves.data(), n_queries, log_fold, trace->d, pub));
                                vx_fri_fold_public_digest(log_lde, betas, NL, 0, stmt, pub);
                                return (int32_t)VX_OK;
                            }});
    VX_TRY(g.prove(fold));
    return pack_blob(ctx, "fri queries", VX_FQRY_MAGIC, {(uint64_t)log_lde, NL, n_queries}, {&g.job[0], &g.job[1], &g.job[2]}, blob_out, blob_cap, blob_len);
}
}  // extern "C"
