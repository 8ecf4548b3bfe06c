// Rows (log2) and AIR id of every table of the circuits as a function of the request -- stated once, for the provers and the host
// verifier (vx_verify.hip): that both sides size a table the same way is a soundness condition.  Host-only inline functions, no
// device code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "stark_proof.h"
#include "vx_internal.h"

// BlakeChainAir (hash chain / header hash): 16 rows per compression, at least one copy of the 2^16-row XOR tables
// (blk::TABLE_LOG in air_blake.cuh; vx_verify.hip sees both and asserts that they agree)
constexpr int VX_BLAKE_TABLE_LOG = 16;
static inline int blake_log_n(size_t chunks) {
    int log_n = VX_BLAKE_TABLE_LOG;
    while (((size_t)1 << log_n) < 16 * chunks) ++log_n;
    return log_n;
}
// ShaChainAir (authority-set commitment): 64 rows per SHA-256 compression, 2n - 1 compressions for n keys
static inline int sha_log_n(size_t n_keys) {
    int log_n = 6;
    while (((size_t)1 << log_n) < 64 * (2 * n_keys - 1)) ++log_n;
    return log_n;
}
// ShaTreeAir (the two Merkle trees): one AIR per supported max_headers (0 = none), 256 rows per leaf
static inline int tree_air_id(uint32_t max_headers) { return max_headers == 256 ? 7 : max_headers == 512 ? 8 : max_headers == 16 ? 9 : 0; }
static inline int tree_log_n(uint32_t max_headers) {
    int l = 8;
    while ((1u << (l - 8)) < max_headers) ++l;
    return l;
}
// the EdDSA tables by the number of signatures they verify: 256 rows per signature (one slot stays idle: 255 of 2^16 / 256) / 160 rows per hash
// (SLOT_ROWS in air_sha512.cuh, no idle slot needed: 6 = floor(2^10 / 160), 204 = floor(2^15 / 160)).
// The prover needs floor(2n/3) + 1 of the n authorities (justification.rs:164-186), so it verifies exactly that many.
static inline size_t sig_quorum(size_t n_auth) { return 2 * n_auth / 3 + 1; }
static inline int ed_log_n(size_t n_sig) { return n_sig <= 255 ? 16 : 17; }
static inline int ed_air_id(size_t n_sig) { return n_sig <= 255 ? VX_AIR_ED25519_16 : VX_AIR_ED25519; }
static inline int s512_log_n(size_t n_sig) { return n_sig <= 6 ? 10 : n_sig <= 204 ? 15 : 16; }
static inline int s512_air_id(size_t n_sig) { return n_sig <= 6 ? VX_AIR_SHA512_10 : n_sig <= 204 ? VX_AIR_SHA512_15 : VX_AIR_SHA512; }
// the aggregation tables: the smallest power of two that holds the request (the provers refuse more than 2^26 rows)
static inline int ceil_log2(size_t x) {
    int l = 0;
    while (((size_t)1 << l) < x) ++l;
    return l;
}
// MerkleOpenAir: one 32-row block per level of each of the n_idx paths (>= 5: n_idx, depth >= 1)
static inline int vx_merkle_open_log_n(size_t n_idx, int depth) { return ceil_log2(32 * n_idx * (size_t)depth); }
// LeafSpongeAir: one 32-row block per 8 words of each of the n_idx rows (>= 5)
static inline size_t sponge_blocks(size_t leaf_len) { return (leaf_len + 7) / 8; }
static inline int leaf_sponge_log_n(size_t n_idx, size_t leaf_len) { return ceil_log2(32 * n_idx * sponge_blocks(leaf_len)); }
// FriFoldAir: NL fold rows and log_lde - 4 NL bit rows per query, at least 2^5 rows
static inline int fri_fold_log_n(size_t n_queries, int log_lde, size_t n_layers) {
    const int l = ceil_log2(n_queries * (size_t)(log_lde - 3 * (int)n_layers));
    return l < 5 ? 5 : l;
}
// The three tables of a FRI query phase (vx_fri_queries_prove / vx_fri_queries_verify): n_layers layer trees of depth
// log_lde - 4 (l + 1), every leaf 32 words.  MerkleOpenSetAir: one path per (query, layer); LeafSpongeSetAir: one leaf of four
// blocks per (query, layer); FriFoldAir as above
static inline int fri_queries_open_log_n(size_t n_queries, int log_lde, size_t n_layers) {
    size_t levels = 0;
    for (size_t l = 0; l < n_layers; ++l) levels += (size_t)(log_lde - 4 * ((int)l + 1));
    return ceil_log2(32 * n_queries * levels);
}
static inline int fri_queries_sponge_log_n(size_t n_queries, size_t n_layers) { return ceil_log2(32 * n_queries * n_layers * 4); }
// FriCombineAir: cm + ca + nq absorb rows and log_lde bit rows per query, at least 2^5 rows
static inline int fri_combine_log_n(size_t n_queries, int log_lde, size_t cm, size_t ca, size_t nq) {
    const int l = ceil_log2(n_queries * (cm + ca + nq + (size_t)log_lde));
    return l < 5 ? 5 : l;
}
// LeafNoopAir: one row per opening of a leaf of at most 4 words, at least 2^5 rows
static inline int leaf_noop_log_n(size_t n_idx) {
    const int l = ceil_log2(n_idx);
    return l < 5 ? 5 : l;
}
// The tables of a STARK proof's Merkle openings (vx_stark_openings_prove / vx_stark_openings_verify), in bus order: the openings
// table (MerkleOpenSetAir, one path per (query, tree): main, auxiliary when ca > 0, quotient, the NL layer trees), then one
// LeafSpongeSetAir table per distinct leaf length above 4 among {cm, ca, 2 2^a}, by ascending length (a row of at most 4 words is
// its own digest: the quotient rows, and any other tree that short, have no sponge).  Rows: 32 per level of every path, 32 per 8
// words of every leaf, each table at the smallest log_n >= 5.  false: a tree without a level, more than 8 layers, or a table of
// more than 2^26 rows.
// The tables of such a group: the openings table, n_sponge sponge tables and, in the query-phase group, three more; the inner-proof
// group (stark_inner_tables below) has the transcript table behind them.
struct StarkGroupTables {
    static constexpr int MAX = 8, MAX_SPONGE = 3;  // Inner with three leaf lengths above 4
    int n = 0, n_sponge = 0;
    int air[MAX], log_n[MAX];
    size_t leaf_len[MAX];  // of the sponge tables, 0 elsewhere
    size_t noop_per_query = 0;  // query-phase group
};
static inline bool stark_openings_tables(int LN, size_t cm, size_t ca, int a, size_t NL, size_t n_queries, StarkGroupTables* t) {
    if (LN < 1 || LN > 40 || a < 1 || a > 5 || NL > 8 || n_queries < 1 || n_queries > ((size_t)1 << 20) || cm < 1 || cm > ((size_t)1 << 20) || ca > ((size_t)1 << 20)) return false;
    if (NL && (int)NL * a >= LN) return false;
    size_t levels = (size_t)LN * (ca ? 3 : 2);
    for (size_t l = 0; l < NL; ++l) levels += (size_t)(LN - a * ((int)l + 1));
    const size_t lens[3] = {cm, ca, NL ? (size_t)2 << a : 0}, per_query[3] = {1, 1, NL};
    t->n = 1, t->air[0] = VX_AIR_MERKLE_OPEN_SET, t->leaf_len[0] = 0;
    t->log_n[0] = ceil_log2(32 * n_queries * levels);
    for (;;) {  // the next length above the last one taken
        size_t next = 0;
        for (size_t L : lens)
            if (L > 4 && L > t->leaf_len[t->n - 1] && (!next || L < next)) next = L;
        if (!next) break;
        size_t leaves = 0;
        for (int k = 0; k < 3; ++k)
            if (lens[k] == next) leaves += per_query[k];
        t->air[t->n] = VX_AIR_LEAF_SPONGE_SET, t->leaf_len[t->n] = next, t->log_n[t->n] = ceil_log2(32 * n_queries * leaves * sponge_blocks(next));
        ++t->n;
    }
    t->n_sponge = t->n - 1;
    for (int k = 0; k < t->n; ++k) {
        if (t->log_n[k] < 5) t->log_n[k] = 5;
        if (t->log_n[k] > 26) return false;
    }
    return true;
}
// The tables of a STARK proof's whole query phase (vx_stark_queries_prove / vx_stark_queries_verify), in bus order: the tables of
// stark_openings_tables (FriFoldAir needs a = 4 and at least one layer: the layer leaves have 32 words), then LeafNoopAir (one row
// per opening of a leaf of at most 4 words: the quotient tree always, main and auxiliary when that narrow), FriCombineAir and
// FriFoldAir.  The tables are proven under the configuration of the inner proof, and a FRI plan can overshoot: with arity 4,
// final_poly_bits 0 and cap height 0 a table of 2^7 rows would be folded twice, below degree one (plonky2's ConstantArityBits
// asserts there) -- no final polynomial is left and no proof of that size exists.  Such a table is proven at the next size that
// has a plan (its rows behind the claims are idle), prover and proof bound alike; the verifier reads a table's size from its proof.
// false: what stark_openings_tables refuses, a != 4, no layer, no index bit left, or a table of more than 2^26 rows.
static inline bool fri_plan_ok(int log_n, const vx_stark_config& cfg) {
    int d = log_n;
    for (int a : stark_proof::fri_arity_plan(log_n, cfg)) d -= a;
    return d >= 0;
}
static inline bool stark_queries_tables(int LN, size_t cm, size_t ca, int a, size_t NL, size_t n_queries, const vx_stark_config& cfg, StarkGroupTables* t) {
    if (a != 4 || NL < 1 || LN - 4 * (int)NL < 1 || !stark_openings_tables(LN, cm, ca, a, NL, n_queries, t)) return false;
    t->noop_per_query = 1 + (cm <= 4) + (ca && ca <= 4);
    const int extra_air[3] = {VX_AIR_LEAF_NOOP, VX_AIR_FRI_COMBINE, VX_AIR_FRI_FOLD};
    const int extra_log[3] = {leaf_noop_log_n(n_queries * t->noop_per_query), fri_combine_log_n(n_queries, LN, cm, ca, 4), fri_fold_log_n(n_queries, LN, NL)};
    for (int k = 0; k < 3; ++k) {
        if (extra_log[k] > 26) return false;
        t->air[t->n] = extra_air[k], t->log_n[t->n] = extra_log[k], t->leaf_len[t->n] = 0, ++t->n;
    }
    for (int k = 0; k < t->n; ++k) {
        while (t->log_n[k] <= 26 && !fri_plan_ok(t->log_n[k], cfg)) ++t->log_n[k];
        if (t->log_n[k] > 26) return false;
    }
    return true;
}
// TranscriptAir (vx_stark_transcripts_prove): one 32-row block per duplex of every chain, at least 2^5 rows, proven at the next size
// that has a FRI plan under the configuration (as above; the rows behind the chains are idle).  Above 26: the callers refuse.
static inline int transcript_log_n(size_t blocks, const vx_stark_config& cfg) {
    int l = ceil_log2(32 * blocks);
    if (l < 5) l = 5;
    while (l <= 26 && !fri_plan_ok(l, cfg)) ++l;
    return l;
}
// The tables of a STARK proof's query phase AND transcript on one bus (vx_stark_inner_prove / vx_stark_inner_verify), in bus order: the
// tables of stark_queries_tables, then TranscriptAir with the one chain of `blocks` duplexes.  false: what stark_queries_tables
// refuses, or a transcript table of more than 2^26 rows.
static inline bool stark_inner_tables(int LN, size_t cm, size_t ca, int a, size_t NL, size_t n_queries, size_t blocks, const vx_stark_config& cfg, StarkGroupTables* t) {
    if (!stark_queries_tables(LN, cm, ca, a, NL, n_queries, cfg, t)) return false;
    const int log_n = transcript_log_n(blocks, cfg);
    if (log_n > 26) return false;
    t->air[t->n] = VX_AIR_TRANSCRIPT, t->log_n[t->n] = log_n, t->leaf_len[t->n] = 0, ++t->n;
    return true;
}
// The three groups nest, and so do their table lists: a LEVEL names how much of a proof one bus proves.  Everything else a level
// fixes -- magic, header, names, refusal texts -- is stark_level in vx_bus.h; callers reach the lists above through here.  `blocks`:
// the duplexes of the transcript chain (Inner; the verifier states 0: it reads a table's rows from its proof).
enum class StarkLevel { Openings, Queries, Inner };
static inline bool stark_level_tables(StarkLevel level, int LN, size_t cm, size_t ca, int a, size_t NL, size_t n_queries, size_t blocks, const vx_stark_config& cfg, StarkGroupTables* t) {
    return level == StarkLevel::Openings  ? stark_openings_tables(LN, cm, ca, a, NL, n_queries, t)
           : level == StarkLevel::Queries ? stark_queries_tables(LN, cm, ca, a, NL, n_queries, cfg, t)
                                          : stark_inner_tables(LN, cm, ca, a, NL, n_queries, blocks, cfg, t);
}
