// Host-side plumbing shared by every prover of "several tables on one logUp bus", implemented in vx_bus.hip: the circuit provers
// and the aggregation provers.  The tables of one statement must use the same lookup challenges, drawn after every trace is
// committed: the rendezvous and the bookkeeping of such a group are bus_meet.h (host-pure); TableGroup below is the group on the
// device -- a prover says which tables there are (TableSpec), which one runs on the caller's context and thread, and in which order
// failures are reported.  What only the aggregation provers share -- the hook of a table alone on its bus, the blob writer, the blob
// formats and the public inputs of their AIRs, which the verifier (vx_verify.hip) rebuilds with the same functions -- is declared
// here as well.
#pragma once
#include <array>
#include <functional>
#include <initializer_list>
#include <vector>

#include "bus_meet.h"
#include "glh_poseidon.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

// the hook of a table that is alone on its bus (the other party is the verifier): the lookup challenges are the shared-challenge
// transcript of this one table's (public inputs, trace cap); `party` is unused
int32_t vx_one_table_hook(void* party, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cw, uint64_t* chal, size_t n_chal);
// one table's context and proof
struct TableJob {
    vx_ctx* c = nullptr;
    std::vector<uint64_t> proof;
    size_t len = 0;
};
// Proves one table into j.proof / j.len: proof bound -> size j.proof -> allocate the n_cols << log_n trace on `c` -> gen ->
// vx_stark_prove_impl with the party's hook -> free the trace.  gen(c, trace, pub) writes the trace and the n_pub public
// inputs and may refuse the statement (vx_fail on `c`); nothing is proven then.
using TableGen = std::function<int32_t(vx_ctx* c, vx_buf* trace, uint64_t* pub)>;
int32_t run_table(vx_ctx* c, TableJob& j, int air_id, int log_n, size_t n_cols, size_t n_pub, const vx_stark_config* cfg, const vx_chal_hook* hook, int consume_trace,
                  const TableGen& gen);
// A table of a group, described once.  Without a `gen` the trace and the public inputs exist before the group proves (rotate's
// epoch-end table): `trace` and `pub` are set by the time TableGroup::prove is called.
struct TableSpec {
    const char* name;  // for messages
    int air_id, log_n;
    size_t n_cols, n_pub;
    int consume_trace;
    TableGen gen;
    vx_buf* trace = nullptr;
    const uint64_t* pub = nullptr;
};
// AIR id and rows of a table: what its proof bound depends on
struct TableShape {
    int air_id, log_n;
};
// *n_words = hdr_words + the vx_stark_proof_bound of every table
int32_t vx_tables_proof_bound(const vx_stark_config* cfg, size_t hdr_words, std::initializer_list<TableShape> tables, size_t* n_words);
int32_t vx_tables_proof_bound(const vx_stark_config* cfg, size_t hdr_words, const TableShape* tables, size_t n_tables, size_t* n_words);
// The tables of one statement on the device, in table order.  prove(): the table `here` (-1: none) is proven on the caller's
// context and thread, every other local table on a host thread of its own and on the next of the chain of side contexts behind
// `ctx`, in table order (every table has a context of its own: own stream, scratch, pool); they meet at their challenge hooks.
// Returns VX_OK when every local proof exists in job[]; otherwise the failure of the first table in `order` (default: `here`,
// then the rest in table order) that failed on its own -- not one released by another's failure -- as "<what>: <its message>" on
// `ctx`.  Leaving the group earlier, by any path, fails its local tables at the rendezvous (the other shards of a sharded proof
// are not left waiting).  Whatever the gens refer to must be declared before the group.
struct TableGroup {
    vx_ctx* ctx;
    const vx_stark_config* cfg;
    const char* what;
    TableSpec spec[BusGroup::MAX];
    TableJob job[BusGroup::MAX];
    vx_chal_hook hook[BusGroup::MAX];
    BusGroup g;
    TableGroup(vx_ctx* ctx, const vx_stark_config* cfg, const char* what) : ctx(ctx), cfg(cfg), what(what) {}
    ~TableGroup() { g.finish(); }
    int add(TableSpec s, int bus = 0, bool local = true);
    int32_t contexts(int here);  // assigns job[k].c (prove does it, unless the caller needed a table's context earlier)
    int32_t prove(int here, std::vector<int> order = {});

   private:
    int32_t run(int k);
    bool have_contexts = false;
};
// An aggregation blob (the formats below): magic, the request words, one length per proof, the proofs.  Sets *blob_len and
// writes the blob, or fails with VX_ERR_BUFSZ ("<what>: the blob needs N words, buffer has M") when blob_out cannot hold it.
int32_t pack_blob(vx_ctx* ctx, const char* what, uint64_t magic, std::initializer_list<uint64_t> request, std::initializer_list<const TableJob*> jobs, uint64_t* blob_out,
                  size_t blob_cap, size_t* blob_len);
// ... for a number of tables known only at run time (vx_stark_openings_prove)
int32_t pack_blob(vx_ctx* ctx, const char* what, uint64_t magic, const uint64_t* request, size_t n_request, const TableJob* const* jobs, size_t n_jobs, uint64_t* blob_out, size_t blob_cap,
                  size_t* blob_len);

// The three tables of a justification -- authority-set commitment (ShaChainAir, sends the chosen signers' keys), Ed25519
// (EdAir) and SHA-512 (Sha512Air) -- added to `g` as the next three parties of `bus`; returns the index of the first.  The prover
// verifies exactly floor(2n/3) + 1 signatures (the first signed ones).  `pre` (may be empty) runs on the commitment's thread before
// anything is proven: the native statement checks whose failure must name the error.  Bit t of `mask`: table t is proven here.
int vx_justification_add(TableGroup& g, const vx_justification* just, std::function<int32_t(vx_ctx*)> pre, int bus = 0, unsigned mask = 7);
// the shapes of the three for n_sig verified signatures (the proof bound assumes the quorum)
std::array<TableShape, 3> vx_justification_shapes(size_t n_authorities, size_t n_sig);
size_t vx_justification_proof_bound(const vx_stark_config* cfg, size_t n_authorities, int32_t* rc);
// verifier side: expected public inputs and AIR ids of the three tables for the request; the counts are read from the
// proofs' own public inputs (ppub_chain[8] authorities, ppub_ed[0] signatures) and must satisfy signed * 3 > authorities * 2
int32_t vx_justification_expect(const uint64_t* ppub_chain, size_t n_chain, const uint64_t* ppub_ed, size_t n_ed, size_t n_s512, const uint8_t authority_set_hash[32],
                                uint64_t authority_set_id, const uint8_t block_hash[32], uint32_t block_number, uint64_t round, uint64_t spub[10], uint64_t epub[2],
                                uint64_t hpub[15], int air[3], char* err, size_t errlen);

// ---- rotate blob (written by vx_rotate_prove in vx_rotate.hip, read by vx_rotate_verify in vx_verify.hip)
static const uint64_t VX_ROT_MAGIC = 0x3354415458525856ULL;  // "VXRXTAT3"
// magic, set id, block, n_new, header hash (4), set hash (4), new set hash (4), proof lengths: header hash, current-set commitment,
// new-set commitment, Ed25519; parent hash (4); SHA-512 proof length, the precommit's round, start_position, epoch-end proof length
static constexpr size_t VX_ROT_HDR = 28;

// ---- Merkle-openings blob (written by vx_merkle_openings_prove in vx_merkle_open_air.hip, read by vx_merkle_openings_verify in
// vx_verify.hip): magic, log2(n_leaves), number of openings, length of the MerkleOpenAir proof that follows
static const uint64_t VX_MOPEN_MAGIC = 0x314e45504f4d5856ULL;  // "VXMOPEN1"
static constexpr size_t VX_MOPEN_HDR = 4;
// ---- Merkle-rows blob (written by vx_merkle_rows_prove in vx_leaf_sponge_air.hip, read by vx_merkle_rows_verify in vx_verify.hip):
// magic, log2(n_leaves), leaf_len, number of openings, lengths of the MerkleOpenAir and the LeafSpongeAir proof that follow
static const uint64_t VX_MROWS_MAGIC = 0x3153574f524d5856ULL;  // "VXMROWS1"
static constexpr size_t VX_MROWS_HDR = 6;
// ---- FRI-fold blob (written by vx_fri_fold_prove in vx_fri_fold_air.hip, read by vx_fri_fold_verify in vx_verify.hip): magic,
// log2 of the inner proof's LDE, fold layers, queries, length of the FriFoldAir proof that follows
static const uint64_t VX_FFOLD_MAGIC = 0x31444c4f46465856ULL;  // "VXFFOLD1"
static constexpr size_t VX_FFOLD_HDR = 5;
// The public inputs of the aggregation AIRs from the claims, prover and verifier alike (each defined beside its AIR's witness).
// MerkleOpenAir: root, depth, the digest of the claims [n_idx][5] = (index, leaf digest); claims == nullptr leaves the digest to
// the caller (vx_merkle_rows_verify, which never sees the leaf digests, takes it from the proof)
void vx_merkle_open_public(const uint64_t root[4], int depth, const uint64_t* claims, size_t n_idx, uint64_t pub[9]);
// LeafSpongeAir: L, B, the tail flags, the digest of the claims [n_idx][1 + leaf_len] = (index, row)
void vx_leaf_sponge_public(size_t leaf_len, const uint64_t* claims, size_t n_idx, uint64_t pub[14]);
// FriFoldAir: from betas [n_layers][2], ev0 [n_queries][2], leaves [n_queries][n_layers][32]
void vx_fri_fold_public(int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries,
                        uint64_t pub[24]);
// ... with a digest the caller states (the statement digest of vx_fri_queries_prove: its verifier holds no leaves)
void vx_fri_fold_public_digest(int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t digest[4], uint64_t pub[24]);


// ---- FRI-queries blob (written by vx_fri_queries_prove in vx_fri_queries.hip, read by vx_fri_queries_verify in vx_verify.hip):
// magic, log2 of the inner proof's LDE, fold layers, queries, lengths of the MerkleOpenSetAir, the LeafSpongeSetAir and the
// FriFoldAir proof that follow
static const uint64_t VX_FQRY_MAGIC = 0x3130595251465856ULL;  // "VXFQRY01"
static constexpr size_t VX_FQRY_HDR = 7;
// The set tables (several trees in one table).  Their public inputs, stated once for prover and verifier: MerkleOpenSetAir has the
// four words of a digest it does not constrain; LeafSpongeSetAir L, B, the tail flags and such a digest.  The digest is the claims
// digest of the set where a table is made alone (vx_*_set_air_trace), the STATEMENT digest in vx_fri_queries_prove.
static constexpr int VX_OPEN_SET_MAX_TREES = 64;
void vx_merkle_open_set_public(const uint64_t digest[4], uint64_t pub[4]);
void vx_leaf_sponge_set_public(size_t leaf_len, const uint64_t digest[4], uint64_t pub[14]);
// the statement of a FRI query phase: hash_n_to_hash_no_pad(log_lde, NL, n_q, betas, final_poly, the NL roots, (index, ev_0) of
// every query) -- everything the verifier puts on the bus is a function of it
void vx_fri_queries_statement(int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len, const uint64_t* roots, const uint64_t* index,
                              const uint64_t* ev0, size_t n_queries, uint64_t digest[4]);
// the witnesses of the set tables on the device (vx_merkle_open_air.hip, vx_leaf_sponge_air.hip) and FriFoldAir's, with its native
// statement check (vx_fri_fold_air.hip), for the circuit prover
int32_t vx_merkle_open_set_trace_dev(vx_ctx* ctx, const vx_tree* const* trees, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx, int log_n,
                                     uint64_t* trace_d, uint64_t pub_out[4]);
// leaves of FRI layers: tree t is the layer evals_d[t] of 2^(log_leaves[t] + 4) extension values in natural order; tree_leaves[t]
// (may be nullptr as a whole): the leaf digests of the tree the leaves must hash to -- VX_ERR_STATEMENT otherwise
int32_t vx_leaf_sponge_set_trace_dev(vx_ctx* ctx, const uint64_t* const* evals_d, const int* log_leaves, const uint64_t* const* tree_leaves, size_t n_trees, const uint64_t* tree_of,
                                     const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, uint64_t pub_out[14]);
int32_t vx_fri_fold_trace_dev(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves,
                              size_t n_queries, int log_n, uint64_t* trace_d, uint64_t pub_out[24]);
// folds every query natively on the host: VX_ERR_STATEMENT on `ctx`, naming query and layer, when a chain does not hold or does
// not end in the final polynomial; VX_ERR_ARG for claims out of range
int32_t vx_fri_fold_check_dev(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len, const uint64_t* index, const uint64_t* ev0,
                              const uint64_t* leaves, size_t n_queries);

// ---- STARK-openings blob (written by vx_stark_openings_prove in vx_stark_groups.hip, read by vx_stark_openings_verify in
// vx_verify.hip): magic, the shape words of the inner proof (log_lde, cm, ca, arity_bits, fold layers, cap_height, queries), the
// number of tables, one length per table, the proofs in bus order (stark_openings_tables, vx_table_shapes.h)
static const uint64_t VX_SOPEN_MAGIC = 0x314e45504f535856ULL;  // "VXSOPEN1"
static constexpr size_t VX_SOPEN_HDR = 9;                       // before the lengths
static constexpr uint64_t VX_SOPEN_TREE0 = 8;                   // main / auxiliary / quotient = TREE0 + 0 / 1 / 2; layer l = l
// the two-to-one fold of a cap of canonical words down to one digest: the root the openings table proves paths to
void vx_cap_fold(const uint64_t* cap, int cap_height, uint64_t root[4]);
// The Merkle side of a vx_stark_prove proof as claims: one per (query, tree), queries outermost in proof order, inside a query the
// order of the query record -- main, auxiliary (ca > 0), quotient, layers 0..NL-1.  Filled by the verifier's own query phase
// (vx_verify.hip) whenever it has a sink (StarkQueries below).
struct StarkOpenings {
    int LN = 0, a = 0, cap_h = 0;
    size_t cm = 0, ca = 0, NL = 0, n_queries = 0;
    std::vector<uint64_t> tree;   // the trees of a query, in record order
    std::vector<uint64_t> caps;   // [tree.size()][4 << cap_h], in that order
    std::vector<uint64_t> index;  // [n_queries]: x_index
    struct Claim {
        uint64_t tree, index;  // index: x_index for the commitment trees, x_index >> a (l + 1) for layer l
        size_t leaf, leaf_len;  // the leaf words: leaves[leaf .. leaf + leaf_len), a layer leaf with its `within` slot filled
        size_t sib;             // where the path's 4 (log_leaves - cap_h) sibling words start in the proof
        int n_sib;              // log_leaves - cap_h of its tree: the levels of the path
    };
    std::vector<Claim> claims;
    std::vector<uint64_t> leaves;
    int log_leaves(uint64_t t) const { return t >= VX_SOPEN_TREE0 ? LN : LN - a * ((int)t + 1); }
    std::array<uint64_t, 7> shape_words() const { return {{(uint64_t)LN, cm, ca, (uint64_t)a, NL, (uint64_t)cap_h, n_queries}}; }
    // the folded root of every tree, [tree.size()][4] in record order: what prover and verifier both call "the roots"
    std::vector<uint64_t> roots() const {
        std::vector<uint64_t> r(4 * tree.size());
        for (size_t k = 0; k < tree.size(); ++k) vx_cap_fold(caps.data() + k * ((size_t)4 << cap_h), cap_h, r.data() + 4 * k);
        return r;
    }
};
// the statement of a proof's openings, the four digest words of every table: hash_n_to_hash_no_pad(the shape words, the folded
// root of every tree in record order, per query the index and the leaf words of every tree in record order).  roots: [tree.size()][4]
void vx_stark_openings_statement(const StarkOpenings& so, const uint64_t* roots, uint64_t digest[4]);
// The witness of the openings tables (MerkleOpenAir, MerkleOpenSetAir) on the device, made by vx_merkle_open_air.hip from one
// description of a request for all its sources.  Without stored pairs (nodes_d == nullptr) the trace kernel reads the trees: their
// node storage holds every node of every path.  From AUTHENTICATION PATHS no tree is in HBM and the levels of a path are a chain:
// vx_merkle_paths_states_dev walks every path once on ctx->stream -- siblings below the cap from `siblings`, above it from the fold
// of the tree's cap --, stores the pair entering every level and waits; *bad_out = the first opening that does not reach its root
// (VX_ERR_STATEMENT), n_idx when all do.  Tree t (< n_trees <= 64) has 2^log_leaves[t] leaves (0: no such tree) and the cap
// caps[t][4 << cap_height]; opening i enters with leaf_dev[i] (4 digest words on the device) when leaf_dev and leaf_dev[i] are
// set, else leaf_digests[4 i ..]; siblings: the 4 (log_leaves - cap_height) words of every opening, one after the other.
// vx_merkle_paths_trace_dev only launches the trace kernel over the witness, on any context of the device.  The witness owns its
// pool block (of the context that made it) and returns it when it goes.
struct MerkleOpenWitness {
    Scratch sc;
    std::vector<uint64_t> tables;  // the host's copy of the uploaded tables: alive until the uploads have been waited for
    uint64_t *upper_d = nullptr, *trees_d = nullptr, *path_d = nullptr, *blk_d = nullptr, *claims_d = nullptr;
    uint64_t *leaf_d = nullptr, *sibp_d = nullptr, *dig_d = nullptr, *sib_d = nullptr, *nodes_d = nullptr, *bad_d = nullptr;  // paths only
    size_t n_idx = 0, n_active = 0;
};
int32_t vx_merkle_paths_states_dev(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                                   const uint64_t* leaf_digests, const uint64_t* const* leaf_dev, const uint64_t* siblings, size_t n_idx, MerkleOpenWitness* w, size_t* bad_out);
int32_t vx_merkle_paths_trace_dev(vx_ctx* c, const MerkleOpenWitness& w, int log_n, uint64_t* trace_d);
// The witness of the sponge tables (LeafSpongeAir, LeafSpongeSetAir) on the device, made by vx_leaf_sponge_air.hip from one
// tree's leaf data, from FRI layers or from ROWS handed over directly: leaf i is then the row rows[i][leaf_len] (host, canonical
// words) of leaf leaf_idx[i] of tree tree_of[i]; all share leaf_len >= 5.  vx_leaf_sponge_rows_states_dev enqueues the chains on
// ctx->stream and leaves digests_d [n_idx][4] for the paths; vx_leaf_sponge_rows_trace_dev only launches the trace kernel.  The
// witness owns its pool block as above.
struct LeafSpongeWitness {
    Scratch sc;
    uint64_t *states_d = nullptr, *idx_d = nullptr, *claims_d = nullptr, *digests_d = nullptr, *set_d = nullptr, *rows_d = nullptr;
    // 1 + the first opening whose digest is not its tree's (~0: none).  The rows form has no tree to compare with (the path the
    // digest enters is the check) and never reads the word.
    uint64_t* bad_d = nullptr;
    size_t n_idx = 0, n_blk = 0, leaf_len = 0;
};
int32_t vx_leaf_sponge_rows_states_dev(vx_ctx* ctx, size_t leaf_len, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* rows, size_t n_idx, LeafSpongeWitness* w);
int32_t vx_leaf_sponge_rows_trace_dev(vx_ctx* c, const LeafSpongeWitness& w, int log_n, uint64_t* trace_d);

// LeafNoopAir (vx_leaf_noop_air.hip): the openings of leaves of at most 4 words, which are their own digest.  Opening i is leaf
// leaf_idx[i] of tree tree_of[i] with leaf_len[i] in 1..4 words, rows[i][4] zero-padded (host, canonical).  Its public inputs are
// the four words of a digest it does not constrain, prover and verifier alike.  vx_leaf_noop_check: the ranges, VX_ERR_ARG on `ctx`;
// vx_leaf_noop_trace_dev uploads the openings and launches the trace kernel on ctx->stream.
void vx_leaf_noop_public(const uint64_t digest[4], uint64_t pub[4]);
int32_t vx_leaf_noop_check(vx_ctx* ctx, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* leaf_len, const uint64_t* rows, size_t n_idx);
int32_t vx_leaf_noop_trace_dev(vx_ctx* ctx, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* leaf_len, const uint64_t* rows, size_t n_idx, int log_n, uint64_t* trace_d);

// ---- FRI-combine blob (written by vx_fri_combine_prove in vx_fri_combine_air.hip, read by vx_fri_combine_verify in vx_verify.hip):
// magic, log2 of the inner proof's LDE, main / auxiliary / quotient columns, queries, length of the FriCombineAir proof that follows
static const uint64_t VX_FCOMB_MAGIC = 0x31424d4f43465856ULL;  // "VXFCOMB1"
static constexpr size_t VX_FCOMB_HDR = 7;
// ---- FRI-combine-fold blob (vx_fri_combine_fold_prove / _verify): magic, log_lde, cm, ca, nq, fold layers, queries, lengths of
// the FriCombineAir and the FriFoldAir proof that follow
static const uint64_t VX_FCFLD_MAGIC = 0x31444c4643465856ULL;  // "VXFCFLD1"
static constexpr size_t VX_FCFLD_HDR = 9;
// What FriCombineAir's statement is made of besides the queries: the inner proof's shape, alpha, zeta and the openings at zeta
// (open_local / open_next [cm + ca][2], open_quot [nq][2]).  The trace domain has 2^(log_lde - rate_bits) rows: zeta' = zeta w_n.
struct FriCombineStmt {
    int log_lde, rate_bits;
    size_t cm, ca, nq;
    const uint64_t *alpha, *zeta, *open_local, *open_next, *open_quot;
};
// ranges and canonical words of the claims (index [n], rows [n][cm + ca + nq], ev0 [n][2]); VX_ERR_ARG on `ctx`
int32_t vx_fri_combine_check_claims(vx_ctx* ctx, const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries);
// alpha^c, zeta', y0, y1: computed once per proof by prover and verifier alike
void vx_fri_combine_reduced(const FriCombineStmt& st, uint64_t alphac[2], uint64_t zetan[2], uint64_t y0[2], uint64_t y1[2]);
// FriCombineAir's public inputs: with the claims digest hash_n_to_hash_no_pad(shape, alpha, zeta, openings, (index, rows, ev_0) of
// every query), or with a digest the caller states (the group's statement digest)
void vx_fri_combine_public(const FriCombineStmt& st, uint64_t tree0, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries, uint64_t pub[22]);
void vx_fri_combine_public_digest(const FriCombineStmt& st, uint64_t tree0, const uint64_t digest[4], uint64_t pub[22]);
// log_lde, rate_bits, cm, ca, nq, n_queries, alpha, zeta, the openings: the head of both digests
void vx_fri_combine_statement_words(const FriCombineStmt& st, size_t n_queries, std::vector<uint64_t>& w);
int32_t vx_fri_combine_trace_dev(vx_ctx* ctx, const FriCombineStmt& st, uint64_t tree0, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries, int log_n,
                                 uint64_t* trace_d, uint64_t pub_out[22]);
// combines every query natively on the host: VX_ERR_STATEMENT on `ctx`, naming the query, when a claimed ev_0 differs or x = zeta
int32_t vx_fri_combine_check_dev(vx_ctx* ctx, const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries);
// the combination natively on the host -> ev0_out [n_queries][2]; VX_ERR_STATEMENT on `ctx` when x = zeta or zeta w_n
int32_t vx_fri_combine_host(vx_ctx* ctx, const FriCombineStmt& st, const uint64_t* index, const uint64_t* rows, size_t n_queries, uint64_t* ev0_out);
// the statement digest of vx_fri_combine_fold_prove: both tables' four digest words
void vx_fri_combine_fold_statement(const FriCombineStmt& st, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len, const uint64_t* index,
                                   const uint64_t* rows, const uint64_t* leaves, size_t n_queries, uint64_t digest[4]);

// ---- STARK-queries blob (written by vx_stark_queries_prove in vx_stark_groups.hip, read by vx_stark_queries_verify in
// vx_verify.hip): magic, the 7 shape words of the inner proof (as VXSOPEN1), the number of tables, one length per table, the proofs
// in bus order (stark_queries_tables, vx_table_shapes.h)
static const uint64_t VX_SQRY_MAGIC = 0x3130595251535856ULL;  // "VXSQRY01"
static constexpr size_t VX_SQRY_HDR = 9;                      // before the lengths
// What the verifier's query phase does with the openings of a proof.  Walked: it walks every path itself (vx_stark_verify).
// Delegated: the paths are left to the tables of a bus group -- none is walked and no sibling word is read.  Deferred: the paths
// are left to a check that runs once the pass has ended (DeferredPaths below) -- none is walked here, but every word of the proof is
// scanned as in Walked: the check will read the siblings.  QueryFree: the whole query phase is left to the tables -- only the
// indices are derived, no word at or behind the query records is read, and the proof may end there.
enum class QueryPhase { Walked, Delegated, Deferred, QueryFree };
// The whole query phase of a vx_stark_prove proof as claims, the ONE sink of the verifier's query phase: the Merkle side (`so`: trees
// 0..7 the layers, 8 / 9 / 10 main / auxiliary / quotient) and the arithmetic side, from one replay of the verifier's code.  Query-free
// only the head is filled: so.claims / so.leaves / rows / leaves / ev0 / ev_last stay empty, so.index holds the derived indices.
struct StarkQueries {
    StarkOpenings so;
    int rate_bits = 0;
    size_t nq = 0;
    uint64_t alpha[2] = {0, 0}, zeta[2] = {0, 0};
    std::vector<uint64_t> openings;  // local [c][2], next [c][2], quotient [nq][2]
    std::vector<uint64_t> betas, final_poly;
    std::vector<uint64_t> rows, leaves, ev0, ev_last;  // [query][c + nq], [query][layer][2 arity] (`within` filled), [query][2]: ev_0, the accepted ev_NL
    FriCombineStmt stmt() const {
        const size_t c = so.cm + so.ca;
        return FriCombineStmt{so.LN, rate_bits, so.cm, so.ca, nq, alpha, zeta, openings.data(), openings.data() + 2 * c, openings.data() + 4 * c};
    }
};
// The openings that passes in the Deferred mode recorded, of one proof or of every table of a blob, as ONE batch: the arguments of
// vx_merkle_check (include/vx.h), every array in the order the walked verifier would have met the openings.
struct MerkleBatch {
    int cap_height = 0;
    std::vector<uint64_t> caps;  // [log_leaves.size()][4 << cap_height]
    std::vector<int> log_leaves;
    std::vector<uint64_t> tree_of, leaf_idx, leaf_len, leaves, siblings;
};
// Checks every opening of a batch: VX_OK with *first_bad = the first one that misses its cap (SIZE_MAX: none), or the code of a
// failure of its own with the reason in err.  glh::merkle_path_ok one after the other (vx_stark_verify_deferred), or one launch of
// k_merkle_check (vx_merkle_check.hip: the _dev verifiers).
using PathChecker = std::function<int32_t(const MerkleBatch&, size_t* first_bad, char* err, size_t errlen)>;
// The deferred form of the host verifiers (vx_verify.hip): a verifier runs in its own order with every proof read in the Deferred
// mode through pass(), which keeps the openings the proof's query phase recorded -- of a pass that stopped inside its query phase,
// those it had met by then.  settle() then has them checked together and gives the answer of the walked verifier: the first
// opening that fails, in the order they were met, wins over the verdict the verifier itself came to -- the walked verifier would
// have stopped there first.
struct DeferredPaths {
    explicit DeferredPaths(PathChecker check) : check(std::move(check)) {}
    // vx_stark_verify_ext's arguments and answer
    int32_t pass(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public, const uint64_t* ext_chal,
                 const uint64_t** apub_out, int* log_n_out, char* err, size_t errlen);
    int32_t settle(int32_t verdict, char* err, size_t errlen);

    PathChecker check;
    MerkleBatch batch;
    enum { TRACE, AUX, QUOT, LAYER };
    struct Opening {
        int kind;  // which tree of its proof
        size_t layer, query;
    };
    std::vector<Opening> opening;  // of every claim of the batch
};
// the checker of the _dev verifiers: the batch through vx_merkle_check, one launch on `ctx` (vx_merkle_check.hip)
PathChecker vx_merkle_check_paths(vx_ctx* ctx);
// verifies `proof` as vx_stark_verify_ext does with its query phase in `mode`, and fills *out
int32_t vx_stark_queries_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                const uint64_t* ext_chal, QueryPhase mode, StarkQueries* out, char* err, size_t errlen);
// ... delegated, for the openings group: VX_ERR_ARG for more than 8 fold layers
int32_t vx_stark_openings_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                                 const uint64_t* ext_chal, StarkQueries* out, char* err, size_t errlen);
// the statement of a proof's query phase, the four digest words of every table: hash_n_to_hash_no_pad(the 7 shape words, alpha, zeta,
// the openings local / next / quotient, betas, the final polynomial, the folded root of every tree in record order, the index of
// every query).  No row word and no leaf word: they are in committed traces.  roots: [so.tree.size()][4]
void vx_stark_queries_statement(const StarkQueries& sq, const uint64_t* roots, uint64_t digest[4]);

// The Merkle side of the proof-sourced group prover (every level; defined in vx_stark_groups.hip): everything its first
// 1 + n_sponge tables read, gathered from the claims and the proof that carries the paths.  It holds pool blocks of `ctx` until the
// group has proven, so it is declared before the TableGroup.
struct StarkMerkleSide {
    static constexpr int N_TREE_IDS = (int)VX_SOPEN_TREE0 + 3;
    // sponge_len: the leaf lengths of the n_sponge (<= 3) sponge tables, in table order (vx_table_shapes.h)
    StarkMerkleSide(vx_ctx* ctx, const char* what, const StarkOpenings& so, const uint64_t* proof, const size_t* sponge_len, int n_sponge);
    // the sponge chains of every leaf longer than 4 words, one launch per length (their digests enter the paths on the device),
    // then every path walked once: "<what>: query Q: the path of ... does not reach the root of its tree" (VX_ERR_STATEMENT) otherwise
    int32_t launch();
    // the openings table and the sponge tables as the next 1 + n_sponge tables of `g`, with ts.log_n[k] rows (log2) and the public
    // inputs of stark_table_public (ts, sq and stmt outlive the group); returns the index of the openings table
    int add_tables(TableGroup& g, const StarkGroupTables& ts, const StarkQueries& sq, const uint64_t* stmt);

    vx_ctx* ctx;
    const char* what;  // the group's name in messages
    const StarkOpenings& so;
    int n_sponge;
    size_t sponge_len[3] = {0, 0, 0};
    MerkleOpenWitness paths;
    LeafSpongeWitness sponge[3];
    int log_leaves[N_TREE_IDS] = {0};
    std::vector<uint64_t> caps, roots;                            // [N_TREE_IDS][4 << cap_h] by tree id; [so.tree.size()][4] in record order
    std::vector<uint64_t> tree_of, leaf_idx, leaf_dig, sibs;      // per claim; leaf_dig: a row of at most 4 words is its own digest, zero-padded
    std::vector<const uint64_t*> leaf_dev;                        // per claim: where the sponge leaves its digest (nullptr: leaf_dig)
    std::vector<uint64_t> s_tree[3], s_idx[3], s_rows[3];         // per sponge table: its openings as rows
    std::vector<size_t> s_who[3];                                 // ... and which claims they are
    std::vector<uint64_t> n_tree, n_idx, n_len, n_rows;           // the openings of the leaves of at most 4 words, rows [.][4] (LeafNoopAir's)
};

// ---- STARK-transcripts blob (written by vx_stark_transcripts_prove in vx_transcript_air.hip, read by vx_stark_transcripts_verify in
// vx_verify.hip): magic, the request -- n chains, then per chain n_obs, n_chal and the n_chal claimed challenges as (absorbed, value)
// --, the length of the TranscriptAir proof that follows
static const uint64_t VX_STRN_MAGIC = 0x31304e5254535856ULL;  // "VXSTRN01"
// One chain of TranscriptAir as claims: the words its transcript absorbs, in order, and every challenge it yields as (words absorbed
// when it was drawn, value).  The prover takes them from a glh::TranscriptRecord, the verifier from its own replay over the claimed
// challenger (the words) and from the blob (the challenges).
struct TranscriptClaim {
    const uint64_t* words;
    size_t n_obs;
    const uint64_t* chal;  // [n_chal][2]
    size_t n_chal;
};
// the statement of a group of transcripts, TranscriptAir's four digest words, prover and verifier alike: hash_n_to_hash_no_pad(n, per
// chain n_obs and n_chal, per chain the observed words, per chain (absorbed, value) of every challenge)
void vx_stark_transcripts_statement(const TranscriptClaim* chains, size_t n, uint64_t digest[4]);
void vx_transcript_public(const uint64_t digest[4], uint64_t pub[4]);
// The witness of TranscriptAir on the device (vx_transcript_air.hip): chain c is the record of a transcript -- words, block plan,
// challenges -- made by the ONE challenger (glh::RecordingChallenger).  Uploads the words and the plan, walks every chain
// (k_transcript_states), writes the trace and, when chal_out is set, hands back the challenges the DEVICE drew, chain after chain.
int32_t vx_transcript_trace_dev(vx_ctx* ctx, const glh::TranscriptRecord* chains, size_t n_chains, int log_n, uint64_t* trace_d, uint64_t* chal_out);
// verifies `proof` as vx_stark_verify_ext does over the recording challenger and hands out what its transcript did: the whole proof
// (the query phase is walked) or its head alone (the indices are derived, no record is read)
int32_t vx_stark_transcript_record(const vx_stark_config* cfg, const uint64_t* proof, size_t len, const uint64_t* ext_chal, glh::TranscriptRecord* out, char* err, size_t errlen);

// ---- STARK-inner blob (written by vx_stark_inner_prove in vx_stark_groups.hip, read by vx_stark_inner_verify in vx_verify.hip): magic,
// the 7 shape words of the inner proof (as VXSQRY01), the number of tables, n_obs, n_chal, the n_chal claimed challenges as
// (absorbed, value), one length per table, the proofs in bus order (stark_inner_tables, vx_table_shapes.h)
static const uint64_t VX_SINR_MAGIC = 0x3130524e49535856ULL;  // "VXSINR01"
static constexpr size_t VX_SINR_HDR = 11;                     // before the claims
// The ONE replay of the prover's side: the verifier's code over the recording challenger with the paths delegated -> the claims of
// the query phase and what the transcript did.  head_ok: a proof that ends at its head is read query-free (the proof bound).
int32_t vx_stark_inner_replay(const vx_stark_config* cfg, const uint64_t* proof, size_t len, const uint64_t* ext_chal, bool head_ok, StarkQueries* sq, glh::TranscriptRecord* rec, char* err,
                              size_t errlen);
// the statement of an inner proof, the four digest words of every table of its group, prover and verifier alike:
// hash_n_to_hash_no_pad(the 7 shape words, n_obs, n_chal, the observed words, (absorbed, value) of every challenge).  Everything the
// query-phase digest held is a function of these words: alpha, zeta, betas and indices are claimed challenges, the openings, the
// final polynomial and the caps (hence the folded roots) are observed words.
void vx_stark_inner_statement(const std::array<uint64_t, 7>& shape, const TranscriptClaim& chain, uint64_t digest[4]);

// ---- The three proof-sourced groups as LEVELS of one group (StarkLevel, vx_table_shapes.h): what a level fixes besides its table
// list, stated once for the one prover body (vx_stark_groups.hip) and the one verifier body (vx_verify.hip).
struct StarkLevelInfo {
    uint64_t magic;
    size_t hdr;              // words before the claims (Inner) or the lengths
    const char* name;        // "<name>: ..." in messages
    const char* blob_name;   // "bad <blob_name> blob"
    const char* no_group;    // the proof's shape has no group of this level
    const char* unbalanced;  // the bus of the group does not close against the verifier's messages
};
static inline const StarkLevelInfo& stark_level(StarkLevel level) {
    static const StarkLevelInfo LEVELS[3] = {
        {VX_SOPEN_MAGIC, VX_SOPEN_HDR, "stark openings", "stark-openings",
         "stark openings: the proof's shape has no openings group (cap height above 16, a tree without a level, or a table of more than 2^26 rows)",
         "the openings the tables prove are not the ones of this proof (the lookup bus does not balance)"},
        {VX_SQRY_MAGIC, VX_SQRY_HDR, "stark queries", "stark-queries",
         "stark queries: the proof's shape has no query-phase group (no fold layer or more than 8, no index bit left, cap height above 16, or a table of more than 2^26 rows)",
         "the query phase the tables prove is not the one of this proof (the lookup bus does not balance)"},
        {VX_SINR_MAGIC, VX_SINR_HDR, "stark inner", "stark-inner",
         "stark inner: the proof's shape has no query-phase group (no fold layer or more than 8, no index bit left, cap height above 16, or a table of more than 2^26 rows)",
         "the query phase and the transcript the tables prove are not the ones of this proof and these claims (the lookup bus does not balance)"},
    };
    return LEVELS[(int)level];
}
// The request words of a level's blob, between the magic and the per-table lengths, for the writer (pack_blob) and the reader
// (read_blob): the 7 shape words and the table count; Inner: then n_obs, n_chal and the claims of its one chain.
static inline std::vector<uint64_t> stark_group_request(StarkLevel level, const StarkOpenings& so, int n_tables, const TranscriptClaim& chain) {
    const std::array<uint64_t, 7> sw = so.shape_words();
    std::vector<uint64_t> r(sw.begin(), sw.end());
    r.push_back((uint64_t)n_tables);
    if (level == StarkLevel::Inner) {
        r.push_back(chain.n_obs), r.push_back(chain.n_chal);
        r.insert(r.end(), chain.chal, chain.chal + 2 * chain.n_chal);
    }
    return r;
}
// The statement digest of a level, the four digest words of every table (the three functions above: their word lists are protocol).
// roots: so.roots(); chain: Inner only.
void stark_group_statement(StarkLevel level, const StarkQueries& sq, const uint64_t* roots, const TranscriptClaim& chain, uint64_t digest[4]);
// The public inputs of table k of a group, prover (after its trace) and verifier (what it expects) alike: writes them to `pub` and
// returns their count, at most VX_STARK_TABLE_MAX_PUB.
static constexpr size_t VX_STARK_TABLE_MAX_PUB = 24;
size_t stark_table_public(const StarkGroupTables& ts, int k, const StarkQueries& sq, const uint64_t stmt[4], uint64_t* pub);

// ---- bus-group blob (written by vx_bus_group_prove in vx_bus_group.hip, read by vx_bus_group_verify in vx_verify.hip): magic, the
// number of tables, one length per proof, the proofs in bus order.  No AIR id: registered ids are per process, the verifier states its own.
static const uint64_t VX_BGRP_MAGIC = 0x3130505247425856ULL;  // "VXBGRP01"
static constexpr size_t VX_BGRP_HDR = 2;                      // before the lengths
// What a generic group needs to know of an AIR, compiled or registered (vx_verify.hip: the host file holds both registries)
struct AirProgram;
struct BusAirShape {
    int cols = 0, pub = 0, aux = 0, chal = 0, auxpub = 0;
    const AirProgram* prog = nullptr;  // a registered program
};
bool vx_air_bus_shape(int air_id, BusAirShape* out);
// The admission rules of a generic group, stated once for bound, prover, check and verifier: 1 .. VX_BUS_GROUP_MAX_TABLES tables, every
// one a known AIR with a logUp round of 4 challenges and one published total and at most BusMeet::MAX_PUB public inputs (n_public
// may be nullptr: not stated).  VX_ERR_ARG with the reason, naming the table.  shapes (optional): [n]
int32_t vx_bus_group_admit(const int32_t* air_ids, const size_t* n_public, size_t n, BusAirShape* shapes, char* err, size_t errlen);
// the outside messages of a generic group: canonical words, tags below 2^16.  `code` is what a refusal returns (the prover's
// VX_ERR_ARG, the verifier's VX_ERR_STATEMENT)
int32_t vx_bus_outside_ok(const uint64_t* outside, size_t n_outside, int32_t code, char* err, size_t errlen);
// Does the bus of these proofs close against the outside messages?  The published totals x rows under the proofs' shared challenges
// plus sum m / D -- nothing is verified.  VX_ERR_STATEMENT with the reason when it does not (or a proof is too short to read).
int32_t vx_bus_group_closes(const vx_stark_config* cfg, const uint64_t* const* proofs, const size_t* lens, size_t n, const uint64_t* outside, size_t n_outside, char* err, size_t errlen);

static constexpr uint32_t VX_MAX_HEADER_SIZE = 35840;  // consts.rs:16
static inline void be_limbs(const uint8_t h[32], uint64_t out[8]) {
    for (int j = 0; j < 8; ++j)
        out[j] = ((uint64_t)h[4 * j] << 24) | ((uint64_t)h[4 * j + 1] << 16) | ((uint64_t)h[4 * j + 2] << 8) | h[4 * j + 3];
}
