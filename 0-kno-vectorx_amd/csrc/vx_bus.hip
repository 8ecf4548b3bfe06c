// Implementation of vx_bus.h: the group of "tables on one bus" on the device (TableGroup: contexts, threads, traces, proofs and
// the one rule for which failure the caller sees; the rendezvous itself is bus_meet.cpp), the runner of one table, the three
// tables of a justification, and what the aggregation provers share: the hook of a table alone on its bus, the proof bound of a
// list of tables and the writer of their blobs.  Host code only: the kernels of every table live with their AIR (vx_*_air.hip).
#include <string.h>

#include <memory>

#include "vx_bus.h"
#include "vx_table_shapes.h"

int32_t vx_one_table_hook(void*, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cw, uint64_t* chal, size_t n_chal) {
    vx_shared_challenges_n(&pub, &n_pub, &cap, 1, cw, chal, n_chal);
    return VX_OK;
}

int32_t vx_tables_proof_bound(const vx_stark_config* cfg, size_t hdr_words, const TableShape* tables, size_t n_tables, size_t* n_words) {
    size_t total = hdr_words;
    for (size_t k = 0; k < n_tables; ++k) {
        size_t w = 0;
        VX_TRY(vx_stark_proof_bound(tables[k].air_id, cfg, tables[k].log_n, &w));
        total += w;
    }
    *n_words = total;
    return VX_OK;
}
int32_t vx_tables_proof_bound(const vx_stark_config* cfg, size_t hdr_words, std::initializer_list<TableShape> tables, size_t* n_words) {
    return vx_tables_proof_bound(cfg, hdr_words, tables.begin(), tables.size(), n_words);
}
std::array<TableShape, 3> vx_justification_shapes(size_t n_authorities, size_t n_sig) {
    return {{{VX_AIR_SHA_CHAIN, sha_log_n(n_authorities)}, {ed_air_id(n_sig), ed_log_n(n_sig)}, {s512_air_id(n_sig), s512_log_n(n_sig)}}};
}
size_t vx_justification_proof_bound(const vx_stark_config* cfg, size_t n_authorities, int32_t* rc_out) {
    const auto sh = vx_justification_shapes(n_authorities, sig_quorum(n_authorities));
    size_t w = 0;
    *rc_out = vx_tables_proof_bound(cfg, 0, {sh[0], sh[1], sh[2]}, &w);
    return w;
}

// sizes j.proof for a proof of this shape
static int32_t size_proof(TableJob& j, int air_id, int log_n, const vx_stark_config* cfg) {
    size_t bound = 0;
    VX_TRY(vx_stark_proof_bound(air_id, cfg, log_n, &bound));
    j.proof.resize(bound);
    return VX_OK;
}
int32_t run_table(vx_ctx* c, TableJob& j, int air_id, int log_n, size_t n_cols, size_t n_pub, const vx_stark_config* cfg, const vx_chal_hook* hook, int consume_trace,
                  const TableGen& gen) {
    VX_TRY(size_proof(j, air_id, log_n, cfg));
    vx_buf* trace = nullptr;
    VX_TRY(vx_alloc(c, n_cols << log_n, &trace));
    uint64_t pub[BusMeet::MAX_PUB];
    int32_t r = gen(c, trace, pub);
    if (r == VX_OK) r = vx_stark_prove_impl(c, air_id, cfg, trace->d, trace->n, consume_trace, log_n, pub, n_pub, j.proof.data(), j.proof.size(), &j.len, hook);
    (void)vx_free(c, trace);
    return r;
}
int TableGroup::add(TableSpec s, int bus, bool local) {
    const int k = g.add(bus, local);
    spec[k] = std::move(s);
    hook[k] = {vx_bus_hook, &g.t[k].party};
    return k;
}
int32_t TableGroup::contexts(int here) {
    if (have_contexts) return VX_OK;
    vx_ctx* c = ctx;
    for (int k = 0; k < g.n; ++k)
        if (g.local(k)) job[k].c = k == here ? ctx : (c = c ? vx_side_ctx(c) : nullptr);
    VX_CHECK(c, "%s: no side context for every table (the provers meet at their challenge hooks, each on a context of its own)", what);
    have_contexts = true;
    return VX_OK;
}
int32_t TableGroup::run(int k) {
    const TableSpec& s = spec[k];
    TableJob& j = job[k];
    if (s.gen) return run_table(j.c, j, s.air_id, s.log_n, s.n_cols, s.n_pub, cfg, &hook[k], s.consume_trace, s.gen);
    VX_TRY(size_proof(j, s.air_id, s.log_n, cfg));
    return vx_stark_prove_impl(j.c, s.air_id, cfg, s.trace->d, s.trace->n, s.consume_trace, s.log_n, s.pub, s.n_pub, j.proof.data(), j.proof.size(), &j.len, &hook[k]);
}
int32_t TableGroup::prove(int here, std::vector<int> order) {
    VX_TRY(contexts(here));
    for (int k = 0; k < g.n; ++k)
        if (g.local(k) && k != here) {
            job[k].c->err.clear();  // (a side context outlives the call: whatever it says afterwards is this table's)
            g.start(k, [this, k] {
                (void)hipSetDevice(job[k].c->device);
                return run(k);
            });
        }
    if (here >= 0) g.run_here(here, [&] { return run(here); });
    g.finish();
    if (order.empty()) {
        if (here >= 0) order.push_back(here);
        for (int k = 0; k < g.n; ++k)
            if (k != here) order.push_back(k);
    }
    int who = -1;
    const int32_t rc = g.first_error(order, &who);
    if (rc == VX_OK || (who >= 0 && who == here)) return rc;  // (the table proven here has left its message on `ctx`)
    if (who < 0) return vx_fail(ctx, rc, "%s: %s", what, BusGroup::ALL_RELEASED);
    const char* msg = vx_last_error(job[who].c);
    if (!msg[0]) return vx_fail(ctx, rc, "%s: the %s table failed", what, spec[who].name);
    if (strncmp(msg, what, strlen(what)) == 0) return vx_fail(ctx, rc, "%s", msg);  // (it names the prover already)
    return vx_fail(ctx, rc, "%s: %s", what, msg);
}
int32_t pack_blob(vx_ctx* ctx, const char* what, uint64_t magic, const uint64_t* request, size_t n_request, const TableJob* const* jobs, size_t n_jobs, uint64_t* blob_out, size_t blob_cap,
                  size_t* blob_len) {
    size_t total = 1 + n_request + n_jobs;
    for (size_t k = 0; k < n_jobs; ++k) total += jobs[k]->len;
    *blob_len = total;
    if (!blob_out || blob_cap < total) return vx_fail(ctx, VX_ERR_BUFSZ, "%s: the blob needs %zu words, buffer has %zu", what, total, blob_cap);
    uint64_t* w = blob_out;
    *w++ = magic;
    for (size_t k = 0; k < n_request; ++k) *w++ = request[k];
    for (size_t k = 0; k < n_jobs; ++k) *w++ = jobs[k]->len;
    for (size_t k = 0; k < n_jobs; ++k) memcpy(w, jobs[k]->proof.data(), jobs[k]->len * 8), w += jobs[k]->len;
    return VX_OK;
}
int32_t pack_blob(vx_ctx* ctx, const char* what, uint64_t magic, std::initializer_list<uint64_t> request, std::initializer_list<const TableJob*> jobs, uint64_t* blob_out,
                  size_t blob_cap, size_t* blob_len) {
    return pack_blob(ctx, what, magic, request.begin(), request.size(), jobs.begin(), jobs.size(), blob_out, blob_cap, blob_len);
}

int vx_justification_add(TableGroup& g, const vx_justification* just, std::function<int32_t(vx_ctx*)> pre, int bus, unsigned mask) {
    // the signatures the proof verifies: the first floor(2n/3) + 1 signed authorities (more would only cost rows); when fewer
    // signed, all of them -- the native threshold check refuses the justification before anything is proven
    const size_t n_auth = just->num_authorities;
    auto chosen = std::make_shared<std::vector<uint8_t>>(n_auth, 0);  // (shared by the gens of the three tables)
    size_t n_sig = 0;
    for (size_t i = 0; i < n_auth && n_sig < sig_quorum(n_auth); ++i)
        if (just->validator_signed[i]) (*chosen)[i] = 1, ++n_sig;
    const auto sh = vx_justification_shapes(n_auth, n_sig);
    const int sl = sh[0].log_n, el = sh[1].log_n, hl = sh[2].log_n;
    const int first = g.add({"authority-set commitment", sh[0].air_id, sl, VX_SHA_AIR_COLS, 10, 0,
                             [=](vx_ctx* c, vx_buf* st, uint64_t* spub) {
                                 if (pre) VX_TRY(pre(c));
                                 uint8_t com[32];
                                 VX_TRY(vx_sha_chain_trace_dev(c, just->pubkeys, n_auth, chosen->data(), 1, sl, st->d, spub, com));
                                 if (memcmp(com, just->authority_set_hash, 32) != 0) return vx_fail(c, VX_ERR_STATEMENT, "authority-set commitment mismatch");
                                 return (int32_t)VX_OK;
                             }},
                            bus, mask & 1);
    g.add({"Ed25519", sh[1].air_id, el, VX_ED_AIR_COLS, 2, 0,
           [=](vx_ctx* c, vx_buf* et, uint64_t* epub) { return vx_ed_trace_dev(c, just->pubkeys, just->signatures, just->precommit, 53, chosen->data(), n_auth, el, 1, et->d, epub); }},
          bus, mask >> 1 & 1);
    g.add({"SHA-512", sh[2].air_id, hl, VX_SHA512_AIR_COLS, 15, 0,
           [=](vx_ctx* c, vx_buf* ht, uint64_t* hpub) { return vx_sha512_trace_dev(c, just->pubkeys, just->signatures, just->precommit, chosen->data(), n_auth, hl, 1, ht->d, hpub); }},
          bus, mask >> 2 & 1);
    return first;
}
