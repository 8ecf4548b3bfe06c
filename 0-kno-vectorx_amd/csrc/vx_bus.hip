// Implementation of vx_bus.h: the rendezvous at which the tables of one statement draw their shared lookup challenges
// (BusMeet), the runner / starter / join of "one table on a bus" that both circuit provers use, the three tables of a
// justification, and what the aggregation provers (vx_merkle_openings_prove, vx_merkle_rows_prove, vx_fri_fold_prove) share: the
// hook of a table alone on its bus and the writer of their blobs.  Host code only: the kernels of every table live with their AIR (vx_*_air.hip).
#include <string.h>

#include "vx_bus.h"
#include "vx_table_shapes.h"

void BusMeet::finish_locked(size_t cap_words) {
    if (done) return;
    if (xch && xch->fn) {
        // slot t: [state (0 absent, 1 present, 2 failed), n_pub, pub[MAX_PUB], cap[cap_words]]; the shards' arrays are summed
        const size_t slot = 2 + MAX_PUB + cap_words;
        std::vector<uint64_t> w((size_t)n_parties * slot, 0);
        for (int t = 0; t < n_parties; ++t)
            if (local[t]) {
                uint64_t* q = w.data() + (size_t)t * slot;
                if (deposited[t] && pub[t].size() <= (size_t)MAX_PUB && cap[t].size() == cap_words) {
                    q[0] = 1, q[1] = pub[t].size();
                    memcpy(q + 2, pub[t].data(), pub[t].size() * 8);
                    memcpy(q + 2 + MAX_PUB, cap[t].data(), cap_words * 8);
                } else q[0] = 2;
            }
        if (xch->fn(xch->user, w.data(), w.size()) != 0) failed = true;
        for (int t = 0; t < n_parties && !failed; ++t) {
            const uint64_t* q = w.data() + (size_t)t * slot;
            if (q[0] != 1 || q[1] > (uint64_t)MAX_PUB) failed = true;  // a table nobody proved, one proved twice, or one whose prover gave up
            else if (!local[t]) pub[t].assign(q + 2, q + 2 + q[1]), cap[t].assign(q + 2 + MAX_PUB, q + 2 + MAX_PUB + cap_words);
        }
    }
    done = true;
    cv.notify_all();
}
int32_t BusMeet::meet(BusMeet* r, int who, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cap_words, uint64_t* chal, size_t n_chal) {
    std::unique_lock<std::mutex> lk(r->m);
    r->pub[who].assign(pub, pub + n_pub);
    r->cap[who].assign(cap, cap + cap_words);
    r->deposited[who] = true;
    ++r->arrived;
    r->capw = cap_words;
    if (r->arrived == r->n_local()) r->finish_locked(cap_words);
    r->cv.wait(lk, [&] { return r->done || (r->failed && !r->xch); });
    if (r->failed) return VX_ERR_STATEMENT;  // another table's prover gave up
    const uint64_t *pubs[MAX], *caps[MAX];
    size_t ns[MAX];
    for (int t = 0; t < r->n_parties; ++t) pubs[t] = r->pub[t].data(), ns[t] = r->pub[t].size(), caps[t] = r->cap[t].data();
    uint64_t c[4];
    vx_shared_challenges_n(pubs, ns, caps, (size_t)r->n_parties, cap_words, c, 4);
    for (size_t q = 0; q < n_chal && q < 4; ++q) chal[q] = c[q];
    return VX_OK;
}
void BusMeet::fail(int who) {
    std::lock_guard<std::mutex> lk(m);
    failed = true;
    if (xch && who >= 0 && who < n_parties && local[who] && !deposited[who] && !done) {
        // a sharded proof: the other shards are (or will be) inside the exchange -- this table arrives as a failure marker
        deposited[who] = false;
        ++arrived;
        local_failed[who] = true;
        if (arrived == n_local()) finish_locked(capw);
    }
    cv.notify_all();
}
int32_t vx_bus_hook(void* u, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cw, uint64_t* chal, size_t n_chal) {
    BusParty* p = (BusParty*)u;
    return BusMeet::meet(p->rv, p->who, pub, n_pub, cap, cw, chal, n_chal);
}
int32_t vx_one_table_hook(void*, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cw, uint64_t* chal, size_t n_chal) {
    vx_shared_challenges_n(&pub, &n_pub, &cap, 1, cw, chal, n_chal);
    return VX_OK;
}

size_t vx_justification_proof_bound(const vx_stark_config* cfg, size_t n_authorities, int32_t* rc_out) {
    size_t w2 = 0, w4 = 0, w5 = 0;
    int32_t rc = vx_stark_proof_bound(VX_AIR_SHA_CHAIN, cfg, sha_log_n(n_authorities), &w2);
    if (rc == VX_OK) rc = vx_stark_proof_bound(ed_air_id(sig_quorum(n_authorities)), cfg, ed_log_n(sig_quorum(n_authorities)), &w4);
    if (rc == VX_OK) rc = vx_stark_proof_bound(s512_air_id(sig_quorum(n_authorities)), cfg, s512_log_n(sig_quorum(n_authorities)), &w5);
    *rc_out = rc;
    return w2 + w4 + w5;
}

// sizes j.proof for a proof of this shape
static int32_t size_proof(TableJob& j, int air_id, int log_n, const vx_stark_config* cfg) {
    size_t bound = 0;
    VX_TRY(vx_stark_proof_bound(air_id, cfg, log_n, &bound));
    j.proof.resize(bound);
    return VX_OK;
}
int32_t prove_table(vx_ctx* c, TableJob& j, int air_id, int log_n, const vx_stark_config* cfg, const vx_chal_hook* hook, int consume_trace, vx_buf* trace, const uint64_t* pub,
                    size_t n_pub) {
    VX_TRY(size_proof(j, air_id, log_n, cfg));
    return vx_stark_prove_impl(c, air_id, cfg, trace->d, trace->n, consume_trace, log_n, pub, n_pub, j.proof.data(), j.proof.size(), &j.len, hook);
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
bool start_table(TableJob& j, BusMeet& rv, int who, std::function<int32_t(vx_ctx*, TableJob&)> fn) {
    try {
        j.th = std::thread([&j, &rv, who, fn = std::move(fn)] {
            (void)hipSetDevice(j.c->device);
            j.rc = fn(j.c, j);
            if (j.rc != VX_OK) rv.fail(who);  // do not leave the other provers waiting at their hooks
        });
    } catch (...) {
        rv.fail(who);
        return false;
    }
    return true;
}
int32_t side_contexts(vx_ctx* ctx, size_t n, vx_ctx** out, const char* msg) {
    vx_ctx* c = ctx;
    for (size_t t = 0; t < n; ++t) out[t] = c = c ? vx_side_ctx(c) : nullptr;
    VX_CHECK(c, "%s", msg);
    return VX_OK;
}
int32_t pack_blob(vx_ctx* ctx, const char* what, uint64_t magic, std::initializer_list<uint64_t> request, std::initializer_list<const TableJob*> jobs, uint64_t* blob_out,
                  size_t blob_cap, size_t* blob_len) {
    size_t total = 1 + request.size() + jobs.size();
    for (const TableJob* j : jobs) total += j->len;
    *blob_len = total;
    if (!blob_out || blob_cap < total) return vx_fail(ctx, VX_ERR_BUFSZ, "%s: the blob needs %zu words, buffer has %zu", what, total, blob_cap);
    uint64_t* w = blob_out;
    *w++ = magic;
    for (uint64_t r : request) *w++ = r;
    for (const TableJob* j : jobs) *w++ = j->len;
    for (const TableJob* j : jobs) memcpy(w, j->proof.data(), j->len * 8), w += j->len;
    return VX_OK;
}

int32_t vx_justification_tables_start(vx_ctx* const ctxs[3], const vx_justification* just, const vx_stark_config* cfg, BusMeet* rv, int first,
                                      int32_t (*pre)(vx_ctx*, void*), void* pre_user, JustificationTables* jt, unsigned mask) {
    // the signatures the proof verifies: the first floor(2n/3) + 1 signed authorities (more would only cost rows); when fewer
    // signed, all of them -- the native threshold check refuses the justification before anything is proven
    jt->chosen.assign(just->num_authorities, 0);
    jt->n_sig = 0;
    for (size_t i = 0; i < just->num_authorities && jt->n_sig < sig_quorum(just->num_authorities); ++i)
        if (just->validator_signed[i]) jt->chosen[i] = 1, ++jt->n_sig;
    for (int t = 0; t < 3; ++t) jt->party[t] = {rv, first + t}, jt->hooks[t] = {vx_bus_hook, &jt->party[t]}, jt->job[t].c = ctxs[t];
    const size_t n_auth = just->num_authorities, n_sig = jt->n_sig;
    const uint8_t* chosen = jt->chosen.data();
    auto prove_chain = [=](vx_ctx* c, TableJob& j) -> int32_t {
        if (pre) VX_TRY(pre(c, pre_user));
        const int sl = sha_log_n(n_auth);
        return run_table(c, j, VX_AIR_SHA_CHAIN, sl, VX_SHA_AIR_COLS, 10, cfg, &jt->hooks[0], 0, [=](vx_ctx* c, vx_buf* st, uint64_t* spub) {
            uint8_t com[32];
            VX_TRY(vx_sha_chain_trace_dev(c, just->pubkeys, n_auth, chosen, 1, sl, st->d, spub, com));
            if (memcmp(com, just->authority_set_hash, 32) != 0) return vx_fail(c, VX_ERR_STATEMENT, "authority-set commitment mismatch");
            return (int32_t)VX_OK;
        });
    };
    auto prove_ed = [=](vx_ctx* c, TableJob& j) -> int32_t {
        const int el = ed_log_n(n_sig);
        return run_table(c, j, ed_air_id(n_sig), el, VX_ED_AIR_COLS, 2, cfg, &jt->hooks[1], 0, [=](vx_ctx* c, vx_buf* et, uint64_t* epub) {
            return vx_ed_trace_dev(c, just->pubkeys, just->signatures, just->precommit, 53, chosen, n_auth, el, 1, et->d, epub);
        });
    };
    auto prove_s512 = [=](vx_ctx* c, TableJob& j) -> int32_t {
        const int hl = s512_log_n(n_sig);
        return run_table(c, j, s512_air_id(n_sig), hl, VX_SHA512_AIR_COLS, 15, cfg, &jt->hooks[2], 0, [=](vx_ctx* c, vx_buf* ht, uint64_t* hpub) {
            return vx_sha512_trace_dev(c, just->pubkeys, just->signatures, just->precommit, chosen, n_auth, hl, 1, ht->d, hpub);
        });
    };
    const std::function<int32_t(vx_ctx*, TableJob&)> prove[3] = {prove_chain, prove_ed, prove_s512};
    for (int t = 0; t < 3; ++t) {
        if (!(mask >> t & 1)) continue;  // another shard's table
        if (!start_table(jt->job[t], *rv, first + t, prove[t])) {
            for (int u = t + 1; u < 3; ++u)
                if (mask >> u & 1) rv->fail(first + u);
            return VX_ERR_DEVICE;
        }
    }
    return VX_OK;
}

int32_t vx_justification_tables_join(vx_ctx* ctx, JustificationTables* jt) {
    TableJoin{{&jt->job[0], &jt->job[1], &jt->job[2]}}.join();
    // a prover released from the rendezvous by somebody else's failure reports VX_ERR_STATEMENT without a message
    for (int t = 0; t < 3; ++t)
        if (jt->job[t].rc != VX_OK && vx_last_error(jt->job[t].c)[0]) return vx_fail(ctx, jt->job[t].rc, "%s", vx_last_error(jt->job[t].c));
    for (int t = 0; t < 3; ++t)
        if (jt->job[t].rc != VX_OK) return vx_fail(ctx, jt->job[t].rc, "justification table %d failed", t);
    return VX_OK;
}
