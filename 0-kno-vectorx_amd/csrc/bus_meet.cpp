// Implementation of bus_meet.h: the rendezvous of the tables on one bus and the bookkeeping of a group of them.  Host code,
// standard C++ only.
#include "bus_meet.h"

#include <string.h>

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
    if (xch && who >= 0 && who < n_parties && local[who] && !deposited[who] && !local_failed[who] && !done) {
        // a sharded proof: the other shards are (or will be) inside the exchange -- this table arrives as a failure marker
        ++arrived;
        local_failed[who] = true;
        if (arrived == n_local()) finish_locked(capw);
    }
    cv.notify_all();
}
int32_t vx_bus_hook(void* u, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cw, uint64_t* chal, size_t n_chal) {
    BusParty* p = (BusParty*)u;
    const int32_t rc = BusMeet::meet(p->rv, p->who, pub, n_pub, cap, cw, chal, n_chal);
    p->released = rc != VX_OK;
    return rc;
}

int BusGroup::add(int b, bool local) {
    BusMeet& m = bus[b];
    m.local[m.n_parties] = local;
    t[n].party.rv = &m, t[n].party.who = m.n_parties++;
    return n++;
}
void BusGroup::start(int k, std::function<int32_t()> fn) {
    Table& T = t[k];
    T.started = true;
    try {
        T.th = std::thread([&T, fn = std::move(fn)] {
            T.rc = fn();
            if (T.rc != VX_OK) T.party.rv->fail(T.party.who);
        });
    } catch (...) {
        T.rc = VX_ERR_DEVICE;
        T.party.rv->fail(T.party.who);
    }
}
void BusGroup::run_here(int k, const std::function<int32_t()>& fn) {
    Table& T = t[k];
    T.started = true;
    T.rc = fn();
    if (T.rc != VX_OK) T.party.rv->fail(T.party.who);
}
void BusGroup::finish() {
    for (int k = 0; k < n; ++k)
        if (!t[k].started && local(k)) t[k].started = true, t[k].party.rv->fail(t[k].party.who);
    for (int k = 0; k < n; ++k)
        if (t[k].th.joinable()) t[k].th.join();
}
int32_t BusGroup::first_error(const std::vector<int>& order, int* who) const {
    *who = -1;
    bool any = false;
    for (int k : order) {
        if (t[k].rc == VX_OK) continue;
        any = true;
        if (!t[k].party.released) return *who = k, t[k].rc;
    }
    return any ? VX_ERR_STATEMENT : VX_OK;
}
