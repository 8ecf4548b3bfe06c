// "Several tables on one logUp bus", the part that knows nothing of contexts, devices or proofs (implemented in bus_meet.cpp;
// standard C++ and include/vx.h only, so tests/host/bus_group_check.cpp drives it on a CPU).
//   BusMeet   the rendezvous: the tables of one statement must use the same lookup challenges, drawn after every trace is
//             committed.  Every prover stops after its trace cap (vx_bus_hook), deposits its public inputs + cap, waits for all
//             the others and derives the challenges from the transcript of all (public inputs, cap) pairs in table order.
//   BusGroup  the bookkeeping of the tables that meet there: which are proven here, on which thread, what became of each, and
//             which failure the caller gets to see.  Leaving a group by any path releases whoever waits and joins every thread.
// vx_bus.h puts the device-facing group (contexts, traces, proofs) on top.
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#pragma GCC visibility push(default)  // (as in vx_internal.h: whoever includes the ABI first decides what the library exports)
#include "../../include/vx.h"
#pragma GCC visibility pop

// the challenge derivation (vx_stark.hip); a host program that links the rendezvous alone supplies its own
void vx_shared_challenges_n(const uint64_t* const* pubs, const size_t* n_pubs, const uint64_t* const* caps, size_t k, size_t cap_words, uint64_t* out, size_t n_out);

// A statement proven by several processes (one per GPU, vx_header_range_prove_ex with n_shards > 1): `local[t]` says which
// of the n_parties tables are proven here; once every LOCAL table has arrived -- or failed: a failed table arrives as a
// failure marker, so that the other shards are not left waiting -- one thread calls `xch` with an array of n_parties slots
// (only the local ones filled) and gets the union back.
struct BusMeet {
    static constexpr int MAX = 72, MAX_PUB = 32;
    std::mutex m;
    std::condition_variable cv;
    int n_parties = 0, arrived = 0;
    bool failed = false, done = false;
    std::vector<uint64_t> pub[MAX], cap[MAX];
    bool local[MAX], deposited[MAX], local_failed[MAX];
    size_t capw = 64;  // words of a trace cap (4 << cap_height); set by the caller for a sharded proof, by the first arrival otherwise
    const vx_hr_exchange* xch = nullptr;
    BusMeet() {
        for (int t = 0; t < MAX; ++t) local[t] = true, deposited[t] = local_failed[t] = false;
    }
    int n_local() const {
        int k = 0;
        for (int t = 0; t < n_parties; ++t) k += local[t] ? 1 : 0;
        return k;
    }
    static int32_t meet(BusMeet* r, int who, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cap_words, uint64_t* chal, size_t n_chal);
    void fail(int who);  // the table whose prover gave up (counts as arrived when it had not deposited yet)
    void finish_locked(size_t cap_words);  // all local tables are in: exchange with the other shards (if any), release everybody
};
struct BusParty {
    BusMeet* rv = nullptr;
    int who = 0;
    bool released = false;  // the hook returned a failure: some OTHER table gave up (set by vx_bus_hook, read after the join)
};
// the vx_chal_hook of a party (`party` is its BusParty)
int32_t vx_bus_hook(void* party, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cw, uint64_t* chal, size_t n_chal);

// The tables of one statement, in table order; each is a party of one of (at most) two buses.  A table is run by a function
// that returns VX_OK or its error code and calls vx_bus_hook with the table's party on the way.
struct BusGroup {
    static constexpr int MAX = BusMeet::MAX;
    // what first_error's caller says when it names no table
    static constexpr const char* ALL_RELEASED = "every table that failed here was released at the rendezvous: a table of another shard failed, or the exchange did";
    BusMeet bus[2];  // (rotate proves the tables of two buses as one group; everybody else uses bus 0)
    struct Table {
        BusParty party;
        int32_t rc = VX_OK;
        bool started = false;
        std::thread th;
    };
    Table t[MAX];
    int n = 0;
    BusGroup() = default;
    BusGroup(const BusGroup&) = delete;
    ~BusGroup() { finish(); }
    // the next party of bus b, proven here (`local`) or by another shard; returns its index in the group
    int add(int b = 0, bool local = true);
    // bus 0 is proven by several processes that meet through `xch` (nullptr: by this one alone)
    void shard(const vx_hr_exchange* xch, size_t cap_words) { bus[0].xch = xch, bus[0].capw = cap_words; }
    bool local(int k) const { return t[k].party.rv->local[t[k].party.who]; }
    bool released(int k) const { return t[k].rc != VX_OK && t[k].party.released; }
    // t[k].rc = fn() on a thread of its own / on the caller's; a table that fails -- or whose thread cannot be created
    // (VX_ERR_DEVICE) -- fails at the rendezvous, so that nobody is left waiting for it
    void start(int k, std::function<int32_t()> fn);
    void run_here(int k, const std::function<int32_t()>& fn);
    // fails every local table that was never started, then joins every thread; whatever the threads refer to must outlive it
    void finish();
    // The failure the caller reports: among the tables with rc != VX_OK whose failure is their own (not a release) the first in
    // `order` -> its code, *who = its index.  No failure -> VX_OK; every failing table released -> VX_ERR_STATEMENT; *who = -1.
    int32_t first_error(const std::vector<int>& order, int* who) const;
};
