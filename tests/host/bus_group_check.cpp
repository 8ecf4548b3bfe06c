// The rendezvous and the group bookkeeping of "several tables on one bus" (0-kno-vectorx_amd/csrc/bus_meet.h) driven on a CPU:
// tables are lambdas that call the hook, the challenge derivation is a running multiply-add over all (pub, cap) pairs in table
// order, and the exchange of a sharded proof is a barrier plus the element-wise sum of the slot arrays (the contract of
// vx_hr_exchange).  Every case runs ROUNDS times to vary the interleaving; nothing sleeps.  A hang ends in SIGALRM.
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "../../0-kno-vectorx_amd/csrc/bus_meet.h"

void vx_shared_challenges_n(const uint64_t* const* pubs, const size_t* n_pubs, const uint64_t* const* caps, size_t k, size_t cap_words, uint64_t* out, size_t n_out) {
    uint64_t h = 0x9e3779b97f4a7c15ULL;
    for (size_t t = 0; t < k; ++t) {
        h = h * 6364136223846793005ULL + n_pubs[t] + 1;
        for (size_t i = 0; i < n_pubs[t]; ++i) h = h * 6364136223846793005ULL + pubs[t][i];
        for (size_t i = 0; i < cap_words; ++i) h = h * 6364136223846793005ULL + caps[t][i];
    }
    for (size_t q = 0; q < n_out; ++q) out[q] = h = h * 6364136223846793005ULL + q;
}

namespace {
constexpr int ROUNDS = 200;
constexpr size_t CAPW = 8;
#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAILED %s:%d (round %d): %s\n", __FILE__, __LINE__, round_no, #cond); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)
int round_no = 0;

// table t of a statement: n_pub = t + 1 public inputs and a cap, both functions of t alone
struct Record {
    std::vector<uint64_t> pub, cap;
    explicit Record(int t) : pub((size_t)t + 1), cap(CAPW) {
        for (size_t i = 0; i < pub.size(); ++i) pub[i] = 1000 * (uint64_t)t + i;
        for (size_t i = 0; i < CAPW; ++i) cap[i] = 77 * (uint64_t)t + 5 * i + 1;
    }
};
// the challenges of the n-table statement, derived directly
void expected(int n, uint64_t out[4]) {
    std::vector<Record> r;
    for (int t = 0; t < n; ++t) r.emplace_back(t);
    std::vector<const uint64_t*> pubs, caps;
    std::vector<size_t> ns;
    for (const Record& x : r) pubs.push_back(x.pub.data()), caps.push_back(x.cap.data()), ns.push_back(x.pub.size());
    vx_shared_challenges_n(pubs.data(), ns.data(), caps.data(), (size_t)n, CAPW, out, 4);
}
struct Result {
    std::atomic<int> returned{0};
    uint64_t chal[BusGroup::MAX][4] = {};
};
// what a prover does: (fail before the hook | ) commit, meet the others at the hook, (fail after it | ) finish
std::function<int32_t()> table(BusGroup& g, int k, int t, Result& res, int32_t fail_before = VX_OK, std::function<void()> wait_first = nullptr) {
    return [&g, k, t, &res, fail_before, wait_first] {
        if (wait_first) wait_first();
        int32_t rc = fail_before;
        if (rc == VX_OK) {
            const Record r(t);
            rc = vx_bus_hook(&g.t[k].party, r.pub.data(), r.pub.size(), r.cap.data(), CAPW, res.chal[k], 4);
        }
        ++res.returned;
        return rc;
    };
}
bool same(const uint64_t a[4], const uint64_t b[4]) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }

// 1. three tables, all arrive: everybody gets the derivation over the three pairs in table order, whoever comes first
void all_arrive() {
    uint64_t want[4];
    expected(3, want);
    BusGroup g;
    Result res;
    for (int t = 0; t < 3; ++t) g.add();
    const int here = round_no % 3;
    for (int t = 0; t < 3; ++t)
        if (t != here) g.start(t, table(g, t, t, res));
    g.run_here(here, table(g, here, here, res));
    g.finish();
    int who = 7;
    CHECK(g.first_error({0, 1, 2}, &who) == VX_OK && who == -1);
    for (int t = 0; t < 3; ++t) CHECK(g.t[t].rc == VX_OK && !g.released(t) && same(res.chal[t], want));
}
// 2. one table fails before its hook (every position, on a thread or here): the others are released, the failure is named
void one_fails(int bad, bool bad_here) {
    BusGroup g;
    Result res;
    for (int t = 0; t < 3; ++t) g.add();
    const int here = bad_here ? bad : (bad + 1) % 3;
    for (int t = 0; t < 3; ++t)
        if (t != here) g.start(t, table(g, t, t, res, t == bad ? VX_ERR_OOM : VX_OK));
    g.run_here(here, table(g, here, here, res, here == bad ? VX_ERR_OOM : VX_OK));
    g.finish();
    CHECK(res.returned == 3);
    for (int t = 0; t < 3; ++t) {
        CHECK(!g.t[t].th.joinable());
        if (t == bad) CHECK(g.t[t].rc == VX_ERR_OOM && !g.released(t));
        else CHECK(g.t[t].rc == VX_ERR_STATEMENT && g.released(t));
    }
    int who = -1;
    CHECK(g.first_error({here, (here + 1) % 3, (here + 2) % 3}, &who) == VX_ERR_OOM && who == bad);
}
// 3. two tables fail on their own with different codes: the report order decides
void two_fail() {
    BusGroup g;
    Result res;
    for (int t = 0; t < 3; ++t) g.add();
    g.start(0, table(g, 0, 0, res, VX_ERR_OOM));
    g.start(1, table(g, 1, 1, res));
    g.run_here(2, table(g, 2, 2, res, VX_ERR_ARG));
    g.finish();
    int who = -1;
    CHECK(g.released(1) && !g.released(0) && !g.released(2));
    CHECK(g.first_error({2, 0, 1}, &who) == VX_ERR_ARG && who == 2);
    CHECK(g.first_error({1, 0, 2}, &who) == VX_ERR_OOM && who == 0);
}
// 4. a group abandoned after one of three tables was started: that table is released, the destructor joins it
int32_t abandon_after_one(Result& res, int32_t* rc_of_started, bool* released) {
    BusGroup g;
    for (int t = 0; t < 3; ++t) g.add();
    g.start(1, [&, inner = table(g, 1, 1, res)] {
        *rc_of_started = inner();
        *released = g.t[1].party.released;
        return *rc_of_started;
    });
    return VX_ERR_DEVICE;  // (an early return: a side context that could not be had, say)
}
void abandoned() {
    Result res;
    int32_t rc = VX_OK;
    bool released = false;
    CHECK(abandon_after_one(res, &rc, &released) == VX_ERR_DEVICE);
    CHECK(res.returned == 1 && rc == VX_ERR_STATEMENT && released);
}

// the exchange of two shards in one process: a barrier, then everybody holds the element-wise sum
struct Exchange {
    std::mutex m;
    std::condition_variable cv;
    std::vector<uint64_t> sum;
    int entered = 0;
    std::atomic<bool> in[2] = {{false}, {false}};
    struct End {
        Exchange* x;
        int shard;
    } end[2] = {{this, 0}, {this, 1}};
    vx_hr_exchange fn[2] = {{call, &end[0]}, {call, &end[1]}};
    static int32_t call(void* user, uint64_t* words, size_t n) {
        End* e = (End*)user;
        Exchange* x = e->x;
        std::unique_lock<std::mutex> lk(x->m);
        x->in[e->shard] = true;
        if (x->sum.empty()) x->sum.assign(n, 0);
        if (x->sum.size() != n) return 1;
        for (size_t i = 0; i < n; ++i) x->sum[i] += words[i];
        if (++x->entered == 2) x->cv.notify_all();
        x->cv.wait(lk, [&] { return x->entered == 2; });
        for (size_t i = 0; i < n; ++i) words[i] = x->sum[i];
        return 0;
    }
};
// One shard of a 4-table statement (table t on shard t mod 2).  bad >= 0: that table fails on its own once shard 0 is inside the
// exchange (it has deposited).  abandon: the shard leaves before it starts any table.  Returns what the caller would report.
int32_t shard_of_four(int shard, Exchange& x, Result& res, int bad, bool abandon, int* who) {
    BusGroup g;
    g.shard(&x.fn[shard], CAPW);
    for (int t = 0; t < 4; ++t) g.add(0, t % 2 == shard);
    *who = -1;
    if (abandon) return VX_ERR_OOM;  // (the group goes out of scope with two local tables that were never started)
    auto shard0_in = [&x] {
        while (!x.in[0]) std::this_thread::yield();
    };
    const int first = shard, second = shard + 2;
    g.start(second, table(g, second, second, res, second == bad ? VX_ERR_OOM : VX_OK, second == bad ? std::function<void()>(shard0_in) : nullptr));
    g.run_here(first, table(g, first, first, res, first == bad ? VX_ERR_OOM : VX_OK, first == bad ? std::function<void()>(shard0_in) : nullptr));
    g.finish();
    for (int t = 0; t < 4; ++t) CHECK(!g.t[t].th.joinable());
    return g.first_error({0, 1, 2, 3}, who);
}
// 5. / 6. / 7.  two groups on two threads
void sharded(int bad, bool abandon) {
    uint64_t want[4];
    expected(4, want);
    Exchange x;
    Result res[2];
    int32_t rc[2] = {1, 1};
    int who[2] = {7, 7};
    std::thread other([&] { rc[1] = shard_of_four(1, x, res[1], bad, abandon, &who[1]); });
    rc[0] = shard_of_four(0, x, res[0], bad, false, &who[0]);
    other.join();
    if (bad < 0 && !abandon) {
        CHECK(rc[0] == VX_OK && rc[1] == VX_OK);
        for (int t = 0; t < 4; ++t) CHECK(same(res[t % 2].chal[t], want));
    } else {
        // shard 0 did nothing wrong: both its tables were released by shard 1's failure marker, and it says so
        CHECK(rc[0] == VX_ERR_STATEMENT && who[0] == -1 && res[0].returned == 2);
        if (abandon) CHECK(rc[1] == VX_ERR_OOM && res[1].returned == 0);
        else CHECK(rc[1] == VX_ERR_OOM && who[1] == bad && res[1].returned == 2);
    }
}
}  // namespace

int main() {
    alarm(30);
    for (round_no = 0; round_no < ROUNDS; ++round_no) {
        all_arrive();
        for (int bad = 0; bad < 3; ++bad) one_fails(bad, false), one_fails(bad, true);
        two_fail();
        abandoned();
        sharded(-1, false);
        sharded(1 + 2 * (round_no % 2), false);  // shard 1's table proven here / on a thread
        sharded(-1, true);
    }
    printf("ok %d\n", ROUNDS);
    return 0;
}
