// The balance check of a generic bus group (include/vx.h vx_bus_group_check) on the device: which message of which table and row
// has no partner, found before any trace is committed.  A multiset balance over fingerprints:
//   records   every message with a non-zero multiplicity becomes one record (D.a, D.b, m, origin): D the message's denominator under
//             the CHECK CHALLENGES below, m its signed multiplicity, origin = table << 56 | row << 8 | ordinal in the table's message
//             list.  Two kernels make them, both reading the message list the constraints and the auxiliary round are built from:
//             k_bus_records<Air> for a compiled table (Air::messages with a third sink beside BusLive / BusFractions of bus_aux.cuh: a
//             pair is two records and two ordinals, a helper of one message one; periodic values as there, BusPer<Air>) and
//             k_bus_records_prog for a declared run-time table (the walk of k_bus_aux_prog: busp_walk, bus_aux_prog.cuh).  No
//             inversion, no helper storage.  Each runs twice: the count pass writes how many records a lane has, an exclusive scan over
//             the lanes of ALL tables places them (rocPRIM), the emit pass writes them there -- never one slot per (lane, message).
//             The outside party's records are made on the host and uploaded behind the tables'.
//   match     the records are ordered by the 128-bit key (D.a, D.b) -- rocPRIM's device radix sort, two stable 64-bit passes over
//             (key word, record index): D.b first, then D.a -- and k_bus_match walks them: a record whose predecessor has another key
//             heads a segment, sums the segment's multiplicities in the field, and a non-zero sum counts one unmatched tuple (one
//             atomic per wave) and proposes the segment's lowest origin to a 64-bit atomicMin.  k_bus_net fetches the sum of the
//             segment that won.  Nothing of the result depends on the order the records were written or sorted in.
//             A segment is TWO records in the tables this is for (a sender and a receiver); one lane walking a long segment is a
//             periodic lookup table (BlakeChainAir's XOR table, EdAir's range table, LookupAir), and those tables have no message
//             list here.  The compiled tables that have one: ids 16 .. 23, ShaChainAir (4), ShaTreeAir (7, 8, 9), Sha512Air (11, 13, 14) and
//             EpochEndAir (15).
// THE CHECK CHALLENGES (beta*, gamma*) are fixed: the check runs before anything is committed, so they cannot be a proof's.  They are
// the first four Poseidon round constants (poseidon_constants.h VX_POSEIDON_RC_INIT[0 .. 3], canonical words of plonky2's own
// nothing-up-my-sleeve generator) as two extension elements.  The pair (D.a, D.b) under them is a 128-bit fingerprint of the tuple
// (t0, t1, t2, t3, tag): equal tuples always meet in one segment, so a COLLISION of two different tuples can only merge their segments
// -- it can hide an imbalance (two sums that cancel) or name the wrong one of the merged tuples, never invent an imbalance on a bus
// that closes.  The proof's own challenges, drawn after the commitments, are what soundness rests on; this check names errors.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "air_list.h"
#include "bus_aux.cuh"
#include "bus_aux_prog.cuh"

constexpr uint64_t BUS_CHECK_CHAL[4] = {0xb585f766f2144405ULL, 0x7746a55f43921ad7ULL, 0xb2fb0d31cee799b4ULL, 0x0f6760a4803427d7ULL};
static_assert(BUS_CHECK_CHAL[0] < glh::P && BUS_CHECK_CHAL[1] < glh::P && BUS_CHECK_CHAL[2] < glh::P && BUS_CHECK_CHAL[3] < glh::P, "bus_balance.cuh: canonical check challenges");
constexpr int BUS_MATCH_BLOCK = 256;

struct BusRecords {  // one array per field: the sort reads the key words alone
    uint64_t *hi, *lo, *m, *origin;
};
__host__ __device__ inline uint64_t bus_origin(uint64_t table, uint64_t row, uint64_t ordinal) { return table << 56 | row << 8 | ordinal; }

// ---- compiled tables: the sinks of Air::messages
struct BusRecordCount {
    static constexpr int UNROLL = 1;  // (nothing here wants constant indices: a list's loop stays rolled)
    uint64_t c = 0;
    __device__ __forceinline__ void put(const Fp& ma, const X2<Fp>&, const Fp& mb, const X2<Fp>&) { c += (ma.v[0] != 0) + (mb.v[0] != 0); }
    __device__ __forceinline__ void pair(const Fp& m, const X2<Fp>&, const X2<Fp>&) { c += m.v[0] != 0 ? 2 : 0; }
    __device__ __forceinline__ void single(const Fp& m, const X2<Fp>&) { c += m.v[0] != 0; }
};
struct BusRecordSink {
    static constexpr int UNROLL = 1;
    BusRecords r;
    uint64_t at, end;  // this lane's records: [at, end) from the scan of the count pass
    uint64_t origin;   // table << 56 | row << 8; the ordinal is added here
    uint32_t ord = 0;
    __device__ __forceinline__ void one(const Fp& m, const X2<Fp>& d) {
        if (m.v[0] && at < end) r.hi[at] = d.a.v[0], r.lo[at] = d.b.v[0], r.m[at] = m.v[0], r.origin[at] = origin | ord, ++at;
        ++ord;
    }
    __device__ __forceinline__ void put(const Fp& ma, const X2<Fp>& da, const Fp& mb, const X2<Fp>& db) { one(ma, da), one(mb, db); }
    __device__ __forceinline__ void pair(const Fp& m, const X2<Fp>& da, const X2<Fp>& db) { one(m, da), one(m, db); }
    __device__ __forceinline__ void single(const Fp& m, const X2<Fp>& d) { one(m, d); }
};
// One lane per row, or per BUS_ROWS-row block, as k_bus_aux<Air>.  EMIT false: cnt[lane] = its records; true: the records to
// [offs[lane], offs[lane] + cnt[lane]), never at or behind n_rec.
template <class Air, bool EMIT>
__global__ __launch_bounds__(Air::BUS_BLOCK) void k_bus_records(const uint64_t* __restrict__ tr, size_t n, BusPub pubw, uint64_t* __restrict__ cnt, const uint64_t* __restrict__ offs,
                                                                 BusRecords out, uint64_t n_rec, uint64_t table) {
    const size_t i = blockIdx.x * (size_t)Air::BUS_BLOCK + threadIdx.x;
    if (i >= n / Air::BUS_ROWS) return;
    const size_t row = (size_t)Air::BUS_ROWS * i;
    const RowViewN<1> loc{tr, n, {row}};
    Fp pub[Air::PUB];
#pragma unroll
    for (int q = 0; q < Air::PUB; ++q) pub[q] = Fp::from(pubw.w[q]);
    const bus::Bus<X2<Fp>> bus(Fp::from(BUS_CHECK_CHAL[0]), Fp::from(BUS_CHECK_CHAL[1]), Fp::from(BUS_CHECK_CHAL[2]), Fp::from(BUS_CHECK_CHAL[3]));
    BusPer<Air> pv;
    const Fp* per = pv.at(row);
    if constexpr (EMIT) {
        const uint64_t at = offs[i], end = at + cnt[i];
        BusRecordSink s{out, at, end < n_rec ? end : n_rec, bus_origin(table, row, 0)};
        Air::template messages<Fp>(loc, per, pub, bus, s);
    } else {
        BusRecordCount s;
        Air::template messages<Fp>(loc, per, pub, bus, s);
        cnt[i] = s.c;
    }
}

// ---- declared run-time tables: the walk of k_bus_aux_prog (registers in LDS, instruction words fetched wave-uniformly)
template <bool EMIT>
__global__ __launch_bounds__(BUSP_BLOCK) void k_bus_records_prog(const uint64_t* __restrict__ tr, size_t n, BusProgArgs p, uint64_t* __restrict__ cnt, const uint64_t* __restrict__ offs,
                                                                 BusRecords out, uint64_t n_rec, uint64_t table) {
    extern __shared__ uint64_t busr_lds[];
    const size_t i = blockIdx.x * (size_t)BUSP_BLOCK + threadIdx.x;
    if (i >= (n >> p.block_log)) return;  // (no barrier below: a lane works on LDS words of its own)
    const size_t row = i << p.block_log;
    const gl2 beta{BUS_CHECK_CHAL[0], BUS_CHECK_CHAL[1]}, gamma{BUS_CHECK_CHAL[2], BUS_CHECK_CHAL[3]};
    uint64_t* R = busr_lds + threadIdx.x;
    if constexpr (EMIT) {
        uint64_t at = offs[i], end = at + cnt[i];
        if (end > n_rec) end = n_rec;
        const uint64_t origin = bus_origin(table, row, 0);
        busp_walk(tr, n, row, R, beta, gamma, p, [&](int msg, uint64_t m, gl2 D) {
            if (m && at < end) out.hi[at] = D.a, out.lo[at] = D.b, out.m[at] = m, out.origin[at] = origin | (uint64_t)msg, ++at;
        });
    } else {
        uint64_t c = 0;
        busp_walk(tr, n, row, R, beta, gamma, p, [&](int, uint64_t m, gl2) { c += m != 0; });
        cnt[i] = c;
    }
}

// ---- the order of the records
__global__ __launch_bounds__(BUS_MATCH_BLOCK) void k_bus_iota(uint64_t* __restrict__ v, size_t n) {
    const size_t i = blockIdx.x * (size_t)BUS_MATCH_BLOCK + threadIdx.x;
    if (i < n) v[i] = i;
}
// dst[k][j] = src[k][perm[j]] for the n_arrays (<= 3) arrays
struct BusGather {
    const uint64_t* src[3];
    uint64_t* dst[3];
    int n_arrays;
};
__global__ __launch_bounds__(BUS_MATCH_BLOCK) void k_bus_gather(BusGather g, const uint64_t* __restrict__ perm, size_t n) {
    const size_t j = blockIdx.x * (size_t)BUS_MATCH_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint64_t from = perm[j];
    if (from >= n) return;  // (a permutation: never taken)
    for (int k = 0; k < g.n_arrays; ++k) g.dst[k][j] = g.src[k][from];
}

// ---- the match.  Sorted by (key_hi, key_lo); m and origin in that order.  res[0] the unmatched tuples (starts at 0), res[1] the lowest
// origin among the records of unmatched tuples (starts at ~0); net_of (starts at 0) / low_of have one slot per record, written by heads.
__global__ __launch_bounds__(BUS_MATCH_BLOCK) void k_bus_match(const uint64_t* __restrict__ key_hi, const uint64_t* __restrict__ key_lo, const uint64_t* __restrict__ m,
                                                               const uint64_t* __restrict__ origin, size_t n_rec, unsigned long long* __restrict__ res, uint64_t* __restrict__ net_of,
                                                               uint64_t* __restrict__ low_of) {
    const size_t i = blockIdx.x * (size_t)BUS_MATCH_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n_rec && (i == 0 || key_hi[i] != key_hi[i - 1] || key_lo[i] != key_lo[i - 1])) {  // a segment head
        const uint64_t kh = key_hi[i], kl = key_lo[i];
        uint64_t sum = 0, lo = ~0ull;
        size_t j = i;
        do {
            sum = gl_add(sum, m[j]);
            lo = origin[j] < lo ? origin[j] : lo;
        } while (++j < n_rec && key_hi[j] == kh && key_lo[j] == kl);
        if (sum) bad = true, net_of[i] = sum, low_of[i] = lo, atomicMin(res + 1, (unsigned long long)lo);
    }
    const unsigned long long mask = __ballot(bad);  // one atomic per wave of 64, by its first lane (no lane has returned)
    if (mask && (threadIdx.x & 63) == 0) atomicAdd(res, (unsigned long long)__popcll(mask));
}
// res[2] = the sum of the segment whose lowest origin is res[1] (origins are distinct: one head writes)
__global__ __launch_bounds__(BUS_MATCH_BLOCK) void k_bus_net(const uint64_t* __restrict__ net_of, const uint64_t* __restrict__ low_of, size_t n_rec, unsigned long long* __restrict__ res) {
    const size_t i = blockIdx.x * (size_t)BUS_MATCH_BLOCK + threadIdx.x;
    if (i < n_rec && net_of[i] && low_of[i] == res[1]) res[2] = net_of[i];
}

// ---- which compiled AIRs have a message list (air.cuh "the bus of a table"), from the one list of compiled AIRs
template <class Air, class = void>
struct bus_has_messages : std::false_type {};
template <class Air>
struct bus_has_messages<Air, std::void_t<decltype(Air::BUS_ROWS), decltype(Air::N_HELP)>> : std::true_type {};
template <class Air>
struct BusAirTag {
    using type = Air;
};
// rows that share one set of messages (1 or 32); 0: the AIR is not compiled in, or has no message list
template <class... Airs>
static int bus_records_rows(int air_id, AirList<Airs...>) {
    int rows = 0;
    auto one = [&](auto air) {
        using Air = typename decltype(air)::type;
        if constexpr (bus_has_messages<Air>::value)
            if (Air::ID == air_id) rows = Air::BUS_ROWS;
    };
    (one(BusAirTag<Airs>{}), ...);
    return rows;
}
// one pass of k_bus_records<Air> for the compiled AIR `air_id` on `stream`; false: no such AIR
template <bool EMIT, class... Airs>
static bool bus_records_launch(int air_id, AirList<Airs...>, hipStream_t stream, const uint64_t* tr, size_t n, const uint64_t* pub, uint64_t* cnt, const uint64_t* offs,
                               const BusRecords& out, uint64_t n_rec, uint64_t table) {
    bool done = false;
    auto one = [&](auto air) {
        using Air = typename decltype(air)::type;
        if constexpr (bus_has_messages<Air>::value) {
            if (Air::ID != air_id) return;
            static_assert(Air::PUB <= BUS_PUB_MAX, "bus_balance.cuh: the public inputs go to the kernel by value");
            BusPub pubw{};
            memcpy(pubw.w, pub, Air::PUB * sizeof(uint64_t));
            const size_t lanes = n / Air::BUS_ROWS;
            hipLaunchKernelGGL((k_bus_records<Air, EMIT>), dim3((unsigned)((lanes + Air::BUS_BLOCK - 1) / Air::BUS_BLOCK)), dim3(Air::BUS_BLOCK), 0, stream, tr, n, pubw, cnt, offs, out,
                               n_rec, table);
            done = true;
        }
    };
    (one(BusAirTag<Airs>{}), ...);
    return done;
}
