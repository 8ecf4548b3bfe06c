// The auxiliary round of every table whose helpers hold two messages each, or one (air.cuh "the bus of a table ..."): one witness
// kernel and one gen_aux body for MerkleOpenAir / MerkleOpenSetAir, LeafSpongeAir / LeafSpongeSetAir, LeafNoopAir, FriFoldAir,
// FriCombineAir, TranscriptAir, ShaChainAir, ShaTreeAir, Sha512Air and EpochEndAir.  The kernel reads the messages from the list the AIR's constraints are
// built from (Air::messages with F = Fp), so a table states multiplicities, slots, pairing and helper order once.
//   k_bus_aux<Air>  one lane per row, or per 32-row block (Air::BUS_ROWS).  A first walk of the list looks at the multiplicities
//                   alone (the denominators are dead code in it): a row or block that sends and receives nothing -- idle, or a
//                   row of a query that has no message -- gets zero helpers and inverts nothing.  Otherwise a second walk fills
//                   num_e = m_a D_b + m_b D_a and den_e = D_a D_b (num = m, den = D for a helper of one message), and ONE
//                   extension inversion yields all helpers (Montgomery batch, gl2_batch_div).  Helper e goes to columns
//                   [2 e, 2 e + 1] of all BUS_ROWS rows; the sum of the helpers, the increment of the running sum, to columns
//                   [2 N_HELP, 2 N_HELP + 1] of the first row, zero on the others
//   BusPer<Air>     the periodic values a list reads (Air::BUS_PERIODIC), computed from the row index by Air::bus_periodic -- the
//                   function the host's periodic table is filled from -- and a null pointer for every other table
//   bus_gen_aux     launches it and closes the sum (vx_bus_close_dev scans the increments and publishes total / rows)
// The public inputs go to the kernel by value: at most 24 words in these tables.
// A list's loops are unrolled up to 16 pairs, so that num[] / den[] are indexed by constants and stay in registers.  Two tables are
// past that and keep the arrays on the stack (profiles/README.md): FriFoldAir, whose loop over 16 pairs is, unrolled, above the
// compiler's size limit for a `#pragma unroll` loop (1104 bytes a lane, as the kernel it replaces), and EpochEndAir, whose loop has
// 20 pairs and whose table has 512 rows.
#pragma once
#include <string.h>

#include "air.cuh"
#include "vx_internal.h"

constexpr int BUS_PUB_MAX = 24;
struct BusPub {
    uint64_t w[BUS_PUB_MAX];
};

struct BusLive {  // does the row or block have a message at all?
    static constexpr int UNROLL = 16;  // a list's loops are unrolled here: num[] / den[] below want constant indices
    bool any = false;
    __device__ __forceinline__ void put(const Fp& ma, const X2<Fp>&, const Fp& mb, const X2<Fp>&) { any |= (ma.v[0] | mb.v[0]) != 0; }
    __device__ __forceinline__ void pair(const Fp& m, const X2<Fp>&, const X2<Fp>&) { any |= m.v[0] != 0; }
    __device__ __forceinline__ void single(const Fp& m, const X2<Fp>&) { any |= m.v[0] != 0; }
};
template <int N>
struct BusFractions {  // helper e = num[e] / den[e]
    static constexpr int UNROLL = 16;
    gl2 num[N], den[N];
    int e = 0;
    __device__ __forceinline__ void set(const X2<Fp>& n, const X2<Fp>& d) {
        num[e] = gl2{n.a.v[0], n.b.v[0]}, den[e] = gl2{d.a.v[0], d.b.v[0]};
        ++e;
    }
    __device__ __forceinline__ void put(const Fp& ma, const X2<Fp>& da, const Fp& mb, const X2<Fp>& db) { set(db * ma + da * mb, da * db); }
    __device__ __forceinline__ void pair(const Fp& m, const X2<Fp>& da, const X2<Fp>& db) { set((da + db) * m, da * db); }
    __device__ __forceinline__ void single(const Fp& m, const X2<Fp>& d) { set(X2<Fp>{m, Fp::from(0)}, d); }
};
template <class Air>
struct BusPer {  // the row's periodic values for Air::messages
    Fp v[Air::BUS_PERIODIC ? Air::PERIODIC : 1];
    __device__ __forceinline__ const Fp* at(size_t row) {
        if constexpr (Air::BUS_PERIODIC) {
            uint64_t w[Air::PERIODIC] = {};
            Air::bus_periodic(row, w);
#pragma unroll
            for (int q = 0; q < Air::PERIODIC; ++q) v[q] = Fp::from(w[q]);
            return v;
        } else return nullptr;
    }
};

template <class Air>
__global__ __launch_bounds__(Air::BUS_BLOCK) void k_bus_aux(const uint64_t* __restrict__ tr, uint64_t* __restrict__ aux, size_t n, gl2 beta, gl2 gamma, BusPub pubw) {
    constexpr int N = Air::N_HELP, ROWS = Air::BUS_ROWS;
    const size_t i = blockIdx.x * (size_t)Air::BUS_BLOCK + threadIdx.x;
    if (i >= n / ROWS) return;
    const size_t row = ROWS * i;
    const RowViewN<1> loc{tr, n, {row}};
    Fp pub[Air::PUB];
#pragma unroll
    for (int q = 0; q < Air::PUB; ++q) pub[q] = Fp::from(pubw.w[q]);
    const bus::Bus<X2<Fp>> bus(Fp::from(beta.a), Fp::from(beta.b), Fp::from(gamma.a), Fp::from(gamma.b));
    gl2 h[N];
#pragma unroll
    for (int e = 0; e < N; ++e) h[e] = gl2{0, 0};
    BusPer<Air> pv;
    const Fp* per = pv.at(row);
    BusLive live;
    Air::template messages<Fp>(loc, per, pub, bus, live);
    if (live.any) {
        BusFractions<N> f;
        Air::template messages<Fp>(loc, per, pub, bus, f);
        gl2_batch_div(f.num, f.den, h);
    }
    gl2 sum = h[0];
#pragma unroll
    for (int e = 1; e < N; ++e) sum = gl2_add(sum, h[e]);
#pragma unroll
    for (int e = 0; e < N; ++e) {
        uint64_t *ca = aux + (size_t)(2 * e) * n + row, *cb = aux + (size_t)(2 * e + 1) * n + row;
        const gl2 v = h[e];
#pragma unroll 8
        for (int r = 0; r < ROWS; ++r) ca[r] = v.a, cb[r] = v.b;
    }
    uint64_t *za = aux + (size_t)(2 * N) * n + row, *zb = aux + (size_t)(2 * N + 1) * n + row;
#pragma unroll 8
    for (int r = 0; r < ROWS; ++r) za[r] = r == 0 ? sum.a : 0, zb[r] = r == 0 ? sum.b : 0;  // increments; the scan makes them the running sum
}

template <class Air>
int32_t bus_gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    static_assert(Air::PUB <= BUS_PUB_MAX && (Air::BUS_ROWS == 1 || Air::BUS_ROWS == 32), "bus_aux.cuh: the table's shape");
    const size_t n = (size_t)1 << log_n, lanes = n / Air::BUS_ROWS;
    BusPub pubw{};
    memcpy(pubw.w, pub, Air::PUB * sizeof(uint64_t));
    hipLaunchKernelGGL(k_bus_aux<Air>, dim3((unsigned)((lanes + Air::BUS_BLOCK - 1) / Air::BUS_BLOCK)), dim3(Air::BUS_BLOCK), 0, ctx->stream, trace, aux, n, gl2{chal[0], chal[1]},
                       gl2{chal[2], chal[3]}, pubw);
    VX_HIP(hipGetLastError());
    return vx_bus_close_dev(ctx, aux + (size_t)(2 * Air::N_HELP) * n, log_n, aux_pub);
}
