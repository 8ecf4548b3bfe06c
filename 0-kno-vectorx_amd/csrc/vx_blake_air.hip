// K8: witness/trace generation for BlakeChainAir on the GPU (the header_range circuit that proves it is vx_header_range.hip).
//   kernel A  k_blake_chain: one lane per header -- digest + the chaining value before every
//             128-byte chunk (the only sequential part of BLAKE2b);
//   kernel B  k_blake_trace: one lane per TRACE ROW (block b, r = row mod 16): recomputes
//             the <= 12 rounds it needs from the chunk's chaining value and writes the row
//             packed as 96 words; k_blake_expand unpacks words into the 729 byte / limb / bit
//             cells, a block writing 16 KB runs of one column at a time;
//             k_blake_count: the multiplicities of the two lookup tables, counted from the packed
//             words in block-private LDS histograms (one workgroup per part of the bins and slice
//             of the rows); k_blake_mult adds the slices up into the M1 / M2 columns;
//   kernel C  k_blake_aux: the logUp helper columns once the lookup challenges are known.
// Replaces the curta Blake2b witness generation behind hash_encoded_header
// (/root/reference circuits/builder/header.rs:14-19) for the synthetic header chain.
#include <string.h>

#include "air_blake.cuh"
#include "vx_internal.h"


// SCALE compact mode of a u32 (decoder.rs:39-92): 1 / 2 / 4 / 5 bytes
static uint8_t compact_mode(uint32_t v) { return v < (1u << 6) ? 0 : v < (1u << 14) ? 1 : v < (1u << 30) ? 2 : 3; }

struct BlockDesc {
    uint64_t msg_off;  // byte offset of the 128-byte chunk in the headers buffer; ~0 = padding block
    uint32_t t, inc;
    uint32_t D[8];     // digest register before this block
    uint8_t fin, first, act, mode;  // mode: SCALE compact mode (0..3) of the header's block number
    uint32_t num;      // block number of the header this chunk belongs to
    uint32_t size;     // length of the whole message (< 2^24)
};

__device__ __forceinline__ uint64_t b_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

__device__ __forceinline__ void carries(uint64_t o1, uint64_t o2, uint64_t o3, uint8_t* out) {
    uint64_t lo = (o1 & 0xFFFFFFFFULL) + (o2 & 0xFFFFFFFFULL) + (o3 & 0xFFFFFFFFULL);
    uint64_t klo = lo >> 32;
    uint64_t hi = (o1 >> 32) + (o2 >> 32) + (o3 >> 32) + klo;
    out[0] = (uint8_t)klo;
    out[1] = (uint8_t)(hi >> 32);
}
__device__ __forceinline__ void g_mix(uint64_t* v, int ia, int ib, int ic, int id, uint64_t x, uint64_t y) {
    uint64_t a = v[ia], b = v[ib], c = v[ic], d = v[id];
    uint64_t a1 = a + b + x, d1 = b_rotr(d ^ a1, 32), c1 = c + d1, b1 = b_rotr(b ^ c1, 24);
    uint64_t a2 = a1 + b1 + y, d2 = b_rotr(d1 ^ a2, 16), c2 = c1 + d2, b2 = b_rotr(b1 ^ c2, 63);
    v[ia] = a2, v[ib] = b2, v[ic] = c2, v[id] = d2;
}
__device__ void blake_round(uint64_t* v, const uint64_t* m, int round) {
    const uint8_t* s = blk::ORDER[round + 1];  // ORDER[r] for r = 1..12 is sigma[r-1]
    for (int k = 0; k < 4; ++k) g_mix(v, k, 4 + k, 8 + k, 12 + k, m[s[2 * k]], m[s[2 * k + 1]]);
    for (int j = 0; j < 4; ++j) g_mix(v, j, 4 + (j + 1) % 4, 8 + (j + 2) % 4, 12 + (j + 3) % 4, m[s[8 + 2 * j]], m[s[8 + 2 * j + 1]]);
}
__device__ void blake_init_v(uint64_t* v, const uint64_t* h, uint64_t t, bool fin) {
    for (int i = 0; i < 8; ++i) v[i] = h[i], v[8 + i] = blk::IV[i];
    v[12] ^= t;
    if (fin) v[14] = ~v[14];
}

// one lane per header: digest and the chaining value in front of each chunk
__global__ __launch_bounds__(64) void k_blake_chain(const uint8_t* msgs, size_t stride, const uint32_t* sizes, size_t n,
                                                    const uint32_t* block_base, uint64_t* hchain, uint8_t* digests) {
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t* p = (const uint64_t*)(msgs + i * stride);
    const uint32_t len = sizes[i];
    const uint32_t nchunks = len == 0 ? 1 : (len + 127) / 128;
    uint64_t h[8], m[16], v[16];
    for (int k = 0; k < 8; ++k) h[k] = blk::IV[k];
    h[0] ^= 0x01010020ULL;
    for (uint32_t cidx = 0; cidx < nchunks; ++cidx) {
        uint64_t* hc = hchain + 8 * ((size_t)block_base[i] + cidx);
        for (int k = 0; k < 8; ++k) hc[k] = h[k];
        const bool fin = cidx + 1 == nchunks;
        const uint32_t off = 128 * cidx, rem = fin ? len - off : 128;
        for (int k = 0; k < 16; ++k) {
            uint32_t b = 8 * k;
            uint64_t w = 0;
            if (b < rem) {
                w = p[(off >> 3) + k];
                if (rem - b < 8) w &= (1ULL << (8 * (rem - b))) - 1;
            }
            m[k] = w;
        }
        blake_init_v(v, h, fin ? len : off + 128, fin);
        for (int r = 0; r < 12; ++r) blake_round(v, m, r);
        for (int k = 0; k < 8; ++k) h[k] ^= v[k] ^ v[k + 8];
    }
    uint64_t* d = (uint64_t*)(digests + 32 * i);
    d[0] = h[0], d[1] = h[1], d[2] = h[2], d[3] = h[3];
}

// ---- trace rows ---------------------------------------------------------------------------------------------------
// A row lane that stored its 729 cells one column at a time walked 729 columns 8n bytes apart: the walk's address
// translation, not its bytes, set the time (7.8 ms for 3 GB).  So the row is produced in two steps:
//   k_blake_trace   one lane per trace row (block b, r = row mod 16): recomputes the <= 12 rounds it needs from the
//                   chunk's chaining value and stores the row PACKED as 96 words (stage[w * n + row]);
//   k_blake_expand  one block per (2048 rows, packed word): every cell is (word >> shift) & mask, and a block writes
//                   16 KB runs of one column at a time.
// Packed words: 8 per G (A1 D1 C1 B1 A2 D2 C2 X; L / T are the low 7 bits / top bit of X's bytes), then
constexpr int SW_CAR = 64, SW_MS = 65, SW_MB = 81, SW_HL = 82, SW_D = 90, SW_FLAGS = 94, SW_TN = 95, SW_WIN = 96, N_STAGE = 97;
// SW_CAR: 32 carries x 2 bits; SW_MS: the 16 message words in this row's order; SW_D: 4 words of two limbs;
// SW_FLAGS: ACT FIN FIRST CAP FA MDF0 MDF1 MDF3 (bits 0..7), INC (8..15), CNT (16..23), MK (24..31), E (32..39), SZ (40..63); SW_TN: T (low half),
// NUM (high half); SW_WIN: KOF (bits 0..23), TR (bit 32)
struct ExpandEntry {
    uint16_t col;
    uint8_t shift, bits;
};
__global__ __launch_bounds__(256) void k_blake_trace(const uint8_t* msgs, const BlockDesc* descs, const uint64_t* hchain, size_t n_real,
                                                     uint64_t* __restrict__ stage, size_t n, uint32_t win_off, uint32_t win_len) {
    using namespace blk;
    // n is a multiple of the block size (n >= 2^16)
    const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t b = row >> 4;
    const int r = (int)(row & 15);
    const BlockDesc d = descs[b];
    uint64_t h[8], m[16], v[16];
    if (b < n_real) {
        for (int k = 0; k < 8; ++k) h[k] = hchain[8 * b + k];
        const uint64_t* p = (const uint64_t*)(msgs + d.msg_off);
        for (int k = 0; k < 16; ++k) {
            uint32_t bb = 8 * k;
            uint64_t w = 0;
            if (bb < d.inc) {
                w = p[k];
                if (d.inc - bb < 8) w &= (1ULL << (8 * (d.inc - bb))) - 1;
            }
            m[k] = w;
        }
    } else {  // padding block: the 40-byte message D || compact(number) || 0..
        for (int k = 0; k < 8; ++k) h[k] = IV[k];
        h[0] ^= 0x01010020ULL;
        for (int k = 0; k < 16; ++k) m[k] = k < 4 ? ((uint64_t)d.D[2 * k] | ((uint64_t)d.D[2 * k + 1] << 32)) : 0;
        // bytes 32..: SCALE compact of the last block number in its own mode (decoder.rs:39-92)
        m[4] = d.mode == 0 ? 4ULL * d.num : d.mode == 1 ? 4ULL * d.num + 1 : d.mode == 2 ? 4ULL * d.num + 2 : (3ULL | ((uint64_t)d.num << 8));
    }
    auto st = [&](int w) -> uint64_t& { return stage[(size_t)w * n + row]; };
    auto gw = [&](int k, int slot) -> uint64_t& { return st(8 * k + slot); };  // slot 7 = X (L / T)
    // ---- G area + carries
    blake_init_v(v, h, d.t, d.fin);
    uint64_t carw = 0;
    if (r >= 1 && r <= 12) {
        for (int q = 0; q + 1 < r; ++q) blake_round(v, m, q);
        const uint8_t* sg = ORDER[r];  // sigma of round r - 1
        auto G = [&](int k, uint64_t& va, uint64_t& vb, uint64_t& vc, uint64_t& vd, uint64_t x, uint64_t y) {
            const uint64_t a = va, bq = vb, c = vc, dd = vd;
            const uint64_t a1 = a + bq + x, d1 = b_rotr(dd ^ a1, 32), c1 = c + d1, b1 = b_rotr(bq ^ c1, 24);
            const uint64_t a2 = a1 + b1 + y, d2 = b_rotr(d1 ^ a2, 16), c2 = c1 + d2, b2 = b_rotr(b1 ^ c2, 63);
            gw(k, S_A1) = a1, gw(k, S_D1) = d1, gw(k, S_C1) = c1, gw(k, S_B1) = b1, gw(k, S_A2) = a2, gw(k, S_D2) = d2, gw(k, S_C2) = c2, gw(k, 7) = b1 ^ c2;
            uint8_t car[4];
            carries(a, bq, x, car);
            carries(a1, b1, y, car + 2);
            carw |= ((uint64_t)car[0] | ((uint64_t)car[1] << 2) | ((uint64_t)car[2] << 4) | ((uint64_t)car[3] << 6)) << (8 * k);
            va = a2, vb = b2, vc = c2, vd = d2;
        };
        G(0, v[0], v[4], v[8], v[12], m[sg[0]], m[sg[1]]);
        G(1, v[1], v[5], v[9], v[13], m[sg[2]], m[sg[3]]);
        G(2, v[2], v[6], v[10], v[14], m[sg[4]], m[sg[5]]);
        G(3, v[3], v[7], v[11], v[15], m[sg[6]], m[sg[7]]);
        G(4, v[0], v[5], v[10], v[15], m[sg[8]], m[sg[9]]);
        G(5, v[1], v[6], v[11], v[12], m[sg[10]], m[sg[11]]);
        G(6, v[2], v[7], v[8], v[13], m[sg[12]], m[sg[13]]);
        G(7, v[3], v[4], v[9], v[14], m[sg[14]], m[sg[15]]);
    } else {
        for (int w = 0; w < 64; ++w) st(w) = 0;  // (a lane's later store to the same address wins)
        if (r == 0) {
            for (int w = 0; w < 16; ++w) {
                const int mm = w & 3;
                if (w < 4) gw(4 + w, S_A2) = v[w];
                else if (w < 8) gw(4 + (mm + 3) % 4, 7) = b_rotr(v[w], 1);  // 2 L[j] + T[j-1] = byte j of v[w]
                else if (w < 12) gw(4 + (mm + 2) % 4, S_C2) = v[w];
                else gw(4 + (mm + 1) % 4, S_D2) = v[w];
            }
        } else {
            for (int q = 0; q < 12; ++q) blake_round(v, m, q);
            if (r <= 14)
                for (int w = 0; w < 8; ++w) {
                    const uint64_t u = v[w] ^ v[8 + w];
                    const uint64_t x = r == 13 ? v[w] : u, y = r == 13 ? v[8 + w] : h[w];
                    gw(w, S_D1) = x, gw(w, S_A2) = y, gw(w, S_D2) = b_rotr(x ^ y, 16);
                }
        }
    }
    st(SW_CAR) = carw;
    uint64_t h_out[8];
    if (r >= 13)
        for (int k = 0; k < 8; ++k) h_out[k] = h[k] ^ v[k] ^ v[k + 8];
    // ---- message schedule + bytes of natural word r (range checked as (byte, 0, byte) in T1)
    for (int s = 0; s < 16; ++s) st(SW_MS + s) = m[ORDER[r][s]];
    st(SW_MB) = m[r];
    // ---- H register, digest register
    for (int w = 0; w < 8; ++w) st(SW_HL + w) = r <= 13 ? h[w] : (r == 14 ? h_out[w] : (d.fin ? (w == 0 ? IV[0] ^ 0x01010020ULL : IV[w]) : h_out[w]));
    const bool cap = d.act && d.fin;
    for (int j = 0; j < 4; ++j) st(SW_D + j) = (r == 15 && cap) ? h_out[j] : ((uint64_t)d.D[2 * j] | ((uint64_t)d.D[2 * j + 1] << 32));
    // ---- flags, counters
    uint64_t mk = 0;
    for (int bq = 0; bq < 8; ++bq) mk |= (uint64_t)((uint32_t)(8 * r + bq) < d.inc ? 1 : 0) << bq;
    const uint64_t cnt = d.inc < (uint32_t)(8 * (r + 1)) ? d.inc : (uint32_t)(8 * (r + 1));
    // the row's window: rows 4..8 of a first chunk can hold state-root bytes (right behind the compact number, decoder.rs:121-128),
    // every other row data-root bytes (the last 32 bytes of the message, :132-149).  E[b]: byte 8r + b of this chunk lies in the
    // window's 32 bytes of an active message
    const bool srw = d.first && r >= 4 && r <= 8;
    // win_len > 0 (rotate, bus mode 2): outside those rows the window is bytes [win_off, win_off + win_len) of the message instead
    const uint32_t clen = d.mode == 0 ? 1 : d.mode == 1 ? 2 : d.mode == 2 ? 4 : 5, kof = srw ? 32 + clen : (win_len ? win_off : d.size - 32);
    const uint32_t wlen = (win_len && !srw) ? win_len : 32;
    uint64_t eb = 0;
    for (int bq = 0; bq < 8; ++bq) {
        const uint32_t pos = d.t - d.inc + 8 * r + bq;
        eb |= (uint64_t)((d.act && pos >= kof && pos < kof + wlen && (!win_len || (pos < d.size && !srw))) ? 1 : 0) << bq;
    }
    const uint64_t mdf = d.first ? (uint64_t)(d.mode == 0) | ((uint64_t)(d.mode == 1) << 1) | ((uint64_t)(d.mode == 3) << 2) : 0;
    st(SW_FLAGS) = (uint64_t)d.act | ((uint64_t)d.fin << 1) | ((uint64_t)d.first << 2) | ((uint64_t)(cap ? 1 : 0) << 3) | ((uint64_t)((d.first && d.act) ? 1 : 0) << 4) |
                   (mdf << 5) | ((uint64_t)d.inc << 8) | (cnt << 16) | (mk << 24) | (eb << 32) | ((uint64_t)d.size << 40);
    st(SW_TN) = (uint64_t)d.t | ((uint64_t)d.num << 32);
    st(SW_WIN) = (uint64_t)kof | ((uint64_t)(srw ? 0 : 1) << 32);
}
constexpr int EXP_RPL = 8;  // rows per lane: a block writes 8 x 2 KB = 16 KB of a column per visit
__global__ __launch_bounds__(256) void k_blake_expand(const uint64_t* __restrict__ stage, uint64_t* __restrict__ tr, size_t n, const ExpandEntry* __restrict__ ent,
                                                      const uint32_t* __restrict__ off) {
    const int w = blockIdx.y;
    const size_t row0 = (size_t)blockIdx.x * (256 * EXP_RPL) + threadIdx.x;
    uint64_t x[EXP_RPL];
#pragma unroll
    for (int rr = 0; rr < EXP_RPL; ++rr) {
        const size_t row = row0 + 256 * (size_t)rr;
        x[rr] = row < n ? stage[(size_t)w * n + row] : 0;
    }
    for (uint32_t e = off[w]; e < off[w + 1]; ++e) {
        const ExpandEntry E = ent[e];
        const uint64_t mask = E.bits == 64 ? ~0ULL : ((1ULL << E.bits) - 1);
        uint64_t* c = tr + (size_t)E.col * n;
#pragma unroll
        for (int rr = 0; rr < EXP_RPL; ++rr) {
            const size_t row = row0 + 256 * (size_t)rr;
            if (row < n) c[row] = (x[rr] >> E.shift) & mask;
        }
    }
}
// cell <- (packed word, shift, width) for every main column except the two multiplicities
static void blake_expand_table(std::vector<ExpandEntry>& ent, std::vector<uint32_t>& off) {
    using namespace blk;
    std::vector<std::vector<ExpandEntry>> per(N_STAGE);
    auto add = [&](int w, int col, int shift, int bits) { per[w].push_back(ExpandEntry{(uint16_t)col, (uint8_t)shift, (uint8_t)bits}); };
    for (int k = 0; k < 8; ++k) {
        for (int slot = 0; slot < 7; ++slot)
            for (int j = 0; j < 8; ++j) add(8 * k + slot, GC(k, slot, j), 8 * j, 8);
        for (int j = 0; j < 8; ++j) add(8 * k + 7, GC(k, S_L, j), 8 * j, 7), add(8 * k + 7, GC(k, S_T, j), 8 * j + 7, 1);
        for (int q = 0; q < 4; ++q) add(SW_CAR, CAR(k, q), 8 * k + 2 * q, 2);
    }
    for (int s = 0; s < 16; ++s) add(SW_MS + s, MS(s, 0), 0, 32), add(SW_MS + s, MS(s, 1), 32, 32);
    for (int j = 0; j < 8; ++j) add(SW_MB, MB0 + j, 8 * j, 8);
    for (int w = 0; w < 8; ++w) add(SW_HL + w, HL(w, 0), 0, 32), add(SW_HL + w, HL(w, 1), 32, 32);
    for (int j = 0; j < 4; ++j) add(SW_D + j, D0 + 2 * j, 0, 32), add(SW_D + j, D0 + 2 * j + 1, 32, 32);
    add(SW_FLAGS, ACT, 0, 1), add(SW_FLAGS, FIN, 1, 1), add(SW_FLAGS, FIRST, 2, 1), add(SW_FLAGS, CAP, 3, 1), add(SW_FLAGS, FA, 4, 1);
    add(SW_FLAGS, INC, 8, 8), add(SW_FLAGS, CNT, 16, 8);
    for (int i = 0; i < 8; ++i) add(SW_FLAGS, IB0 + i, 8 + i, 1), add(SW_FLAGS, MK0 + i, 24 + i, 1), add(SW_FLAGS, E0 + i, 32 + i, 1);
    add(SW_FLAGS, SZ, 40, 24);
    add(SW_FLAGS, MDF0, 5, 1), add(SW_FLAGS, MDF1, 6, 1), add(SW_FLAGS, MDF3, 7, 1);
    add(SW_WIN, KOF, 0, 24), add(SW_WIN, TR, 32, 1);
    add(SW_TN, T, 0, 32), add(SW_TN, NUM, 32, 32);
    for (int i = 0; i < 32; ++i) add(SW_TN, TB0 + i, i, 1);
    off.assign(1, 0);
    for (auto& v : per) {
        ent.insert(ent.end(), v.begin(), v.end());
        off.push_back((uint32_t)ent.size());
    }
}
// ---- multiplicities -----------------------------------------------------------------------------------------------
// Every row looks up to 256 (a, b) byte pairs in T1 (key a | b << 8) and 64 in T2: ~100 M lookups on random bins at 2^19 rows.
// As global atomics they held the whole chip for 4 ms while issuing next to nothing.  They are counted in LDS instead:
//   k_blake_count  one workgroup per (part, slice).  A part is a contiguous range of 2^PART_BITS bins of one table (T1 with
//                  b < 128, T1 with b >= 128, T2 low, T2 high at 15 bits), a slice every CNT_SLICES-th tile of 1024 rows.  The
//                  workgroup re-derives the lookups of its rows from the packed words (the b / d operands of a G are
//                  rotl(B1, 24) ^ C1 and rotl(D1, 32) ^ A1), counts those that fall into its part in a private 32-bit LDS
//                  histogram, and stores it with plain stores to partial[part][slice][bin]; a slice without lookups stores zeros,
//                  so nothing is cleared beforehand.  The (byte, 0, byte) range checks of the message bytes are T1 keys with b = 0.
//   k_blake_mult   adds the slices of the bin that belongs to its row.
// T1 has three lookups for every one of T2, so its parts get three quarters of the workgroups.
#ifndef VX_PART_BITS
#define VX_PART_BITS 15  // 128 KiB of LDS, one workgroup per CU.  14 (64 KiB, twice the parts): 226 us against 142 alone, no better in a proof (profiles/README.md)
#endif
constexpr int PART_BITS = VX_PART_BITS, PART = 1 << PART_BITS, PARTS = 65536 >> PART_BITS;  // PARTS per table
constexpr int CNT_WGS = 256, CNT_THREADS = 1024;                                             // about one workgroup per CU
constexpr int CNT_SLICES1 = 3 * CNT_WGS / (4 * PARTS), CNT_SLICES2 = CNT_WGS / (4 * PARTS);
static_assert(PART_BITS >= 12 && PART_BITS <= 15 && CNT_SLICES2 >= 1, "a part is 16 .. 128 KiB of LDS");
__global__ __launch_bounds__(CNT_THREADS) void k_blake_count(const uint64_t* __restrict__ stage, size_t n, uint32_t* __restrict__ partial) {
    using namespace blk;
    __shared__ uint32_t h[PART];
    const bool t2 = blockIdx.x >= PARTS * CNT_SLICES1;
    const uint32_t wg = t2 ? blockIdx.x - PARTS * CNT_SLICES1 : blockIdx.x, slices = t2 ? CNT_SLICES2 : CNT_SLICES1;
    const uint32_t sub = wg / slices, slice = wg % slices;
    for (int i = threadIdx.x; i < PART; i += CNT_THREADS) h[i] = 0;
    __syncthreads();
    auto look = [&](uint64_t a, uint64_t b) {  // 8 byte lookups (a_j, b_j, .)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t key = (uint32_t)((a >> (8 * j)) & 0xFF) | ((uint32_t)((b >> (8 * j)) & 0xFF) << 8);
            if ((key >> PART_BITS) == sub) atomicAdd(&h[key & (PART - 1)], 1u);
        }
    };
    auto rotl = [](uint64_t x, int s) -> uint64_t { return (x << s) | (x >> (64 - s)); };
    // n is a multiple of the tile (n >= 2^16)
    for (size_t row = (size_t)slice * CNT_THREADS + threadIdx.x; row < n; row += (size_t)slices * CNT_THREADS) {
        const int r = (int)(row & 15);
        auto st = [&](int w) -> uint64_t { return stage[(size_t)w * n + row]; };
        const bool g_row = r >= 1 && r <= 12;
        if (t2) {
            if (g_row) {
#pragma unroll
                for (int k = 0; k < 8; ++k) look(st(8 * k + S_B1), st(8 * k + S_C2));
            }
        } else {
            if (g_row) {  // (d, A1), (b, C1), (D1, A2)
#pragma unroll 4
                for (int k = 0; k < 8; ++k) {
                    const uint64_t a1 = st(8 * k + S_A1), d1 = st(8 * k + S_D1), c1 = st(8 * k + S_C1), b1 = st(8 * k + S_B1), a2 = st(8 * k + S_A2);
                    look(rotl(d1, 32) ^ a1, a1), look(rotl(b1, 24) ^ c1, c1), look(d1, a2);
                }
            } else if (r == 13 || r == 14) {  // the feed-forward XORs
#pragma unroll
                for (int w = 0; w < 8; ++w) look(st(8 * w + S_D1), st(8 * w + S_A2));
            }
            if (sub == 0) look(st(SW_MB), 0);  // the message bytes' range checks
        }
    }
    __syncthreads();
    uint32_t* out = partial + (t2 ? (size_t)65536 * CNT_SLICES1 : 0) + ((size_t)sub * slices + slice) * PART;
    for (int i = threadIdx.x; i < PART; i += CNT_THREADS) out[i] = h[i];
}
// the multiplicity columns: all counts in the first copy of the periodic tables
__global__ __launch_bounds__(256) void k_blake_mult(const uint32_t* __restrict__ partial, uint64_t* tr, size_t n) {
    const size_t row = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (row >= n) return;
    uint64_t m1 = 0, m2 = 0;
    if (row < 65536) {
        const size_t sub = row >> PART_BITS, bin = row & (PART - 1);
        const uint32_t* p1 = partial + sub * CNT_SLICES1 * PART + bin;
        const uint32_t* p2 = partial + (size_t)65536 * CNT_SLICES1 + sub * CNT_SLICES2 * PART + bin;
        for (int s = 0; s < CNT_SLICES1; ++s) m1 += p1[(size_t)s * PART];
        for (int s = 0; s < CNT_SLICES2; ++s) m2 += p2[(size_t)s * PART];
    }
    tr[(size_t)blk::M1 * n + row] = m1;
    tr[(size_t)blk::M2 * n + row] = m2;
}

// ---- auxiliary columns (logUp) --------------------------------------------------------------------------------------
// k_blake_aux: one lane per (row i, unit u); i is the "next" row of the pair (i-1, i).  Units 0..7 = the 16 helper
// elements of G number u (two lookups each, h = m (1/D_u + 1/D_v); the four pairs of a group share ONE extension-field
// inversion, Montgomery's trick); unit 8 = the 4 message-byte range-check helpers and the table helper of row i.  Every
// unit leaves the sum of its helpers in part[u]; k_blake_aux_z adds them up into the running-sum increment
// Z(i) - Z(i-1) = sum_e h_e(i) - ht(i-1), stored at row i-1 and turned into Z by an exclusive scan.
struct AuxArgs {
    const uint64_t* tr;
    uint64_t* aux;
    uint64_t* part;  // [9][2][n]
    size_t n;
    gl2 beta, gamma;
    uint64_t first_number, tree_size, bus_on;  // the block number of leaf 0 (public input 18 in bus mode 1, else 16), public inputs 18, 19
};
#ifndef VX_AUX_WAVES
#define VX_AUX_WAVES 4  // measured: 2 -> 6.7 ms, 3 -> 6.4, 4 -> 4.9 (64 VGPRs + scratch: the kernel lives on occupancy hiding its dependent multiply chains)
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VX_AUX_WAVES, VX_AUX_WAVES))) void k_blake_aux(AuxArgs a) {
    using namespace blk;
    const size_t n = a.n, i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const int unit = blockIdx.y;
    if (i >= n) return;
    const size_t ip = (i + n - 1) & (n - 1);
    const int rl = (int)(ip & 15);  // row index (mod 16) of the LOCAL row: selectors are taken there
    const bool g_on = rl <= 11, m3 = rl <= 13;
    const bus::Bus<gl2> bus(a.beta.a, a.beta.b, a.gamma.a, a.gamma.b);
    auto N = [&](int col) -> uint64_t { return a.tr[(size_t)col * n + i]; };
    auto L = [&](int col) -> uint64_t { return a.tr[(size_t)col * n + ip]; };
    auto store = [&](int e, gl2 h) {
        a.aux[(size_t)(2 * e) * n + i] = h.a;
        a.aux[(size_t)(2 * e + 1) * n + i] = h.b;
    };
    gl2 hsum{0, 0};
    // four pairs (p_q = D_u D_v, s_q = D_u + D_v) -> h_q = s_q / p_q with one inversion
    auto four = [&](gl2* p, gl2* s, int e0) {
        const gl2 c1 = gl2_mul(p[0], p[1]), c2 = gl2_mul(c1, p[2]), c3 = gl2_mul(c2, p[3]);
        gl2 inv = gl2_inv(c3);
        const gl2 i3 = gl2_mul(inv, c2);
        inv = gl2_mul(inv, p[3]);
        const gl2 i2 = gl2_mul(inv, c1);
        inv = gl2_mul(inv, p[2]);
        const gl2 i1 = gl2_mul(inv, p[0]), i0 = gl2_mul(inv, p[1]);
        const gl2 iq[4] = {i0, i1, i2, i3};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const gl2 h = gl2_mul(s[q], iq[q]);
            store(e0 + q, h);
            hsum = gl2_add(hsum, h);
        }
    };
    if (unit < 8) {
        const int k = unit;
        const gl2 bt2 = bus.t2_base();
        auto out_byte_loc = [&](int w, int j) -> uint64_t {
            const int m = w & 3;
            if (w < 8) {  // only b (w = 4..7) and d (w = 12..15) operands enter a lookup
                const int kk = 4 + (m + 3) % 4;
                return 2 * L(GC(kk, S_L, j)) + L(GC(kk, S_T, (j + 7) & 7));
            }
            return L(GC(4 + (m + 1) % 4, S_D2, j));
        };
        auto in_byte = [&](int op, int j) -> uint64_t {
            if (k < 4) return out_byte_loc(4 * op + k, j);
            const int j0 = k - 4;
            if (op == 1) {
                const int kb = (j0 + 1) & 3;
                return 2 * N(GC(kb, S_L, j)) + N(GC(kb, S_T, (j + 7) & 7));
            }
            return N(GC((j0 + 3) & 3, S_D2, j));
        };
        auto denoms = [&](int grp, gl2* dd) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (grp == 0) dd[q] = bus.xor_row(in_byte(3, q), N(GC(k, S_A1, q)), N(GC(k, S_D1, (q + 4) & 7)));
                else if (grp == 1) dd[q] = bus.xor_row(in_byte(1, q), N(GC(k, S_C1, q)), N(GC(k, S_B1, (q + 5) & 7)));
                else if (grp == 2) dd[q] = bus.xor_row(N(GC(k, S_D1, q)), N(GC(k, S_A2, q)), N(GC(k, S_D2, (q + 6) & 7)));
                else dd[q] = bus.t2_row(bt2, N(GC(k, S_B1, q)), N(GC(k, S_C2, q)), N(GC(k, S_L, q)), N(GC(k, S_T, q)));
            }
        };
        // ONE extension-field inversion per lane (Montgomery's trick on two levels): pass 1 multiplies the 8 denominators
        // of every active group into c[grp]; the four c are inverted together; pass 2 recomputes the denominators (the
        // cells come back from cache) and unwinds each group with its 1 / c[grp].
        gl2 cg[4], tot{1, 0};
#pragma unroll 1
        for (int grp = 0; grp < 4; ++grp) {
            cg[grp] = gl2{1, 0};
            if (grp == 2 ? m3 : g_on) {
                gl2 dd[8];
                denoms(grp, dd);
                gl2 c = gl2_mul(dd[0], dd[1]);
#pragma unroll
                for (int q = 2; q < 8; ++q) c = gl2_mul(c, dd[q]);
                cg[grp] = c;
            }
        }
        // prefix products of cg, one inversion, suffix unwinding -> icg[grp] = 1 / cg[grp]
        const gl2 p01 = gl2_mul(cg[0], cg[1]), p012 = gl2_mul(p01, cg[2]);
        tot = gl2_mul(p012, cg[3]);
        gl2 inv = m3 ? gl2_inv(tot) : gl2{1, 0};
        gl2 icg[4];
        icg[3] = gl2_mul(inv, p012), inv = gl2_mul(inv, cg[3]);
        icg[2] = gl2_mul(inv, p01), inv = gl2_mul(inv, cg[2]);
        icg[1] = gl2_mul(inv, cg[0]), icg[0] = gl2_mul(inv, cg[1]);
#pragma unroll 1
        for (int grp = 0; grp < 4; ++grp) {
            const int e0 = (k * 4 + grp) * 4;
            if (grp == 2 ? m3 : g_on) {
                gl2 dd[8], p[4];
                denoms(grp, dd);
#pragma unroll
                for (int q = 0; q < 4; ++q) p[q] = gl2_mul(dd[2 * q], dd[2 * q + 1]);
                // 1 / p[q] = icg * (product of the other three pair products)
                const gl2 p01_ = gl2_mul(p[0], p[1]), p23_ = gl2_mul(p[2], p[3]);
                const gl2 a01 = gl2_mul(icg[grp], p23_), a23 = gl2_mul(icg[grp], p01_);  // 1 / (p0 p1), 1 / (p2 p3)
                const gl2 ip[4] = {gl2_mul(a01, p[1]), gl2_mul(a01, p[0]), gl2_mul(a23, p[3]), gl2_mul(a23, p[2])};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const gl2 h = gl2_mul(gl2_add(dd[2 * q], dd[2 * q + 1]), ip[q]);
                    store(e0 + q, h);
                    hsum = gl2_add(hsum, h);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) store(e0 + q, gl2{0, 0});
            }
        }
    } else {
        gl2 p[4], s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t b0 = N(MB0 + 2 * q), b1 = N(MB0 + 2 * q + 1);
            const gl2 du = bus.xor_row(b0, bus::None{}, b0), dv = bus.xor_row(b1, bus::None{}, b1);
            p[q] = gl2_mul(du, dv), s[q] = gl2_add(du, dv);
        }
        four(p, s, HM0);
        // bus sends of this row (it is the "next" row of its pair; r = its index in the block): byte b under E[b] as (leaf, position
        // in the root, byte, tree) -- state root (tree 0) on rows 4..8 of a first chunk, data root (tree 1) elsewhere
        {
            const int r = (int)(i & 15);
            const uint64_t leaf = gl_sub(N(NUM), a.first_number);
            const uint64_t pos0 = gl_sub(gl_add(gl_sub(N(T), N(INC)), (uint64_t)(8 * r)), N(KOF));
            const gl2 bbase = bus.byte_base(leaf, N(TR));
#pragma unroll 1
            for (int pair = 0; pair < 4; ++pair) {
                gl2 h{0, 0};
                const bool live = a.bus_on && N(ACT);
                const uint64_t e0 = live ? N(E0 + 2 * pair) : 0, e1 = live ? N(E0 + 2 * pair + 1) : 0;
                if (e0 | e1) {
                    const gl2 du = bus.byte(bbase, gl_add(pos0, 2 * pair), N(MB0 + 2 * pair));
                    const gl2 dv = bus.byte(bbase, gl_add(pos0, 2 * pair + 1), N(MB0 + 2 * pair + 1));
                    h = gl2_mul(gl2_add(gl2_scale(dv, e0), gl2_scale(du, e1)), gl2_inv(gl2_mul(du, dv)));
                }
                store(HB0 + pair, h);
                hsum = gl2_add(hsum, h);
            }
        }
        // table helper of this row: ht = M1 / D_t1 + M2 / D_t2
        const uint64_t m1 = N(M1), m2 = N(M2);
        gl2 ht{0, 0};
        if (m1 | m2) {
            const uint64_t ti = i & 65535, ta = ti & 255, tb = ti >> 8, x = ta ^ tb;
            const gl2 d1 = bus.xor_row(ta, tb, x), d2 = bus.t2_row(bus.t2_base(), ta, tb, x & 127, x >> 7);
            ht = gl2_mul(gl2_add(gl2_scale(d2, m1), gl2_scale(d1, m2)), gl2_inv(gl2_mul(d1, d2)));
        }
        store(HT, ht);
    }
    a.part[(size_t)(2 * unit) * n + i] = hsum.a;
    a.part[(size_t)(2 * unit + 1) * n + i] = hsum.b;
}
__global__ __launch_bounds__(256) void k_blake_aux_z(const uint64_t* part, uint64_t* aux, size_t n) {
    using namespace blk;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t ip = (i + n - 1) & (n - 1);
    uint64_t sa = 0, sb = 0;
#pragma unroll
    for (int u = 0; u < 9; ++u) sa = gl_add(sa, part[(size_t)(2 * u) * n + i]), sb = gl_add(sb, part[(size_t)(2 * u + 1) * n + i]);
    aux[(size_t)(2 * ZZ) * n + ip] = gl_sub(sa, aux[(size_t)(2 * HT) * n + ip]);
    aux[(size_t)(2 * ZZ + 1) * n + ip] = gl_sub(sb, aux[(size_t)(2 * HT + 1) * n + ip]);
}

int32_t BlakeAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    const size_t n = (size_t)1 << log_n;
    uint64_t* part = (uint64_t*)vx_pool_alloc(ctx, 18 * n * 8);
    if (!part) return vx_fail(ctx, VX_ERR_OOM, "blake aux: out of device memory");
    AuxArgs a{trace, aux, part, n, gl2{chal[0], chal[1]}, gl2{chal[2], chal[3]}, pub[19] == 1 ? pub[18] : pub[16], pub[18], pub[19]};  // bus mode 1 counts leaves from the range's first block
    hipLaunchKernelGGL(k_blake_aux, dim3((unsigned)((n + 255) / 256), 9), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_blake_aux_z, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint64_t*)part, aux, n);
    const hipError_t e = hipGetLastError();
    vx_pool_free(ctx, part);  // recycled only by later work on the same stream
    if (e != hipSuccess) return vx_fail(ctx, VX_ERR_DEVICE, "blake aux: %s", hipGetErrorString(e));
    return vx_bus_close_dev(ctx, aux + (size_t)(2 * blk::ZZ) * n, log_n, aux_pub);
}

extern "C" {

int32_t vx_blake_chain_trace(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_headers,
                             const uint8_t trusted_hash[32], uint32_t first_block_number, uint32_t tree_size, uint32_t window_offset, uint32_t window_length,
                             int log_n, vx_buf* trace_out, uint64_t public_inputs_out[20], uint8_t* digests_out) {
    if (!ctx || !headers || !sizes || !trusted_hash || !trace_out || !public_inputs_out) return VX_ERR_ARG;
    VX_CHECK(stride % 128 == 0 && stride > 0, "blake trace: stride %zu must be a positive multiple of 128", stride);
    VX_CHECK(n_headers >= 1 && n_headers * stride <= headers->n * 8, "blake trace: headers exceed the buffer");
    VX_CHECK(log_n >= blk::TABLE_LOG && log_n <= 24, "blake trace: log_n %d out of range [16, 24] (the trace holds one copy of the 2^16-row lookup tables)", log_n);
    VX_CHECK((uint64_t)first_block_number + n_headers <= (1ULL << 32), "blake trace: block numbers %u.. overflow 32 bits", first_block_number);
    VX_CHECK(!window_length || (n_headers == 1 && !tree_size && window_offset >= 72 && (uint64_t)window_offset + window_length < (1u << 24)),
             "blake trace: a byte window (offset %u, length %u) goes with one header, no Merkle tree, and starts behind the state root", window_offset, window_length);
    VX_CHECK(window_length || window_offset == 0 || (tree_size && window_offset < first_block_number), "blake trace: a leaf offset (%u) goes with tree_size != 0", window_offset);
    const size_t n = (size_t)1 << log_n, n_blocks = n >> 4;
    VX_CHECK(trace_out->n >= n * blk::COLS, "blake trace: trace buffer holds %zu < %zu elements", trace_out->n, n * (size_t)blk::COLS);
    std::vector<uint32_t> base(n_headers);
    size_t n_real = 0;
    for (size_t i = 0; i < n_headers; ++i) {
        const uint32_t clen = (uint32_t[]){1, 2, 4, 5}[compact_mode(first_block_number + (uint32_t)i)];  // parent hash + compact number must fit
        VX_CHECK(sizes[i] <= stride && sizes[i] >= 32 + clen && sizes[i] < (1u << 24), "blake trace: header %zu has size %u", i, sizes[i]);
        VX_CHECK(!tree_size || sizes[i] >= 104,
                 "blake trace: header %zu has size %u (shorter than 104 bytes its state root and data root would share trace rows; no Avail header is)", i, sizes[i]);
        base[i] = (uint32_t)n_real;
        n_real += (sizes[i] + 127) / 128;
    }
    VX_CHECK(n_real <= n_blocks, "blake trace: %zu compressions do not fit 2^%d rows (%zu blocks)", n_real, log_n, n_blocks);
    // device scratch: sizes | block_base | digests | hchain | descs
    const size_t w_sizes = (n_headers * 4 + 7) / 8, w_dig = n_headers * 4, w_hc = n_real * 8;
    const size_t w_desc = (n_blocks * sizeof(BlockDesc) + 7) / 8;
    const size_t w_hist = (size_t)65536 * (CNT_SLICES1 + CNT_SLICES2) / 2;  // a slice of uint32 counters per table bin: CNT_SLICES1 for T1, CNT_SLICES2 for T2
    std::vector<ExpandEntry> ent;
    std::vector<uint32_t> eoff;
    blake_expand_table(ent, eoff);
    VX_CHECK(ent.size() == (size_t)blk::COLS - 2, "blake trace: expansion table covers %zu of %d columns", ent.size(), blk::COLS - 2);
    const size_t w_ent = (ent.size() * sizeof(ExpandEntry) + 7) / 8, w_eoff = (eoff.size() * 4 + 7) / 8, w_stage = (size_t)N_STAGE * n;
    uint64_t* sc;
    VX_TRY(vx_scratch(ctx, 2 * w_sizes + w_dig + w_hc + w_desc + w_hist + w_ent + w_eoff + w_stage, &sc));
    uint32_t* d_sizes = (uint32_t*)sc;
    uint32_t* d_base = (uint32_t*)(sc + w_sizes);
    uint8_t* d_dig = (uint8_t*)(sc + 2 * w_sizes);
    uint64_t* d_hc = sc + 2 * w_sizes + w_dig;
    BlockDesc* d_desc = (BlockDesc*)(d_hc + w_hc);
    uint32_t* d_hist = (uint32_t*)(d_hc + w_hc + w_desc);
    ExpandEntry* d_ent = (ExpandEntry*)(d_hc + w_hc + w_desc + w_hist);
    uint32_t* d_eoff = (uint32_t*)(d_hc + w_hc + w_desc + w_hist + w_ent);
    uint64_t* d_stage = d_hc + w_hc + w_desc + w_hist + w_ent + w_eoff;
    VX_HIP(hipMemcpyAsync(d_ent, ent.data(), ent.size() * sizeof(ExpandEntry), hipMemcpyHostToDevice, ctx->stream));
    VX_HIP(hipMemcpyAsync(d_eoff, eoff.data(), eoff.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    VX_HIP(hipMemcpyAsync(d_sizes, sizes, n_headers * 4, hipMemcpyHostToDevice, ctx->stream));
    VX_HIP(hipMemcpyAsync(d_base, base.data(), n_headers * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_blake_chain, dim3((unsigned)((n_headers + 63) / 64)), dim3(64), 0, ctx->stream, (const uint8_t*)headers->d,
                       stride, (const uint32_t*)d_sizes, n_headers, (const uint32_t*)d_base, d_hc, d_dig);
    VX_HIP(hipGetLastError());
    std::vector<uint8_t> dig(32 * n_headers);
    VX_HIP(hipMemcpyAsync(dig.data(), d_dig, dig.size(), hipMemcpyDeviceToHost, ctx->stream));
    VX_HIP(vx_wait(ctx));
    // block descriptors (host): the link rule is checked here too, so a broken chain fails loudly
    std::vector<BlockDesc> descs(n_blocks);
    uint8_t D[32];
    memcpy(D, trusted_hash, 32);
    size_t bi = 0;
    for (size_t i = 0; i < n_headers; ++i) {
        const uint32_t nch = (sizes[i] + 127) / 128;
        for (uint32_t cidx = 0; cidx < nch; ++cidx, ++bi) {
            BlockDesc& d = descs[bi];
            memset(&d, 0, sizeof d);
            d.fin = cidx + 1 == nch;
            d.first = cidx == 0;
            d.act = 1;
            d.inc = d.fin ? sizes[i] - 128 * cidx : 128;
            d.t = d.fin ? sizes[i] : 128 * (cidx + 1);
            d.msg_off = i * stride + 128 * (size_t)cidx;
            d.num = first_block_number + (uint32_t)i;
            d.mode = compact_mode(d.num);
            d.size = sizes[i];
            memcpy(d.D, D, 32);
        }
        memcpy(D, dig.data() + 32 * i, 32);
    }
    for (; bi < n_blocks; ++bi) {
        BlockDesc& d = descs[bi];
        memset(&d, 0, sizeof d);
        d.fin = d.first = 1;
        d.act = 0;
        d.inc = d.t = d.size = 40;
        d.msg_off = ~0ULL;
        d.num = first_block_number + (uint32_t)n_headers - 1;
        d.mode = compact_mode(d.num);
        memcpy(d.D, D, 32);
    }
    VX_HIP(hipMemcpyAsync(d_desc, descs.data(), n_blocks * sizeof(BlockDesc), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_blake_trace, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint8_t*)headers->d,
                       (const BlockDesc*)d_desc, (const uint64_t*)d_hc, n_real, d_stage, n, window_offset, window_length);
    VX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_blake_count, dim3(PARTS * (CNT_SLICES1 + CNT_SLICES2)), dim3(CNT_THREADS), 0, ctx->stream, (const uint64_t*)d_stage, n, d_hist);
    VX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_blake_expand, dim3((unsigned)((n + 256 * EXP_RPL - 1) / (256 * EXP_RPL)), N_STAGE), dim3(256), 0, ctx->stream,
                       (const uint64_t*)d_stage, trace_out->d, n, (const ExpandEntry*)d_ent, (const uint32_t*)d_eoff);
    VX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_blake_mult, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_hist, trace_out->d, n);
    VX_HIP(hipGetLastError());
    VX_HIP(vx_wait(ctx));  // descs must outlive the kernel
    for (int j = 0; j < 8; ++j) {
        uint32_t a, b;
        memcpy(&a, trusted_hash + 4 * j, 4);
        memcpy(&b, D + 4 * j, 4);
        public_inputs_out[j] = a;
        public_inputs_out[8 + j] = b;
    }
    public_inputs_out[16] = first_block_number;
    public_inputs_out[17] = first_block_number + (uint64_t)n_headers - 1;
    // bus mode 1: the block number of leaf 0 = this table's first block minus the headers of the range before it (window_offset
    // doubles as that count when window_length = 0: a map segment of a longer range; 0 = the table starts the range)
    public_inputs_out[18] = window_length ? window_offset : (tree_size ? (uint64_t)first_block_number - window_offset : 0);
    public_inputs_out[19] = window_length ? 2 : (tree_size ? 1 : 0);  // bus mode: 1 the state / data roots go to a Merkle AIR, 2 a window of message bytes
    if (digests_out) memcpy(digests_out, dig.data(), dig.size());
    return VX_OK;
}

}  // extern "C"
