// The 22 partial rounds of the Poseidon permutation with the state kept in the TRANSFORM DOMAIN of the linear layer
// (VX_POSEIDON_FREQ_PARTIAL in poseidon.cuh).  poseidon_mds_part runs every layer as  three length-4 real FFTs -> a 3x3 block
// product per frequency -> three inverse FFTs.  Between two partial rounds the inverse FFTs of one layer are undone by the
// forward FFTs of the next; only the s-box on element 0 happens in the time domain.  So the state of a partial round is held
// as the twelve transform components  u0[a], u2[a], ur[a], ui[a]  (a = 0, 1, 2;  U1 = ur + i ui):
//     u0[a] = x[a] + x[3+a] + x[6+a] + x[9+a]      u2[a] = x[a] - x[3+a] + x[6+a] - x[9+a]
//     ur[a] = x[a] - x[6+a]                         ui[a] = x[9+a] - x[3+a]
// and a round does the block products only.  With a0 / a2 / (r, i) the block products of poseidon_mds_part, the layer's output
// is  y[3q+c] = 16 a0[c] + (-1)^q a2[c] + {r, -i, -r, i}[q][c]  (+ 8 x[0] on y[0], the diagonal), so ITS transform is
//     u0'[c] = y[c] + y[3+c] + y[6+c] + y[9+c] = 64 a0[c]        u2'[c] = 4 a2[c]
//     ur'[c] = y[c] - y[6+c] = 2 r[c]                            ui'[c] = y[9+c] - y[3+c] = 2 i[c]
// plus 8 x[0] on u0'[0], u2'[0], ur'[0] (the transform of e0 is 1, 1, 1 + 0 i).  Element 0 of the output is read off directly,
//     y[0] = 16 a0[0] + a2[0] + r[0] + 8 x[0],
// (the same value as (u0'[0] + u2'[0] + 2 ur'[0]) / 4, without a multiplication by 4^-1), recombined to a 64-bit word, sent
// through constant add and s-box, and the result t takes its place: t - y[0] is added to u0'[0], u2'[0], ur'[0].
//
// Representation.  A component is the pair (l, h), int64 and int32, standing for the INTEGER l + h 2^48, which is congruent
// mod p = 2^64 - 2^32 + 1 to the transform of the state -- not equal to it: components are differences (signed) and a
// normalisation only keeps the residue.  B = 2^48 below.  A 64-bit word w enters as (w mod B, w >> 48): l < B, h < 2^16.
//   normalise(l, h):  hh = h + (l >> 48);  h' = hh mod 2^16;  l' = (l mod B) + (hh >> 16) (2^32 - 1)      [2^64 = 2^32 - 1]
//     arithmetic shifts; |hh| < 2^31 gives |hh >> 16| <= 2^15:   -2^47 < l' < B + 2^47 = 1.5 B,   0 <= h' < 2^16.
// The frequencies do not mix and grow differently: a component of u0' is a sum with absolute coefficients 64 (1 + 2 + 1) = 256,
// of u2' 4 (1 + 2 + 8) = 44, of ur' / ui' 2 (3 + 5 + 17) = 50.  So u0 is normalised after EVERY round and the other nine after
// every SECOND round (ALL = false / true, eleven pairs); e = 8 x[0] + t - y[0] has |e_l| < 10 B, |e_h| < 10 2^16.
//   into a round A (ALL = false) -- from the entry FFTs of split words, or from a round B:
//       |u0_l| <= 4 B, |u2_l| <= 2 B, |ur_l|, |ui_l| <= 1.5 B           (highs: the same multiples of 2^16)
//   out of it:  |u0'_l| <= 256 4 B + 10 B (normalised: < 1.5 B),  |u2'_l| <= 44 2 B + 10 B = 98 B,  |ur'_l|, |ui'_l| <= 75 B + 10 B = 85 B
//   out of the round B that follows:  |u0'_l| <= 256 1.5 B + 10 B,  |u2'_l| <= 44 98 B + 10 B = 4322 B,  |ur'_l|, |ui'_l| <= 50 85 B + 10 B = 4260 B
//   so every low part stays below 4322 B < 2^60.1 and every high part below 4322 2^16 < 2^28.1 (no normalisation after the entry
//   FFTs is needed), and y[0] = 16 a0[0] + a2[0] + r[0] + 8 x[0] has |y_l| <= 16 6 B + 11 98 B + 25 85 B + 8 B = 3307 B in a
//   round B, 16 16 B + 11 2 B + 25 1.5 B + 8 B < 324 B in a round A; the exit layer (after a round B) < 160 B with its constants.
// y[0] may be negative as an integer: K p with K = 2^12 is added in split form, K p = KH 2^48 + KL with KH = K (2^16 - 1) >
// 3307 2^16 and KL = K (2^48 - 2^32 + 1) > 3307 B, which makes both parts positive (< 2^61, < 2^29); then the recombination is
// the one of poseidon_mds with 48 / 16 for 52 / 12.  tests/test_poseidon_freq_host.py runs this very code on a CPU against
// glh::poseidon and checks the bounds above through PFREQ_TRACK / PFREQ_TRACK_Y.
//
// Plain C++ (as gl96.h): the s-box, the constant add and the round-constant table belong to the caller.
#pragma once
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define PFREQ_FN __device__ __forceinline__
#elif defined(__HIPCC__)
#define PFREQ_FN __host__ __device__ inline
#else
#define PFREQ_FN static inline
#endif
#if defined(__clang__)
#define PFREQ_UNROLL _Pragma("unroll")
#else
#define PFREQ_UNROLL
#endif

namespace pfreq {

constexpr int LB = 48, HB = 16;
constexpr uint64_t ML = (1ULL << LB) - 1;
constexpr uint64_t EPS = 0xFFFFFFFFULL;
constexpr uint64_t KL = (ML + 1 - EPS) << 12;           // K (2^48 - 2^32 + 1)
constexpr uint32_t KH = ((1u << HB) - 1) << 12;         // K (2^16 - 1)
constexpr int64_t BOUND_L = 4322LL << LB;               // stated bounds on a component / on an output before K p is added
constexpr int32_t BOUND_H = 4322 << HB;
constexpr int64_t BOUND_YL = 3307LL << LB;
constexpr int32_t BOUND_YH = 3307 << HB;

// components 0..2 = u0[a], 3..5 = u2[a], 6..8 = ur[a], 9..11 = ui[a]
struct State {
    int64_t l[12];
    int32_t h[12];
};

// Two hints for the device compiler, no-ops in value.  keep: the compiler must not re-associate across a 64-bit value (left alone
// it distributes the layer's power-of-two factors over the sums and multiplies by 15 and 30).  minus_one: -1 as a number it cannot
// see, so that  m + u (-1)  for a 32-bit signed u stays one v_mad_i64_i32 instead of a sign extension and a two-instruction subtraction.
PFREQ_FN void keep(int64_t& x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#else
    (void)x;
#endif
}
PFREQ_FN void keep(int32_t&) {}
PFREQ_FN int32_t minus_one() {
    int32_t k = -1;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(k));
#endif
    return k;
}

// the three forward FFTs of one part (the first third of poseidon_mds_part)
template <class T, class TIn>
PFREQ_FN void fft_in(const TIn* x, T* u) {
PFREQ_UNROLL
    for (int a = 0; a < 3; ++a) {
        const T x0 = (T)x[a], x1 = (T)x[3 + a], x2 = (T)x[6 + a], x3 = (T)x[9 + a];
        const T A = x0 + x2, B = x1 + x3;
        u[a] = A + B;
        u[3 + a] = A - B;
        u[6 + a] = x0 - x2;
        u[9 + a] = x3 - x1;
    }
}

// the block products of one part (the middle third of poseidon_mds_part), unscaled: a[0..2] = a0, a[3..5] = a2, a[6..8] = r,
// a[9..11] = i.  Written as sums of the positive terms minus sums of the negative ones: a 64-bit (x << k) + y is one instruction
// (k <= 4), a 64-bit subtraction two.
template <class T>
PFREQ_FN void block(const T* u, T* a) {
    const T *u0 = u, *u2 = u + 3, *ur = u + 6, *ui = u + 9;
    const T s0 = u0[0] + u0[1] + u0[2];
    a[0] = s0 + u0[2], a[1] = s0 + u0[0], a[2] = s0 + u0[1];
    T P, N;
#define PFREQ_PN(i, pos, neg) P = pos, N = neg, keep(P), keep(N), a[i] = P - N, keep(a[i])
    PFREQ_PN(3, 8 * u2[2], 2 * u2[1] + u2[0]);
    PFREQ_PN(4, 0, 8 * u2[0] + 2 * u2[2] + u2[1]);
    PFREQ_PN(5, 2 * u2[0], 8 * u2[1] + u2[2]);
    // e1 = ((2,-1), (-4,1), (16,1)), wrapped terms times -i: the six sums of poseidon_mds_part with their products expanded
    PFREQ_PN(6, 16 * ui[1] + 2 * ur[0] + ui[0] + ur[1] + ur[2], 4 * ui[2]);
    PFREQ_PN(9, 4 * ur[2] + 2 * ui[0] + ui[1] + ui[2], 16 * ur[1] + ur[0]);
    PFREQ_PN(7, 16 * ui[2] + 2 * ur[1] + ui[1] + ur[2], 4 * ur[0] + ui[0]);
    PFREQ_PN(10, 2 * ui[1] + ur[0] + ui[2], 16 * ur[2] + 4 * ui[0] + ur[1]);
    PFREQ_PN(8, 16 * ur[0] + 2 * ur[2] + ui[2], 4 * ur[1] + ui[0] + ui[1]);
    PFREQ_PN(11, 16 * ui[0] + 2 * ui[2] + ur[0] + ur[1], 4 * ui[1] + ur[2]);
#undef PFREQ_PN
    keep(a[0]), keep(a[1]), keep(a[2]);
}

// l + h 2^48 with 0 <= l < 2^61, 0 <= h < 2^29 as a 64-bit word (any representative):
//   h 2^48 = (h >> 16) 2^64 + (h mod 2^16) 2^48;  w = (h >> 16) eps + l < 2^62;  the 32-bit add into the high word carries 2^64 = eps
PFREQ_FN uint64_t join(uint64_t l, uint32_t h) {
    const uint64_t w = (uint64_t)(h >> HB) * EPS + l;
    uint32_t yhi;
    const bool carry = __builtin_add_overflow((uint32_t)(w >> 32), h << (32 - HB), &yhi);
    const uint64_t y = ((uint64_t)yhi << 32) | (uint32_t)w;
    return y + (carry ? EPS : 0);  // after a carry yhi < the high word of w: no second carry
}

PFREQ_FN void normalise(int64_t& l, int32_t& h) {
    const int32_t hh = h + (int32_t)(l >> LB);
    const int32_t u = hh >> HB;
    h = hh & (int32_t)((1u << HB) - 1);
    // (l mod B) + u 2^32 - u
    const uint32_t mhi = ((uint32_t)((uint64_t)l >> 32) & (uint32_t)(ML >> 32)) + (uint32_t)u;
    l = (int64_t)(((uint64_t)mhi << 32) | (uint32_t)l) + (int64_t)u * (int64_t)minus_one();
}

// twelve 64-bit words (any representatives) -> the state of the first partial round
PFREQ_FN void enter(const uint64_t* s, State& u) {
    uint64_t xl[12];
    uint32_t xh[12];
PFREQ_UNROLL
    for (int i = 0; i < 12; ++i) {
        xl[i] = s[i] & ML;
        xh[i] = (uint32_t)(s[i] >> LB);
    }
    fft_in<int64_t>(xl, u.l);
    fft_in<int32_t>(xh, u.h);
}

// First half of a partial round: the block products of the layer whose input (transformed) is u and whose time-domain element 0
// was x0.  u becomes the transform of the layer's output WITHOUT its element-0 terms (round_put adds them); returns element 0 of
// the output, y[0], as a 64-bit word.
PFREQ_FN uint64_t round_y0(State& u, uint64_t x0) {
    int64_t al[12];
    int32_t ah[12];
    block<int64_t>(u.l, al);
    block<int32_t>(u.h, ah);
    const int64_t yl = 16 * al[0] + al[3] + al[6] + 8 * (int64_t)(x0 & ML);
    const int32_t yh = 16 * ah[0] + ah[3] + ah[6] + 8 * (int32_t)(x0 >> LB);
#ifdef PFREQ_TRACK_Y
    PFREQ_TRACK_Y(yl, yh);
#endif
PFREQ_UNROLL
    for (int c = 0; c < 3; ++c) {
        u.l[c] = 64 * al[c], u.h[c] = 64 * ah[c];
        u.l[3 + c] = 4 * al[3 + c], u.h[3 + c] = 4 * ah[3 + c];
        u.l[6 + c] = 2 * al[6 + c], u.h[6 + c] = 2 * ah[6 + c];
        u.l[9 + c] = 2 * al[9 + c], u.h[9 + c] = 2 * ah[9 + c];
    }
    return join((uint64_t)yl + KL, (uint32_t)yh + KH);
}
// Second half: t (the s-box output) takes the place of y0 as element 0 of the time-domain state, and the diagonal term 8 x0 of the
// layer joins: e = 8 x0 + t - y0 on u0[0], u2[0], ur[0].  Then u0 is normalised, and with ALL the other nine components too.
template <bool ALL>
PFREQ_FN void round_put(State& u, uint64_t x0, uint64_t y0, uint64_t t) {
    const int64_t el = 8 * (int64_t)(x0 & ML) + (int64_t)(t & ML) - (int64_t)(y0 & ML);
    const int32_t eh = 8 * (int32_t)(x0 >> LB) + (int32_t)(t >> LB) - (int32_t)(y0 >> LB);
    u.l[0] += el, u.l[3] += el, u.l[6] += el;
    u.h[0] += eh, u.h[3] += eh, u.h[6] += eh;
#ifdef PFREQ_TRACK
PFREQ_UNROLL
    for (int i = 0; i < 12; ++i) PFREQ_TRACK(u.l[i], u.h[i]);
#endif
PFREQ_UNROLL
    for (int i = 0; i < (ALL ? 12 : 3); ++i) normalise(u.l[i], u.h[i]);
PFREQ_UNROLL
    for (int i = 0; i < 12; ++i) keep(u.l[i]);
}

// The layer that ends the partial rounds: block products, inverse FFTs, the diagonal term and the twelve constants rc[0..11] of the
// next (full) round; s = twelve 64-bit words (any representatives).  u must come out of a round_put<true>.
PFREQ_FN void leave(const State& u, uint64_t x0, const uint64_t* rc, uint64_t* s) {
    int64_t al[12], yl[12];
    int32_t ah[12], yh[12];
    block<int64_t>(u.l, al);
    block<int32_t>(u.h, ah);
PFREQ_UNROLL
    for (int c = 0; c < 3; ++c) {
        const int64_t tl = 16 * al[c], pl = tl + al[3 + c], ml = tl - al[3 + c];
        yl[c] = pl + al[6 + c], yl[3 + c] = ml - al[9 + c], yl[6 + c] = pl - al[6 + c], yl[9 + c] = ml + al[9 + c];
        const int32_t th = 16 * ah[c], ph = th + ah[3 + c], mh = th - ah[3 + c];
        yh[c] = ph + ah[6 + c], yh[3 + c] = mh - ah[9 + c], yh[6 + c] = ph - ah[6 + c], yh[9 + c] = mh + ah[9 + c];
    }
    yl[0] += 8 * (int64_t)(x0 & ML);
    yh[0] += 8 * (int32_t)(x0 >> LB);
PFREQ_UNROLL
    for (int r = 0; r < 12; ++r) {
        const uint64_t c = rc[r];
        const int64_t vl = yl[r] + (int64_t)(c & ML);
        const int32_t vh = yh[r] + (int32_t)(c >> LB);
#ifdef PFREQ_TRACK_Y
        PFREQ_TRACK_Y(vl, vh);
#endif
        s[r] = join((uint64_t)vl + KL, (uint32_t)vh + KH);
    }
}

}  // namespace pfreq
