// Host-side Goldilocks (table generation, transcript, verifier) and its quadratic extension F[X]/(X^2 - 7).  Standard C++.
#pragma once
#include <stdint.h>

namespace glh {
static const uint64_t P = 0xFFFFFFFF00000001ULL;
static inline uint64_t add(uint64_t a, uint64_t b) {
    uint64_t s = a + b;
    return (s < a || s >= P) ? s - P : s;
}
static inline uint64_t sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + (P - b); }
// x mod p for any 128-bit x, without the 128-bit division `% P` compiles to (__umodti3, ~30 ns -- the host transcript absorbs
// thousands of elements per proof): x = lo + hl 2^64 + hh 2^96 = lo - hh + hl (2^32 - 1) (mod p), 2^64 = 2^32 - 1, 2^96 = -1.
static inline uint64_t reduce128(unsigned __int128 x) {
    const uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64), hh = hi >> 32, hl = hi & 0xFFFFFFFFULL;
    uint64_t t0, t2;
    if (__builtin_sub_overflow(lo, hh, &t0)) t0 -= 0xFFFFFFFFULL;  // + p (mod 2^64); t0 >= 2^64 - 2^32 here, cannot wrap again
    if (__builtin_add_overflow(t0, hl * 0xFFFFFFFFULL, &t2)) t2 += 0xFFFFFFFFULL;  // - p (mod 2^64); the wrapped sum is < 2^64 - 2^32
    return t2 >= P ? t2 - P : t2;
}
static inline uint64_t mul(uint64_t a, uint64_t b) { return reduce128((unsigned __int128)a * b); }
static inline uint64_t pow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    while (e) {
        if (e & 1) r = mul(r, a);
        a = mul(a, a);
        e >>= 1;
    }
    return r;
}
static inline uint64_t inv(uint64_t a) { return pow(a, P - 2); }
static const uint64_t ROOT_2_32 = 1753635133440165772ULL;  // 7^((p-1)/2^32)
static inline uint64_t root(int log_n) {
    uint64_t r = ROOT_2_32;
    for (int i = 32; i > log_n; --i) r = mul(r, r);
    return r;
}
}  // namespace glh

// The host extension-field element: the prover's transcript values, the verifier's constraints at zeta (Air::eval<Fx>).  Both words
// are canonical (< P).
struct Fx {
    uint64_t a, b;
    Fx operator+(Fx o) const { return {glh::add(a, o.a), glh::add(b, o.b)}; }
    Fx operator-(Fx o) const { return {glh::sub(a, o.a), glh::sub(b, o.b)}; }
    Fx operator*(Fx o) const {
        return {glh::add(glh::mul(a, o.a), glh::mul(7, glh::mul(b, o.b))), glh::add(glh::mul(a, o.b), glh::mul(b, o.a))};
    }
    static Fx from(uint64_t x) { return {x % glh::P, 0}; }
};
static inline Fx fx_scale(Fx x, uint64_t s) { return {glh::mul(x.a, s), glh::mul(x.b, s)}; }
static inline Fx fx_inv(Fx x) {
    const uint64_t ni = glh::inv(glh::sub(glh::mul(x.a, x.a), glh::mul(7, glh::mul(x.b, x.b))));
    return {glh::mul(x.a, ni), glh::mul(glh::sub(0, x.b), ni)};
}
static inline Fx fx_pow(Fx x, uint64_t e) {
    Fx r{1, 0};
    while (e) {
        if (e & 1) r = r * x;
        x = x * x;
        e >>= 1;
    }
    return r;
}
static inline bool fx_eq(Fx x, Fx y) { return x.a == y.a && x.b == y.b; }
