// Host check of 0-kno-vectorx_amd/csrc/poseidon_freq.h (the partial rounds of the Poseidon permutation in the transform domain of
// the linear layer) against glh::poseidon: the 22 partial rounds alone and the whole permutation, on random and corner-case states,
// with canonical and non-canonical s-box outputs.  Prints "ok <max |l| >> 48> <max |h| >> 16> <max |y_l| >> 48> <max |y_h| >> 16>" (the
// extreme parts seen, in units of 2^48 / 2^16, rounded up) or the first mismatch.  Built and run by tests/test_poseidon_freq_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static int64_t g_max_l = 0, g_max_yl = 0;
static int64_t g_max_h = 0, g_max_yh = 0;
static inline void track(int64_t v, int64_t& m) {
    const int64_t a = v < 0 ? -v : v;
    if (a > m) m = a;
}
#define PFREQ_TRACK(l, h) (track((l), g_max_l), track((h), g_max_h))
#define PFREQ_TRACK_Y(l, h) (track((l), g_max_yl), track((h), g_max_yh))
#include "../../0-kno-vectorx_amd/csrc/glh_poseidon.h"
#include "../../0-kno-vectorx_amd/csrc/poseidon_freq.h"

static const uint64_t P = glh::P;
static const uint64_t RCF[360] = VX_POSEIDON_RC_FOLDED_INIT;  // partial rounds carry one constant, for element 0
static const uint64_t RC[360] = VX_POSEIDON_RC_INIT;
static const uint64_t MDS[12] = VX_POSEIDON_MDS_CIRC_INIT;

static uint64_t rng_s = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
    uint64_t z = (rng_s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL, z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
static uint64_t canon(uint64_t x) { return x >= P ? x - P : x; }
// x^7 as ANY 64-bit representative, the way the device s-box leaves it: mode 0 canonical, 1 the larger representative where one
// exists (values below 2^32 - 1), 2 either
static uint64_t sbox(uint64_t x, int mode) {
    x = canon(x);
    const uint64_t x2 = glh::mul(x, x), x3 = glh::mul(x2, x), x4 = glh::mul(x2, x2);
    uint64_t t = glh::mul(x3, x4);
    if (t < 0xFFFFFFFFULL && (mode == 1 || (mode == 2 && (rnd() & 1)))) t += P;
    return t;
}
static uint64_t add_nc(uint64_t a, uint64_t b) {  // gl_add_nc of gl.cuh
    uint64_t s;
    const bool c = __builtin_add_overflow(a, b, &s);
    return s + (c ? 0xFFFFFFFFULL : 0);
}
static void mds_ref(uint64_t* s) {
    uint64_t o[12];
    for (int row = 0; row < 12; ++row) {
        unsigned __int128 acc = 0;
        for (int i = 0; i < 12; ++i) acc += (unsigned __int128)canon(s[(i + row) % 12]) * MDS[i];
        if (row == 0) acc += (unsigned __int128)canon(s[0]) * VX_POSEIDON_MDS_DIAG0;
        o[row] = glh::reduce128(acc);
    }
    for (int i = 0; i < 12; ++i) s[i] = o[i];
}

// s = the state after the s-boxes of round 3 (any representatives) -> the state after the layer of round 25 plus round 26's
// constants: what poseidon_partial_freq of poseidon.cuh does, with the same calls
static void partial_freq(uint64_t* s, int mode) {
    int rc = 48;
    pfreq::State u;
    pfreq::enter(s, u);
    uint64_t x0 = s[0];
    for (int r = 0; r < 11; ++r) {
        uint64_t y0 = pfreq::round_y0(u, x0);
        uint64_t t = sbox(add_nc(y0, RCF[rc]), mode);
        pfreq::round_put<false>(u, x0, y0, t);
        x0 = t;
        y0 = pfreq::round_y0(u, x0);
        t = sbox(add_nc(y0, RCF[rc + 12]), mode);
        pfreq::round_put<true>(u, x0, y0, t);
        x0 = t;
        rc += 24;
    }
    pfreq::leave(u, x0, &RCF[rc], s);
}
// the same 23 layers and 22 s-boxes in the time domain
static void partial_ref(uint64_t* s) {
    int rc = 48;
    for (int r = 0; r < 22; ++r) {
        mds_ref(s);
        s[0] = sbox(glh::add(s[0], RCF[rc]), 0);
        rc += 12;
    }
    mds_ref(s);
    for (int i = 0; i < 12; ++i) s[i] = glh::add(s[i], RCF[rc + i]);
}
// the whole permutation over the folded constants with the partial rounds in the transform domain
static void permute_freq(uint64_t* s, int mode) {
    int rc = 12;
    for (int i = 0; i < 12; ++i) s[i] = add_nc(s[i], RCF[i]);
    for (int r = 0; r < 3; ++r) {
        for (int i = 0; i < 12; ++i) s[i] = sbox(s[i], mode);
        mds_ref(s);
        for (int i = 0; i < 12; ++i) s[i] = add_nc(s[i], RCF[rc + i]);
        rc += 12;
    }
    for (int i = 0; i < 12; ++i) s[i] = sbox(s[i], mode);
    partial_freq(s, mode);
    rc += 12 * 23;
    for (int r = 0; r < 3; ++r) {
        for (int i = 0; i < 12; ++i) s[i] = sbox(s[i], mode);
        mds_ref(s);
        for (int i = 0; i < 12; ++i) s[i] = add_nc(s[i], RCF[rc + i]);
        rc += 12;
    }
    for (int i = 0; i < 12; ++i) s[i] = sbox(s[i], mode);
    mds_ref(s);
}

static const uint64_t EDGE[] = {0, P - 1, 0xFFFFFFFFULL, (1ULL << 52) - 1, 1ULL << 52, (1ULL << 48) - 1, 1ULL << 48, ~0ULL, 1, P, 0xFFFFFFFF00000000ULL};
static const int NEDGE = sizeof(EDGE) / sizeof(EDGE[0]);

static int check(const uint64_t* in, int mode, const char* what, int idx) {
    uint64_t a[12], b[12];
    // the 22 partial rounds alone: any 64-bit words go in
    for (int i = 0; i < 12; ++i) a[i] = b[i] = in[i];
    partial_freq(a, mode), partial_ref(b);
    for (int i = 0; i < 12; ++i)
        if (canon(a[i]) != b[i]) {
            printf("partial rounds mismatch: %s %d mode %d element %d: %016llx != %016llx\n", what, idx, mode, i, (unsigned long long)canon(a[i]), (unsigned long long)b[i]);
            return 1;
        }
    // the whole permutation against the one of the host prover and verifier (unfolded constants)
    for (int i = 0; i < 12; ++i) a[i] = in[i], b[i] = canon(in[i]);
    permute_freq(a, mode), glh::poseidon(b);
    for (int i = 0; i < 12; ++i)
        if (canon(a[i]) != b[i]) {
            printf("permutation mismatch: %s %d mode %d element %d: %016llx != %016llx\n", what, idx, mode, i, (unsigned long long)canon(a[i]), (unsigned long long)b[i]);
            return 1;
        }
    return 0;
}

int main() {
    (void)RC;
    uint64_t s[12];
    for (int mode = 0; mode < 3; ++mode) {
        for (int e = 0; e < NEDGE; ++e) {  // every word the same edge value
            for (int i = 0; i < 12; ++i) s[i] = EDGE[e];
            if (check(s, mode, "edge", e)) return 1;
        }
        for (int e = 0; e < NEDGE; ++e)  // one edge value among eleven others: the extremes of the differences u2 / ur / ui
            for (int f = 0; f < NEDGE; ++f)
                for (int pat = 0; pat < 4; ++pat) {
                    for (int i = 0; i < 12; ++i) s[i] = ((pat == 0 ? i / 3 : pat == 1 ? i / 6 : pat == 2 ? i : i / 3 + 1) & 1) ? EDGE[e] : EDGE[f];
                    if (check(s, mode, "pattern", (e * NEDGE + f) * 4 + pat)) return 1;
                }
        for (int it = 0; it < 4000; ++it) {
            for (int i = 0; i < 12; ++i) s[i] = (it & 1) || (rnd() & 3) ? rnd() : EDGE[rnd() % NEDGE];
            if (check(s, mode, "random", it)) return 1;
        }
    }
    const long long ul = (long long)((g_max_l + ((1LL << 48) - 1)) >> 48), uh = (long long)((g_max_h + 0xFFFF) >> 16);
    const long long yl = (long long)((g_max_yl + ((1LL << 48) - 1)) >> 48), yh = (long long)((g_max_yh + 0xFFFF) >> 16);
    // the bounds poseidon_freq.h states
    if (g_max_l > pfreq::BOUND_L || g_max_h > pfreq::BOUND_H || g_max_yl > pfreq::BOUND_YL || g_max_yh > pfreq::BOUND_YH) {
        printf("bound exceeded: %lld %lld %lld %lld\n", ul, uh, yl, yh);
        return 1;
    }
    printf("ok %lld %lld %lld %lld\n", ul, uh, yl, yh);
    return 0;
}
