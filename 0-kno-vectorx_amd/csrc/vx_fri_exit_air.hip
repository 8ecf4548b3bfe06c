// Witness of FriExitAir (air_library.fri_exit_builder(), a constraint program with declared bus messages; layout: fri_exit_layout.h):
// what a verifier does with the challenges an inner proof's transcript yields behind the final polynomial -- the proof-of-work
// check, value mod N per query index, the point x_NL behind the folds and the final polynomial's value there.
//   k_fri_exit_trace  one lane per ROW.  Every cell is a closed-form function of (v, the row's position in its 128-row block): the
//                     bits and their prefix sums are shifts of v, the flags and counters are comparisons with public lengths, the
//                     point is one small power, and a Horner row recomputes its prefix of at most 64 steps from the coefficients
//                     (in L2 after the first wave).  Adjacent lanes store adjacent rows of a column; idle rows are written too.
//                     The table is a few thousand rows and latency-bound, so nothing here is tuned.
// The auxiliary round and the quotient are the generic kernels of a run-time AIR (k_bus_aux_prog, k_quotient_prog).
// Parity: tests/test_gpu_fri_exit.py compares the trace cell for cell with tests/fri_exit_ref.py, which runs the recurrences.
#include <string.h>

#include <vector>

#include "fri_exit_layout.h"
#include "gl.cuh"
#include "glh_poseidon.h"
#include "vx_internal.h"

namespace {

struct ExitArgs {
    const uint64_t* values;  // [n_blocks]: the PoW response, then the index challenges; canonical (checked by the host)
    const uint64_t* fpoly;   // [final_len][2], canonical (checked by the host)
    size_t n_blocks, n;
    int LN, FB, pow_bits, final_len;
    uint64_t w, g, ord_pow;  // w_FB, 7^(16^NL), the PoW response's ordinal
    uint64_t* tr;            // [FRI_EXIT_COLS][n]
};

// the bits of v above row r as an integer: what the weighted sum holds on row r (all of v behind the bit rows)
__device__ __forceinline__ uint64_t bits_above(uint64_t v, int r) { return r == 0 ? 0 : r >= 64 ? v : (v >> (64 - r)) << (64 - r); }

__global__ __launch_bounds__(64) void k_fri_exit_trace(ExitArgs a) {
    const size_t i = blockIdx.x * (size_t)64 + threadIdx.x;
    if (i >= a.n) return;
    uint64_t* out = a.tr + i;
    auto put = [&](int col, uint64_t v) { out[(size_t)col * a.n] = v; };
    const size_t blk = i >> FRI_EXIT_BLOCK_LOG;
    const int r = (int)(i & (FRI_EXIT_BLOCK - 1));
    if (blk >= a.n_blocks) {  // an idle block: all zero but the ordinal, which goes by position
#pragma unroll
        for (int j = 0; j < FRI_EXIT_COLS; ++j) put(j, j == FRI_EXIT_ORD ? a.ord_pow + blk : 0);
        return;
    }
    const uint64_t v = a.values[blk];
    const bool ispow = blk == 0;
    const int L = ispow ? a.pow_bits : 64 - a.LN;  // the prefix flag's length
    const int fb = ispow ? 0 : a.FB, flen = ispow ? 0 : a.final_len;
    const uint64_t bit = r < 64 ? (v >> (63 - r)) & 1 : 0;
    const bool f = r < L, ef = r >= L && r < L + fb;
    const uint64_t above = bits_above(v, r), keep = L >= 64 ? 0 : ~(uint64_t)0 >> L;
    put(FRI_EXIT_BIT, bit), put(FRI_EXIT_V, above);
    put(FRI_EXIT_F, f), put(FRI_EXIT_C, f ? (uint64_t)(L - r) : 0);
    put(FRI_EXIT_EF, ef), put(FRI_EXIT_C2, r <= L ? (uint64_t)fb : ef ? (uint64_t)(fb - (r - L)) : 0);
    put(FRI_EXIT_G, f ? 0 : bit), put(FRI_EXIT_EB, ef ? bit : 0);
    put(FRI_EXIT_IDX, above & keep);
    // the point: exponent step j is index bit LN - 1 - j with weight 2^j
    const int steps = r <= L ? 0 : (r - L < fb ? r - L : fb);
    uint64_t e_row = 0, e_all = 0;
    for (int j = 0; j < fb; ++j) {
        const uint64_t bj = ((v >> (a.LN - 1 - j)) & 1) << j;
        e_all |= bj;
        if (j < steps) e_row |= bj;
    }
    put(FRI_EXIT_W, r == 0 || r > L + fb ? 0 : r <= L ? a.w : gl_sqr_n(a.w, r - L));
    put(FRI_EXIT_X, r == 0 || L == 0 ? 0 : gl_mul(a.g, gl_pow(a.w, e_row)));
    // all ones so far over the top 32 bits, held over the low 32
    const int tr_ = r < 32 ? r : 32;
    put(FRI_EXIT_T, r == 0 || r >= 64 ? 0 : (uint64_t)((v >> (64 - tr_)) == (~(uint64_t)0 >> (64 - tr_))));
    // the Horner steps from row 63: the row holds the accumulator BEFORE its step
    const int done = r <= FRI_EXIT_HORNER_ROW ? 0 : (r - FRI_EXIT_HORNER_ROW < flen ? r - FRI_EXIT_HORNER_ROW : flen);
    const bool hf = r >= FRI_EXIT_HORNER_ROW && r < FRI_EXIT_HORNER_ROW + flen;
    const int k = flen - done;
    put(FRI_EXIT_HF, hf), put(FRI_EXIT_K, (uint64_t)k);
    put(FRI_EXIT_CA, hf ? a.fpoly[2 * (k - 1)] : 0), put(FRI_EXIT_CB, hf ? a.fpoly[2 * (k - 1) + 1] : 0);
    gl2 acc{0, 0};
    if (done) {
        const uint64_t x = gl_mul(a.g, gl_pow(a.w, e_all));
        for (int s = 0; s < done; ++s) {
            const uint64_t* c = a.fpoly + 2 * (flen - 1 - s);
            acc = gl2{gl_add(gl_mul(acc.a, x), c[0]), gl_add(gl_mul(acc.b, x), c[1])};
        }
    }
    put(FRI_EXIT_ACC, acc.a), put(FRI_EXIT_ACC + 1, acc.b);
    put(FRI_EXIT_ACT, 1), put(FRI_EXIT_ISPOW, ispow), put(FRI_EXIT_ORD, a.ord_pow + blk);
}

constexpr size_t MAX_QUERIES = (size_t)1 << 18;
// what can be told from the statement alone; the text names the limit that was missed
const char* statement_wrong(int log_lde, size_t n_layers, int pow_bits, uint64_t ord_pow, uint64_t absorbed, const uint64_t* final_poly, size_t final_len) {
    if (n_layers < 1 || n_layers > (size_t)FRI_EXIT_MAX_LAYERS) return "fri exit: the fold layers are not 1 .. 8";
    if (log_lde < 5 || log_lde > 32) return "fri exit: log_lde is not 5 .. 32";
    if (log_lde - 4 * (int)n_layers < 1) return "fri exit: no index bit is left behind the fold layers (FB < 1)";
    if (pow_bits < 0 || pow_bits > 64) return "fri exit: pow_bits is not 0 .. 64";
    if (final_len < 1) return "fri exit: a final polynomial has at least one coefficient";
    if (final_len > (size_t)FRI_EXIT_MAX_FINAL_LEN) return "fri exit: a final polynomial of more than 64 coefficients does not fit the Horner rows of a block";
    if ((ord_pow >> 32) || (absorbed >> 32)) return "fri exit: ORD_POW or ABSORBED is 2^32 or more";
    for (size_t i = 0; i < 2 * final_len; ++i)
        if (final_poly[i] >= glh::P) return "fri exit: non-canonical final-polynomial word";
    return nullptr;
}

void public_inputs(int log_lde, size_t n_layers, int pow_bits, uint64_t ord_pow, uint64_t absorbed, const uint64_t* final_poly, size_t final_len, uint64_t* pub) {
    const uint64_t e16 = (uint64_t)1 << (4 * n_layers);  // 16^NL
    pub[FRI_EXIT_PUB_ORD_POW] = ord_pow, pub[FRI_EXIT_PUB_ABSORBED] = absorbed, pub[FRI_EXIT_PUB_POW_BITS] = (uint64_t)pow_bits;
    pub[FRI_EXIT_PUB_SKIP] = (uint64_t)(64 - log_lde), pub[FRI_EXIT_PUB_FB] = (uint64_t)log_lde - 4 * n_layers;
    pub[FRI_EXIT_PUB_W] = glh::pow(glh::root(log_lde), e16), pub[FRI_EXIT_PUB_G] = glh::pow(7, e16), pub[FRI_EXIT_PUB_FINAL_LEN] = final_len;
    std::vector<uint64_t> w(pub, pub + FRI_EXIT_PUB_DIGEST);
    w.insert(w.end(), final_poly, final_poly + 2 * final_len);
    glh::hash_no_pad(w.data(), w.size(), pub + FRI_EXIT_PUB_DIGEST);
}

}  // namespace

extern "C" {
int vx_fri_exit_log_n(size_t n_queries) {
    int log_n = FRI_EXIT_BLOCK_LOG + 1;
    while (log_n < 63 && ((size_t)1 << (log_n - FRI_EXIT_BLOCK_LOG)) < n_queries + 1) ++log_n;
    return log_n;
}

int32_t vx_fri_exit_public(int log_lde, size_t n_layers, int pow_bits, uint64_t ord_pow, uint64_t absorbed, const uint64_t* final_poly, size_t final_len, uint64_t* public_out) {
    if (!final_poly || !public_out || statement_wrong(log_lde, n_layers, pow_bits, ord_pow, absorbed, final_poly, final_len)) return VX_ERR_ARG;
    public_inputs(log_lde, n_layers, pow_bits, ord_pow, absorbed, final_poly, final_len, public_out);
    return VX_OK;
}

int32_t vx_fri_exit_statement(const uint64_t* words, size_t n_words, uint64_t digest_out[4]) {
    if (!words || !digest_out || n_words == 0) return VX_ERR_ARG;
    for (size_t i = 0; i < n_words; ++i)
        if (words[i] >= glh::P) return VX_ERR_ARG;
    glh::hash_no_pad(words, n_words, digest_out);
    return VX_OK;
}

int32_t vx_fri_exit_air_trace(vx_ctx* ctx, int log_lde, size_t n_layers, int pow_bits, uint64_t ord_pow, uint64_t absorbed, const uint64_t* values, size_t n_queries,
                              const uint64_t* final_poly, size_t final_len, int log_n, vx_buf* trace_out, uint64_t* public_out) {
    if (!ctx || !values || !final_poly || !trace_out || !public_out) return VX_ERR_ARG;
    const char* why = statement_wrong(log_lde, n_layers, pow_bits, ord_pow, absorbed, final_poly, final_len);
    VX_CHECK(!why, "%s (log_lde %d, %zu layers, pow_bits %d, final_len %zu)", why, log_lde, n_layers, pow_bits, final_len);
    VX_CHECK(n_queries >= 1 && n_queries <= MAX_QUERIES, "fri exit: %zu queries (1..2^18)", n_queries);
    const size_t n_blocks = n_queries + 1;
    VX_CHECK(log_n >= vx_fri_exit_log_n(n_queries) && log_n <= 26, "fri exit: %zu blocks of %d rows do not fit 2^%d rows (at most 2^26)", n_blocks, (int)FRI_EXIT_BLOCK, log_n);
    VX_CHECK(trace_out->n >= ((size_t)FRI_EXIT_COLS << log_n), "fri exit: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows", trace_out->n, (int)FRI_EXIT_COLS, log_n);
    for (size_t i = 0; i < n_blocks; ++i) VX_CHECK(values[i] < glh::P, "fri exit: non-canonical challenge value %zu", i);
    if (pow_bits > 0 && (values[0] >> (64 - pow_bits)) != 0)
        return vx_fail(ctx, VX_ERR_STATEMENT, "fri exit: proof of work invalid (the response has a bit among its top %d)", pow_bits);
    public_inputs(log_lde, n_layers, pow_bits, ord_pow, absorbed, final_poly, final_len, public_out);
    Scratch sc;
    uint64_t *values_d, *fpoly_d;
    sc.add(values_d, n_blocks), sc.add(fpoly_d, 2 * final_len);
    sc.alloc(ctx);
    ExitArgs a{};
    a.values = values_d, a.fpoly = fpoly_d, a.n_blocks = n_blocks, a.n = (size_t)1 << log_n;
    a.LN = log_lde, a.FB = log_lde - 4 * (int)n_layers, a.pow_bits = pow_bits, a.final_len = (int)final_len;
    a.w = public_out[FRI_EXIT_PUB_W], a.g = public_out[FRI_EXIT_PUB_G], a.ord_pow = ord_pow, a.tr = trace_out->d;
    sc.up(values_d, values, n_blocks * 8), sc.up(fpoly_d, final_poly, 2 * final_len * 8);
    if (sc.ok()) {
        hipLaunchKernelGGL(k_fri_exit_trace, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, ctx->stream, a);
        sc.launched();
    }
    return sc.status("fri exit");
}
}  // extern "C"
