// Witness of EpochEndAir (air_epoch.cuh): the ScheduledChange log of the epoch-end header, one row per authority record.
//   k_epoch_rows  one lane per row (512): copies the row's bytes out of the header on the device, sets the row flags and the
//                 bits of the first length byte
// The auxiliary columns are bus_aux.cuh's, from the AIR's own message list: one lane per row, 22 helpers.
// Parity: tests/test_gpu_epoch_air.py compares trace, auxiliary columns and public inputs with oracle/epoch_air.py.
#include <string.h>

#include "air_epoch.cuh"
#include "bus_aux.cuh"

namespace {
using namespace epo;

__global__ __launch_bounds__(64) void k_epoch_rows(const uint8_t* __restrict__ header, uint32_t log_pos, uint32_t plen, uint32_t n_auth, uint64_t* __restrict__ tr) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x, n = 1u << LOG_N;
    if (row >= n) return;
    const uint8_t* p = header + log_pos;  // the consensus flag
    const bool pre = row == 0, val = row >= 1 && row <= n_auth, dly = row == n_auth + 1;
    const uint32_t base = pre ? 0 : plen + 40 * (row - 1), cnt = pre ? plen : val ? 40 : dly ? 4 : 0;
    for (uint32_t j = 0; j < NB; ++j) tr[(size_t)j * n + row] = j < cnt ? p[base + j] : 0;
    tr[(size_t)V * n + row] = val, tr[(size_t)DL * n + row] = dly;
    for (int i = 0; i < 6; ++i) tr[(size_t)(Q0 + i) * n + row] = pre ? ((p[5] >> 2) >> i) & 1 : 0;
}
}  // namespace

int32_t EpochEndAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<EpochEndAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

// header_d: the header bytes on the device (header_bytes of them readable).  The prefix is parsed here (rotate.rs:74-174: its two
// compact lengths are public inputs of the table); the validator records are copied as they are -- a header whose records do not
// satisfy rotate.rs:243-274 yields a trace no proof exists for (vx_verify_epoch_end_header names the failing rule).
int32_t vx_epoch_end_trace_dev(vx_ctx* ctx, const uint8_t* header_d, size_t header_bytes, uint32_t start_position, uint32_t num_authorities, uint64_t bus_on, uint64_t* trace_d,
                               uint64_t pub_out[10], uint32_t* window_length_out) {
    const uint32_t n = 1u << LOG_N;
    VX_CHECK(num_authorities >= 1 && num_authorities <= n - 2, "epoch-end trace: %u authorities (the table holds %u)", num_authorities, n - 2);
    VX_CHECK((uint64_t)start_position + 1 + 17 <= header_bytes, "epoch-end trace: start position %u leaves no room for the 17-byte prefix", start_position);
    uint8_t p[17];
    VX_HIP(hipMemcpyAsync(p, header_d + start_position + 1, 17, hipMemcpyDeviceToHost, ctx->stream));
    VX_HIP(vx_wait(ctx));
    if (p[0] != 4 || memcmp(p + 1, "FRNK", 4) != 0) return vx_fail(ctx, VX_ERR_STATEMENT, "epoch-end trace: consensus flag / engine id");
    const int m1 = p[5] & 3, len1 = len_of(m1);
    if (m1 == 3 && p[5] != 3) return vx_fail(ctx, VX_ERR_STATEMENT, "epoch-end trace: compact int (length)");
    if (p[5 + len1] != 1) return vx_fail(ctx, VX_ERR_STATEMENT, "epoch-end trace: scheduled change flag");
    const uint8_t* e = p + 6 + len1;
    const int m2 = e[0] & 3, len2 = len_of(m2);
    const uint32_t w2 = (uint32_t)e[0] | ((uint32_t)e[1] << 8), w4 = w2 | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
    const uint32_t val = m2 == 0 ? e[0] >> 2 : m2 == 1 ? w2 >> 2 : m2 == 2 ? w4 >> 2 : ((uint32_t)e[1] | ((uint32_t)e[2] << 8) | ((uint32_t)e[3] << 16) | ((uint32_t)e[4] << 24));
    if (val != num_authorities || (m2 == 3 && e[0] != 3)) return vx_fail(ctx, VX_ERR_STATEMENT, "epoch-end trace: authority count");
    const uint32_t plen = 6 + len1 + len2, wlen = plen + 40 * num_authorities + 4;
    VX_CHECK((uint64_t)start_position + 1 + wlen <= header_bytes, "epoch-end trace: the log of %u authorities runs past the header buffer", num_authorities);
    hipLaunchKernelGGL(k_epoch_rows, dim3(n / 64), dim3(64), 0, ctx->stream, header_d, start_position + 1, plen, num_authorities, trace_d);
    VX_HIP(hipGetLastError());
    pub_out[0] = num_authorities, pub_out[1] = bus_on ? 1 : 0;
    for (int a = 0; a < 4; ++a) pub_out[2 + a] = a == m1, pub_out[6 + a] = a == m2;
    if (window_length_out) *window_length_out = wlen;
    return VX_OK;
}

extern "C" int32_t vx_epoch_end_trace(vx_ctx* ctx, const vx_buf* header, uint32_t start_position, uint32_t num_authorities, uint32_t bus_on, vx_buf* trace_out,
                                      uint64_t public_inputs_out[10], uint32_t* window_length_out) {
    if (!ctx || !header || !trace_out || !public_inputs_out) return VX_ERR_ARG;
    VX_CHECK(trace_out->n >= ((size_t)COLS << LOG_N), "epoch-end trace: trace buffer holds %zu elements, 2^%d rows need %zu", trace_out->n, LOG_N, (size_t)COLS << LOG_N);
    return vx_epoch_end_trace_dev(ctx, (const uint8_t*)header->d, header->n * 8, start_position, num_authorities, bus_on, trace_out->d, public_inputs_out, window_length_out);
}
