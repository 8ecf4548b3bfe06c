// The round walk of one PoseidonAir block (air_library.py poseidon_builder: 48 columns, 32 rows per permutation), shared by the
// witness kernels of the tables built from such blocks (k_poseidon_air_trace in vx_poseidon.hip, k_merkle_open_trace in
// vx_merkle_open_air.hip, k_leaf_sponge_trace in vx_leaf_sponge_air.hip), and the broadcast of a block's own columns.  The 30 rounds run in the PLAIN schedule (constant layer, s-box, MDS: the rows of the table are the
// states entering each round, not the folded form the hashing kernels use).
#pragma once
#include "gl.cuh"
#include "poseidon_constants.h"

static __constant__ uint64_t POSEIDON_RC_PLAIN[360] = VX_POSEIDON_RC_INIT;

// Writes the state, x^2, x^4 and x^7 of rows row0 .. row0 + 31 of a column-major trace of n rows (columns 0..47) for the input
// state s (canonical); rows 30 and 31 hold the output, which s holds on return.
__device__ __forceinline__ void poseidon_air_walk(uint64_t (&s)[12], uint64_t* tr, size_t n, size_t row0) {
    constexpr uint32_t C[12] = VX_POSEIDON_MDS_CIRC_INIT;
#pragma unroll 1
    for (int r = 0; r < 32; ++r) {
        const size_t row = row0 + r;
        const bool full = r < 4 || (r >= 26 && r < 30);
        uint64_t y[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const uint64_t x = r < 30 ? gl_add(s[i], POSEIDON_RC_PLAIN[12 * r + i]) : s[i];
            const uint64_t a = gl_mul(x, x), b = gl_mul(a, a), t = gl_mul(gl_mul(x, a), b);
            tr[(size_t)i * n + row] = s[i];
            tr[(size_t)(12 + i) * n + row] = a;
            tr[(size_t)(24 + i) * n + row] = b;
            tr[(size_t)(36 + i) * n + row] = t;
            y[i] = (full || i == 0) ? t : x;
        }
        if (r < 30) {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                unsigned __int128 acc = q == 0 ? (unsigned __int128)y[0] * VX_POSEIDON_MDS_DIAG0 : 0;
#pragma unroll
                for (int i = 0; i < 12; ++i) acc += (unsigned __int128)y[(i + q) % 12] * C[i];
                s[q] = gl_reduce128((uint64_t)(acc >> 64), (uint64_t)acc);
            }
        }
    }
}

// The columns a block holds constant: writes v[j] to rows row0 .. row0 + 31 of column col0 + j, j < N (unrolled over j: v[] stays
// in registers).
template <int N>
__device__ __forceinline__ void poseidon_air_block_cols(const uint64_t (&v)[N], uint64_t* tr, size_t n, int col0, size_t row0) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        uint64_t* col = tr + (size_t)(col0 + j) * n + row0;
        const uint64_t x = v[j];
#pragma unroll 8
        for (int r = 0; r < 32; ++r) col[r] = x;
    }
}
