// libvxprove internals: context, device buffers, host-side field helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <map>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/vx.h"
#pragma GCC visibility pop
#include "glh.h"

// Issue priority of the tail kernels (tree tops, small-tree leaves, query-phase gathers): they never fill the chip and do under 2 %
// of a proof's VALU work, but run beside resident hash / NTT waves, and VALU issue goes by priority before age.  -DVX_TAIL_PRIO=0
// is the A/B (profiles/README.md).  Nothing that can fill the chip may raise its priority.
#ifndef VX_TAIL_PRIO
#define VX_TAIL_PRIO 1
#endif
#if VX_TAIL_PRIO
#define VX_TAIL_KERNEL_ENTRY() __builtin_amdgcn_s_setprio(3)
#else
#define VX_TAIL_KERNEL_ENTRY() ((void)0)
#endif

struct vx_buf {
    uint64_t* d;
    size_t n;
};

// three-level power table of a base b: lvl[0][j] = b^j, lvl[1][j] = b^(j<<11), lvl[2][j] = b^(j<<22), j < 2048
struct PowTab {
    uint64_t* d;  // 3*2048 on device
};

// How the tables of one proof (a context and the chain of side contexts behind it) reach the GPU; chosen when the host's context
// is made (VX_TABLE_STREAMS, vx_core.hip) and inherited by its side contexts.
enum { VX_TABLE_STREAMS_OWN = 0, VX_TABLE_STREAMS_SHARED = 1 };

struct vx_ctx {
    int device;
    hipStream_t stream;
    bool stream_owned;  // false: a side context in shared mode, `stream` is its parent's and is not destroyed with it
    int table_streams;  // VX_TABLE_STREAMS_*
    hipEvent_t ev0, ev1;
    hipEvent_t ev_wait;  // shared mode: what vx_wait records and waits for (no timing)
    std::string err;
    PowTab tw_fwd, tw_inv;       // base = omega_{2^32}, omega_{2^32}^-1
    uint64_t *w12_fwd, *w12_inv;  // omega_4096^e, e < 2048
    std::map<uint64_t, PowTab> shift_tabs;
    std::map<int, uint64_t*> tw2;  // key = log_s * 2 + inverse: two-level table of w_{2^log_s}
    uint64_t* scratch;
    size_t scratch_n;
    void* pinned;  // small pinned staging area
    size_t pinned_n;
    // device memory pool: blocks are recycled by exact (rounded) size instead of hipFree'd -- a
    // proof allocates tens of GB and hipMalloc/hipFree of such blocks costs far more than the kernels.
    // All work is on ctx->stream, so a recycled block is safe to hand out again immediately (in shared mode too: the contexts of a
    // proof then enqueue on ONE in-order stream, and a block never leaves the pool of the context that allocated it).
    std::map<size_t, std::vector<void*>> pool_free;
    std::map<void*, size_t> pool_live;
    // a second context on the same device (own scratch and pool; own stream unless table_streams is shared), made on first use: independent small proofs
    // (the authority-set commitment STARKs) run on it from a host thread while this context proves the hash chain
    vx_ctx* side = nullptr;
    // periodic columns of an AIR on the LDE coset, by (air id, degree bits, rate bits): identical for every proof of a shape
    std::map<uint64_t, uint64_t*> periodic_cache;
};
vx_ctx* vx_side_ctx(vx_ctx* ctx);  // nullptr if it cannot be created
// Every internal "wait for this context's work".  Own mode: hipStreamSynchronize(ctx->stream).  Shared mode: an event recorded on the
// stream now and waited for -- what THIS context has enqueued (and whatever the proof's other tables enqueued before the record),
// not the kernels another table's thread enqueues afterwards.  Called from the one host thread that drives ctx.
hipError_t vx_wait(vx_ctx* ctx);
void* vx_pool_alloc(vx_ctx* ctx, size_t bytes);
void vx_pool_free(vx_ctx* ctx, void* p);
void vx_pool_trim(vx_ctx* ctx);
int32_t vx_fail(vx_ctx* ctx, int32_t code, const char* fmt, ...);

// One pool block carved into word regions.  Every region is named once, with its size (add), before the block is taken (alloc):
// the total and every offset come from that one list.  The copies go on ctx->stream and stop at the first error, which status()
// reports.  The block returns to the pool with the object; a witness that outlives the function that made it holds the object.
// add() keeps the ADDRESS of the caller's pointer until alloc() sets it: the pointers must not move in between, so the object
// (and a witness that holds it) is neither copied nor moved, and add and alloc happen in one frame.  Before alloc() nothing is
// copied and status() is the allocation's failure (vx_fail takes the null context).
struct Scratch {
    vx_ctx* ctx = nullptr;
    uint64_t* base = nullptr;
    size_t words = 0;
    hipError_t err = hipSuccess;
    std::vector<std::pair<uint64_t**, size_t>> regions;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() {
        if (base) vx_pool_free(ctx, base);
    }
    void add(uint64_t*& p, size_t n) { regions.push_back({&p, words}), words += n; }
    void alloc(vx_ctx* c) {
        ctx = c, base = (uint64_t*)vx_pool_alloc(c, words * 8);
        for (auto& r : regions) *r.first = base ? base + r.second : nullptr;
    }
    bool ok() const { return base && err == hipSuccess; }
    void keep(hipError_t e) {
        if (err == hipSuccess) err = e;
    }
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (ok()) err = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
    }
    void up(void* dst, const void* src, size_t bytes) { copy(dst, src, bytes, hipMemcpyHostToDevice); }
    void down(void* dst, const void* src, size_t bytes) { copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    void fill(void* dst, int byte, size_t bytes) {
        if (ok()) err = hipMemsetAsync(dst, byte, bytes, ctx->stream);
    }
    void launched() { keep(hipGetLastError()); }  // after a kernel launch
    void sync() {
        if (ok()) err = vx_wait(ctx);
    }
    int32_t status(const char* what) const {
        if (!base) return vx_fail(ctx, VX_ERR_OOM, "%s: out of device memory", what);
        return err == hipSuccess ? VX_OK : vx_fail(ctx, VX_ERR_DEVICE, "%s: %s", what, hipGetErrorString(err));
    }
};

struct vx_tree {
    uint64_t* levels;  // level 0 (leaf digests, 4*n) followed by each parent level up to the cap
    size_t n_leaves;
    int cap_height;
    size_t total;  // uint64 count
};

#define VX_HIP(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return vx_fail(ctx, e_ == hipErrorOutOfMemory ? VX_ERR_OOM : VX_ERR_DEVICE, "%s: %s", \
                           #call, hipGetErrorString(e_));                                         \
    } while (0)
#define VX_CHECK(cond, ...)                                   \
    do {                                                      \
        if (!(cond)) return vx_fail(ctx, VX_ERR_ARG, __VA_ARGS__); \
    } while (0)
#define VX_TRY(call)            \
    do {                        \
        int32_t r_ = (call);    \
        if (r_ != VX_OK) return r_; \
    } while (0)

int32_t vx_get_shift_tab(vx_ctx* ctx, uint64_t base, PowTab* out);
int32_t vx_scratch(vx_ctx* ctx, size_t n_u64, uint64_t** out);
int32_t vx_merkle_build_dev(vx_ctx* ctx, const uint64_t* data, size_t n_leaves, size_t leaf_len, int layout,
                            int cap_height, vx_tree** out);

int32_t vx_ntt_dev(vx_ctx* ctx, uint64_t* d, int log_n, size_t n_cols, size_t col_stride, int inverse, uint64_t shift, int order);
int32_t vx_lde_dev(vx_ctx* ctx, const uint64_t* src, int log_n, size_t n_cols, int rate_bits, uint64_t shift, int src_kind,
                   uint64_t* dst, uint64_t* coeffs_out);
int32_t vx_gather_rows_dev(vx_ctx* ctx, const uint64_t* lde, int log_N, size_t n_cols, const uint64_t* leaf_idx, size_t n_idx,
                           uint64_t* out);
// enqueue-only forms of the three query-phase gathers: indices and destination on the device, nothing uploaded, copied back or waited
// for (the prover's query phase launches all of a table's gathers into one scratch region and makes one round trip)
void vx_gather_rows_enqueue(vx_ctx* ctx, const uint64_t* lde, int log_N, size_t n_cols, const uint64_t* idx_d, size_t n_idx, uint64_t* out_d);
void vx_merkle_open_enqueue(vx_ctx* ctx, const vx_tree* tree, const uint64_t* idx_d, size_t n_idx, uint64_t* out_d);
void vx_fri_leaves_enqueue(vx_ctx* ctx, const uint64_t* evals, int log_n, int arity_bits, const uint64_t* idx_d, size_t n_idx, uint64_t* out_d);
int32_t vx_fri_fold_dev(vx_ctx* ctx, const uint64_t* evals, int log_n, int arity_bits, const uint64_t beta[2], uint64_t shift,
                        uint64_t* out);
int32_t vx_fri_layer_tree_dev(vx_ctx* ctx, const uint64_t* evals, int log_n, int arity_bits, int cap_height, vx_tree** out);
int32_t vx_fri_leaves_dev(vx_ctx* ctx, const uint64_t* evals, int log_n, int arity_bits, const uint64_t* leaf_idx, size_t n_idx,
                          uint64_t* out);

// two-level root table for one sub-transform size: lo[j] = w_S^j (j < 2^lo_bits), hi[j] = w_S^(j << lo_bits)
struct Tw2 {
    const uint64_t* lo;
    const uint64_t* hi;
    int lo_bits;
};
int32_t vx_get_tw2(vx_ctx* ctx, int log_s, int inverse, Tw2* out);
int32_t vx_lde_consume_dev(vx_ctx* ctx, uint64_t* values, int log_n, size_t n_cols, int rate_bits, uint64_t shift, uint64_t* dst);
// Called by the prover once the trace cap of an AIR with an auxiliary round is known; fills `chal` (n_chal values) with
// lookup challenges that depend on EVERY table sharing the bus (typically by proving the other table from inside).
struct vx_chal_hook {
    int32_t (*fn)(void* user, const uint64_t* pub, size_t n_pub, const uint64_t* cap, size_t cap_words, uint64_t* chal, size_t n_chal);
    void* user;
};
int32_t vx_stark_prove_impl(vx_ctx* ctx, int air_id, const vx_stark_config* cfg, uint64_t* trace_d, size_t trace_len, int consume_trace,
                            int log_n, const uint64_t* public_inputs, size_t n_public, uint64_t* proof_out, size_t proof_cap,
                            size_t* proof_len, const vx_chal_hook* hook = nullptr);
void vx_shared_challenges_n(const uint64_t* const* pubs, const size_t* n_pubs, const uint64_t* const* caps, size_t k, size_t cap_words, uint64_t* out, size_t n_out);
void vx_shared_challenges(const uint64_t* pub_a, size_t n_a, const uint64_t* cap_a, const uint64_t* pub_b, size_t n_b, const uint64_t* cap_b,
                          size_t cap_words, uint64_t* out, size_t n_out);
// verifier with externally derived lookup challenges (nullptr = drawn from the proof's own transcript); apub_out (optional)
// receives a pointer to the values published with the auxiliary cap, and log_n_out the degree bits
int32_t vx_stark_verify_ext(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int expect_air, const uint64_t* expect_public,
                            size_t n_expect_public, const uint64_t* ext_chal, const uint64_t** apub_out, int* log_n_out, char* err, size_t errlen);
int32_t vx_lde_keep_dev(vx_ctx* ctx, const uint64_t* values, int log_n, size_t n_cols, int rate_bits, uint64_t shift, uint64_t* coef_brev,
                        uint64_t* dst);
int32_t vx_scan_cols_dev(vx_ctx* ctx, uint64_t* data, int log_n, size_t n_cols, uint64_t* totals_host);
int32_t vx_sha_tree_trace_dev(vx_ctx* ctx, const uint8_t* state_roots, const uint8_t* data_roots, size_t n_leaves, int log_tree, uint64_t* trace_d,
                              uint64_t pub_out[17]);
int32_t vx_bus_close_dev(vx_ctx* ctx, uint64_t* z_cols, int log_n, uint64_t aux_pub[2]);
int32_t vx_ed_trace_dev(vx_ctx* ctx, const uint8_t* pubkeys, const uint8_t* sigs, const uint8_t* msg, uint32_t msg_len, const uint8_t* signed_flags, size_t n_sigs,
                        int log_n, uint64_t bus_on, uint64_t* trace_d, uint64_t pub_out[2]);
int32_t vx_sha512_trace_dev(vx_ctx* ctx, const uint8_t* pubkeys, const uint8_t* sigs, const uint8_t* msg, const uint8_t* flags, size_t n_sigs, int log_n, uint64_t bus_on,
                            uint64_t* trace_d, uint64_t pub_out[15]);
int32_t vx_epoch_end_trace_dev(vx_ctx* ctx, const uint8_t* header_d, size_t header_bytes, uint32_t start_position, uint32_t num_authorities, uint64_t bus_on, uint64_t* trace_d,
                               uint64_t pub_out[10], uint32_t* window_length_out);
int32_t vx_sha_chain_trace_dev(vx_ctx* ctx, const uint8_t* pubkeys, size_t n_keys, const uint8_t* signed_flags, uint64_t bus_on, int log_n, uint64_t* trace_d,
                               uint64_t public_inputs_out[10], uint8_t commitment_out[32]);
int32_t vx_merkle_open_trace_dev(vx_ctx* ctx, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx, int log_n, uint64_t* trace_d, uint64_t pub_out[9]);
void vx_merkle_levels_launch(vx_ctx* ctx, uint64_t* levels, size_t n_leaves, size_t cap);
