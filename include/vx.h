/*
 * vx.h -- C ABI of libvxprove, the MI355X-native (gfx950) backend for the
 * header_range proving path of VectorX (reference: AsherBond/0-kno-vectorx).
 *
 * The reference has no FFI of its own: its seams are the
 * `Circuit::prove` library call (circuits/header_range.rs:167-170) and cargo's
 * dependency-override mechanism (Cargo.toml:101-106).  Each group below names
 * the upstream routine (plonky2 v0.2.0 / starkyx v1.0.0 / plonky2x v1.1.0,
 * pinned at Cargo.lock:4848-4910, 7232-7249) that a `[patch]`-ed Rust shim
 * would forward to this library, and the in-tree call site that reaches it.
 * INTEGRATION.md shows the Rust `extern "C"` stubs.
 *
 * Conventions
 *   - plain C, no exceptions; every call returns int32_t: 0 = VX_OK, <0 = VX_ERR_*;
 *     vx_last_error(ctx) returns a message for the last failure on that ctx.
 *   - field elements: canonical (< p = 2^64-2^32+1) little-endian uint64_t;
 *     extension elements (D = 2, X^2 = 7): two consecutive uint64_t (c0, c1).
 *   - matrices are COLUMN-MAJOR: one polynomial / trace column is contiguous.
 *   - the caller owns host buffers; vx_buf are device (HBM) buffers owned by
 *     the ctx that allocated them.
 *   - EXTENTS: a vx_buf may be longer than the extent a call documents (the one
 *     exception: a vx_bus_table's trace).  An output's extent starts at the
 *     buffer's first word, or at the offset argument where there is one.  EVERY
 *     word of it is written -- the idle rows, idle slots and padding blocks of a
 *     trace included, whatever the buffer held before -- and NO word outside it.
 *     A `const vx_buf*` input is left intact, as is every word around it.
 *     (tests/test_gpu_extents.py holds every entry point to this.)
 *   - a vx_ctx is bound to one device and one HIP stream; calls are
 *     asynchronous on that stream; vx_sync / vx_download block.  Not
 *     thread-safe: one ctx per host thread.
 */
#ifndef VX_H
#define VX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vx_ctx vx_ctx;
typedef struct vx_buf vx_buf;
typedef struct vx_tree vx_tree;

enum {
    VX_OK = 0,
    VX_ERR_ARG = -1,      /* bad argument (shape, range, null) */
    VX_ERR_DEVICE = -2,   /* HIP runtime failure / no gfx950 device */
    VX_ERR_OOM = -3,      /* device allocation failed */
    VX_ERR_BUFSZ = -4,    /* caller buffer too small; needed size reported */
    VX_ERR_STATEMENT = -5,/* the header_range statement does not hold for the witness
                             (the reference panics / fails an in-circuit assert) */
    VX_ERR_POW = -6       /* proof-of-work search exhausted */
};

/* ---- lifecycle ------------------------------------------------------------ */
int32_t vx_ctx_create(int device, vx_ctx** out);
int32_t vx_ctx_destroy(vx_ctx* ctx);
int32_t vx_sync(vx_ctx* ctx);
const char* vx_last_error(const vx_ctx* ctx);
const char* vx_backend_name(void); /* "hip-gfx950" */
/* elapsed milliseconds between two points of the ctx stream (HIP events):
 * vx_timer_start records, vx_timer_stop records + synchronises and returns ms. */
int32_t vx_timer_start(vx_ctx* ctx);
int32_t vx_timer_stop(vx_ctx* ctx, float* ms);
/* How the circuit provers' tables reach the GPU (environment, read by vx_ctx_create and inherited by the side contexts a prover
 * makes behind the ctx): VX_TABLE_STREAMS = own (a stream per table), shared (the tables of one proof on the ctx's one stream:
 * for several proofs in flight where hardware queues are few; the latency of one proof alone rises) or auto (the default: shared
 * when GPU_MAX_HW_QUEUES is 4 or less).  The decision itself, host only: the two strings as getenv returns them (NULL = unset)
 * -> 0 own, 1 shared.  Results are the same bytes in either mode. */
int32_t vx_table_streams_mode(const char* table_streams, const char* hw_queues);

/* ---- memory --------------------------------------------------------------- */
int32_t vx_alloc(vx_ctx* ctx, size_t n_u64, vx_buf** out);
int32_t vx_free(vx_ctx* ctx, vx_buf* buf);
int32_t vx_upload(vx_ctx* ctx, vx_buf* dst, size_t dst_off, const uint64_t* src, size_t n_u64);
int32_t vx_download(vx_ctx* ctx, const vx_buf* src, size_t src_off, uint64_t* dst, size_t n_u64);
int32_t vx_copy(vx_ctx* ctx, vx_buf* dst, size_t dst_off, const vx_buf* src, size_t src_off, size_t n_u64);
/* fill with canonical pseudo-random field elements (SplitMix64 of seed+index, reduced mod p) */
int32_t vx_fill_random(vx_ctx* ctx, vx_buf* dst, size_t off, size_t n_u64, uint64_t seed);
void* vx_buf_devptr(const vx_buf* buf);
size_t vx_buf_len(const vx_buf* buf);

/* ---- K1: Goldilocks batch arithmetic (plonky2_field::goldilocks_field; test surface) */
int32_t vx_field_batch_add(vx_ctx* ctx, const vx_buf* a, const vx_buf* b, vx_buf* out, size_t n);
int32_t vx_field_batch_sub(vx_ctx* ctx, const vx_buf* a, const vx_buf* b, vx_buf* out, size_t n);
int32_t vx_field_batch_mul(vx_ctx* ctx, const vx_buf* a, const vx_buf* b, vx_buf* out, size_t n);
/* Field::batch_multiplicative_inverse; 0 maps to 0 */
int32_t vx_field_batch_inv(vx_ctx* ctx, const vx_buf* a, vx_buf* out, size_t n);
int32_t vx_ext_batch_mul(vx_ctx* ctx, const vx_buf* a, const vx_buf* b, vx_buf* out, size_t n_ext);

/* ---- K2: batched radix-2 NTT (plonky2_field::fft::{fft,ifft}, polynomial::{coset_fft,coset_ifft})
 * buf holds n_cols columns of n = 2^log_n elements at column stride `col_stride`
 * (elements), the first at element `off`.  Natural order in and out, in place: the n words of
 * every column are written; the col_stride - n words between two columns, and everything
 * before `off` and behind the last column, are not touched.
 *   inverse = 0: values[i] = sum_k coeff[k] * (shift * w^i)^k        (coset_fft; shift 0/1 = plain fft)
 *   inverse = 1: the inverse map, including the 1/n factor           (coset_ifft / ifft)
 * order: VX_ORDER_NATURAL, or VX_ORDER_BITREV to leave a FORWARD result (or take an
 * INVERSE input) in bit-reversed positions and skip the permutation pass. */
enum { VX_ORDER_NATURAL = 0, VX_ORDER_BITREV = 1 };
int32_t vx_ntt(vx_ctx* ctx, vx_buf* buf, size_t off, int log_n, size_t n_cols, size_t col_stride,
               int inverse, uint64_t shift, int order);

/* ---- K3: low-degree extension (plonky2::fri::oracle::PolynomialBatch::{from_values,from_coeffs})
 * src: n_cols columns of n values (natural order) or, with VX_LDE_SRC_COEFFS, coefficients.
 * dst: n_cols columns of N = n << rate_bits evaluations on the coset shift*<w_N>, column-major,
 *      NATURAL order within a column: dst[c*N + i] = P_c(shift * w_N^i).  plonky2's leaf j
 *      (after its transpose + reverse_index_bits) is row i = bitrev_N(j); vx_merkle_build
 *      and vx_lde_rows take that mapping into account, no transposed copy is ever made.
 * coeffs_out (optional, may be NULL): n_cols columns of n coefficients (natural order).
 * src is preserved. */
enum { VX_LDE_SRC_VALUES = 0, VX_LDE_SRC_COEFFS = 1 };
int32_t vx_lde(vx_ctx* ctx, const vx_buf* src, int log_n, size_t n_cols, int rate_bits, uint64_t shift,
               int src_kind, vx_buf* dst, vx_buf* coeffs_out);
/* gather plonky2 leaves: for each of n_idx leaf indices j, the n_cols values of row bitrev(j)
 * -> out[k*n_cols + c] on the HOST (PolynomialBatch::get_lde_values) */
int32_t vx_lde_rows(vx_ctx* ctx, const vx_buf* lde, int log_N, size_t n_cols, const uint64_t* leaf_idx,
                    size_t n_idx, uint64_t* out);

/* ---- K4: Poseidon-Goldilocks + Merkle caps (plonky2::hash::{poseidon,hashing,merkle_tree}) */
/* in-place permutation of n states of 12 elements (state-major: 12 consecutive per state) */
int32_t vx_poseidon_permute_batch(vx_ctx* ctx, vx_buf* states, size_t n);
/* MerkleTree::new(leaves, cap_height).  Layouts of `data`:
 *   VX_LEAVES_ROW_MAJOR: leaf j = data[j*leaf_len .. +leaf_len)
 *   VX_LEAVES_COLS_BITREV: data is column-major [leaf_len][n_leaves]; leaf j = row bitrev(j)
 *                          of every column (the layout vx_lde produces)
 *   VX_LEAVES_COLS: column-major, leaf j = row j. */
enum { VX_LEAVES_ROW_MAJOR = 0, VX_LEAVES_COLS_BITREV = 1, VX_LEAVES_COLS = 2 };
int32_t vx_merkle_build(vx_ctx* ctx, const vx_buf* data, size_t off, size_t n_leaves, size_t leaf_len,
                        int layout, int cap_height, vx_tree** out);
int32_t vx_merkle_free(vx_ctx* ctx, vx_tree* tree);
/* cap_out: 4 * 2^cap_height elements (host) */
int32_t vx_merkle_cap(vx_ctx* ctx, const vx_tree* tree, uint64_t* cap_out);
/* MerkleTree::prove for n_idx leaves: siblings_out[k][log2(n_leaves)-cap_height][4] (host) */
int32_t vx_merkle_open(vx_ctx* ctx, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx,
                       uint64_t* siblings_out);
/* leaf digests (4*n_leaves, device->host), test surface */
int32_t vx_merkle_leaf_digests(vx_ctx* ctx, const vx_tree* tree, uint64_t* out);

/* ---- K6: FRI (plonky2::fri::{prover,verifier,reduction_strategies}) */
/* One reduction step.  evals: N = 2^log_n extension values of a polynomial on the coset
 * shift*<w_N>, NATURAL order (evals[i] = P(shift*w_N^i), interleaved c0,c1).  Writes the
 * N >> arity_bits values of P'(y) = sum_i beta^i P_i(y) (P(x) = sum_i x^i P_i(x^arity)) on
 * the coset shift^arity * <w_{N/arity}>, natural order -- the values
 * fri_committed_trees obtains by folding coefficients and re-running coset_fft. */
int32_t vx_fri_fold(vx_ctx* ctx, const vx_buf* evals, int log_n, int arity_bits, const uint64_t beta[2],
                    uint64_t shift, vx_buf* out);
/* Merkle tree over a FRI layer: leaf j = the `arity` extension values whose natural indices
 * are bitrev(j*arity + t), t < arity (reverse_index_bits + chunk + flatten of prover.rs). */
int32_t vx_fri_layer_tree(vx_ctx* ctx, const vx_buf* evals, int log_n, int arity_bits, int cap_height,
                          vx_tree** out);
/* FriInitialTreeProof / FriQueryStep evals: the flattened `arity` extension values of each of
 * n_idx leaves of a FRI layer (MerkleTree::get on the layer tree) -> out[k][2*arity] (host) */
int32_t vx_fri_leaves(vx_ctx* ctx, const vx_buf* evals, int log_n, int arity_bits, const uint64_t* leaf_idx,
                      size_t n_idx, uint64_t* out);
/* fri_proof_of_work: smallest nonce w such that Poseidon(state with state[pos] = w)[7] has
 * `bits` leading zero bits.  (Upstream's parallel find_any returns an arbitrary valid nonce;
 * see DESIGN.md section 6.) */
int32_t vx_fri_pow(vx_ctx* ctx, const uint64_t state[12], int pos, int bits, uint64_t* nonce);

/* ---- K5/K7 + K6 query phase: generic STARK prover (starky v0.2.0 `prove_with_commitment` over
 * plonky2 v0.2.0 PolynomialBatch / FRI; reached in the reference through curta's hash/EdDSA
 * STARKs -- circuits/builder/header.rs:18, justification.rs:140,156,237 -- and, for the
 * Plonk side, through every `circuit.prove`, circuits/header_range.rs:167).
 * trace: n_cols(air) columns of 2^log_n rows, column-major, resident in HBM.
 * proof_out: caller buffer of proof_cap uint64 words; *proof_len receives the length; returns
 * VX_ERR_BUFSZ (with *proof_len set) when the buffer is too small.  Proof layout: DESIGN.md. */
typedef struct vx_stark_config {
    int32_t rate_bits;       /* 1: blowup 2, constraint degree <= 3 */
    int32_t cap_height;      /* 4 */
    int32_t num_queries;     /* 84 */
    int32_t pow_bits;        /* 16 */
    int32_t arity_bits;      /* ConstantArityBits(4, 5) */
    int32_t final_poly_bits;
} vx_stark_config;
/* The AIRs of the statements are COMPILED INTO the library: 1 Fibonacci and 2 "cubic mixer" pin the
 * generic prover, 5 is the smallest AIR with an auxiliary (lookup / logUp) commitment round.  A host can add its own at run
 * time as a constraint PROGRAM (vx_air_register below; its auxiliary round is filled by a host callback, or on the GPU from
 * declared bus messages: vx_air_register_bus).  The tables of the
 * header_range / rotate statements, each declared with its trace generator below: 6 Blake2b header chain
 * (VX_AIR_BLAKE_CHAIN), 4 SHA-256 authority-set commitment (VX_AIR_SHA_CHAIN), 7 / 8 / 9 SHA-256 Merkle trees of 256 /
 * 512 / 16 leaves, 10 / 12 Ed25519 (2^17 / 2^16 rows), 11 / 14 / 13 SHA-512 (2^16 / 2^15 / 2^10 rows), 15 epoch-end log.
 * 16 (VX_AIR_MERKLE_OPEN) proves a batch of Poseidon Merkle openings: the first aggregation table, see vx_merkle_openings_prove.
 * 17 (VX_AIR_LEAF_SPONGE) hashes the opened leaf rows to those openings' digests: the second one, see vx_merkle_rows_prove.
 * 18 (VX_AIR_FRI_FOLD) proves the FRI fold chain of every query: the third one, see vx_fri_fold_prove.
 * 19 (VX_AIR_MERKLE_OPEN_SET) / 20 (VX_AIR_LEAF_SPONGE_SET) are 16 / 17 for several trees in one table: see vx_fri_queries_prove.
 * 21 (VX_AIR_FRI_COMBINE) proves the FRI combination of every query, the value the fold chain starts from: see vx_fri_combine_prove.
 * 22 (VX_AIR_LEAF_NOOP) turns the openings of leaves of at most 4 words, which are their own digest, into row words: see LeafNoopAir.
 * 23 (VX_AIR_TRANSCRIPT) proves the Fiat-Shamir transcripts of up to 64 inner proofs: see vx_stark_transcripts_prove. */
enum { VX_AIR_FIBONACCI = 1, VX_AIR_MIX = 2, VX_AIR_LOOKUP = 5 };
int32_t vx_stark_default_config(vx_stark_config* cfg);
/* Run-time AIR descriptor (SURVEY 8b `vx_air_desc`): the constraint system of a starky-style AIR as a straight-line program over a
 * register file, the form a Rust host would lower `Stark::eval_packed_generic` / `eval_ext_circuit` to (starky v0.2.0 stark.rs; the
 * reference reaches it through curta's AirParser).  The same program is run by the GPU quotient kernel (one LDE point per lane,
 * registers in LDS), by the host verifier (at zeta, in the quadratic extension) and, restated, by oracle/air_program.py.
 * One instruction = one uint64:  bits 0..7 opcode, 8..15 destination register d, 16..31 operand a, 32..47 operand b, 48..63 zero.
 *   LOC d, a      r[d] = local row, column a            NXT d, a     r[d] = next row, column a
 *   PER d, a      r[d] = periodic column a              PUB d, a     r[d] = public input a
 *   CONST d, a    r[d] = consts[a]                      ADD / SUB / MUL d, a, b   r[d] = r[a] op r[b]
 *   CHAL d, a     r[d] = lookup challenge a          APUB d, a    r[d] = word a of the values published with the auxiliary cap
 *   ASSERT a            r[a] = 0 on EVERY row (the wrap-around pair included)
 *   ASSERT_TRANSITION a r[a] (x - w^-1): every row pair but the wrap-around      ASSERT_FIRST a / ASSERT_LAST a: on that row only
 * Constraints are consumed in program order (the order is protocol, as for the compiled AIRs).  Registration checks every operand,
 * that no register is read before it is written, that constants and periodic values are canonical, and the DEGREE of every
 * asserted expression (columns and periodic columns count 1; ASSERT <= 3, the three others <= 2: rate_bits 1 carries degree 3).
 * Periodic column q has 2^periodic_log[q] values (<= 2^16), given back to back.
 * AUXILIARY ROUND (lookup / logUp arguments, starky's `lookups()`): a program may declare aux_cols further columns, n_challenges
 * base-field challenges (<= 8; extension elements are pairs) and n_aux_public published extension values (<= 4).  After the trace
 * cap the prover draws the challenges and calls gen_aux -- the HOST's witness generator for this round: trace = the main columns
 * [cols][2^log_n] and aux_out = [aux_cols][2^log_n], both resident in HBM as buffers of `ctx` (use the library's primitives or
 * the host's own kernels on vx_buf_devptr, on the ctx stream); aux_public_out receives 2 * n_aux_public words.  The rows the
 * program sees hold the main columns followed by the auxiliary ones (LOC / NXT a >= cols).  Extension-field arithmetic
 * (F[X]/(X^2 - 7)) is written out in base-field instructions by whoever writes the program (air_program.py does).  A program with
 * aux_cols > 0 and gen_aux NULL can be verified, not proven.
 * A program is immutable once registered and its id
 * (>= VX_AIR_USER_BASE, never reused) works wherever an AIR id does: vx_quotient_eval, vx_stark_aux_trace, vx_stark_proof_bound,
 * vx_stark_prove, vx_stark_verify.  Registration is process-wide, thread-safe, needs no GPU; a verifier must register the SAME
 * program (the proof does not carry it).  vx_air_unregister retires the id. */
enum { VX_AIRP_LOC = 1, VX_AIRP_NXT = 2, VX_AIRP_PER = 3, VX_AIRP_PUB = 4, VX_AIRP_CONST = 5, VX_AIRP_ADD = 6, VX_AIRP_SUB = 7, VX_AIRP_MUL = 8,
       VX_AIRP_ASSERT = 9, VX_AIRP_ASSERT_TRANSITION = 10, VX_AIRP_ASSERT_FIRST = 11, VX_AIRP_ASSERT_LAST = 12, VX_AIRP_CHAL = 13, VX_AIRP_APUB = 14 };
enum { VX_AIR_USER_BASE = 4096, VX_AIRP_MAX_REGS = 32, VX_AIRP_MAX_COLS = 65535, VX_AIRP_MAX_CODE = 1 << 20, VX_AIRP_MAX_PERIOD_LOG = 16 };
typedef int32_t (*vx_air_gen_aux_fn)(void* user, vx_ctx* ctx, const vx_buf* trace, int log_n, const uint64_t* challenges,
                                     const uint64_t* public_inputs, vx_buf* aux_out, uint64_t* aux_public_out);
typedef struct vx_air_program {
    uint32_t cols, n_public, n_periodic, n_regs;
    const uint8_t* periodic_log;      /* [n_periodic] */
    const uint64_t* periodic_values;  /* sum of 2^periodic_log[q] values */
    const uint64_t* consts;
    uint32_t n_consts;
    const uint64_t* code;
    uint32_t n_code;
    uint32_t aux_cols, n_challenges, n_aux_public; /* auxiliary round: all zero = none */
    vx_air_gen_aux_fn gen_aux;
    void* gen_aux_user;
} vx_air_program;
int32_t vx_air_register(const vx_air_program* program, int* air_id, char* err, size_t errlen);
int32_t vx_air_unregister(int air_id);
/* BUS MESSAGES of a run-time AIR: instead of writing the logUp block of its constraints by hand and filling the auxiliary round
 * in a callback, a program may DECLARE the messages its rows send and receive, as the compiled bus tables do (csrc/air.cuh "the
 * bus of a table").  From the one declaration vx_air_register_bus derives the helper constraints and the running-sum constraint
 * (appended to the program's own, as ordinary instructions) and the GPU fills the auxiliary columns and the published total
 * (k_bus_aux_prog); there is no callback.
 * The MESSAGE PROGRAM is straight-line register code in the instruction word above, over a register file of its own (n_regs <=
 * VX_BUSP_MAX_REGS: registration lowers it into the 32 registers of a constraint program and keeps VX_BUSP_LOWER_REGS of them for
 * denominators and helpers), with a constant table of its own.  It admits LOC (main columns only), PER, PUB, CONST, ADD, SUB, MUL and
 *   BUSP_SLOT d, a   slot d (0..3) of the next message = r[a]; a slot that is not set is absent (contributes 0)
 *   BUSP_MSG a, b    closes the message: tag b (a constant below 2^16), signed multiplicity r[a] (sent m, received 0 - m); clears the slots
 * A message (t0, t1, t2, t3, tag) has the denominator D = beta + t0 + gamma t1 + gamma^2 t2 + gamma^3 t3 + gamma^4 tag in
 * F[X]/(X^2 - 7), beta = challenges (0, 1), gamma = challenges (2, 3).  Messages pair up in program order: messages 2e and 2e + 1
 * share helper e = m_a / D_a + m_b / D_b (an odd count leaves the last helper with one message).  With N_HELP = ceil(messages / 2)
 * the auxiliary layout is the compiled tables': helper e at auxiliary columns 2e, 2e + 1, the running sum at 2 N_HELP, 2 N_HELP + 1;
 * the program must declare aux_cols = 2 N_HELP + 2, n_challenges = 4, n_aux_public = 1 (total / rows) and no gen_aux.
 * block_log = 0: one set of helpers per row, the sum advances on every row (step_periodic < 0).  block_log = 5: one set per block of
 * 32 rows, read from the block's first row and written to all 32, and the sum advances where periodic column step_periodic is 1
 * (period 32; 1 at position 0, 0 elsewhere).  No other block_log is supported.
 * The appended constraints, in order: per helper the two halves of h D_a D_b - m_a D_b - m_b D_a (h D - m for a single message),
 * then the two halves of z' - z - sum h [* per[step]] + total, all as ASSERT.  The degree rules above apply to them: with two messages to
 * a helper a slot has degree at most 1 and a multiplicity at most 2. */
enum { VX_BUSP_SLOT = 64, VX_BUSP_MSG = 65 };
enum { VX_BUSP_LOWER_REGS = 20, VX_BUSP_MAX_REGS = 12, VX_BUSP_MAX_HELPERS = 19, VX_BUSP_MAX_CODE = 1 << 14 };
typedef struct vx_air_bus {
    const uint64_t* code;   /* the message program */
    uint32_t n_code;
    const uint64_t* consts;
    uint32_t n_consts;
    uint32_t n_regs;
    uint32_t block_log;     /* 0 or 5 */
    int32_t step_periodic;  /* block_log 5: the periodic column that is 1 on a block's first row; block_log 0: negative */
} vx_air_bus;
int32_t vx_air_register_bus(const vx_air_program* program, const vx_air_bus* bus, int* air_id, char* err, size_t errlen);
/* The witness of PoseidonAir -- the Poseidon permutation as a STARK table (0-kno-vectorx_amd/air_library.py poseidon_builder: 48
 * columns, one round per row, 32 rows per permutation; the constraint program ships with the library and is registered by the
 * host): states = n_perm x 12 input words, trace_out = [48][32 * n_perm] column-major with the state, x^2, x^4 and x^7 of every
 * round row; rows 30 / 31 of a block hold the permutation's output.  n_perm a power of two.  What a recursive verifier's hashing
 * table is filled with (plonky2 v0.2.0 hash/poseidon.rs; reached from Circuit::prove's recursion, circuits/header_range.rs:167). */
int32_t vx_poseidon_air_trace(vx_ctx* ctx, const vx_buf* states, size_t n_perm, vx_buf* trace_out);
/* ---- MerkleOpenAir: a batch of Merkle openings of ONE Poseidon tree proven in one STARK table (AIR id VX_AIR_MERKLE_OPEN; compiled:
 * csrc/air_merkle_open.cuh) -- verify_merkle_proof_to_cap (plonky2 v0.2.0 hash/merkle_proofs.rs) for any number of leaves of a
 * vx_tree, the first table of proof aggregation: a verifier accepts this table instead of walking the paths.
 * One path of D = log2(n_leaves) levels is D blocks of 32 rows (one two-to-one compression each, PoseidonAir's columns and
 * constraints); the table has no positional shape, so any number of paths of any depth fit the one AIR id at any log_n >= 5.
 * PROVEN: for every opening (index, leaf digest) that the verifier names, the path from that leaf digest with the index bits as
 * directions ends in the ROOT, the two-to-one fold of the tree's cap down to one digest (the cap itself at cap height 0).  The
 * openings leave the table as messages on its logUp bus and the VERIFIER IS THE OTHER PARTY of that bus: the proof is accepted
 * iff the table's published total equals the sum over the verifier's own claims.  Public inputs (9): root (4), D, and the claims
 * digest hash_n_to_hash_no_pad((index, d0, d1, d2, d3) of every opening, in order), which makes the lookup challenges depend on
 * the claims.  The opened leaf ROWS are hashed in-proof by LeafSpongeAir (below: vx_merkle_rows_prove, whose claims are rows, not
 * digests).  This table has one tree; MerkleOpenSetAir (below: vx_fri_queries_prove) takes several.  STILL OUTSIDE (the next
 * tables): the evaluation at zeta and the transcript stay on the host (the FRI fold is FriFoldAir, the FRI combination FriCombineAir, below).
 * vx_merkle_open_air_trace: the witness on its own (test surface) -- leaf_idx: n_idx >= 1 leaf indices (host; duplicates
 *   allowed); trace_out: [VX_MERKLE_OPEN_AIR_COLS][2^log_n] with 2^log_n >= 32 n_idx D; blocks behind the paths are idle.
 * vx_merkle_openings_prove: trace + proof at the smallest such log_n (>= 5) under lookup challenges that are the shared-challenge
 *   transcript of this one table's (public inputs, trace cap).  Blob: the magic "VXMOPEN1", log2(n_leaves), n_idx, the proof's
 *   length; then the table proof (vx_stark_prove layout).  VX_ERR_BUFSZ (with *blob_len set) when the buffer is too small.
 * vx_merkle_openings_verify (host only, walks no Merkle path): rebuilds the public inputs from cap / leaf_idx / leaf_digests
 *   (n_idx x 4 words), recomputes the challenges from the proof's cap, verifies the table under them and accepts iff
 *   published total x 2^log_n = sum over the claims of 1/D_lo + 1/D_hi (the two messages of an opening: (index, d0, d1, 0) and
 *   (index, d2, d3, 1)). */
enum { VX_AIR_MERKLE_OPEN = 16, VX_MERKLE_OPEN_AIR_COLS = 66, VX_MERKLE_OPEN_AIR_AUX_COLS = 4 };
int32_t vx_merkle_open_air_trace(vx_ctx* ctx, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx, int log_n, vx_buf* trace_out,
                                 uint64_t public_out[9]);
int32_t vx_merkle_openings_proof_bound(const vx_stark_config* cfg, size_t n_leaves, size_t n_idx, size_t* n_words);
int32_t vx_merkle_openings_prove(vx_ctx* ctx, const vx_stark_config* cfg, const vx_tree* tree, const uint64_t* leaf_idx, size_t n_idx,
                                 uint64_t* blob_out, size_t blob_cap, size_t* blob_len);
int32_t vx_merkle_openings_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const uint64_t* cap, int cap_height,
                                  int log_leaves, const uint64_t* leaf_idx, const uint64_t* leaf_digests, size_t n_idx, char* err, size_t errlen);
/* ---- LeafSpongeAir: the opened leaf ROWS of one Poseidon tree hashed in one STARK table (AIR id VX_AIR_LEAF_SPONGE; compiled:
 * csrc/air_leaf_sponge.cuh) -- hash_n_to_hash_no_pad (plonky2 v0.2.0 hash/hashing.rs) of any number of rows of one length, the
 * second table of proof aggregation: a STARK verifier holds the opened rows, never their digests.  One row of leaf_len words is
 * B = ceil(leaf_len / 8) blocks of 32 rows (one permutation each, PoseidonAir's columns and constraints; the sponge overwrites
 * the rate part, a tail block overwrites its first leaf_len mod 8 words only); no positional shape, so any number of rows of any
 * length >= 5 fit the one AIR id at any log_n >= 5.  leaf_len <= 4 is hash_or_noop's no-op -- the digest is the zero-padded row
 * itself and vx_merkle_openings_prove / _verify cover it -- so every entry point below REFUSES leaf_len < 5 with VX_ERR_ARG.
 * Public inputs (14): leaf_len, B, eight tail flags w_i = [word i of a last block is absorbed], and the row-claims digest
 * hash_n_to_hash_no_pad((index, row[0 .. leaf_len)) of every opening, in order), which makes the lookup challenges depend on
 * the claims.  Bus: every block sends the words it absorbs as (index, position, word) messages of a second kind, and the last
 * block of a row receives the two messages (index, digest) that MerkleOpenAir sends -- that kind is closed BETWEEN the tables.
 * vx_leaf_sponge_air_trace: the witness on its own (test surface) -- data / off / n_leaves / leaf_len / layout as vx_merkle_build
 *   takes them; leaf_idx: n_idx >= 1 leaf indices (host; duplicates allowed); trace_out: [VX_LEAF_SPONGE_AIR_COLS][2^log_n]
 *   with 2^log_n >= 32 n_idx B; blocks behind the rows are idle.  Returns the public inputs.
 * vx_merkle_rows_prove: MerkleOpenAir + LeafSpongeAir for the openings leaf_idx of `tree`, each at its smallest log_n, as two
 *   parties of ONE logUp bus: the lookup challenges are the shared-challenge transcript of both (public inputs, trace cap) pairs,
 *   openings first.  data / off / leaf_len / layout must be what `tree` was built from: every computed digest is compared with
 *   the tree's leaf digest first, and VX_ERR_STATEMENT is returned (nothing proven) when one differs.  Blob: the magic
 *   "VXMROWS1", log2(n_leaves), leaf_len, n_idx, the two proofs' lengths; then the MerkleOpenAir proof and the LeafSpongeAir
 *   proof (vx_stark_prove layout).  VX_ERR_BUFSZ (with *blob_len set) when the buffer is too small.
 * vx_merkle_rows_verify (host only; walks no Merkle path and hashes no leaf): the claims are (leaf_idx[i], rows[i][leaf_len]).
 *   It rebuilds LeafSpongeAir's public inputs entirely and MerkleOpenAir's root and depth from its own arguments.  It cannot
 *   know the leaf digests, so MerkleOpenAir's four claims-digest words are taken from that proof's own public inputs (checked
 *   canonical): they only feed the transcript -- the digests themselves are bound by the sponge table's committed trace, which
 *   receives every opening the first table sends.  It recomputes the shared challenges, verifies both tables under them and
 *   accepts iff  total_open x 2^log_n_open + total_sponge x 2^log_n_sponge = sum over the claims and j < leaf_len of
 *   1 / D_row(index, j, row[j]).  Its row-claims digest costs as many permutations as hashing the rows would; what it no longer
 *   does is anything per tree level, and the row bus is one whose other party a later table (FRI fold, evaluation at zeta)
 *   replaces.  Several trees of one leaf length in one table: LeafSpongeSetAir (below).  STILL OUTSIDE: a per-tree leaf length,
 *   the evaluation at zeta, the transcript (the FRI fold: FriFoldAir). */
enum { VX_AIR_LEAF_SPONGE = 17, VX_LEAF_SPONGE_AIR_COLS = 66, VX_LEAF_SPONGE_AIR_AUX_COLS = 12 };
int32_t vx_leaf_sponge_air_trace(vx_ctx* ctx, const vx_buf* data, size_t off, size_t n_leaves, size_t leaf_len, int layout, const uint64_t* leaf_idx,
                                 size_t n_idx, int log_n, vx_buf* trace_out, uint64_t public_out[14]);
int32_t vx_merkle_rows_proof_bound(const vx_stark_config* cfg, size_t n_leaves, size_t leaf_len, size_t n_idx, size_t* n_words);
int32_t vx_merkle_rows_prove(vx_ctx* ctx, const vx_stark_config* cfg, const vx_tree* tree, const vx_buf* data, size_t off, size_t leaf_len, int layout,
                             const uint64_t* leaf_idx, size_t n_idx, uint64_t* blob_out, size_t blob_cap, size_t* blob_len);
int32_t vx_merkle_rows_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const uint64_t* cap, int cap_height, int log_leaves,
                              size_t leaf_len, const uint64_t* leaf_idx, const uint64_t* rows, size_t n_idx, char* err, size_t errlen);
/* ---- FriFoldAir: the FRI fold chain of every query of one inner proof in one STARK table (AIR id VX_AIR_FRI_FOLD; compiled:
 * csrc/air_fri_fold.cuh) -- the per-query loop of verify_fri_proof (plonky2 v0.2.0 fri/verifier.rs: compute_evaluation at arity 16,
 * x <- x^16, index >>= 4; vx_stark_verify does the same on the host), the third table of proof aggregation and the first that
 * carries field arithmetic of a STARK verifier's query phase.  It is compiled for arity_bits = 4 (vx_stark_default_config): every
 * entry point that takes a configuration REFUSES another arity with VX_ERR_ARG.
 * The inner proof: an LDE of 2^log_lde points, n_layers >= 1 fold layers with challenges betas[n_layers][2], log_lde - 4 n_layers
 * >= 1 index bits left, and a final polynomial final_poly[final_len][2].  A CLAIM is one query: index (< 2^log_lde), ev0[2] (the
 * FRI combination the chain starts from) and leaves[n_layers][32] (the 16 extension values of the query's leaf in every layer,
 * the slot index's own value included).  PROVEN per claim: leaf_l[(index >> 4l) & 15] = ev_l, ev_(l+1) = the interpolant of
 * leaf_l's coset at beta_l, with x_0 = 7 w^bitrev(index) and x_(l+1) = x_l^16; ev_NL leaves the table.  One row per (query,
 * layer) and one per remaining index bit; no positional shape, so any number of queries fits the one AIR id at any log_n >= 5
 * (default configuration, 2^21 LDE: 9 rows per query, 84 queries in 2^10 rows).  Public inputs (24): n_layers, rows per query,
 * 1 / w, TREE0, eight betas (zero behind n_layers) and the claims digest hash_n_to_hash_no_pad((index, ev0, leaves) of every
 * query, in order).  Bus: a fold row receives the 32 words of its leaf as row messages (leaf index, position, word, tree =
 * TREE0 + layer) -- what LeafSpongeSetAir sends in vx_fri_queries_prove; the verifier of vx_fri_fold_verify sends them itself
 * -- a query's first row receives (index, ev0, 0) and its first bit row sends (index, ev_NL, 1).
 * vx_fri_fold_air_trace: the witness on its own (test surface; host claims, nothing is checked beyond ranges) -- trace_out:
 *   [VX_FRI_FOLD_AIR_COLS][2^log_n] with 2^log_n >= n_queries (log_lde - 3 n_layers); rows behind the queries are idle.
 * vx_fri_fold_prove: folds every query natively on the host first and returns VX_ERR_STATEMENT, naming query and layer, when
 *   leaf_l[within] != ev_l or final_poly(x_NL) != ev_NL; then trace + proof at the smallest log_n (>= 5) with TREE0 = 0, under
 *   lookup challenges that are the shared-challenge transcript of this one table.  Blob: the magic "VXFFOLD1", log_lde, n_layers,
 *   n_queries, the proof's length; then the table proof.  VX_ERR_BUFSZ (with *blob_len set) when the buffer is too small.
 * vx_fri_fold_verify (host only, FOLDS NOTHING): rebuilds every public input from its arguments, recomputes the challenges,
 *   verifies the table under them and accepts iff published total x 2^log_n = sum over the claims of - 1/D_row over every leaf
 *   word, - 1/D(index, ev0, 0), + 1/D(index, final_poly(x_NL), 1): per query one exponentiation and one Horner evaluation.
 * vx_stark_fri_claims (host only, prover-side): replays a vx_stark_prove proof (it is verified on the way) and hands out its FRI
 *   side as claims: betas_out[16] (zero behind n_layers), the final polynomial, and per query the index, ev0, optionally the
 *   ev_NL the verifier accepted (ev_last_out may be NULL), and the FULL leaves of every layer -- the proof omits the slot
 *   `within`, which is filled with the value the chain enters the layer with.  final_cap / leaves_cap are in words, query_cap in
 *   queries; VX_ERR_BUFSZ (sizes set) when one is too small.
 * STILL OUTSIDE here: the leaves' Merkle side (vx_fri_queries_prove, below, puts it on the same bus), the FRI combination
 * (FriCombineAir, below: vx_fri_combine_fold_prove closes ev_0 between the two tables), the evaluation at zeta, the transcript, and
 * the final-polynomial evaluation, which stays the verifier's single Horner per query. */
enum { VX_AIR_FRI_FOLD = 18, VX_FRI_FOLD_AIR_COLS = 120, VX_FRI_FOLD_AIR_AUX_COLS = 36 };
int32_t vx_fri_fold_air_trace(vx_ctx* ctx, int log_lde, const uint64_t* betas, size_t n_layers, uint64_t tree0, const uint64_t* index, const uint64_t* ev0,
                              const uint64_t* leaves, size_t n_queries, int log_n, vx_buf* trace_out, uint64_t public_out[24]);
int32_t vx_fri_fold_proof_bound(const vx_stark_config* cfg, int log_lde, size_t n_layers, size_t n_queries, size_t* n_words);
int32_t vx_fri_fold_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len,
                          const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries, uint64_t* blob_out, size_t blob_cap, size_t* blob_len);
int32_t vx_fri_fold_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly,
                           size_t final_len, const uint64_t* index, const uint64_t* ev0, const uint64_t* leaves, size_t n_queries, char* err, size_t errlen);
int32_t vx_stark_fri_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int* log_lde, size_t* n_layers, size_t* final_len, size_t* n_queries,
                            uint64_t betas_out[16], uint64_t* final_poly_out, size_t final_cap, uint64_t* index_out, uint64_t* ev0_out, uint64_t* ev_last_out, size_t query_cap,
                            uint64_t* leaves_out, size_t leaves_cap, char* err, size_t errlen);
/* ---- FriExitAir: an inner proof's query indices, proof of work and FRI exits in one STARK table.  NOT a compiled AIR: the
 * constraint program ships with the library (0-kno-vectorx_amd/air_library.py fri_exit_builder(), registered by the host with
 * vx_air_register_bus; columns and public inputs: csrc/fri_exit_layout.h) and is proven together with the compiled tables by the
 * generic bus group (vx_bus_group_prove); its witness is the library's, as PoseidonAir's is.
 * The statement, for one inner proof: an LDE of 2^log_lde points, n_layers (1..8) fold layers of arity 16, FB = log_lde - 4 n_layers
 * >= 1, pow_bits, n_queries, a final polynomial of final_len (1..64) extension coefficients.  The table holds 1 + n_queries blocks
 * of 128 rows, one per challenge value v of chain 0 behind the final polynomial: the proof-of-work response (ordinal ord_pow), then
 * the index challenges (ordinals ord_pow + 1 + q), all drawn with `absorbed` words absorbed.  PROVEN per block: the 64 bits of v,
 * MSB first, are boolean, spell an integer below p = 2^64 - 2^32 + 1 and sum to the value the block RECEIVES as (0, ordinal,
 * absorbed, v) under tag 13 (TranscriptAir sends it); the PoW response has its top pow_bits bits zero; a query's index is the low
 * log_lde bits of v, its point behind the folds x_NL = 7^(16^NL) w_FB^brev(index >> 4 NL, FB), and the final polynomial's value
 * there -- every coefficient RECEIVED as (k, c_k.a, c_k.b) under tag 14, which whoever holds the proof head sends n_queries times
 * -- is RECEIVED as (index, value, 1) under tag 10, the exit FriFoldAir sends.  A verifier with this table on its bus computes no
 * value mod N, no proof-of-work shift, no x^(16^NL) and no Horner evaluation.  Public inputs (12): ord_pow, absorbed, pow_bits,
 * 64 - log_lde, FB, w_FB, 7^(16^NL), final_len and four statement-digest words the table does not constrain.
 * vx_fri_exit_air_trace: the witness -- values: the 1 + n_queries challenge values (host); trace_out: [21][2^log_n] with 2^log_n
 *   >= 128 (1 + n_queries); blocks behind the values are idle (all zero but the ordinal column, which goes by position).
 *   public_out[12]: as vx_fri_exit_public.  VX_ERR_ARG: a non-canonical value, a log_n too small or above 26, n_layers outside
 *   1..8, FB < 1, final_len outside 1..64; VX_ERR_STATEMENT ("proof of work invalid"): a response with a bit among its top pow_bits.
 * vx_fri_exit_public (host only, the verifier's side): the 12 public inputs, the digest being hash_n_to_hash_no_pad(the other
 *   eight, the final polynomial's words).  VX_ERR_ARG for the same shapes.
 * vx_fri_exit_log_n: the smallest log_n that holds the blocks; the caller raises it to a size with a FRI plan.
 * vx_fri_exit_statement (host only): hash_n_to_hash_no_pad of the canonical words the caller lays out -- the ONE statement digest
 *   that the tables of an exit group carry as their last four public inputs (lib.py fri_exit_statement_words states the layout). */
int32_t vx_fri_exit_air_trace(vx_ctx* ctx, int log_lde, size_t n_layers, int pow_bits, uint64_t ord_pow, uint64_t absorbed, const uint64_t* values, size_t n_queries,
                              const uint64_t* final_poly, size_t final_len, int log_n, vx_buf* trace_out, uint64_t* public_out);
int32_t vx_fri_exit_public(int log_lde, size_t n_layers, int pow_bits, uint64_t ord_pow, uint64_t absorbed, const uint64_t* final_poly, size_t final_len, uint64_t* public_out);
int vx_fri_exit_log_n(size_t n_queries);
int32_t vx_fri_exit_statement(const uint64_t* words, size_t n_words, uint64_t digest_out[4]);
/* ---- The FRI query phase on one bus: the layer leaves opened, hashed and folded (vx_fri_queries_prove).  An inner proof's FRI
 * has n_layers layer trees with different roots and depths (log_lde - 4 (l + 1)), every leaf 32 words.  Two SET tables carry
 * several trees in one table:
 *   MerkleOpenSetAir (AIR id VX_AIR_MERKLE_OPEN_SET; csrc/air_merkle_open.cuh): MerkleOpenAir with six more block-constant columns
 *     TREE, ROOT[4], DEPTH.  Root and depth are no public inputs: the END block of a path SENDS them (TAG_ROOT: 2 tree + half, two
 *     root words, depth) and whoever knows the trees receives them.  Openings go out as (index, two digest words, half + 2 tree).
 *     Public inputs (4): a digest the table does not constrain.
 *   LeafSpongeSetAir (AIR id VX_AIR_LEAF_SPONGE_SET; csrc/air_leaf_sponge.cuh): LeafSpongeAir with one more block-constant column
 *     TREE; row words go out with their tree in the fourth slot, the digest is received with it.  L, B and the tail flags stay public
 *     inputs (14 as in LeafSpongeAir): all trees of one table share a leaf length.
 * vx_merkle_open_set_air_trace / vx_leaf_sponge_set_air_trace: the witnesses on their own (test surfaces).  Opening i is leaf
 *   leaf_idx[i] of tree tree_of[i] (< n_trees <= 64; duplicates allowed); trace_out: [VX_*_SET_AIR_COLS][2^log_n].  The sponge
 *   surface takes FRI layers: evals[t] holds 2^(log_leaves[t] + 4) extension values in natural order, as vx_fri_layer_tree reads
 *   them (leaf j = the 16 values at bitrev(16 j + t)); L = 32.  public_out: the public inputs, whose digest is the claims digest of
 *   the set -- hash_n_to_hash_no_pad of (tree, index, leaf digest) resp. (tree, index, row) of every opening in order.
 * vx_fri_queries_prove: trees[l] / evals[l]: the tree vx_fri_layer_tree built (arity_bits 4, one cap height <= log_lde - 4
 *   n_layers for all layers) and the layer it was built from, l < n_layers <= 8; index[n_queries] < 2^log_lde.  Gathers ev_0 and
 *   every query's leaf in every layer on the device, folds every query natively first (VX_ERR_STATEMENT names query and layer; a
 *   layer that does not hash to its tree's leaves is VX_ERR_STATEMENT too; nothing is proven then), and proves MerkleOpenSetAir
 *   (one path per (query, layer)), LeafSpongeSetAir (one leaf per (query, layer)) and FriFoldAir (TREE0 = 0: tree id = layer) under
 *   shared challenges, in that bus order.  The four digest words of all three tables are the STATEMENT digest:
 *   hash_n_to_hash_no_pad(log_lde, n_layers, n_queries, betas, final_poly, the n_layers roots, (index, ev_0) of every query), a
 *   root being the two-to-one fold of a cap.  VX_ERR_ARG: arity_bits != 4, n_layers > 8, cap height > log_lde - 4 n_layers, a
 *   table of more than 2^26 rows.  Blob: "VXFQRY01", log_lde, n_layers, n_queries, three lengths, three proofs.
 * vx_fri_queries_verify (host only): holds the layer caps caps[n_layers][4 << cap_height], the betas, the final polynomial and
 *   (index, ev0) per query -- NO leaves; walks no path, hashes no leaf, folds nothing.  Rebuilds every public input of all three
 *   tables from its arguments, sends (index, ev_0) of every query, receives (index, final_poly(x_NL)) and, per layer, the two
 *   halves of (root of caps[l], depth log_lde - 4 (l + 1)); accepts iff all three tables verify and the bus balances.
 * STILL OUTSIDE here: the commitment trees' Merkle side and binding to the layer trees vx_stark_prove builds itself -- both are
 * vx_stark_openings_prove (below), which proves every tree's openings from the paths a proof carries; ev_0 comes from FriCombineAir
 * (below), not yet on this three-table bus. */
enum { VX_AIR_MERKLE_OPEN_SET = 19, VX_MERKLE_OPEN_SET_AIR_COLS = 72, VX_MERKLE_OPEN_SET_AIR_AUX_COLS = 6 };
enum { VX_AIR_LEAF_SPONGE_SET = 20, VX_LEAF_SPONGE_SET_AIR_COLS = 67, VX_LEAF_SPONGE_SET_AIR_AUX_COLS = 12 };
int32_t vx_merkle_open_set_air_trace(vx_ctx* ctx, const vx_tree* const* trees, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx, int log_n,
                                     vx_buf* trace_out, uint64_t public_out[4]);
int32_t vx_leaf_sponge_set_air_trace(vx_ctx* ctx, const vx_buf* const* evals, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx, size_t n_idx,
                                     int log_n, vx_buf* trace_out, uint64_t public_out[14]);
int32_t vx_fri_queries_proof_bound(const vx_stark_config* cfg, int log_lde, size_t n_layers, size_t n_queries, size_t* n_words);
int32_t vx_fri_queries_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly, size_t final_len,
                             const vx_tree* const* trees, const vx_buf* const* evals, const uint64_t* index, size_t n_queries, uint64_t* blob_out, size_t blob_cap, size_t* blob_len);
int32_t vx_fri_queries_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, int log_lde, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly,
                              size_t final_len, const uint64_t* caps, int cap_height, const uint64_t* index, const uint64_t* ev0, size_t n_queries, char* err, size_t errlen);
/* ---- A STARK proof's Merkle openings proven from the paths it carries (vx_stark_openings_prove).  Every Merkle-side prover above
 * takes vx_tree handles and buffers resident on the device; an aggregator holds proof BYTES.  A vx_stark_prove proof carries, per
 * query, the opened rows of its three commitment trees, the leaves of its FRI layers and every sibling up to the caps: that is
 * the whole witness of MerkleOpenSetAir and LeafSpongeSetAir, no new AIR and no new bus tag.
 * Conventions (prover, verifier and tests/stark_openings_ref.py alike): layer l is tree l, main / auxiliary / quotient are trees
 *   8 / 9 / 10; inside a query the order of the query record -- main, auxiliary (only when the AIR has auxiliary columns),
 *   quotient, layers 0..NL-1 --, queries outermost in proof order, duplicates included.  Leaf index: x_index for the commitment
 *   trees, x_index >> a (l + 1) for layer l (a = arity_bits, any the configuration allows); log_leaves: LN resp. LN - a (l + 1);
 *   leaf lengths cm, ca, 4 and 2 2^a, the `within` slot of a layer leaf filled with the verifier's running evaluation.
 * vx_stark_merkle_claims (host only, prover-side): replays a proof with the verifier's own code in its DELEGATED mode -- every
 *   check except the Merkle paths runs, no sibling word is read by it -- and hands out shape_out = (LN, cm, ca, a, NL, cap_height,
 *   n_queries), the trees of a query cap_tree_out[*n_trees] with their caps caps_out[*n_trees][4 << cap_height], and per opening
 *   (tree, index, leaf_len), the leaf words one after the other in leaves_out and the 4 (log_leaves - cap_height) sibling words
 *   one after the other in siblings_out.  ext_chal (may be NULL) as in a bus group: the lookup challenges the proof was made
 *   under.  caps_cap / leaves_cap / siblings_cap are in words, claims_cap in openings; VX_ERR_BUFSZ (all sizes set) when one is too
 *   small; VX_ERR_ARG for more than 8 fold layers.
 * vx_merkle_paths_air_trace: the witness of MerkleOpenSetAir from paths (test surface; mirrors vx_merkle_open_set_air_trace cell by
 *   cell).  Tree t < n_trees <= 64 has 2^log_leaves[t] leaves (0: no such tree) and the cap caps[t][4 << cap_height]; opening i
 *   enters with leaf_digests[i][4] and the 4 (log_leaves - cap_height) words of its path in `siblings`, one opening after the
 *   other.  16 lanes per path walk the chain (siblings above the cap come from the fold of the cap) and store what enters every
 *   level; a path that does not reach the folded root is VX_ERR_STATEMENT.
 * vx_leaf_sponge_rows_air_trace: the witness of LeafSpongeSetAir from rows handed over directly (test surface): rows[i][leaf_len],
 *   leaf_len >= 5, canonical words; public_out as vx_leaf_sponge_set_air_trace.
 * vx_stark_openings_prove: extracts the claims (the inner proof is verified on the way), runs the sponge chains and the paths once
 *   on the device -- a path that does not reach its root is VX_ERR_STATEMENT naming query and tree, nothing is proven then -- and
 *   proves, under shared challenges and in this bus order, MerkleOpenSetAir (one path per claim) and one LeafSpongeSetAir table per
 *   distinct leaf length above 4 among {cm, ca, 2 2^a}, by ascending length: 1 to 4 tables.  Rows: 32 per level of every path,
 *   32 per 8 words of every leaf, each table at the smallest log_n >= 5; VX_ERR_ARG above 2^26.  The four digest words of every
 *   table are the STATEMENT digest: hash_n_to_hash_no_pad(shape words, the folded root of every tree in record order, per query the
 *   index and the leaf words of every tree in record order).  Blob: "VXSOPEN1", the 7 shape words, the table count, one length per
 *   table, the proofs.  vx_stark_openings_proof_bound reads the head of the inner proof alone.
 * vx_stark_openings_verify (host only): verifies the inner proof in the delegated mode against expect_air / expect_public (0 / NULL:
 *   not checked) and the group with it as the outside party: per claim it receives root(tree, lo / hi) with depth log_leaves, every
 *   word of a row longer than 4 words, and the opening itself of a row that is its own digest.  Walks no path, hashes no leaf, reads
 *   no sibling: the siblings are dead weight in a proof verified this way.  The statement digest costs about as many permutations as
 *   hashing the rows would; what disappears is everything per tree level.
 * The query arithmetic on this same bus: vx_stark_queries_prove (below), where FriCombineAir / FriFoldAir take the verifier's place.
 * STILL OUTSIDE: the constraint identity at zeta; the transcript joins this bus in vx_stark_inner_prove (below). */
int32_t vx_stark_merkle_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t shape_out[7], size_t* n_trees,
                               uint64_t cap_tree_out[11], uint64_t* caps_out, size_t caps_cap, size_t* n_claims, uint64_t* tree_out, uint64_t* index_out, uint64_t* leaf_len_out,
                               size_t claims_cap, size_t* leaves_len, uint64_t* leaves_out, size_t leaves_cap, size_t* siblings_len, uint64_t* siblings_out, size_t siblings_cap,
                               char* err, size_t errlen);
int32_t vx_merkle_paths_air_trace(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                                  const uint64_t* leaf_digests, const uint64_t* siblings, size_t n_idx, int log_n, vx_buf* trace_out, uint64_t public_out[4]);
int32_t vx_leaf_sponge_rows_air_trace(vx_ctx* ctx, size_t leaf_len, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* rows, size_t n_idx, int log_n,
                                      vx_buf* trace_out, uint64_t public_out[14]);
int32_t vx_stark_openings_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, size_t* n_words);
int32_t vx_stark_openings_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                                size_t* blob_len);
int32_t vx_stark_openings_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const uint64_t* proof, size_t proof_len, int expect_air,
                                 const uint64_t* expect_public, size_t n_public, const uint64_t* ext_chal, char* err, size_t errlen);
/* ---- FriCombineAir: the FRI combination of every query of one inner proof in one STARK table (AIR id VX_AIR_FRI_COMBINE; compiled:
 * csrc/air_fri_combine.cuh) -- what a STARK verifier computes per query before the fold loop (plonky2 v0.2.0 fri/verifier.rs
 * fri_combine_initial; vx_stark_verify does the same on the host), the fourth table of proof aggregation.
 * The inner proof: an LDE of 2^log_lde points over a trace of 2^(log_lde - rate_bits) rows, cm main, ca auxiliary (may be 0) and
 * nq quotient columns (c = cm + ca), the challenge alpha[2], the point zeta[2], and the openings open_local[c][2], open_next[c][2],
 * open_quot[nq][2].  A CLAIM is one query: index (< 2^log_lde), rows[c + nq] (the opened main, auxiliary and quotient row, back to
 * back) and ev0[2].  PROVEN per claim, with y0 = sum alpha^j local_j + sum alpha^(c+j) quot_j, y1 = sum alpha^j next_j:
 *   s1 = sum_(j<c) alpha^j w_j,  s0 = s1 + sum_(j<nq) alpha^(c+j) q_j,  x = 7 w^bitrev(index, log_lde),
 *   ev0 = alpha^c (s0 - y0) / (x - zeta) + (s1 - y1) / (x - zeta w_n).
 * One word per absorb row, c + nq absorb rows and log_lde bit rows per query; no positional shape, so any number of queries of any
 * shape fits the one AIR id at any log_n >= 5 (the hash-chain table, 2^21 LDE: 1046 rows per query, 84 queries in 2^17 rows).
 * Public inputs (22): rows per query, cm, ca, nq, TREE0, w, alpha, alpha^c, zeta, zeta w_n, y0, y1 and the claims digest
 * hash_n_to_hash_no_pad(log_lde, rate_bits, cm, ca, nq, n_queries, alpha, zeta, the openings, (index, rows, ev0) of every query).
 * Bus: every absorb row receives its word as a row message (index, position in its tree's row, word, tree = TREE0 + 0 main / 1
 * auxiliary / 2 quotient) -- what a leaf sponge over the commitment trees sends; the verifier of vx_fri_combine_verify sends them
 * itself -- and the query's last row sends (index, ev0, 0), the entry FriFoldAir receives.
 * vx_fri_combine_air_trace: the witness on its own (test surface; host claims, nothing is checked beyond ranges) -- trace_out:
 *   [VX_FRI_COMBINE_AIR_COLS][2^log_n] with 2^log_n >= n_queries (c + nq + log_lde); rows behind the queries are idle.
 * vx_fri_combine_prove: combines every query natively on the host first and returns VX_ERR_STATEMENT, naming the query, when the
 *   claimed ev0 differs or x = zeta; then trace + proof at the smallest log_n (>= 5) with TREE0 = 8 (behind FriFoldAir's layer
 *   ids), rate_bits from the configuration, under lookup challenges that are the shared-challenge transcript of this one table.
 *   Blob: the magic "VXFCOMB1", log_lde, cm, ca, nq, n_queries, the proof's length; then the table proof.  VX_ERR_BUFSZ (with
 *   *blob_len set) when the buffer is too small; VX_ERR_ARG for an index outside the LDE or a table of more than 2^26 rows.
 * vx_fri_combine_verify (host only, COMBINES NOTHING per query): computes y0, y1, alpha^c and zeta w_n once, rebuilds every public
 *   input, recomputes the challenges, verifies the table and accepts iff published total x 2^log_n = sum over the claims of
 *   - 1/D_row over every row word + 1/D(index, ev0, 0).
 * vx_stark_combine_claims (host only, prover-side): replays a vx_stark_prove proof (it is verified on the way) and hands out the
 *   combination's claims: the shape, alpha, zeta, openings_out (local, next, quotient back to back: 4 c + 2 nq words) and per query
 *   the index, ev0 and the c + nq row words.  openings_cap / rows_cap are in words, query_cap in queries; VX_ERR_BUFSZ (sizes
 *   set) when one is too small.
 * vx_fri_combine_fold_prove / _verify: FriCombineAir (TREE0 = 8) and FriFoldAir (TREE0 = 0, unchanged) as two parties of ONE bus,
 *   combine first: (index, ev0, 0) closes BETWEEN the tables, so the verifier is handed NO ev0.  Its arguments: the shape, alpha,
 *   zeta, the openings, betas, the final polynomial and per query the index, rows and leaves[n_layers][32].  Both tables' digest
 *   words are one statement digest over all of them.  Accepts iff both tables verify and sum of total x 2^log_n = sum over the
 *   queries of - the row words - the leaf words + 1/D(index, final_poly(x_NL), 1).  The prover runs the native combination and
 *   fold checks first (VX_ERR_STATEMENT names query and stage).  Blob: "VXFCFLD1", log_lde, cm, ca, nq, n_layers, n_queries, two
 *   lengths, two proofs.
 * STILL OUTSIDE: the Merkle side of the commitment trees (a per-tree leaf length), binding to the layer trees vx_stark_prove
 * builds itself, the constraint identity at zeta and the transcript. */
enum { VX_AIR_FRI_COMBINE = 21, VX_FRI_COMBINE_AIR_COLS = 28, VX_FRI_COMBINE_AIR_AUX_COLS = 4 };
int32_t vx_fri_combine_air_trace(vx_ctx* ctx, int log_lde, int rate_bits, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2], const uint64_t* open_local,
                                 const uint64_t* open_next, const uint64_t* open_quot, uint64_t tree0, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0, size_t n_queries,
                                 int log_n, vx_buf* trace_out, uint64_t public_out[22]);
int32_t vx_fri_combine_proof_bound(const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, size_t n_queries, size_t* n_words);
int32_t vx_fri_combine_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2],
                             const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* index, const uint64_t* rows, const uint64_t* ev0,
                             size_t n_queries, uint64_t* blob_out, size_t blob_cap, size_t* blob_len);
int32_t vx_fri_combine_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2],
                              const uint64_t zeta[2], const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* index, const uint64_t* rows,
                              const uint64_t* ev0, size_t n_queries, char* err, size_t errlen);
int32_t vx_stark_combine_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int* log_lde, size_t* cm, size_t* ca, size_t* nq, size_t* n_queries,
                                uint64_t alpha_out[2], uint64_t zeta_out[2], uint64_t* openings_out, size_t openings_cap, uint64_t* index_out, uint64_t* ev0_out, size_t query_cap,
                                uint64_t* rows_out, size_t rows_cap, char* err, size_t errlen);
int32_t vx_fri_combine_fold_proof_bound(const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, size_t n_layers, size_t n_queries, size_t* n_words);
int32_t vx_fri_combine_fold_prove(vx_ctx* ctx, const vx_stark_config* cfg, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2], const uint64_t zeta[2],
                                  const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* betas, size_t n_layers, const uint64_t* final_poly,
                                  size_t final_len, const uint64_t* index, const uint64_t* rows, const uint64_t* leaves, size_t n_queries, uint64_t* blob_out, size_t blob_cap,
                                  size_t* blob_len);
int32_t vx_fri_combine_fold_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, int log_lde, size_t cm, size_t ca, size_t nq, const uint64_t alpha[2],
                                   const uint64_t zeta[2], const uint64_t* open_local, const uint64_t* open_next, const uint64_t* open_quot, const uint64_t* betas, size_t n_layers,
                                   const uint64_t* final_poly, size_t final_len, const uint64_t* index, const uint64_t* rows, const uint64_t* leaves, size_t n_queries, char* err,
                                   size_t errlen);
/* ---- LeafNoopAir: the openings of leaves that are their own digest in one STARK table (AIR id VX_AIR_LEAF_NOOP; compiled:
 * csrc/air_leaf_noop.cuh) -- a Poseidon tree whose leaves have at most 4 words does not hash them (plonky2 v0.2.0 hash_or_noop): the
 * leaf digest is the zero-padded row.  That is the quotient tree of every vx_stark_prove proof and any commitment tree of at most 4
 * columns.  One row per opening: ACT, TREE, IDX, the four words W and four flags E (word j exists); E_0 = ACT, the flags only fall,
 * a word that does not exist is zero.  The row RECEIVES the opening's two open_of(TREE, IDX, ., ., half) messages (what
 * MerkleOpenSetAir sends) and SENDS row_of(TREE, IDX, j, W_j) for every word that exists (what FriCombineAir receives): the no-op
 * counterpart of LeafSpongeSetAir.  The length of a leaf is NOT a public input -- one table carries leaves of several lengths; the
 * receiver's public column counts decide which words must arrive, so the balance of the bus forces the flags.  Public inputs: four
 * digest words the table does not constrain.  Any log_n >= 5; idle rows are zero.
 * vx_leaf_noop_air_trace: the witness on its own (test surface) -- opening i is leaf leaf_idx[i] of tree tree_of[i] with
 *   leaf_len[i] in 1..4 words, rows[i][4] zero-padded; trace_out: [VX_LEAF_NOOP_AIR_COLS][2^log_n] with 2^log_n >= n_idx;
 *   public_out: hash_n_to_hash_no_pad of (tree, index, length, the four words) of every opening.  VX_ERR_ARG: a length outside
 *   1..4, a non-canonical word, a non-zero word behind the length, a table that is too small. */
enum { VX_AIR_LEAF_NOOP = 22, VX_LEAF_NOOP_AIR_COLS = 11, VX_LEAF_NOOP_AIR_AUX_COLS = 8 };
int32_t vx_leaf_noop_air_trace(vx_ctx* ctx, const uint64_t* tree_of, const uint64_t* leaf_idx, const uint64_t* leaf_len, const uint64_t* rows, size_t n_idx, int log_n,
                               vx_buf* trace_out, uint64_t public_out[4]);
/* ---- The whole query phase of a vx_stark_prove proof on ONE bus (csrc/vx_stark_groups.hip): the group of
 * vx_stark_openings_prove with LeafNoopAir, FriCombineAir (TREE0 = 8) and FriFoldAir (TREE0 = 0) in the verifier's place on the row
 * bus, five to seven tables in this order: MerkleOpenSetAir (one path per claim), one LeafSpongeSetAir per distinct leaf length above
 * 4 among {cm, ca, 32} ascending, LeafNoopAir (one row per claim of a leaf of at most 4 words: the quotient tree always),
 * FriCombineAir, FriFoldAir.  Conventions as vx_stark_openings_prove: layer l is tree l, main / auxiliary / quotient are trees 8 / 9 /
 * 10, the record order inside a query and duplicate indices are kept, the `within` slot of a layer leaf holds the running evaluation.
 * vx_stark_queries_prove: the claims come from ONE replay of the verifier's code; the native checks run first -- a path that misses
 *   its root, an ev_0 or a fold that differs, an inner proof the verifier refuses: VX_ERR_STATEMENT naming query and tree or layer,
 *   nothing is proven.  VX_ERR_ARG: arity_bits != 4, no FRI layer or more than 8, log_lde - 4 layers < 1, a table above 2^26 rows.
 *   The four digest words of every table are ONE statement digest: hash_n_to_hash_no_pad(the 7 shape words, alpha, zeta, the openings
 *   local / next / quotient, betas, the final polynomial, the folded root of every tree in record order, the index of every query) --
 *   no row word and no leaf word.  Blob: "VXSQRY01", the 7 shape words, the table count, one length per table, the proofs.
 * vx_stark_queries_verify (host only): runs the inner proof's transcript, proof of work, constraint identity at zeta,
 *   reduce_openings and the query-index derivation in the verifier's QUERY-FREE mode, which reads no word at or behind the query
 *   records: `proof` is the whole proof or its head alone (everything before the first query record); any other length is refused.
 *   It rebuilds every public input of every table from the head and is the outside party of the bus: per query it RECEIVES
 *   root(tree, lo / hi) with depth log_leaves for every tree of the record and fri(index, final_poly(x_NL), 1); it sends nothing.  Per
 *   query one exponentiation and one Horner evaluation remain; the query records (over 90 % of a proof) are dead weight.
 * vx_stark_proof_head_words: where the query records of a proof start -- the length of the head vx_stark_queries_verify accepts --
 *   from the proof's header and the configuration alone; nothing is verified.
 * STILL OUTSIDE here: the transcript (vx_stark_inner_prove below puts TranscriptAir on this same bus), the constraint identity at
 * zeta and the final-polynomial evaluation. */
int32_t vx_stark_proof_head_words(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, size_t* head_words);
int32_t vx_stark_queries_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, size_t* n_words);
int32_t vx_stark_queries_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                               size_t* blob_len);
int32_t vx_stark_queries_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const uint64_t* proof, size_t proof_len, int expect_air,
                                const uint64_t* expect_public, size_t n_public, const uint64_t* ext_chal, char* err, size_t errlen);
/* ---- TranscriptAir: the Fiat-Shamir transcripts of 1..64 inner proofs -- chains -- in one STARK table (AIR id VX_AIR_TRANSCRIPT;
 * compiled: csrc/air_transcript.cuh): the duplex challenger of plonky2 v0.2.0 iop/challenger.rs, one 32-row PoseidonAir
 * block per duplex.  A block RECEIVES obs(chain, position, word) for every word it absorbs and SENDS chal(chain, ordinal, absorbed,
 * value) for every challenge popped from its output; `absorbed` = the words the chain had absorbed when the challenge was drawn.
 * Public inputs: four statement-digest words the table does not constrain.  Any log_n >= 5; idle blocks permute the zero state.
 * vx_transcript_air_trace: the witness on its own (test surface).  Chain c has n_ops[c] run lengths in `ops` (the chains' lists one
 *   after the other): observe count, challenge count, observe count, ... starting with an observe count, zero allowed; `words`: the
 *   observed words of all chains in order (n_words = the sum of the observe counts).  trace_out: [VX_TRANSCRIPT_AIR_COLS][2^log_n];
 *   public_out: the statement digest below; chal_out: one word per challenge drawn, chain after chain (the caller sizes it by the sum
 *   of the challenge counts).  VX_ERR_ARG: a non-canonical word, no chain or more than 64, an empty chain, a chain whose first
 *   operation draws from an empty sponge, a table that is too small ("do not fit").
 * vx_stark_transcript_claims (host only): replays one vx_stark_prove proof -- the whole proof, or its head alone as
 *   vx_stark_proof_head_words cuts it -- with the verifier's own code over a recording challenger and hands out the words its
 *   transcript absorbs (obs_out) and every challenge as (absorbed, value) (chal_out: 2 words each).  ext_chal as vx_stark_verify_ext.
 *   *n_obs / *n_chal are always set on VX_OK and VX_ERR_BUFSZ (a buffer too small; the buffers may be NULL to ask for the sizes).
 * vx_stark_transcripts_prove: proofs[i] (lens[i] words; ext_chals may be NULL, ext_chals[i] NULL: drawn lookup challenges) is chain i.
 *   Every inner proof is verified natively first: a refusal is VX_ERR_STATEMENT naming the proof, nothing is proven.  One
 *   TranscriptAir table at the smallest log_n >= 5 that holds the chains and has a FRI plan; VX_ERR_ARG above 2^26 rows or 64 proofs.
 *   Statement digest: hash_n_to_hash_no_pad(n, per chain n_obs and n_chal, per chain the observed words, per chain (absorbed, value)
 *   of every challenge).  Blob: "VXSTRN01", n, per chain n_obs, n_chal and the claimed challenges as (absorbed, value), the length
 *   of the table's proof, the proof.
 * vx_stark_transcripts_verify (host only): verifies every inner proof with its transcript answered from the blob's claims -- NO
 *   Poseidon permutation runs for an inner transcript; proof of work, query indices, the constraint identity at zeta and (for a whole
 *   proof) the walked query phase use the claimed values; a head alone is read query-free.  Then it is the outside party of the bus:
 *   per chain it SENDS obs(c, i, w_i) for the words it absorbed and RECEIVES chal(c, j, A_j, v_j).  Error texts name the chain.
 * Stand-alone this does not lower the verifier's permutation count: the statement digest hashes the same words; on the
 * bus of the query phase (vx_stark_inner_prove below) it does. */
enum { VX_AIR_TRANSCRIPT = 23, VX_TRANSCRIPT_AIR_COLS = 93, VX_TRANSCRIPT_AIR_AUX_COLS = 18, VX_TRANSCRIPT_MAX_CHAINS = 64 };
int32_t vx_transcript_air_trace(vx_ctx* ctx, size_t n_chains, const size_t* n_ops, const uint64_t* ops, const uint64_t* words, size_t n_words, int log_n, vx_buf* trace_out,
                                uint64_t public_out[4], uint64_t* chal_out);
int32_t vx_stark_transcript_claims(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, size_t* n_obs, uint64_t* obs_out, size_t obs_cap,
                                   size_t* n_chal, uint64_t* chal_out, size_t chal_cap, char* err, size_t errlen);
int32_t vx_stark_transcripts_proof_bound(const vx_stark_config* cfg, const uint64_t* const* proofs, const size_t* lens, size_t n, const uint64_t* const* ext_chals, size_t* n_words);
int32_t vx_stark_transcripts_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* const* proofs, const size_t* lens, size_t n, const uint64_t* const* ext_chals,
                                   uint64_t* blob_out, size_t blob_cap, size_t* blob_len);
int32_t vx_stark_transcripts_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const uint64_t* const* proofs, const size_t* lens, size_t n,
                                    const uint64_t* const* ext_chals, char* err, size_t errlen);
/* ---- An inner proof's query phase AND transcript on ONE bus (csrc/vx_stark_groups.hip): the tables of
 * vx_stark_queries_prove in their order, then TranscriptAir with one chain (id 0) -- six to eight tables.  The tags of the two halves
 * do not meet.  Argument conventions as vx_stark_queries_*; the bound takes ext_chal because the transcript's block count depends on it.
 * vx_stark_inner_prove: claims and chain come from ONE replay of the verifier's code over the recording challenger; the native checks
 *   and the refusals are those of vx_stark_queries_prove (texts under "stark inner:").  The four digest words of every table are ONE
 *   statement digest: hash_n_to_hash_no_pad(the 7 shape words, n_obs, n_chal, the observed words in order, (absorbed, value) of every
 *   challenge in order) -- alpha, zeta, betas and indices are claimed challenges, the openings, the final polynomial and the caps are
 *   observed words: nothing is hashed twice.
 *   Blob: "VXSINR01", the 7 shape words, the table count, n_obs, n_chal, the n_chal claimed challenges as (absorbed, value), one
 *   length per table, the proofs in bus order.
 * vx_stark_inner_verify (host only): `proof` is the whole inner proof or its head alone, any other length is refused.  The claims are
 *   parsed as vx_stark_transcripts_verify does; the inner proof is verified QUERY-FREE with its transcript answered from the claims --
 *   NO Poseidon permutation runs for the inner transcript, the only hashing of the head is the statement digest; proof of work, the
 *   constraint identity at zeta, reduce_openings and the indices (value mod N) use the claimed values.  It rebuilds every public input
 *   of every table from the head, the claims and the digest, and is the outside party of both halves: per query it RECEIVES
 *   root(tree, lo / hi) for every tree of the record and fri(index, final_poly(x_NL), 1); it SENDS obs(0, i, w_i) for every observed
 *   word and RECEIVES chal(0, j, A_j, v_j).
 * STILL OUTSIDE: the constraint identity at zeta (next: it receives alpha and zeta from the transcript table on this bus), the index
 * and proof-of-work checks, the final-polynomial evaluation, more than one inner proof per group. */
int32_t vx_stark_inner_proof_bound(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, size_t* n_words);
int32_t vx_stark_inner_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, const uint64_t* ext_chal, uint64_t* blob_out, size_t blob_cap,
                             size_t* blob_len);
int32_t vx_stark_inner_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const uint64_t* proof, size_t proof_len, int expect_air,
                              const uint64_t* expect_public, size_t n_public, const uint64_t* ext_chal, char* err, size_t errlen);
/* ---- A generic bus group: ANY tables on one logUp bus, proven together under shared lookup challenges (csrc/vx_bus_group.hip; the
 * verifier in csrc/vx_verify.hip).  What the fixed group provers above are for their lists of tables, for a list the caller states:
 * compiled tables, run-time tables (vx_air_register_bus), or both.  The traces exist already (the *_air_trace entry points, or the
 * host's own); the group proves them in the order given, which is the order of the shared-challenge transcript.
 * ADMITTED is any AIR id, compiled or registered, whose auxiliary round takes 4 lookup challenges and publishes 1 value (total /
 * rows): every bus table of the library and every vx_air_register_bus program.  VX_ERR_ARG, naming the table: an unknown id, an AIR
 * without such a round (it would never reach the rendezvous), n_public above 32, n = 0 or n > VX_BUS_GROUP_MAX_TABLES, a trace that
 * is not cols << log_n words.  (Every table runs on a context of its own, chained behind `ctx`; the chain has no fixed length, so
 * the limit is the one chosen here.)
 * OUTSIDE MESSAGES: the messages of the party that is not a table -- the verifier of an aggregation proof, which holds the claims.
 * Each is VX_BUS_MSG_WORDS canonical words (t0, t1, t2, t3, tag, m): the tag below 2^16, an absent slot 0, m the signed
 * multiplicity as a field word with the sign of BUSP_MSG (sent m, received 0 - m).  n_outside = 0 states a closed bus.  The bus
 * closes when   sum over the tables of total x rows  +  sum over the outside messages of m / D  =  0.
 * vx_bus_group_check: the BALANCE CHECK on the device, before anything is proven -- which message of which table and row has no
 *   partner.  Every table needs a message list: a vx_air_register_bus program, or a compiled AIR with ids 4 (the SHA-256
 *   chain), 7 .. 9 (the SHA-256 Merkle tree), 11 / 13 / 14 (the SHA-512 table), 15 (the epoch-end table) or 16 .. 23; any other
 *   compiled AIR (BlakeChainAir, EdAir, LookupAir: periodic lookup tables) is VX_ERR_ARG naming the table.  *out: n_unmatched = 0 when the bus closes; otherwise the number of distinct
 *   tuples whose multiplicities do not cancel and the lowest (table, row, message) among their messages.  It compares 128-bit
 *   fingerprints of the tuples: a collision can hide or mis-name an imbalance, never invent one.
 * vx_bus_group_prove: runs the check first when every table has a message list -- VX_ERR_STATEMENT naming table, AIR, row, message,
 *   net multiplicity and the number of unmatched tuples, nothing proven; otherwise the published totals are summed with the outside
 *   messages after the proofs exist (VX_ERR_STATEMENT "the bus does not close").  Waits for ctx's work before the group starts; the
 *   traces are left intact.  Blob: the magic "VXBGRP01", n, one length per proof, the proofs.  AIR ids are not part of the blob's
 *   request: registered ids are per process and the verifier states its own.  VX_ERR_BUFSZ (with *blob_len set) when the buffer is
 *   too small.  vx_bus_group_proof_bound: the words such a blob needs at most (no GPU; only air_id and log_n of a table are read).
 * vx_bus_group_verify (host only): every proof under the shared challenges against its expected AIR id and public inputs, and the
 *   bus against the outside messages.  VX_ERR_STATEMENT with the reason: a non-canonical outside word, a tag of 2^16 or more, n
 *   different from the blob's, an unexpected AIR id or public input, a zero denominator, a bus that does not balance. */
enum { VX_BUS_GROUP_MAX_TABLES = 16, VX_BUS_MSG_WORDS = 6 };
typedef struct vx_bus_table {   /* prover side */
    int32_t air_id, log_n;
    const vx_buf* trace;              /* [cols][2^log_n] on the context's device; left intact */
    const uint64_t* public_inputs;
    size_t n_public;
} vx_bus_table;
typedef struct vx_bus_expect {  /* verifier side */
    int32_t air_id;
    const uint64_t* public_inputs;
    size_t n_public;
} vx_bus_expect;
typedef struct vx_bus_unmatched {
    uint64_t n_unmatched;             /* distinct tuples whose multiplicities do not sum to 0; 0 = the bus closes */
    int32_t table;                    /* of the record reported: index into tables, or n for an outside message */
    uint32_t message;                 /* ordinal in that table's message list (program order / Air::messages order); 0 outside */
    uint64_t row;                     /* row (first row of the block for block tables); index into `outside` for the outside party */
    uint64_t net;                     /* the tuple's multiplicity sum over ALL parties, canonical field word */
} vx_bus_unmatched;
int32_t vx_bus_group_proof_bound(const vx_stark_config* cfg, const vx_bus_table* tables, size_t n, size_t* n_words);
int32_t vx_bus_group_prove(vx_ctx* ctx, const vx_stark_config* cfg, const vx_bus_table* tables, size_t n, const uint64_t* outside, size_t n_outside, uint64_t* blob_out,
                           size_t blob_cap, size_t* blob_len);
int32_t vx_bus_group_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, const vx_bus_expect* expect, size_t n, const uint64_t* outside, size_t n_outside,
                            char* err, size_t errlen);
int32_t vx_bus_group_check(vx_ctx* ctx, const vx_bus_table* tables, size_t n, const uint64_t* outside, size_t n_outside, vx_bus_unmatched* out);
/* K5: batched constraint / quotient-polynomial evaluation (starky prover.rs compute_quotient_polys) for an AIR compiled
 * into the library or registered as a program.  trace_lde: column-major [cols][N], N = 2^(log_n + rate_bits), natural order, values on the coset
 * 7 * <w_N>.  out[k*N + i] = (sum_j alpha_k^(K-1-j) c_j(x_i)) / Z_H(x_i) for the two challenges k = 0, 1. */
int32_t vx_quotient_eval(vx_ctx* ctx, int air_id, int rate_bits, const vx_buf* trace_lde, int log_n, const uint64_t alphas[2],
                         const uint64_t* public_inputs, size_t n_public, vx_buf* out);
/* The same evaluation for ANY AIR, an auxiliary round included -- the test surface of the compiled constraint systems: the values
 * need not come from a trace.  trace_lde: [cols + aux cols][N], the main columns then the auxiliary ones (the layout vx_stark_prove
 * evaluates); challenges: the AIR's CHAL lookup challenges; aux_public: the 2 * AUXPUB words published with the auxiliary cap.
 * An AIR without an auxiliary round takes both counts 0.  Every host word must be canonical; an AIR whose row count is fixed
 * (positional columns of the trace's period) takes that log_n only, as the prover does. */
int32_t vx_quotient_eval_aux(vx_ctx* ctx, int air_id, int rate_bits, const vx_buf* trace_lde, int log_n, const uint64_t alphas[2],
                             const uint64_t* public_inputs, size_t n_public, const uint64_t* challenges, size_t n_challenges,
                             const uint64_t* aux_public, size_t n_aux_public, vx_buf* out);
/* K9: the partial products of Plonk's permutation argument, as plonky2 computes them (plonky2 v0.2.0 plonk/prover.rs
 * wires_permutation_partial_products_and_zs, util/partial_products.rs; reached from Circuit::prove, circuits/header_range.rs:167).
 * Rows x_i = g^i of the subgroup of order 2^log_n; wires / sigmas: [n_routed][2^log_n] column-major (sigmas = the values of the
 * sigma polynomials, coset shifts included); k_is: the n_routed coset shifts (host); one challenge pair (beta, gamma).
 *   q_j(i) = (w_j(i) + beta k_j x_i + gamma) / (w_j(i) + beta s_j(i) + gamma),  chunk_c = product of `chunk` consecutive q_j,
 *   out column 0 = Z (Z(x_0) = 1, Z(x_(i+1)) = Z(x_i) * all chunks of row i), column t + 1 = Z(x_i) chunk_0(i) .. chunk_t(i)
 *   for t < m - 1, m = ceil(n_routed / chunk) <= 32 columns in all.  This library's own provers are STARK-only and do not
 * call it (no Plonk layer exists here): it is the primitive a patched plonky2 would forward to. */
int32_t vx_partial_products(vx_ctx* ctx, const vx_buf* wires, const vx_buf* sigmas, int log_n, size_t n_routed, const uint64_t* k_is,
                            uint64_t beta, uint64_t gamma, size_t chunk, vx_buf* out);
/* The auxiliary (lookup / logUp) columns an AIR derives from its trace once the lookup challenges are known -- the step
 * vx_stark_prove runs between the trace cap and the constraint challenges, exposed on its own as a test surface.
 * trace: the AIR's main columns [cols][2^log_n]; challenges: the AIR's CHAL base-field elements (canonical);
 * aux_out: [aux cols][2^log_n]; aux_public_out (may be NULL): the values published with the auxiliary cap. */
int32_t vx_stark_aux_trace(vx_ctx* ctx, int air_id, const vx_buf* trace, int log_n, const uint64_t* public_inputs, size_t n_public,
                           const uint64_t* challenges, size_t n_challenges, vx_buf* aux_out, uint64_t* aux_public_out);
/* upper bound on the proof length (uint64 words) for buffer sizing */
int32_t vx_stark_proof_bound(int air_id, const vx_stark_config* cfg, int log_n, size_t* n_words);
int32_t vx_stark_prove(vx_ctx* ctx, int air_id, const vx_stark_config* cfg, const vx_buf* trace, int log_n,
                       const uint64_t* public_inputs, size_t n_public, uint64_t* proof_out, size_t proof_cap,
                       size_t* proof_len);
/* `circuit.verify` (circuits/header_range.rs:170): host-side verification of a proof produced by
 * vx_stark_prove.  expect_air 0 = any; expect_public may be NULL.  VX_OK, or VX_ERR_STATEMENT with
 * a reason written to err (optional buffer).  Needs no GPU and no ctx. */
int32_t vx_stark_verify(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int expect_air,
                        const uint64_t* expect_public, size_t n_expect_public, char* err, size_t errlen);

/* ---- K8: witness hashing for the header chain
 * (plonky2x curta_blake2b_variable via circuits/builder/header.rs:14-19; SimpleMerkleTree /
 *  sha256 via subchain_verification.rs:213-220, 268-274) */
/* headers: device bytes, n messages at `stride` bytes each (uint8 view of a vx_buf);
 * sizes: n uint32 on the HOST; digests_out: 32*n bytes on the HOST */
int32_t vx_blake2b_256_batch(vx_ctx* ctx, const vx_buf* msgs, size_t stride, const uint32_t* sizes, size_t n,
                             uint8_t* digests_out);
/* 64-byte -> 32-byte SHA-256 of n pairs (host in/out; device compute) */
int32_t vx_sha256_pairs(vx_ctx* ctx, const uint8_t* pairs64, size_t n, uint8_t* out32);

/* ---- K8: BlakeChainAir trace generation (the Blake2b witness behind hash_encoded_header,
 * circuits/builder/header.rs:14-19, and the parent-hash links of
 * circuits/builder/subchain_verification.rs:163-177).  headers as for vx_verify_subchain (stride a
 * multiple of 128).  Writes the column-major MAIN trace (745 columns x 2^log_n rows, 16 rows per
 * compression, padded with inactive blocks; byte cells + the multiplicities of the two 2^16-row XOR
 * lookup tables, so log_n >= 16) into trace_out, the 20 public inputs (trusted hash, target hash as
 * 32-bit little-endian limbs, first and last block number, tree_size, bus flag) and optionally the digests
 * (host).  tree_size = 16 / 256 / 512: the state roots (decoder.rs:121-128) and data roots (:132-149) of the
 * headers go onto the logUp bus towards a ShaTreeAir of that many leaves (vx_header_range_prove proves both
 * tables under shared challenges); tree_size = 0: a stand-alone hash-chain proof.  window_length > 0 (one header, tree_size 0;
 * rotate): bytes [window_offset, window_offset + window_length) of the header go onto the bus instead, towards the
 * epoch-end table (vx_epoch_end_trace); public input 19 is the bus mode (0 / 1 / 2), 18 the tree size or the offset.  The 276
 * auxiliary (logUp) columns are derived inside vx_stark_prove once the lookup challenges exist.
 * The AIR proves that header i carries block number first_block_number + i as a SCALE compact int in
 * whichever of the four modes that number takes (decoder.rs:39-92) and reads the state root right behind it.
 * KNOWN DEVIATION: a header shorter than 104 bytes (whose state root and data root would share trace rows) is
 * refused with VX_ERR_ARG; parent hash + number + three 32-byte roots already exceed that in every Avail header.
 * Prove it with vx_stark_prove(ctx, VX_AIR_BLAKE_CHAIN, ...). */
enum { VX_AIR_BLAKE_CHAIN = 6, VX_BLAKE_AIR_COLS = 745, VX_BLAKE_AIR_AUX_COLS = 276 };
int32_t vx_blake_chain_trace(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_headers,
                             const uint8_t trusted_hash[32], uint32_t first_block_number, uint32_t tree_size, uint32_t window_offset, uint32_t window_length,
                             int log_n, vx_buf* trace_out, uint64_t public_inputs_out[20], uint8_t* digests_out);

/* ---- K8: ShaChainAir trace generation (compute_authority_set_commitment, justification.rs:127-162):
 * the chained SHA-256 commitment h_0 = SHA256(pk_0), h_i = SHA256(h_{i-1} || pk_i) over n_keys 32-byte
 * keys (host buffer).  Writes the 414-column trace (64 rows per compression, 2*n_keys - 1
 * compressions, padded with idle blocks), the 10 public inputs (the commitment as big-endian words, the
 * number of keys, bus_on) and optionally the 32 commitment bytes.  signed_flags (may be NULL = none) marks
 * the keys whose signatures the EdDSA table verifies; with bus_on they are sent to it over the lookup bus
 * (bus_on = 0: a stand-alone proof).  Prove with vx_stark_prove(ctx, VX_AIR_SHA_CHAIN, ...). */
enum { VX_AIR_SHA_CHAIN = 4, VX_SHA_AIR_COLS = 414, VX_SHA_AIR_AUX_COLS = 4, VX_SHA_TREE_AIR_COLS = 412 /* the Merkle AIRs 7 / 8 / 9 */ };
int32_t vx_sha_chain_trace(vx_ctx* ctx, const uint8_t* pubkeys, size_t n_keys, const uint8_t* signed_flags, uint32_t bus_on, int log_n, vx_buf* trace_out,
                           uint64_t public_inputs_out[10], uint8_t commitment_out[32]);

/* ---- K8: EdAir trace generation (the curve half of the 300 conditional EdDSA verifications, justification.rs:229-243):
 * n_signatures authorities (pubkey 32 B, signature R || S 64 B, flag), all over the same message (the 53-byte precommit);
 * the flagged ones take the slots of the table in order (slot s = the s-th flagged authority; its index rides along for
 * the bus), 256 rows per slot, at least one slot stays idle: 2^16 rows serve up to 255 signatures -- 2/3 of 300.  Writes
 * the 839-column trace and the 2 public inputs (number of signatures, bus_on); VX_ERR_STATEMENT when one does not verify.  bus_on = 0 makes a stand-alone table (nothing sent to the SHA-512 / authority-set tables).
 * Prove with vx_stark_prove(ctx, VX_AIR_ED25519 (2^17 rows) or VX_AIR_ED25519_16 (2^16 rows), ...). */
enum { VX_AIR_ED25519 = 10, VX_AIR_ED25519_16 = 12, VX_ED_AIR_COLS = 839, VX_ED_AIR_AUX_COLS = 688 };
int32_t vx_ed_trace(vx_ctx* ctx, const uint8_t* pubkeys, const uint8_t* signatures, const uint8_t* message, uint32_t message_len, const uint8_t* signed_flags,
                    size_t n_signatures, int log_n, uint32_t bus_on, vx_buf* trace_out, uint64_t public_inputs_out[2]);

/* ---- K8: Sha512Air trace generation (the hash half of the same verifications): H_i = SHA-512(R_i || A_i || message) for
 * every flagged authority, in compact slots of 160 rows in EdAir's order (2^15 rows hold 204 slots).  Writes the
 * 801-column trace and the 15 public inputs (message words 8..14 of the first block as (lo, hi) halves, bus_on).
 * message_len must be 53 (the precommit).  Prove with vx_stark_prove(ctx, VX_AIR_SHA512 (2^16 rows), VX_AIR_SHA512_15
 * (2^15) or VX_AIR_SHA512_10 (2^10), ...). */
enum { VX_AIR_SHA512 = 11, VX_AIR_SHA512_10 = 13, VX_AIR_SHA512_15 = 14, VX_SHA512_AIR_COLS = 801, VX_SHA512_AIR_AUX_COLS = 4 };
int32_t vx_sha512_trace(vx_ctx* ctx, const uint8_t* pubkeys, const uint8_t* signatures, const uint8_t* message, uint32_t message_len, const uint8_t* signed_flags,
                        size_t n_signatures, int log_n, uint32_t bus_on, vx_buf* trace_out, uint64_t public_inputs_out[15]);

/* ---- K8: EpochEndAir trace generation (verify_epoch_end_header in-proof, circuits/builder/rotate.rs:74-276): the
 * ScheduledChange log of the epoch-end header -- consensus flag 4, "FRNK", a SCALE compact length, flag 1, the compact
 * number of new authorities, num_authorities records (32-byte key, weight 1 as u64 LE), a zero u32 delay -- starting at byte
 * start_position + 1 of `header` (resident in HBM), one row per record in a 512-row table.  The table RECEIVES those bytes
 * over the logUp bus from the Blake2b table that hashes the header (vx_blake_chain_trace with window_offset =
 * start_position + 1, window_length = *window_length_out) and SENDS the keys to the new set's ShaChainAir (vx_sha_chain_trace
 * with bus_on = 2), so the new authority-set commitment is the commitment of exactly those header bytes.  Writes the 52-column
 * trace and the 10 public inputs (num_authorities, bus_on, one-hot byte lengths 1/2/4/5 of the two compact ints).
 * VX_ERR_STATEMENT when the prefix is not the log's; the records themselves are checked by the proof (and named by
 * vx_verify_epoch_end_header).  Prove with vx_stark_prove(ctx, VX_AIR_EPOCH_END, ..., log_n = 9). */
enum { VX_AIR_EPOCH_END = 15, VX_EPOCH_END_AIR_COLS = 52, VX_EPOCH_END_AIR_AUX_COLS = 46, VX_EPOCH_END_LOG_ROWS = 9 };
int32_t vx_epoch_end_trace(vx_ctx* ctx, const vx_buf* header, uint32_t start_position, uint32_t num_authorities, uint32_t bus_on, vx_buf* trace_out,
                           uint64_t public_inputs_out[10], uint32_t* window_length_out);

/* ---- statement level: verify_subchain (circuits/builder/subchain_verification.rs:56-303)
 * headers: n_fetched encoded headers (blocks trusted+1 .. target) resident in HBM at `stride`
 * bytes each (zero padded), sizes on the host.  max_headers = 256 / 512
 * (bin/header_range_{256,512}.rs:15).  Runs the map stage (Blake2b header hashes, header
 * decoding, link checks, 8-leaf SHA-256 roots) and the reduce tree on the GPU and returns the
 * 96-byte public output target_header_hash || state_root_merkle_root || data_root_merkle_root
 * (circuits/header_range.rs:56-58).  VX_ERR_STATEMENT if a chain rule is violated. */
int32_t vx_verify_subchain(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes,
                           size_t n_fetched, uint32_t max_headers, uint32_t trusted_block,
                           const uint8_t trusted_hash[32], uint32_t target_block, uint8_t out96[96]);

/* ---- decoders on their own (test surface for the reference's literal vectors, decoder.rs:238-249 and :388-395).
 * vx_decode_header_batch = decode_header (circuits/builder/decoder.rs:104-157) over n encoded headers in HBM (layout as
 * vx_verify_subchain): block number and mode of the SCALE compact int at byte 32 (decode_compact_int, :39-92; all four
 * modes), ok = 0 where the mode-3 upper-bits assertion (:83-89) fails, parent hash = bytes 0..32, state root at offset
 * 33 / 34 / 36 / 37 by mode (:121-128), data root = the 32 bytes at size - 32, or at 0 for a size-0 padding header
 * (:132-149).  Outputs are host arrays of n (x 32) entries.
 * vx_decode_precommit_batch = decode_precommit (:159-200) over n 53-byte messages (host in / host out, device compute):
 * ok = (byte 0 == 1), block hash [1..33), LE u32 block number, LE u64 round, LE u64 authority set id. */
int32_t vx_decode_header_batch(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n, uint32_t* numbers_out,
                               uint8_t* modes_out, uint8_t* ok_out, uint8_t* parent_out, uint8_t* state_root_out, uint8_t* data_root_out);
int32_t vx_decode_precommit_batch(vx_ctx* ctx, const uint8_t* precommits, size_t n, uint8_t* ok_out, uint8_t* hash_out, uint32_t* block_number_out,
                                  uint64_t* round_out, uint64_t* set_id_out);

/* ---- justification, statement level (circuits/builder/justification.rs:195-257 and the hint's native
 * checks :29-83 -> circuits/input/mod.rs:241-260).  All byte arrays are host buffers.
 * vx_ed25519_verify_batch: ok_out[i] = 1 valid, 0 invalid, 2 skipped (enabled[i] == 0); semantics of
 * ed25519-dalek `verify` (canonical s, compress([s]B - [k]A) == R), the reference's verify_signature.
 * vx_verify_simple_justification: authority-set commitment == authority_set_hash, precommit matches
 * (block number, set id, block hash), every validator marked signed has a valid signature over the
 * precommit, signed * 3 > num_authorities * 2.  pubkeys / signatures / validator_signed have
 * max_authorities entries (32 / 64 / 1 bytes each).  VX_ERR_STATEMENT when any rule fails. */
int32_t vx_ed25519_verify_batch(vx_ctx* ctx, const uint8_t* pubkeys, const uint8_t* sigs, const uint8_t* msg, uint32_t msg_len,
                                const uint8_t* enabled, size_t n, uint8_t* ok_out);
int32_t vx_verify_simple_justification(vx_ctx* ctx, uint32_t block_number, const uint8_t block_hash[32],
                                       uint64_t authority_set_id, const uint8_t authority_set_hash[32],
                                       const uint8_t precommit[53], const uint8_t* pubkeys, const uint8_t* signatures,
                                       const uint8_t* validator_signed, uint32_t num_authorities, uint32_t max_authorities);

/* ---- top level: HeaderRangeCircuit::prove (circuits/header_range.rs:26-59 via Circuit::prove, :167).
 * Inputs as vx_verify_subchain.  Output blob (uint64 words): the magic "HRRANGE6" (VX_HR_BLOB_MAGIC), max_headers,
 * trusted_block, target_block, the 96 public output bytes (12 words), word 16 = S, the number of MAP SEGMENTS of the hash-chain
 * table (1 = one table over the whole range), words 17..20 = the lengths of the authority-set commitment, Merkle, Ed25519 and
 * SHA-512 proofs, word 21 = the round of the precommit, words 22 .. 22 + S = the lengths of the S hash-chain proofs: a header
 * of VX_HR_BLOB_FIXED_WORDS + S words; then the proofs -- the S segments in range order (BlakeChainAir), commitment
 * (ShaChainAir), SHA-256 Merkle trees (ShaTreeAir), Ed25519 (EdAir), SHA-512 (Sha512Air); the commitment / Ed25519 / SHA-512
 * proofs are empty when no justification was given.  EVERY statement of the circuit is inside these STARKs:
 * the tables share one logUp bus under challenges drawn after all their trace caps; the Merkle table's public inputs are the
 * two roots and the number of headers, which forces it to take every header's roots from the bus.
 * MAP SEGMENTS (the reference's MapReduce jobs, circuits/builder/subchain_verification.rs:72-79, 81-232): segment s proves the
 * headers of a contiguous part of the range -- it starts from the hash segment s - 1 ends with, numbers its blocks on and counts
 * its Merkle leaves from the first block of the range; the verifier checks those links between the segments' public inputs
 * (the reference's reduce step, :233-289, without recursion).  Segments are independent tables: vx_header_range_prove_ex can
 * prove a subset of the tables on this GPU (n_shards > 1, one process per GPU) -- the shards of one proof exchange their trace
 * caps once (vx_hr_exchange) and vx_header_range_merge puts their partial blobs together.  Not done: the proofs of a request
 * are not aggregated into one succinct proof (S segments open S times the columns: a segmented blob is larger). */
#define VX_HR_BLOB_MAGIC 0x3645474e41525248ULL /* "HRRANGE6" little-endian */
enum { VX_HR_BLOB_FIXED_WORDS = 22, VX_HR_MAX_SEGMENTS = 64 };
/* The justification witness of circuits/vars.rs:40-46 (host buffers; what HintSimpleJustification
 * returns, justification.rs:69-82) plus the two EVM inputs it is checked against. */
typedef struct vx_justification {
    uint64_t authority_set_id;
    const uint8_t* authority_set_hash; /* 32 bytes */
    const uint8_t* precommit;          /* 53 bytes */
    const uint8_t* pubkeys;            /* max_authorities x 32 */
    const uint8_t* signatures;         /* max_authorities x 64 */
    const uint8_t* validator_signed;   /* max_authorities x 1 */
    uint32_t num_authorities, max_authorities;
} vx_justification;
int32_t vx_header_range_proof_bound(const vx_stark_config* cfg, size_t n_chunks, size_t n_authorities, size_t* n_words);
/* just may be NULL (subchain only); otherwise verify_simple_justification for (target_block, target
 * header hash) is checked on the GPU before proving, as HeaderRangeCircuit::define does (:49-54). */
int32_t vx_header_range_prove(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_fetched,
                              uint32_t max_headers, uint32_t trusted_block, const uint8_t trusted_hash[32],
                              uint32_t target_block, const vx_justification* just, const vx_stark_config* cfg,
                              uint8_t out96[96], uint64_t* proof_out, size_t proof_cap, size_t* proof_len);
/* The same proof with the hash-chain table split into n_segments map segments (1 .. VX_HR_MAX_SEGMENTS, at most one per
 * header; a segment is never smaller than the 2^16-row lookup tables, so more segments than compressions / 4096 only add
 * padding), and optionally only the tables of shard `shard` of `n_shards`: table t in bus order (segments, Merkle, commitment,
 * Ed25519, SHA-512) belongs to shard t mod n_shards.  With n_shards > 1 every shard calls this function on its own GPU with the
 * SAME inputs; `exchange` is called once per proof on each shard, from a prover thread, and must return the element-wise
 * (wrapping) SUM over the shards of the word array it is given (an all-reduce: every shard fills only the slots of its own
 * tables -- public inputs and trace cap -- so the sum is the union).  The blob then holds the local proofs only (the other
 * lengths are 0); vx_header_range_merge makes the request's blob from the shards' blobs.  n_shards = 1: exchange is not used. */
typedef struct vx_hr_exchange {
    int32_t (*fn)(void* user, uint64_t* words, size_t n_words); /* 0 = ok */
    void* user;
} vx_hr_exchange;
int32_t vx_header_range_proof_bound_ex(const vx_stark_config* cfg, size_t n_chunks, size_t n_authorities, uint32_t n_segments, size_t* n_words);
int32_t vx_header_range_prove_ex(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_fetched,
                                 uint32_t max_headers, uint32_t trusted_block, const uint8_t trusted_hash[32],
                                 uint32_t target_block, const vx_justification* just, const vx_stark_config* cfg,
                                 uint32_t n_segments, uint32_t shard, uint32_t n_shards, const vx_hr_exchange* exchange,
                                 uint8_t out96[96], uint64_t* proof_out, size_t proof_cap, size_t* proof_len);
/* blobs of the n_shards shards of ONE proof (same request, same segment count) -> the request's blob; host only */
int32_t vx_header_range_merge(const uint64_t** blobs, const size_t* blob_lens, size_t n_blobs, uint64_t* out, size_t out_cap, size_t* out_len,
                              char* err, size_t errlen);
/* HeaderRangeCircuit verify: checks the blob of vx_header_range_prove against the request (the five fields of the
 * circuit's 80-byte EVM input, header_range.rs:30-37) and the claimed 96 output bytes: every table's STARK under the
 * shared lookup challenges, the bus balance, and -- when the blob carries a justification -- that the committed
 * authority set is authority_set_hash, that more than 2/3 of it signed, and that what it signed is the precommit for
 * (target header hash, target_block, authority_set_id).  authority_set_hash = NULL for a blob proven without one. */
int32_t vx_header_range_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, uint32_t max_headers,
                               uint32_t trusted_block, const uint8_t trusted_hash[32], uint64_t authority_set_id,
                               const uint8_t* authority_set_hash /* 32 B or NULL */, uint32_t target_block, const uint8_t out96[96], char* err,
                               size_t errlen);

/* ---- RotateCircuit: circuits/rotate.rs:80-109, circuits/builder/rotate.rs:74-323 ----
 * EVM input = u64 authority_set_id || bytes32 authority_set_hash (40 B, dummy_rotate.rs:11-14);
 * output = bytes32 new authority set hash.  The RotateHint witness (rotate.rs:29-63, vars.rs RotateStruct)
 * is passed flat: the epoch-end header (device buffer of >= MAX_HEADER_SIZE bytes, zero padded past
 * header_size, as get_header_rotate builds it, input/mod.rs:848-858), its size, the epoch-end block number,
 * target_header_num_authorities, next_authority_set_start_position and the new pubkeys (host, n x 32). */
/* verify_epoch_end_header (builder/rotate.rs:176-276) on the GPU, one lane per validator slot. */
int32_t vx_verify_epoch_end_header(vx_ctx* ctx, const vx_buf* header, uint32_t num_authorities, uint32_t start_position,
                                   const uint8_t* new_pubkeys, uint32_t max_authorities);
int32_t vx_rotate_proof_bound(const vx_stark_config* cfg, size_t n_chunks, size_t n_cur_authorities, size_t n_new_authorities,
                              size_t* n_words);
/* RotateMethods::rotate (builder/rotate.rs:278-323) + Circuit::prove.  Six STARKs on two logUp buses: (A) the justification
 * by the current set (`just`, required): its commitment, the Ed25519 and the SHA-512 tables; (B) the Blake2b header hash, which
 * sends the bytes behind start_position to the epoch-end table (verify_epoch_end_header in-proof), which sends the keys it
 * reads there to the new set's commitment -- out32.  Every rule is also checked natively first and named in the error.
 * The log must lie inside the first header_size bytes (the hashed ones) and behind byte 72.
 * VX_ERR_STATEMENT where the reference circuit's assertions (or the hint's panics) would fail. */
int32_t vx_rotate_prove(vx_ctx* ctx, const vx_buf* header, uint32_t header_size, uint32_t epoch_end_block_number,
                        uint32_t num_authorities, uint32_t start_position, const uint8_t* new_pubkeys,
                        const vx_justification* just, const vx_stark_config* cfg, uint8_t out32[32], uint64_t* proof_out,
                        size_t proof_cap, size_t* proof_len);
int32_t vx_rotate_verify(const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, uint64_t authority_set_id,
                         const uint8_t authority_set_hash[32], const uint8_t out32[32], char* err, size_t errlen);

/* ---- Verifying on the GPU: every Merkle opening of a verification checked in one launch (csrc/vx_merkle_check.hip) ----
 * A proof's verification on the host is mostly its Merkle openings, walked one after the other (per opening: one permutation per 8
 * leaf words, one per tree level).  The verifiers below run everything else on the host as before and leave the openings to ONE
 * launch of k_merkle_check: 16 lanes per opening, the row absorbed as hash_or_noop does, the path walked with two_to_one, the cap
 * entry compared; the kernel stores one word, the first opening that fails.
 * vx_merkle_check: the check on its own.  All pointers are host pointers and the layout is what vx_stark_merkle_claims hands out:
 *   tree t (< n_trees) has 2^log_leaves[t] leaves under the cap caps[t][4 << cap_height]; claim i opens leaf leaf_idx[i] of tree
 *   tree_of[i] with a row of leaf_len[i] >= 1 words; the rows lie one after the other in `leaves` (leaves_len words in all), the
 *   4 (log_leaves - cap_height) sibling words of every claim, leaf level first, one after the other in `siblings`.
 *   VX_OK with *first_bad = SIZE_MAX when every claim reaches its cap entry (index >> (log_leaves - cap_height)); VX_ERR_STATEMENT
 *   with *first_bad = the smallest failing claim; VX_ERR_ARG for a non-canonical word, an index outside its tree, a tree with
 *   log_leaves < cap_height (or above 40), cap_height above 16, lengths that do not add up.  n_claims = 0: VX_OK, nothing is launched.
 *   The words are staged through a pool block of `ctx` on its stream and the call waits before it returns; the ctx stays usable
 *   after a refusal.
 * vx_stark_verify_dev / vx_header_range_verify_dev / vx_rotate_verify_dev: the arguments of their host namesakes behind a ctx, and
 *   for every input the same code and the same reason in err -- the query and tree a failing opening names included.  The host
 *   verifier checks in sequence; to answer as it does, the proof is scanned for non-canonical words whole (siblings included), the
 *   host pass runs with the openings recorded instead of walked, and the openings recorded up to the point where the pass ended --
 *   at its end, or at a refusal of its own -- are checked on the device: the first that fails wins over the pass's own refusal,
 *   the host verifier would have met it first.  A blob's tables are read in the host verifier's order, tables behind the first
 *   refused one are not read, and the openings of all tables read go to the device in one launch.  A failure of the device
 *   itself: VX_ERR_DEVICE / VX_ERR_OOM with the reason in err.
 * vx_stark_verify_deferred (host only, test surface): the same deferred-order code with the host's own path check in place of the
 *   kernel; answers as vx_stark_verify does. */
int32_t vx_merkle_check(vx_ctx* ctx, const uint64_t* caps, int cap_height, const int* log_leaves, size_t n_trees, const uint64_t* tree_of, const uint64_t* leaf_idx,
                        const uint64_t* leaf_len, const uint64_t* leaves, size_t leaves_len, const uint64_t* siblings, size_t siblings_len, size_t n_claims, size_t* first_bad);
int32_t vx_stark_verify_dev(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int expect_air, const uint64_t* expect_public, size_t n_expect_public,
                            char* err, size_t errlen);
int32_t vx_header_range_verify_dev(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, uint32_t max_headers, uint32_t trusted_block,
                                   const uint8_t trusted_hash[32], uint64_t authority_set_id, const uint8_t* authority_set_hash /* 32 B or NULL */, uint32_t target_block,
                                   const uint8_t out96[96], char* err, size_t errlen);
int32_t vx_rotate_verify_dev(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* blob, size_t blob_len, uint64_t authority_set_id, const uint8_t authority_set_hash[32],
                             const uint8_t out32[32], char* err, size_t errlen);
int32_t vx_stark_verify_deferred(const vx_stark_config* cfg, const uint64_t* proof, size_t proof_len, int expect_air, const uint64_t* expect_public, size_t n_expect_public, char* err,
                                 size_t errlen);

/* ---- multi-GPU: proofs are independent, one per rank; the only exchange is this gather ----
 * All-gathers `n_words` u64 words per rank over RCCL on the ctx stream: out (host, world * n_words words, rank
 * order) is filled on EVERY rank; blobs must have the same length on all ranks (pad to the proof bound).
 * `nccl_comm` is an ncclComm_t the caller created (ncclCommInitRank, one rank per GPU); the RCCL symbols are
 * looked up in the process at call time, so the library has no link-time dependency on RCCL and uses the same
 * copy the caller's communicator belongs to.  VX_ERR_DEVICE if RCCL is not loaded or the collective fails. */
int32_t vx_gather_proofs(vx_ctx* ctx, void* nccl_comm, int world, const uint64_t* mine, size_t n_words, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* VX_H */
