"""ctypes binding of libvxprove.so (C ABI: include/vx.h)."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VX_LIB_PATH") or os.path.join(_HERE, "libvxprove.so")  # VX_LIB_PATH: A/B builds of the same library (tools/ab_kernels.py)
P = 2**64 - 2**32 + 1

VX_ORDER_NATURAL, VX_ORDER_BITREV = 0, 1
VX_LDE_SRC_VALUES, VX_LDE_SRC_COEFFS = 0, 1
VX_LEAVES_ROW_MAJOR, VX_LEAVES_COLS_BITREV, VX_LEAVES_COLS = 0, 1, 2
ERR_NAMES = {-1: "VX_ERR_ARG", -2: "VX_ERR_DEVICE", -3: "VX_ERR_OOM", -4: "VX_ERR_BUFSZ", -5: "VX_ERR_STATEMENT", -6: "VX_ERR_POW"}

# every symbol include/vx.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "vx_ctx_create", "vx_ctx_destroy", "vx_sync", "vx_last_error", "vx_backend_name", "vx_timer_start", "vx_timer_stop", "vx_table_streams_mode",
    "vx_alloc", "vx_free", "vx_upload", "vx_download", "vx_copy", "vx_fill_random", "vx_buf_devptr", "vx_buf_len",
    "vx_field_batch_add", "vx_field_batch_sub", "vx_field_batch_mul", "vx_field_batch_inv", "vx_ext_batch_mul",
    "vx_ntt", "vx_lde", "vx_lde_rows",
    "vx_poseidon_permute_batch", "vx_merkle_build", "vx_merkle_free", "vx_merkle_cap", "vx_merkle_open", "vx_merkle_leaf_digests",
    "vx_fri_fold", "vx_fri_layer_tree", "vx_fri_leaves", "vx_fri_pow",
    "vx_stark_default_config", "vx_stark_proof_bound", "vx_stark_prove", "vx_stark_verify", "vx_header_range_proof_bound", "vx_header_range_prove", "vx_header_range_verify",
    "vx_header_range_proof_bound_ex", "vx_header_range_prove_ex", "vx_header_range_merge",
    "vx_blake2b_256_batch", "vx_sha256_pairs", "vx_verify_subchain", "vx_blake_chain_trace",
    "vx_ed25519_verify_batch", "vx_verify_simple_justification", "vx_sha_chain_trace",
    "vx_verify_epoch_end_header", "vx_rotate_proof_bound", "vx_rotate_prove", "vx_rotate_verify",
    "vx_gather_proofs", "vx_quotient_eval", "vx_quotient_eval_aux", "vx_decode_header_batch", "vx_decode_precommit_batch", "vx_stark_aux_trace",
    "vx_ed_trace", "vx_sha512_trace", "vx_epoch_end_trace", "vx_partial_products", "vx_air_register", "vx_air_register_bus", "vx_air_unregister", "vx_poseidon_air_trace",
    "vx_merkle_open_air_trace", "vx_merkle_openings_proof_bound", "vx_merkle_openings_prove", "vx_merkle_openings_verify",
    "vx_leaf_sponge_air_trace", "vx_merkle_rows_proof_bound", "vx_merkle_rows_prove", "vx_merkle_rows_verify",
    "vx_fri_fold_air_trace", "vx_fri_fold_proof_bound", "vx_fri_fold_prove", "vx_fri_fold_verify", "vx_stark_fri_claims",
    "vx_fri_exit_air_trace", "vx_fri_exit_public", "vx_fri_exit_log_n", "vx_fri_exit_statement",
    "vx_merkle_open_set_air_trace", "vx_leaf_sponge_set_air_trace", "vx_fri_queries_proof_bound", "vx_fri_queries_prove", "vx_fri_queries_verify",
    "vx_fri_combine_air_trace", "vx_fri_combine_proof_bound", "vx_fri_combine_prove", "vx_fri_combine_verify", "vx_stark_combine_claims",
    "vx_fri_combine_fold_proof_bound", "vx_fri_combine_fold_prove", "vx_fri_combine_fold_verify",
    "vx_stark_merkle_claims", "vx_merkle_paths_air_trace", "vx_leaf_sponge_rows_air_trace", "vx_stark_openings_proof_bound", "vx_stark_openings_prove", "vx_stark_openings_verify",
    "vx_leaf_noop_air_trace", "vx_stark_queries_proof_bound", "vx_stark_queries_prove", "vx_stark_queries_verify", "vx_stark_proof_head_words",
    "vx_transcript_air_trace", "vx_stark_transcript_claims", "vx_stark_transcripts_proof_bound", "vx_stark_transcripts_prove", "vx_stark_transcripts_verify",
    "vx_stark_inner_proof_bound", "vx_stark_inner_prove", "vx_stark_inner_verify",
    "vx_bus_group_proof_bound", "vx_bus_group_prove", "vx_bus_group_verify", "vx_bus_group_check",
    "vx_merkle_check", "vx_stark_verify_dev", "vx_header_range_verify_dev", "vx_rotate_verify_dev", "vx_stark_verify_deferred",
]

VX_AIR_FIBONACCI, VX_AIR_MIX, VX_AIR_BLAKE_CHAIN, VX_AIR_LOOKUP = 1, 2, 6, 5
VX_BLAKE_AIR_COLS, VX_BLAKE_AIR_AUX_COLS = 745, 276
VX_AIR_SHA_TREE = {256: 7, 512: 8, 16: 9}
VX_AIR_SHA_CHAIN, VX_SHA_AIR_COLS, VX_SHA_AIR_AUX_COLS, VX_SHA_TREE_AIR_COLS = 4, 414, 4, 412
VX_AIR_ED25519 = {17: 10, 16: 12}
VX_ED_AIR_COLS, VX_ED_AIR_AUX_COLS = 839, 688
VX_AIR_SHA512 = {16: 11, 15: 14, 10: 13}
VX_SHA512_AIR_COLS, VX_SHA512_AIR_AUX_COLS = 801, 4
VX_AIR_EPOCH_END, VX_EPOCH_END_AIR_COLS, VX_EPOCH_END_AIR_AUX_COLS = 15, 52, 46
VX_AIR_MERKLE_OPEN, VX_MERKLE_OPEN_AIR_COLS, VX_MERKLE_OPEN_AIR_AUX_COLS = 16, 66, 4
VX_AIR_LEAF_SPONGE, VX_LEAF_SPONGE_AIR_COLS, VX_LEAF_SPONGE_AIR_AUX_COLS = 17, 66, 12
VX_AIR_FRI_FOLD, VX_FRI_FOLD_AIR_COLS, VX_FRI_FOLD_AIR_AUX_COLS = 18, 120, 36
VX_AIR_MERKLE_OPEN_SET, VX_MERKLE_OPEN_SET_AIR_COLS, VX_MERKLE_OPEN_SET_AIR_AUX_COLS = 19, 72, 6
VX_AIR_LEAF_SPONGE_SET, VX_LEAF_SPONGE_SET_AIR_COLS, VX_LEAF_SPONGE_SET_AIR_AUX_COLS = 20, 67, 12
VX_AIR_FRI_COMBINE, VX_FRI_COMBINE_AIR_COLS, VX_FRI_COMBINE_AIR_AUX_COLS = 21, 28, 4
VX_AIR_LEAF_NOOP, VX_LEAF_NOOP_AIR_COLS, VX_LEAF_NOOP_AIR_AUX_COLS = 22, 11, 8
VX_AIR_TRANSCRIPT, VX_TRANSCRIPT_AIR_COLS, VX_TRANSCRIPT_AIR_AUX_COLS, VX_TRANSCRIPT_MAX_CHAINS = 23, 93, 18, 64
FRI_EXIT_AIR_COLS, FRI_EXIT_AIR_AUX_COLS, FRI_EXIT_PUBLIC, FRI_EXIT_BLOCK, FRI_EXIT_MAX_FINAL_LEN = 21, 6, 12, 128, 64  # csrc/fri_exit_layout.h: a shipped program, no compiled AIR
TAG_ROW, TAG_FRI, TAG_OBS, TAG_CHAL, TAG_FIN = 9, 10, 12, 13, 14  # csrc/air_bus.cuh: the tags an exit group's outside party uses


class JustificationStruct(C.Structure):
    _fields_ = [("authority_set_id", C.c_uint64), ("authority_set_hash", C.c_void_p), ("precommit", C.c_void_p), ("pubkeys", C.c_void_p),
                ("signatures", C.c_void_p), ("validator_signed", C.c_void_p), ("num_authorities", C.c_uint32), ("max_authorities", C.c_uint32)]


class PackedJustification:
    """Host buffers of a synth.Justification in the layout vx_justification expects (kept alive here)."""

    def __init__(self, just, max_authorities=None):
        n = len(just.pubkeys)
        mx = n if max_authorities is None else max_authorities
        self.pk = np.zeros(32 * mx, dtype=np.uint8)
        self.sg = np.zeros(64 * mx, dtype=np.uint8)
        self.en = np.zeros(mx, dtype=np.uint8)
        self.pk[: 32 * n] = np.frombuffer(b"".join(just.pubkeys), dtype=np.uint8)
        self.sg[: 64 * n] = np.frombuffer(b"".join(just.signatures), dtype=np.uint8)
        self.en[:n] = np.array(just.signed, dtype=np.uint8)
        self.sh = np.frombuffer(bytes(just.authority_set_hash), dtype=np.uint8).copy()
        self.pc = np.frombuffer(bytes(just.precommit), dtype=np.uint8).copy()
        self.struct = JustificationStruct(just.set_id, self.sh.ctypes.data, self.pc.ctypes.data, self.pk.ctypes.data, self.sg.ctypes.data,
                                          self.en.ctypes.data, just.num_authorities, mx)


class StarkConfig(C.Structure):
    _fields_ = [("rate_bits", C.c_int32), ("cap_height", C.c_int32), ("num_queries", C.c_int32), ("pow_bits", C.c_int32),
                ("arity_bits", C.c_int32), ("final_poly_bits", C.c_int32)]


class AirProgramStruct(C.Structure):  # include/vx.h vx_air_program
    _fields_ = [("cols", C.c_uint32), ("n_public", C.c_uint32), ("n_periodic", C.c_uint32), ("n_regs", C.c_uint32),
                ("periodic_log", C.c_void_p), ("periodic_values", C.c_void_p), ("consts", C.c_void_p), ("n_consts", C.c_uint32),
                ("code", C.c_void_p), ("n_code", C.c_uint32), ("aux_cols", C.c_uint32), ("n_challenges", C.c_uint32), ("n_aux_public", C.c_uint32),
                ("gen_aux", C.c_void_p), ("gen_aux_user", C.c_void_p)]


class AirBusStruct(C.Structure):  # include/vx.h vx_air_bus
    _fields_ = [("code", C.c_void_p), ("n_code", C.c_uint32), ("consts", C.c_void_p), ("n_consts", C.c_uint32), ("n_regs", C.c_uint32),
                ("block_log", C.c_uint32), ("step_periodic", C.c_int32)]


class BusTableStruct(C.Structure):  # include/vx.h vx_bus_table
    _fields_ = [("air_id", C.c_int32), ("log_n", C.c_int32), ("trace", C.c_void_p), ("public_inputs", C.c_void_p), ("n_public", C.c_size_t)]


class BusExpectStruct(C.Structure):  # include/vx.h vx_bus_expect
    _fields_ = [("air_id", C.c_int32), ("public_inputs", C.c_void_p), ("n_public", C.c_size_t)]


class BusUnmatchedStruct(C.Structure):  # include/vx.h vx_bus_unmatched
    _fields_ = [("n_unmatched", C.c_uint64), ("table", C.c_int32), ("message", C.c_uint32), ("row", C.c_uint64), ("net", C.c_uint64)]


VX_BUS_GROUP_MAX_TABLES, VX_BUS_MSG_WORDS = 16, 6
BusUnmatched = collections.namedtuple("BusUnmatched", "n_unmatched table message row net")  # what Context.bus_group_check reports
VX_BUSP_SLOT, VX_BUSP_MSG = 64, 65
VX_BUSP_LOWER_REGS, VX_BUSP_MAX_REGS, VX_BUSP_MAX_HELPERS, VX_BUSP_MAX_CODE = 20, 12, 19, 1 << 14

# include/vx.h vx_air_gen_aux_fn: (user, ctx, trace vx_buf*, log_n, challenges, public inputs, aux_out vx_buf*, aux_public_out) -> int32
AIR_GEN_AUX_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))
_air_callbacks = []  # registered programs live for the life of the process: so do their callbacks


class VxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


def build(force=False):
    """Compile libvxprove.so for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VxError(-2, f"{LIB_PATH} is missing: run __graft_entry__.build(); there is no CPU fallback")
    # A proof runs its tables on five or six streams and several proofs are in flight: the HIP runtime's default of 4 hardware
    # queues per process serialises them (measured: 7.26 -> 7.86 proofs/s with 16).  Read when the runtime initialises, so it
    # must be in the environment before the first HIP call of the process; the library's own constructor sets it too.
    if not os.environ.get("VX_NO_PY_ENV"):  # (tools/ab_hw_queues_ctor.sh measures the constructor alone)
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int32, C.c_uint64
    sig = {
        "vx_ctx_create": [C.c_int, C.POINTER(vp)], "vx_ctx_destroy": [vp], "vx_sync": [vp],
        "vx_timer_start": [vp], "vx_timer_stop": [vp, C.POINTER(C.c_float)],
        "vx_alloc": [vp, sz, C.POINTER(vp)], "vx_free": [vp, vp],
        "vx_upload": [vp, vp, sz, vp, sz], "vx_download": [vp, vp, sz, vp, sz], "vx_copy": [vp, vp, sz, vp, sz, sz],
        "vx_fill_random": [vp, vp, sz, sz, u64],
        "vx_field_batch_add": [vp, vp, vp, vp, sz], "vx_field_batch_sub": [vp, vp, vp, vp, sz],
        "vx_field_batch_mul": [vp, vp, vp, vp, sz], "vx_field_batch_inv": [vp, vp, vp, sz], "vx_ext_batch_mul": [vp, vp, vp, vp, sz],
        "vx_ntt": [vp, vp, sz, C.c_int, sz, sz, C.c_int, u64, C.c_int],
        "vx_lde": [vp, vp, C.c_int, sz, C.c_int, u64, C.c_int, vp, vp],
        "vx_lde_rows": [vp, vp, C.c_int, sz, vp, sz, vp],
        "vx_poseidon_permute_batch": [vp, vp, sz],
        "vx_merkle_build": [vp, vp, sz, sz, sz, C.c_int, C.c_int, C.POINTER(vp)], "vx_merkle_free": [vp, vp],
        "vx_merkle_cap": [vp, vp, vp], "vx_merkle_open": [vp, vp, vp, sz, vp], "vx_merkle_leaf_digests": [vp, vp, vp],
        "vx_fri_fold": [vp, vp, C.c_int, C.c_int, vp, u64, vp], "vx_fri_layer_tree": [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)],
        "vx_fri_leaves": [vp, vp, C.c_int, C.c_int, vp, sz, vp], "vx_fri_pow": [vp, vp, C.c_int, C.c_int, C.POINTER(u64)],
        "vx_stark_default_config": [C.POINTER(StarkConfig)],
        "vx_stark_proof_bound": [C.c_int, C.POINTER(StarkConfig), C.c_int, C.POINTER(sz)],
        "vx_header_range_proof_bound": [C.POINTER(StarkConfig), sz, sz, C.POINTER(sz)],
        "vx_header_range_prove": [vp, vp, sz, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.POINTER(JustificationStruct), C.POINTER(StarkConfig), vp, vp, sz, C.POINTER(sz)],
        "vx_header_range_proof_bound_ex": [C.POINTER(StarkConfig), sz, sz, C.c_uint32, C.POINTER(sz)],
        "vx_header_range_prove_ex": [vp, vp, sz, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.POINTER(JustificationStruct), C.POINTER(StarkConfig),
                                     C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, sz, C.POINTER(sz)],
        "vx_header_range_merge": [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_char_p, sz],
        "vx_stark_verify": [C.POINTER(StarkConfig), vp, sz, C.c_int, vp, sz, C.c_char_p, sz],
        "vx_header_range_verify": [C.POINTER(StarkConfig), vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_char_p, sz],
        "vx_stark_prove": [vp, C.c_int, C.POINTER(StarkConfig), vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_blake2b_256_batch": [vp, vp, sz, vp, sz, vp], "vx_sha256_pairs": [vp, vp, sz, vp],
        "vx_verify_subchain": [vp, vp, sz, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp],
        "vx_blake_chain_trace": [vp, vp, sz, vp, sz, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp],
        "vx_ed25519_verify_batch": [vp, vp, vp, vp, C.c_uint32, vp, sz, vp],
        "vx_sha_chain_trace": [vp, vp, sz, vp, C.c_uint32, C.c_int, vp, vp, vp],
        "vx_ed_trace": [vp, vp, vp, vp, C.c_uint32, vp, sz, C.c_int, C.c_uint32, vp, vp],
        "vx_sha512_trace": [vp, vp, vp, vp, C.c_uint32, vp, sz, C.c_int, C.c_uint32, vp, vp],
        "vx_epoch_end_trace": [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp],
        "vx_verify_simple_justification": [vp, C.c_uint32, vp, u64, vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32],
        "vx_verify_epoch_end_header": [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32],
        "vx_rotate_proof_bound": [C.POINTER(StarkConfig), sz, sz, sz, C.POINTER(sz)],
        "vx_rotate_prove": [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(JustificationStruct), C.POINTER(StarkConfig), vp, vp, sz, C.POINTER(sz)],
        "vx_rotate_verify": [C.POINTER(StarkConfig), vp, sz, u64, vp, vp, C.c_char_p, sz],
        "vx_gather_proofs": [vp, vp, C.c_int, vp, sz, vp],
        "vx_quotient_eval": [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, sz, vp],
        "vx_quotient_eval_aux": [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, sz, vp, sz, vp, sz, vp],
        "vx_partial_products": [vp, vp, vp, C.c_int, sz, vp, u64, u64, sz, vp],
        "vx_decode_header_batch": [vp, vp, sz, vp, sz, vp, vp, vp, vp, vp, vp],
        "vx_decode_precommit_batch": [vp, vp, sz, vp, vp, vp, vp, vp],
        "vx_stark_aux_trace": [vp, C.c_int, vp, C.c_int, vp, sz, vp, sz, vp, vp],
        "vx_air_register": [C.POINTER(AirProgramStruct), C.POINTER(C.c_int), C.c_char_p, sz],
        "vx_air_register_bus": [C.POINTER(AirProgramStruct), C.POINTER(AirBusStruct), C.POINTER(C.c_int), C.c_char_p, sz], "vx_air_unregister": [C.c_int],
        "vx_poseidon_air_trace": [vp, vp, sz, vp],
        "vx_merkle_open_air_trace": [vp, vp, vp, sz, C.c_int, vp, vp],
        "vx_merkle_openings_proof_bound": [C.POINTER(StarkConfig), sz, sz, C.POINTER(sz)],
        "vx_merkle_openings_prove": [vp, C.POINTER(StarkConfig), vp, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_merkle_openings_verify": [C.POINTER(StarkConfig), vp, sz, vp, C.c_int, C.c_int, vp, vp, sz, C.c_char_p, sz],
        "vx_leaf_sponge_air_trace": [vp, vp, sz, sz, sz, C.c_int, vp, sz, C.c_int, vp, vp],
        "vx_merkle_rows_proof_bound": [C.POINTER(StarkConfig), sz, sz, sz, C.POINTER(sz)],
        "vx_merkle_rows_prove": [vp, C.POINTER(StarkConfig), vp, vp, sz, sz, C.c_int, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_merkle_rows_verify": [C.POINTER(StarkConfig), vp, sz, vp, C.c_int, C.c_int, sz, vp, vp, sz, C.c_char_p, sz],
        "vx_fri_fold_air_trace": [vp, C.c_int, vp, sz, C.c_uint64, vp, vp, vp, sz, C.c_int, vp, vp],
        "vx_fri_fold_proof_bound": [C.POINTER(StarkConfig), C.c_int, sz, sz, C.POINTER(sz)],
        "vx_fri_exit_air_trace": [vp, C.c_int, sz, C.c_int, C.c_uint64, C.c_uint64, vp, sz, vp, sz, C.c_int, vp, vp],
        "vx_fri_exit_public": [C.c_int, sz, C.c_int, C.c_uint64, C.c_uint64, vp, sz, vp], "vx_fri_exit_log_n": [sz], "vx_fri_exit_statement": [vp, sz, vp],
        "vx_fri_fold_prove": [vp, C.POINTER(StarkConfig), C.c_int, vp, sz, vp, sz, vp, vp, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_fri_fold_verify": [C.POINTER(StarkConfig), vp, sz, C.c_int, vp, sz, vp, sz, vp, vp, vp, sz, C.c_char_p, sz],
        "vx_merkle_open_set_air_trace": [vp, vp, sz, vp, vp, sz, C.c_int, vp, vp],
        "vx_leaf_sponge_set_air_trace": [vp, vp, vp, sz, vp, vp, sz, C.c_int, vp, vp],
        "vx_fri_queries_proof_bound": [C.POINTER(StarkConfig), C.c_int, sz, sz, C.POINTER(sz)],
        "vx_fri_queries_prove": [vp, C.POINTER(StarkConfig), C.c_int, vp, sz, vp, sz, vp, vp, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_fri_queries_verify": [C.POINTER(StarkConfig), vp, sz, C.c_int, vp, sz, vp, sz, vp, C.c_int, vp, vp, sz, C.c_char_p, sz],
        "vx_fri_combine_air_trace": [vp, C.c_int, C.c_int, sz, sz, sz, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp, sz, C.c_int, vp, vp],
        "vx_fri_combine_proof_bound": [C.POINTER(StarkConfig), C.c_int, sz, sz, sz, sz, C.POINTER(sz)],
        "vx_fri_combine_prove": [vp, C.POINTER(StarkConfig), C.c_int, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_fri_combine_verify": [C.POINTER(StarkConfig), vp, sz, C.c_int, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, C.c_char_p, sz],
        "vx_stark_combine_claims": [C.POINTER(StarkConfig), vp, sz, C.POINTER(C.c_int), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), vp, vp, vp, sz, vp, vp, sz, vp, sz,
                                    C.c_char_p, sz],
        "vx_fri_combine_fold_proof_bound": [C.POINTER(StarkConfig), C.c_int, sz, sz, sz, sz, sz, C.POINTER(sz)],
        "vx_fri_combine_fold_prove": [vp, C.POINTER(StarkConfig), C.c_int, sz, sz, sz, vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_fri_combine_fold_verify": [C.POINTER(StarkConfig), vp, sz, C.c_int, sz, sz, sz, vp, vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, C.c_char_p, sz],
        "vx_stark_fri_claims": [C.POINTER(StarkConfig), vp, sz, C.POINTER(C.c_int), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), vp, vp, sz, vp, vp, vp, sz, vp, sz, C.c_char_p, sz],
        "vx_stark_merkle_claims": [C.POINTER(StarkConfig), vp, sz, vp, vp, C.POINTER(sz), vp, vp, sz, C.POINTER(sz), vp, vp, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp, sz, C.c_char_p, sz],
        "vx_merkle_paths_air_trace": [vp, vp, C.c_int, vp, sz, vp, vp, vp, vp, sz, C.c_int, vp, vp],
        "vx_leaf_sponge_rows_air_trace": [vp, sz, vp, vp, vp, sz, C.c_int, vp, vp],
        "vx_stark_openings_proof_bound": [C.POINTER(StarkConfig), vp, sz, C.POINTER(sz)],
        "vx_stark_openings_prove": [vp, C.POINTER(StarkConfig), vp, sz, vp, vp, sz, C.POINTER(sz)],
        "vx_stark_openings_verify": [C.POINTER(StarkConfig), vp, sz, vp, sz, C.c_int, vp, sz, vp, C.c_char_p, sz],
        "vx_leaf_noop_air_trace": [vp, vp, vp, vp, vp, sz, C.c_int, vp, vp],
        "vx_stark_queries_proof_bound": [C.POINTER(StarkConfig), vp, sz, C.POINTER(sz)],
        "vx_stark_proof_head_words": [C.POINTER(StarkConfig), vp, sz, C.POINTER(sz)],
        "vx_stark_queries_prove": [vp, C.POINTER(StarkConfig), vp, sz, vp, vp, sz, C.POINTER(sz)],
        "vx_stark_queries_verify": [C.POINTER(StarkConfig), vp, sz, vp, sz, C.c_int, vp, sz, vp, C.c_char_p, sz],
        "vx_transcript_air_trace": [vp, sz, vp, vp, vp, sz, C.c_int, vp, vp, vp],
        "vx_stark_transcript_claims": [C.POINTER(StarkConfig), vp, sz, vp, C.POINTER(sz), vp, sz, C.POINTER(sz), vp, sz, C.c_char_p, sz],
        "vx_stark_transcripts_proof_bound": [C.POINTER(StarkConfig), vp, vp, sz, vp, C.POINTER(sz)],
        "vx_stark_transcripts_prove": [vp, C.POINTER(StarkConfig), vp, vp, sz, vp, vp, sz, C.POINTER(sz)],
        "vx_stark_transcripts_verify": [C.POINTER(StarkConfig), vp, sz, vp, vp, sz, vp, C.c_char_p, sz],
        "vx_stark_inner_proof_bound": [C.POINTER(StarkConfig), vp, sz, vp, C.POINTER(sz)],
        "vx_stark_inner_prove": [vp, C.POINTER(StarkConfig), vp, sz, vp, vp, sz, C.POINTER(sz)],
        "vx_stark_inner_verify": [C.POINTER(StarkConfig), vp, sz, vp, sz, C.c_int, vp, sz, vp, C.c_char_p, sz],
        "vx_bus_group_proof_bound": [C.POINTER(StarkConfig), C.POINTER(BusTableStruct), sz, C.POINTER(sz)],
        "vx_bus_group_prove": [vp, C.POINTER(StarkConfig), C.POINTER(BusTableStruct), sz, vp, sz, vp, sz, C.POINTER(sz)],
        "vx_bus_group_verify": [C.POINTER(StarkConfig), vp, sz, C.POINTER(BusExpectStruct), sz, vp, sz, C.c_char_p, sz],
        "vx_bus_group_check": [vp, C.POINTER(BusTableStruct), sz, vp, sz, C.POINTER(BusUnmatchedStruct)],
        "vx_merkle_check": [vp, vp, C.c_int, vp, sz, vp, vp, vp, vp, sz, vp, sz, sz, C.POINTER(sz)],
        "vx_stark_verify_dev": [vp, C.POINTER(StarkConfig), vp, sz, C.c_int, vp, sz, C.c_char_p, sz],
        "vx_header_range_verify_dev": [vp, C.POINTER(StarkConfig), vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_char_p, sz],
        "vx_rotate_verify_dev": [vp, C.POINTER(StarkConfig), vp, sz, u64, vp, vp, C.c_char_p, sz],
        "vx_stark_verify_deferred": [C.POINTER(StarkConfig), vp, sz, C.c_int, vp, sz, C.c_char_p, sz],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes, f.restype = args, i32
    L.vx_last_error.argtypes, L.vx_last_error.restype = [vp], C.c_char_p
    L.vx_backend_name.argtypes, L.vx_backend_name.restype = [], C.c_char_p
    L.vx_buf_devptr.argtypes, L.vx_buf_devptr.restype = [vp], vp
    L.vx_buf_len.argtypes, L.vx_buf_len.restype = [vp], sz
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def default_stark_config(**over):
    cfg = StarkConfig()
    load_library().vx_stark_default_config(C.byref(cfg))
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _words(x):
    """contiguous uint64 words, or None for an argument that is left out"""
    return None if x is None else np.ascontiguousarray(x, dtype=np.uint64)


def _host_verify(name, cfg, *args, ctx=None):
    """One call of a host `vx_*_verify`: the configuration (None: the default), then `args` -- an array goes as its pointer, None as
    NULL --, then a 256-byte buffer for the reason.  Raises VxError(rc, reason) unless it returns VX_OK.
    ctx: the handle a `_dev` form takes in front (its Merkle openings are checked on that context's device)."""
    cfg = cfg or default_stark_config()
    err = C.create_string_buffer(256)
    rc = getattr(load_library(), name)(*([] if ctx is None else [ctx]), C.byref(cfg), *[_ptr(a) if isinstance(a, np.ndarray) else a for a in args], err, 256)
    if rc != 0:
        raise VxError(rc, err.value.decode())


def stark_verify(proof, cfg=None, expect_air=0, expect_public=None, _symbol="vx_stark_verify", _ctx=None):
    """Host-side verification (no GPU needed).  Raises VxError(VX_ERR_STATEMENT) with the reason."""
    pr, pub = _words(proof), _words(expect_public)
    _host_verify(_symbol, cfg, pr, pr.size, expect_air, pub, 0 if pub is None else pub.size, ctx=_ctx)


def stark_verify_deferred(proof, cfg=None, expect_air=0, expect_public=None):
    """stark_verify with the Merkle openings recorded during the host pass and checked after it, in the order and with the answers of
    stark_verify: the code Context.stark_verify runs, with the host's path check in place of the kernel (no GPU needed)."""
    stark_verify(proof, cfg, expect_air, expect_public, _symbol="vx_stark_verify_deferred")


def air_register(cols, n_public, code, consts=(), periodic=(), n_regs=None, aux_cols=0, n_challenges=0, n_aux_public=0, gen_aux=None, _bus=None):
    """Register a constraint program (include/vx.h vx_air_register; no GPU needed) and return its AIR id.
    code: uint64 instruction words; consts: canonical field elements; periodic: a list of columns, each 2^k values;
    n_regs: registers used (default: the highest register the code names + 1).  air_program.AirBuilder writes these.
    Auxiliary round: aux_cols / n_challenges / n_aux_public and gen_aux(ctx_handle, trace_handle, log_n, challenges, public_inputs,
    aux_handle) -> list of 2 * n_aux_public published words -- the host's generator of the auxiliary columns (the handles are
    the C ABI's vx_ctx* / vx_buf*: Context.adopt / Buffer.adopt wrap them)."""
    L = load_library()
    code = np.ascontiguousarray(code, dtype=np.uint64)
    consts = np.ascontiguousarray(consts, dtype=np.uint64)
    plog = np.array([max(len(c), 1).bit_length() - 1 for c in periodic], dtype=np.uint8)
    for c, k in zip(periodic, plog):
        if len(c) != 1 << int(k):
            raise ValueError("a periodic column must have a power-of-two number of values")
    pvals = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint64) for c in periodic]) if len(periodic) else np.zeros(0, np.uint64))
    if n_regs is None:
        n_regs = 1 + max([int((w >> 8) & 0xFF) for w in code.tolist()] + [0])
    cb = None
    if gen_aux is not None:
        def trampoline(_user, ctx_h, trace_h, log_n, chal_p, pub_p, aux_h, apub_p):
            try:
                chal = [int(chal_p[i]) for i in range(n_challenges)]
                pub = [int(pub_p[i]) for i in range(n_public)]
                out = gen_aux(ctx_h, trace_h, log_n, chal, pub, aux_h) or []
                if len(out) != 2 * n_aux_public:
                    return -1
                for i, v in enumerate(out):
                    apub_p[i] = int(v)
                return 0
            except Exception:  # noqa: BLE001 -- an exception must not cross the C boundary
                import traceback

                traceback.print_exc()
                return -5
        cb = AIR_GEN_AUX_FN(trampoline)
        _air_callbacks.append(cb)
    st = AirProgramStruct(cols, n_public, len(periodic), n_regs, _ptr(plog) if len(periodic) else None, _ptr(pvals) if len(periodic) else None,
                          _ptr(consts) if consts.size else None, consts.size, _ptr(code) if code.size else None, code.size,
                          aux_cols, n_challenges, n_aux_public, C.cast(cb, C.c_void_p) if cb is not None else None, None)
    air_id, err = C.c_int(0), C.create_string_buffer(256)
    if _bus is None:
        rc = L.vx_air_register(C.byref(st), C.byref(air_id), err, 256)
    else:
        bcode, bconsts = np.ascontiguousarray(_bus["code"], dtype=np.uint64), np.ascontiguousarray(_bus["consts"], dtype=np.uint64)
        bregs = _bus["n_regs"]
        if bregs is None:
            bregs = 1 + max([int((w >> 8) & 0xFF) for w in bcode.tolist() if int(w & 0xFF) < VX_BUSP_SLOT] + [int((w >> 16) & 0xFFFF) for w in bcode.tolist() if int(w & 0xFF) >= VX_BUSP_SLOT] + [0])
        bs = AirBusStruct(_ptr(bcode) if bcode.size else None, bcode.size, _ptr(bconsts) if bconsts.size else None, bconsts.size, bregs, _bus["block_log"], _bus["step_periodic"])
        rc = L.vx_air_register_bus(C.byref(st), C.byref(bs), C.byref(air_id), err, 256)
    if rc != 0:
        raise VxError(rc, err.value.decode())
    return air_id.value


def air_register_bus(cols, n_public, code, bus_code, consts=(), bus_consts=(), periodic=(), n_regs=None, bus_n_regs=None, block_log=0, step_periodic=-1, aux_cols=None,
                     n_challenges=4, n_aux_public=1, gen_aux=None):
    """Register a constraint program that DECLARES its bus messages (include/vx.h vx_air_register_bus; no GPU needed) and return its AIR
    id.  bus_code / bus_consts: the message program (VX_BUSP_SLOT / VX_BUSP_MSG close its messages; air_program.AirBuilder.assemble_bus
    writes it).  The library appends the helper and running-sum constraints to `code` and fills the auxiliary round on the GPU: there is
    no callback (gen_aux is here only so that a caller sees the library refuse it).  aux_cols defaults to what the message count implies."""
    if aux_cols is None:
        n_msgs = sum(1 for w in np.asarray(bus_code, dtype=np.uint64).tolist() if int(w & 0xFF) == VX_BUSP_MSG)
        aux_cols = 2 * ((n_msgs + 1) // 2) + 2
    bus = dict(code=bus_code, consts=bus_consts, n_regs=bus_n_regs, block_log=block_log, step_periodic=step_periodic)
    return air_register(cols, n_public, code, consts, periodic, n_regs, aux_cols, n_challenges, n_aux_public, gen_aux, _bus=bus)


def air_unregister(air_id):
    rc = load_library().vx_air_unregister(air_id)
    if rc != 0:
        raise VxError(rc, "unknown AIR program id %d" % air_id)


HR_FIXED = 22  # fixed words of a header_range blob's header; the lengths of its S hash-chain segments follow
HR_HDR = HR_FIXED + 1  # words before the first proof of an UNSEGMENTED blob (S = 1)
HR_MAGIC = 0x3645474E41525248  # "HRRANGE6"


def blob_segments(blob):
    return int(blob[16])


def split_blob_segments(blob):
    """([hash-chain segment proofs], authority-commitment, Merkle, Ed25519, SHA-512) of a header_range blob (include/vx.h: the last
    two and the commitment are empty when it was proven without a justification; a shard's blob holds its own tables only)."""
    S = blob_segments(blob)
    off = HR_FIXED + S
    segs = []
    for s in range(S):
        ln = int(blob[HR_FIXED + s])
        segs.append(blob[off: off + ln])
        off += ln
    rest = []
    for t in range(4):
        ln = int(blob[17 + t])
        rest.append(blob[off: off + ln])
        off += ln
    return (segs,) + tuple(rest)


def split_blob(blob):
    """(hash-chain, authority-commitment, Merkle, Ed25519, SHA-512) proofs of an unsegmented header_range blob."""
    parts = split_blob_segments(blob)
    assert len(parts[0]) == 1, "a segmented blob: use split_blob_segments"
    return (parts[0][0],) + parts[1:]


class HrExchange(C.Structure):
    _fields_ = [("fn", C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t)), ("user", C.c_void_p)]


def merge_blobs(blobs):
    """The request's blob from the blobs of the shards of one proof (vx_header_range_merge; host only)."""
    L = load_library()
    arrs = [np.ascontiguousarray(b, dtype=np.uint64) for b in blobs]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    lens = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
    out = np.empty(sum(a.size for a in arrs), dtype=np.uint64)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    rc = L.vx_header_range_merge(ptrs, lens, len(arrs), _ptr(out), out.size, C.byref(n), err, 256)
    if rc != 0:
        raise VxError(rc, err.value.decode())
    return out[: n.value]


def header_range_verify(blob, max_headers, trusted_block, trusted_hash, target_block, out96, cfg=None, authority_set_hash=None, authority_set_id=0, _ctx=None):
    b = _words(blob)
    th = np.frombuffer(bytes(trusted_hash), dtype=np.uint8).copy()
    o = np.frombuffer(bytes(out96), dtype=np.uint8).copy()
    ah = None if authority_set_hash is None else np.frombuffer(bytes(authority_set_hash), dtype=np.uint8).copy()
    _host_verify("vx_header_range_verify" if _ctx is None else "vx_header_range_verify_dev", cfg, b, b.size, max_headers, trusted_block, th, authority_set_id, ah, target_block, o, ctx=_ctx)


def rotate_verify(blob, authority_set_id, authority_set_hash, out32, cfg=None, _ctx=None):
    b = _words(blob)
    ah = np.frombuffer(bytes(authority_set_hash), dtype=np.uint8).copy()
    o = np.frombuffer(bytes(out32), dtype=np.uint8).copy()
    _host_verify("vx_rotate_verify" if _ctx is None else "vx_rotate_verify_dev", cfg, b, b.size, authority_set_id, ah, o, ctx=_ctx)


MOPEN_MAGIC, MOPEN_HDR = 0x314E45504F4D5856, 4  # "VXMOPEN1": magic, log2(n_leaves), number of openings, proof length; then the MerkleOpenAir proof


def _cap(cap):
    """a tree's cap as a contiguous [2^cap_height][4] array -> (cap, cap_height)"""
    cp = np.ascontiguousarray(cap, dtype=np.uint64).reshape(-1, 4)
    cap_height = cp.shape[0].bit_length() - 1
    if cp.shape[0] != 1 << cap_height:
        raise ValueError("a cap has a power-of-two number of digests")
    return cp, cap_height


def merkle_openings_verify(blob, cap, log_leaves, leaf_idx, leaf_digests, cfg=None):
    """Host-side check of a vx_merkle_openings_prove blob against the verifier's own claims: the tree's cap [2^cap_height][4],
    log2(n_leaves), and the openings (leaf_idx[i], leaf_digests[i][4]) in order.  Walks no Merkle path; raises VxError with the reason."""
    b = _words(blob)
    cp, cap_height = _cap(cap)
    idx = _words(leaf_idx).reshape(-1)
    dig = _words(leaf_digests).reshape(-1)
    if dig.size != 4 * idx.size:
        raise ValueError("one 4-word digest per opening")
    _host_verify("vx_merkle_openings_verify", cfg, b, b.size, cp, cap_height, log_leaves, idx, dig, idx.size)


MROWS_MAGIC, MROWS_HDR = 0x3153574F524D5856, 6  # "VXMROWS1": magic, log2(n_leaves), leaf_len, openings, two proof lengths; then the MerkleOpenAir and the LeafSpongeAir proof


def merkle_rows_verify(blob, cap, log_leaves, leaf_idx, rows, cfg=None):
    """Host-side check of a vx_merkle_rows_prove blob against the verifier's own claims: the tree's cap [2^cap_height][4],
    log2(n_leaves), and the opened rows (leaf_idx[i], rows[i][leaf_len]) in order.  Walks no Merkle path and hashes no leaf; raises
    VxError with the reason."""
    b = _words(blob)
    cp, cap_height = _cap(cap)
    idx = _words(leaf_idx).reshape(-1)
    rw = _words(rows)
    if rw.ndim != 2 or rw.shape[0] != idx.size:
        raise ValueError("one row [leaf_len] per opening")
    _host_verify("vx_merkle_rows_verify", cfg, b, b.size, cp, cap_height, log_leaves, rw.shape[1], idx, rw, idx.size)


FFOLD_MAGIC, FFOLD_HDR = 0x31444C4F46465856, 5  # "VXFFOLD1": magic, log2 of the inner LDE, fold layers, queries, proof length; then the FriFoldAir proof


def _fri_claims(betas, final_poly, index, ev0, leaves):
    """the claims of FriFoldAir as contiguous arrays: betas [NL][2], final_poly [len][2], index [n], ev0 [n][2], leaves [n][NL][32]"""
    be = np.ascontiguousarray(betas, dtype=np.uint64).reshape(-1, 2)
    fp = np.ascontiguousarray(final_poly, dtype=np.uint64).reshape(-1, 2)
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1)
    ev = np.ascontiguousarray(ev0, dtype=np.uint64).reshape(-1)
    lv = np.ascontiguousarray(leaves, dtype=np.uint64).reshape(-1)
    if ev.size != 2 * idx.size or lv.size != idx.size * be.shape[0] * 32:
        raise ValueError("one ev_0 [2] and one leaf [32] per layer for every query")
    return be, fp, idx, ev, lv


def fri_fold_verify(blob, log_lde, betas, final_poly, index, ev0, leaves, cfg=None):
    """Host-side check of a vx_fri_fold_prove blob against the verifier's own claims: the inner proof's LDE size, betas [NL][2] and
    final polynomial [len][2], and per query (index, ev0 [2], leaves [NL][32]) in order.  Folds nothing; raises VxError with the reason."""
    b = _words(blob)
    be, fp, idx, ev, lv = _fri_claims(betas, final_poly, index, ev0, leaves)
    _host_verify("vx_fri_fold_verify", cfg, b, b.size, log_lde, be, be.shape[0], fp, fp.shape[0], idx, ev, lv, idx.size)


def fri_exit_log_n(n_queries):
    """The smallest log_n whose rows hold FriExitAir's 1 + n_queries blocks of 128; the caller raises it to a size with a FRI plan."""
    return int(load_library().vx_fri_exit_log_n(int(n_queries)))


def fri_exit_public(log_lde, n_layers, pow_bits, ord_pow, absorbed, final_poly):
    """FriExitAir's 12 public inputs from what a verifier knows (host only): ord_pow, absorbed, pow_bits, 64 - log_lde, FB, w_FB,
    7^(16^NL), final_len, and the digest of these with the final polynomial's words.  VxError (VX_ERR_ARG) says which limit a shape
    misses."""
    fp = np.ascontiguousarray(final_poly, dtype=np.uint64).reshape(-1, 2)
    pub = np.zeros(FRI_EXIT_PUBLIC, dtype=np.uint64)
    rc = load_library().vx_fri_exit_public(int(log_lde), int(n_layers), int(pow_bits), int(ord_pow), int(absorbed), _ptr(fp) if fp.size else None, fp.shape[0], _ptr(pub))
    if rc != 0:  # the entry point has no buffer for a reason: the binding names the limit that was missed
        n, fb = fp.shape[0], log_lde - 4 * n_layers
        why = ("%d fold layers (1..8)" % n_layers if not 1 <= n_layers <= 8 else "log_lde %d (5..32)" % log_lde if not 5 <= log_lde <= 32 else
               "%d index bits behind the fold layers (FB, at least 1)" % fb if fb < 1 else "pow_bits %d (0..64)" % pow_bits if not 0 <= pow_bits <= 64 else
               "a final polynomial of %d coefficients (1..%d): more do not fit the Horner rows of a block" % (n, FRI_EXIT_MAX_FINAL_LEN) if not 1 <= n <= FRI_EXIT_MAX_FINAL_LEN else
               "ord_pow or absorbed is 2^32 or more" if max(int(ord_pow), int(absorbed)) >> 32 else "a non-canonical final-polynomial word")
        raise VxError(rc, "fri exit: " + why)
    return pub


_fri_exit_air = None


def fri_exit_air_id():
    """The AIR id of the shipped FriExitAir program (air_library.fri_exit_builder()) in this process: registered on first use, prover
    and verifier alike (a proof does not carry its program)."""
    global _fri_exit_air
    if _fri_exit_air is None:
        from . import air_library

        _fri_exit_air = air_library.fri_exit_builder().register()
    return _fri_exit_air


def _table_log_n(log_n, cfg=None):
    """The rows (log2) a table of at least 2^log_n rows is proven at: the next size whose FRI plan under cfg leaves a final polynomial."""
    cfg = cfg or default_stark_config()
    while True:
        d = log_n
        while d > cfg.final_poly_bits and d + cfg.rate_bits - cfg.arity_bits >= cfg.cap_height:
            d -= cfg.arity_bits
        if d >= 0:
            return log_n
        log_n += 1


def _transcript_ops(n_obs, chal):
    """A chain's run lengths [observe count, challenge count, ...] (what transcript_air_trace takes) from its claims: the challenges
    [n][2] as (words absorbed when it was drawn, value).  -> (ops, the number of duplexes: a counter machine, nothing is hashed)"""
    ops, at = [], 0
    for a, _ in np.asarray(chal, dtype=np.uint64).reshape(-1, 2).tolist():
        if not ops or a != at:
            ops += [a - at, 0]
            at = a
        ops[-1] += 1
    if at != n_obs:
        raise ValueError("the chain ends on observed words that no challenge follows")
    n_in, n_out, blocks = 0, 0, 0
    for j, count in enumerate(ops):
        for _ in range(count):
            if j % 2 == 0:
                n_out, n_in = 0, n_in + 1
                if n_in == 8:
                    blocks, n_in, n_out = blocks + 1, 0, 8
            else:
                if n_in > 0 or n_out == 0:
                    blocks, n_in, n_out = blocks + 1, 0, 8
                n_out -= 1
    return ops, blocks


def fri_exit_statement_words(log_lde, pow_bits, ord_pow, obs, chal, index, ev0, leaves):
    """The words of an exit group's ONE statement digest, everything its outside party states, fixed before the shared lookup
    challenges are drawn: log_lde, pow_bits, ord_pow, n_obs, n_queries, the fold layers; the observed words (the final polynomial
    and the nonce among them); (absorbed, value) of every challenge BELOW ord_pow (the betas among them); per query (index, ev_0,
    leaves).  The challenges from ord_pow on are NOT in it: FriExitAir's trace cap commits them."""
    idx, lv = np.asarray(index, dtype=np.uint64).reshape(-1), np.asarray(leaves, dtype=np.uint64)
    lv = lv.reshape(idx.size, -1)
    claims = np.concatenate([idx.reshape(-1, 1), np.asarray(ev0, dtype=np.uint64).reshape(-1, 2), lv], axis=1)
    head = [int(log_lde), int(pow_bits), int(ord_pow), len(obs), idx.size, lv.shape[1] // 32]
    return np.concatenate([np.array(head, dtype=np.uint64), np.asarray(obs, dtype=np.uint64).reshape(-1), np.asarray(chal, dtype=np.uint64).reshape(-1, 2)[:ord_pow].reshape(-1),
                           claims.reshape(-1)])


def fri_exit_statement(words):
    """hash_n_to_hash_no_pad of an exit group's statement words (host only) -> the four digest words"""
    w, d = _words(words), np.zeros(4, dtype=np.uint64)
    rc = load_library().vx_fri_exit_statement(_ptr(w), w.size, _ptr(d))
    if rc != 0:
        raise VxError(rc, "fri exit: the statement has no words, or a non-canonical one")
    return d


def fri_exits_outside(log_lde, ord_pow, obs, chal, final_poly, index, ev0, leaves):
    """The messages of an exit group's outside party, the verifier: per query the 32 words of every layer's leaf and the entry (index,
    ev_0) of the fold chain SENT; every observed word SENT; the challenges below ord_pow RECEIVED; every coefficient of the final
    polynomial SENT n_queries times.  -> [n][6] words (t0, t1, t2, t3, tag, m)"""
    idx = [int(i) for i in np.asarray(index, dtype=np.uint64).reshape(-1)]
    lv = np.asarray(leaves, dtype=np.uint64).reshape(len(idx), -1, 32)
    ev = np.asarray(ev0, dtype=np.uint64).reshape(-1, 2)
    out = []
    for q, i in enumerate(idx):
        for l in range(lv.shape[1]):
            out += [[i >> (4 * (l + 1)), j, int(lv[q, l, j]), l, TAG_ROW, 1] for j in range(32)]
        out.append([i, int(ev[q, 0]), int(ev[q, 1]), 0, TAG_FRI, 1])
    out += [[0, j, int(w), 0, TAG_OBS, 1] for j, w in enumerate(np.asarray(obs, dtype=np.uint64).reshape(-1))]
    out += [[0, j, int(a), int(v), TAG_CHAL, P - 1] for j, (a, v) in enumerate(np.asarray(chal, dtype=np.uint64).reshape(-1, 2)[:ord_pow].tolist())]
    out += [[k, int(c[0]), int(c[1]), 0, TAG_FIN, len(idx)] for k, c in enumerate(np.asarray(final_poly, dtype=np.uint64).reshape(-1, 2))]
    return np.array(out, dtype=np.uint64)


def _fri_exits_statement(proof, cfg, ext_chal):
    """what prover and verifier of an exit group both derive from the inner proof with the exported claim functions"""
    cfg = cfg or default_stark_config()
    fc = stark_fri_claims(proof, cfg)
    obs, chal = stark_transcript_claims(proof, cfg, ext_chal)
    n_q, NL = fc["index"].size, fc["betas"].shape[0]
    ord_pow = chal.shape[0] - 1 - n_q
    if cfg.arity_bits != 4 or ord_pow < 0:
        raise VxError(-1, "fri exits: the exit group is stated for arity_bits 4 and a transcript that ends on the proof-of-work response and one challenge per query")
    stmt = fri_exit_statement(fri_exit_statement_words(fc["log_lde"], cfg.pow_bits, ord_pow, obs, chal, fc["index"], fc["ev0"], fc["leaves"]))
    ops, blocks = _transcript_ops(obs.size, chal)
    logs = (_table_log_n(max(5, (n_q * (fc["log_lde"] - 3 * NL) - 1).bit_length()), cfg), _table_log_n(max(5, (32 * blocks - 1).bit_length()), cfg), _table_log_n(fri_exit_log_n(n_q), cfg))
    return cfg, fc, obs, chal, ord_pow, stmt, ops, logs


def fri_exits_verify(blob, proof, cfg=None, ext_chal=None):
    """Host-side check of a Context.fri_exits_prove blob against the inner proof it belongs to: three tables on one bus -- FriFoldAir,
    TranscriptAir, FriExitAir -- with the verifier outside (fri_exits_outside).  The verifier holds the fold claims of the proof
    (lib.stark_fri_claims, as vx_fri_fold_verify's caller does) and the challenges below the proof-of-work response; it computes no
    value mod N, no proof-of-work shift, no x^(16^NL) and no Horner evaluation of the final polynomial: the bus forces the claims'
    indices to be the transcript's.  This composition OBTAINS the claims with the exported replays (stark_fri_claims,
    stark_transcript_claims), which run the inner verifier; an aggregation verifier is handed them instead, and nothing here but
    bus_group_verify judges them.  ext_chal reaches the transcript claims; the fold claims come from a proof with drawn lookup
    challenges.  Raises VxError with the reason."""
    cfg, fc, obs, chal, ord_pow, stmt, _, _ = _fri_exits_statement(proof, cfg, ext_chal)
    NL = fc["betas"].shape[0]
    fold_pub = [NL, fc["log_lde"] - 3 * NL, pow(_root(fc["log_lde"]), P - 2, P), 0] + [int(v) for v in fc["betas"].reshape(-1)] + [0] * (16 - 2 * NL) + [int(v) for v in stmt]
    exit_pub = [int(v) for v in fri_exit_public(fc["log_lde"], NL, cfg.pow_bits, ord_pow, obs.size, fc["final_poly"])[:8]] + [int(v) for v in stmt]
    expect = [(VX_AIR_FRI_FOLD, fold_pub), (VX_AIR_TRANSCRIPT, [int(v) for v in stmt]), (fri_exit_air_id(), exit_pub)]
    bus_group_verify(blob, expect, cfg, fri_exits_outside(fc["log_lde"], ord_pow, obs, chal, fc["final_poly"], fc["index"], fc["ev0"], fc["leaves"]))


def _root(log_n):
    """the 2^log_n-th root of unity the library uses (Goldilocks: 7^((p - 1) / 2^32) squared down)"""
    return pow(pow(7, (P - 1) >> 32, P), 1 << (32 - log_n), P)


FQRY_MAGIC, FQRY_HDR = 0x3130595251465856, 7  # "VXFQRY01": magic, log2 of the inner LDE, fold layers, queries, three proof lengths; then the proofs


def fri_queries_verify(blob, log_lde, betas, final_poly, caps, index, ev0, cfg=None):
    """Host-side check of a vx_fri_queries_prove blob against what a succinct verifier holds: the inner proof's LDE size, betas
    [NL][2], the final polynomial [len][2], the layer caps [NL][2^cap_height][4] and per query (index, ev0 [2]) in order.  Holds no
    leaves, walks no path, folds nothing; raises VxError with the reason."""
    b = _words(blob)
    be = _words(betas).reshape(-1, 2)
    fp = _words(final_poly).reshape(-1, 2)
    cp = _words(caps).reshape(be.shape[0], -1, 4)
    idx = _words(index).reshape(-1)
    ev = _words(ev0).reshape(-1)
    cap_height = cp.shape[1].bit_length() - 1
    if ev.size != 2 * idx.size or cp.shape[1] != 1 << cap_height:
        raise ValueError("one ev_0 [2] for every query and one cap of 2^cap_height digests for every layer")
    _host_verify("vx_fri_queries_verify", cfg, b, b.size, log_lde, be, be.shape[0], fp, fp.shape[0], cp, cap_height, idx, ev, idx.size)


def stark_fri_claims(proof, cfg=None):
    """The FRI side of a vx_stark_prove proof (verified on the way) as FriFoldAir's claims -> dict(log_lde, betas [NL][2], final_poly
    [len][2], index [n], ev0 [n][2], ev_last [n][2] -- the ev_NL the verifier accepted --, leaves [n][NL][32], the slot `within` filled)."""
    L = load_library()
    cfg = cfg or default_stark_config()
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    nq = int(cfg.num_queries)
    n_lay = int(pr[9]) if pr.size > 9 and int(pr[9]) <= 16 else 0
    fin = int(pr[10 + n_lay]) if pr.size > 10 + n_lay and int(pr[10 + n_lay]) <= 1 << 27 else 0
    betas, fpoly = np.zeros(16, dtype=np.uint64), np.zeros(2 * max(fin, 1), dtype=np.uint64)
    index, ev0, ev_last = np.zeros(max(nq, 1), dtype=np.uint64), np.zeros(2 * max(nq, 1), dtype=np.uint64), np.zeros(2 * max(nq, 1), dtype=np.uint64)
    leaves = np.zeros(max(nq * n_lay * 32, 1), dtype=np.uint64)
    log_lde, nl, fl, n = C.c_int(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    err = C.create_string_buffer(256)
    rc = L.vx_stark_fri_claims(C.byref(cfg), _ptr(pr), pr.size, C.byref(log_lde), C.byref(nl), C.byref(fl), C.byref(n), _ptr(betas), _ptr(fpoly), fpoly.size, _ptr(index), _ptr(ev0),
                               _ptr(ev_last), index.size, _ptr(leaves), leaves.size, err, 256)
    if rc != 0:
        raise VxError(rc, err.value.decode())
    NL, Q = nl.value, n.value
    return dict(log_lde=log_lde.value, betas=betas[: 2 * NL].reshape(NL, 2), final_poly=fpoly[: 2 * fl.value].reshape(-1, 2), index=index[:Q], ev0=ev0[: 2 * Q].reshape(Q, 2),
                ev_last=ev_last[: 2 * Q].reshape(Q, 2), leaves=leaves[: Q * NL * 32].reshape(Q, NL, 32))


SOPEN_MAGIC, SOPEN_HDR, SOPEN_TREE0 = 0x314E45504F535856, 9, 8  # "VXSOPEN1": magic, the 7 shape words, the table count; then one length per table, the proofs


def stark_merkle_claims(proof, cfg=None, ext_chal=None):
    """The Merkle side of a vx_stark_prove proof as claims (every check of the proof except the paths runs on the way; no GPU needed)
    -> dict(shape (LN, cm, ca, a, NL, cap_height, n_queries), trees [n_trees] (the trees of a query in record order), caps
    [n_trees][2^cap_height][4], tree / index / leaf_len [n_claims], leaves / siblings: one array per claim)."""
    L = load_library()
    cfg = cfg or default_stark_config()
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    ch = None if ext_chal is None else np.ascontiguousarray(ext_chal, dtype=np.uint64)
    shape, trees = np.zeros(7, dtype=np.uint64), np.zeros(11, dtype=np.uint64)
    n_trees, n_claims, n_leaves, n_sibs = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    caps, tree, index, leaf_len = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    leaves, sibs = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    err = C.create_string_buffer(256)
    for _ in range(2):  # the first call sizes the arrays (VX_ERR_BUFSZ with every size set)
        rc = L.vx_stark_merkle_claims(C.byref(cfg), _ptr(pr), pr.size, None if ch is None else _ptr(ch), _ptr(shape), C.byref(n_trees), _ptr(trees), _ptr(caps), caps.size, C.byref(n_claims),
                                      _ptr(tree), _ptr(index), _ptr(leaf_len), tree.size, C.byref(n_leaves), _ptr(leaves), leaves.size, C.byref(n_sibs), _ptr(sibs), sibs.size, err, 256)
        if rc != -4:
            break
        caps = np.zeros(n_trees.value * (4 << int(shape[5])), dtype=np.uint64)
        tree, index, leaf_len = (np.zeros(n_claims.value, dtype=np.uint64) for _ in range(3))
        leaves, sibs = np.zeros(max(n_leaves.value, 1), dtype=np.uint64), np.zeros(max(n_sibs.value, 1), dtype=np.uint64)
    if rc != 0:
        raise VxError(rc, err.value.decode())
    LN, a, cap_h = int(shape[0]), int(shape[3]), int(shape[5])
    depth = [LN - cap_h if t >= SOPEN_TREE0 else LN - a * (int(t) + 1) - cap_h for t in tree]
    lcut, scut = np.cumsum([0] + [int(v) for v in leaf_len]), np.cumsum([0] + [4 * d for d in depth])
    return dict(shape=[int(v) for v in shape], trees=[int(v) for v in trees[: n_trees.value]], caps=caps.reshape(n_trees.value, -1, 4), tree=tree, index=index, leaf_len=leaf_len,
                leaves=[leaves[lcut[i]: lcut[i + 1]] for i in range(tree.size)], siblings=[sibs[scut[i]: scut[i + 1]].reshape(-1, 4) for i in range(tree.size)])


def _stark_group_verify(symbol, blob, proof, cfg, expect_air, expect_public, ext_chal):
    """the three levels of a proof's bus group (stark_openings / _queries / _inner) share one verifier signature"""
    b, pr, pub = _words(blob), _words(proof), _words(expect_public)
    _host_verify(symbol, cfg, b, b.size, pr, pr.size, expect_air, pub, 0 if pub is None else pub.size, _words(ext_chal))


def stark_openings_verify(blob, proof, cfg=None, expect_air=0, expect_public=None, ext_chal=None):
    """Host-side check of a vx_stark_openings_prove blob together with the inner proof it belongs to: the proof is verified in
    the delegated mode (every check except the Merkle paths) and the group proves the paths.  Walks no path, hashes no leaf,
    reads no sibling; raises VxError with the reason."""
    _stark_group_verify("vx_stark_openings_verify", blob, proof, cfg, expect_air, expect_public, ext_chal)


def stark_proof_head(proof, cfg=None):
    """The head of a vx_stark_prove proof: everything before its first query record, all lib.stark_queries_verify reads."""
    L = load_library()
    cfg = cfg or default_stark_config()
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    n = C.c_size_t(0)
    rc = L.vx_stark_proof_head_words(C.byref(cfg), _ptr(pr), pr.size, C.byref(n))
    if rc != 0:
        raise VxError(rc, "stark proof head: not a proof of a known AIR under this configuration")
    return pr[: n.value].copy()


def stark_queries_verify(blob, proof, cfg=None, expect_air=0, expect_public=None, ext_chal=None):
    """Host-side check of a vx_stark_queries_prove blob together with the inner proof it belongs to -- the whole proof or its HEAD
    alone (everything before the first query record; lib.stark_proof_head cuts it): the proof's transcript, proof of work and
    constraint identity at zeta are checked in the query-free mode, which reads no query record, and the group proves the query phase.
    Raises VxError with the reason."""
    _stark_group_verify("vx_stark_queries_verify", blob, proof, cfg, expect_air, expect_public, ext_chal)


class _ProofList:
    """n proofs (and their optional external lookup challenges) as the pointer arrays the transcripts entry points take; the arrays
    they point into are kept alive here"""

    def __init__(self, proofs, ext_chals=None):
        self.proofs = [np.ascontiguousarray(p, dtype=np.uint64) for p in proofs]
        ext = list(ext_chals) if ext_chals is not None else [None] * len(self.proofs)
        if len(ext) != len(self.proofs):
            raise ValueError("one entry of ext_chals (None: drawn challenges) for every proof")
        self.ext = [_words(e) for e in ext]
        self.n = len(self.proofs)
        self.ptrs = (C.c_void_p * max(self.n, 1))(*[p.ctypes.data for p in self.proofs])
        self.lens = (C.c_size_t * max(self.n, 1))(*[p.size for p in self.proofs])
        self.exts = (C.c_void_p * max(self.n, 1))(*[None if e is None else e.ctypes.data for e in self.ext])


def stark_transcript_claims(proof, cfg=None, ext_chal=None):
    """The Fiat-Shamir transcript of a vx_stark_prove proof (whole, or its head alone) as TranscriptAir's claims, from one replay of
    the verifier's code over a recording challenger (no GPU needed) -> (the absorbed words, the challenges [n][2] as (words absorbed
    when it was drawn, value)).  Raises VxError with the reason when the proof is refused."""
    L = load_library()
    cfg = cfg or default_stark_config()
    pr, ch = _words(proof), _words(ext_chal)
    n_obs, n_chal, err = C.c_size_t(0), C.c_size_t(0), C.create_string_buffer(256)
    obs, chal = np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    for _ in range(2):  # the first call sizes the arrays (VX_ERR_BUFSZ with both counts set)
        rc = L.vx_stark_transcript_claims(C.byref(cfg), _ptr(pr), pr.size, None if ch is None else _ptr(ch), C.byref(n_obs), _ptr(obs), obs.size, C.byref(n_chal), _ptr(chal), chal.size, err, 256)
        if rc != -4:
            break
        obs, chal = np.zeros(max(n_obs.value, 1), dtype=np.uint64), np.zeros(max(2 * n_chal.value, 2), dtype=np.uint64)
    if rc != 0:
        raise VxError(rc, err.value.decode())
    return obs[: n_obs.value], chal[: 2 * n_chal.value].reshape(-1, 2)


def stark_transcripts_verify(blob, proofs, cfg=None, ext_chals=None):
    """Host-side check of a vx_stark_transcripts_prove blob together with the inner proofs it belongs to (each whole, or its head
    alone): every proof is verified with its transcript answered from the blob's claims -- no Poseidon permutation runs for an inner
    transcript -- and the TranscriptAir table proves the claims.  Raises VxError with the reason; it names the chain."""
    b, pl = _words(blob), _ProofList(proofs, ext_chals)
    _host_verify("vx_stark_transcripts_verify", cfg, b, b.size, pl.ptrs, pl.lens, pl.n, pl.exts)


SINR_MAGIC, SINR_HDR = 0x3130524E49535856, 11  # "VXSINR01": magic, the 7 shape words, the table count, n_obs, n_chal; then the claims as (absorbed, value), one length per table, the proofs


def split_stark_inner(blob):
    """-> (the 7 shape words, n_obs, the claimed challenges [n_chal][2] as (absorbed, value), the table proofs in bus order) of a
    vx_stark_inner_prove blob"""
    n, n_chal = int(blob[8]), int(blob[10])
    at = SINR_HDR + 2 * n_chal
    out, off = [], at + n
    for k in range(n):
        ln = int(blob[at + k])
        out.append(blob[off: off + ln])
        off += ln
    return [int(v) for v in blob[1:8]], int(blob[9]), np.asarray(blob[SINR_HDR: at], dtype=np.uint64).reshape(-1, 2), tuple(out)


def stark_inner_verify(blob, proof, cfg=None, expect_air=0, expect_public=None, ext_chal=None):
    """Host-side check of a vx_stark_inner_prove blob together with the inner proof it belongs to -- the whole proof or its HEAD alone
    (lib.stark_proof_head cuts it): the proof is verified query-free with its transcript answered from the blob's claims -- no Poseidon
    permutation runs for the inner transcript -- and the group proves the query phase and the claims.  Raises VxError with the reason."""
    _stark_group_verify("vx_stark_inner_verify", blob, proof, cfg, expect_air, expect_public, ext_chal)


FCOMB_MAGIC, FCOMB_HDR = 0x31424D4F43465856, 7  # "VXFCOMB1": magic, log2 of the inner LDE, cm, ca, nq, queries, proof length; then the FriCombineAir proof
FCFLD_MAGIC, FCFLD_HDR = 0x31444C4643465856, 9  # "VXFCFLD1": magic, log2 of the inner LDE, cm, ca, nq, fold layers, queries, two proof lengths; then the proofs


def _combine_claims(cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0=None):
    """the claims of FriCombineAir as contiguous arrays: alpha / zeta [2], open_local / open_next [cm + ca][2], open_quot [nq][2],
    index [n], rows [n][cm + ca + nq], ev0 [n][2] (None: not part of the statement)"""
    al = np.ascontiguousarray(alpha, dtype=np.uint64).reshape(-1)
    ze = np.ascontiguousarray(zeta, dtype=np.uint64).reshape(-1)
    ol = np.ascontiguousarray(open_local, dtype=np.uint64).reshape(-1)
    on = np.ascontiguousarray(open_next, dtype=np.uint64).reshape(-1)
    oq = np.ascontiguousarray(open_quot, dtype=np.uint64).reshape(-1)
    idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1)
    rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
    ev = None if ev0 is None else np.ascontiguousarray(ev0, dtype=np.uint64).reshape(-1)
    c = cm + ca
    if al.size != 2 or ze.size != 2 or ol.size != 2 * c or on.size != 2 * c or oq.size != 2 * nq or rw.size != idx.size * (c + nq) or (ev is not None and ev.size != 2 * idx.size):
        raise ValueError("alpha / zeta [2], openings [cm + ca][2] / [nq][2], one row [cm + ca + nq] and one ev_0 [2] for every query")
    return al, ze, ol, on, oq, idx, rw, ev


def fri_combine_verify(blob, log_lde, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0, cfg=None):
    """Host-side check of a vx_fri_combine_prove blob against the verifier's own claims: the inner proof's shape, alpha, zeta, the
    openings at zeta and per query (index, rows [cm + ca + nq], ev0 [2]) in order.  Combines nothing per query; raises VxError."""
    b = _words(blob)
    al, ze, ol, on, oq, idx, rw, ev = _combine_claims(cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0)
    _host_verify("vx_fri_combine_verify", cfg, b, b.size, log_lde, cm, ca, nq, al, ze, ol, on, oq, idx, rw, ev, idx.size)


def fri_combine_fold_verify(blob, log_lde, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, betas, final_poly, index, rows, leaves, cfg=None):
    """Host-side check of a vx_fri_combine_fold_prove blob: the combine claims WITHOUT ev_0 and the fold claims (betas [NL][2], the
    final polynomial [len][2], leaves [n][NL][32]).  Combines and folds nothing; raises VxError with the reason."""
    b = _words(blob)
    al, ze, ol, on, oq, idx, rw, _ = _combine_claims(cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows)
    be, fp, _, _, lv = _fri_claims(betas, final_poly, index, np.zeros(2 * idx.size, dtype=np.uint64), leaves)
    _host_verify("vx_fri_combine_fold_verify", cfg, b, b.size, log_lde, cm, ca, nq, al, ze, ol, on, oq, be, be.shape[0], fp, fp.shape[0], idx, rw, lv, idx.size)


def stark_combine_claims(proof, cfg=None):
    """The combination side of a vx_stark_prove proof (verified on the way) as FriCombineAir's claims -> dict(log_lde, cm, ca, nq,
    alpha [2], zeta [2], open_local [c][2], open_next [c][2], open_quot [nq][2], index [n], ev0 [n][2], rows [n][c + nq])."""
    L = load_library()
    cfg = cfg or default_stark_config()
    pr = np.ascontiguousarray(proof, dtype=np.uint64)
    log_lde, cm, ca, nq, n = C.c_int(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    alpha, zeta = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    bufs = [np.zeros(1, dtype=np.uint64) for _ in range(4)]  # openings, index, ev0, rows: sized by a first call
    err = C.create_string_buffer(256)
    for _ in range(2):
        op, index, ev0, rows = bufs
        rc = L.vx_stark_combine_claims(C.byref(cfg), _ptr(pr), pr.size, C.byref(log_lde), C.byref(cm), C.byref(ca), C.byref(nq), C.byref(n), _ptr(alpha), _ptr(zeta), _ptr(op), op.size,
                                       _ptr(index), _ptr(ev0), index.size, _ptr(rows), rows.size, err, 256)
        if rc != -4:
            break
        c, absn = cm.value + ca.value, cm.value + ca.value + nq.value
        bufs = [np.zeros(4 * c + 2 * nq.value, dtype=np.uint64), np.zeros(n.value, dtype=np.uint64), np.zeros(2 * n.value, dtype=np.uint64), np.zeros(n.value * absn, dtype=np.uint64)]
    if rc != 0:
        raise VxError(rc, err.value.decode())
    c, Q = cm.value + ca.value, n.value
    return dict(log_lde=log_lde.value, cm=cm.value, ca=ca.value, nq=nq.value, alpha=alpha, zeta=zeta, open_local=op[: 2 * c].reshape(c, 2), open_next=op[2 * c: 4 * c].reshape(c, 2),
                open_quot=op[4 * c: 4 * c + 2 * nq.value].reshape(-1, 2), index=index[:Q], ev0=ev0[: 2 * Q].reshape(Q, 2), rows=rows[: Q * (c + nq.value)].reshape(Q, c + nq.value))


BGRP_MAGIC, BGRP_HDR = 0x3130505247425856, 2  # "VXBGRP01": magic, the number of tables, one length per proof; then the proofs in bus order


def _outside(outside):
    """the outside messages of a generic bus group as contiguous [n][VX_BUS_MSG_WORDS] words (t0, t1, t2, t3, tag, m)"""
    o = np.ascontiguousarray(outside, dtype=np.uint64).reshape(-1, VX_BUS_MSG_WORDS) if len(outside) else np.zeros((0, VX_BUS_MSG_WORDS), dtype=np.uint64)
    return o


def _bus_tables(tables):
    """[(air_id, trace Buffer or None, log_n, public inputs)] -> (the vx_bus_table array, what it points to)"""
    pubs = [np.ascontiguousarray(t[3], dtype=np.uint64).reshape(-1) for t in tables]
    arr = (BusTableStruct * max(len(tables), 1))()
    for k, (t, pub) in enumerate(zip(tables, pubs)):
        arr[k] = BusTableStruct(int(t[0]), int(t[2]), t[1].h.value if t[1] is not None else None, pub.ctypes.data if pub.size else None, pub.size)
    return arr, pubs


def bus_group_proof_bound(tables, cfg=None):
    """The words a vx_bus_group_prove blob of `tables` = [(air_id, trace or None, log_n, public inputs)] needs at most (no GPU needed;
    only the AIR ids and the row counts are read).  A table that is not admitted is a VxError (VX_ERR_ARG) naming it."""
    cfg = cfg or default_stark_config()
    L = load_library()
    arr, _keep = _bus_tables(tables)
    need = C.c_size_t(0)
    rc = L.vx_bus_group_proof_bound(C.byref(cfg), arr, len(tables), C.byref(need))
    if rc != 0:
        if not 1 <= len(tables) <= VX_BUS_GROUP_MAX_TABLES:
            raise VxError(rc, "bus group: %d tables (1..%d)" % (len(tables), VX_BUS_GROUP_MAX_TABLES))
        for k, t in enumerate(tables):  # the bound has no buffer for a reason: ask for every table alone
            one, _k = _bus_tables([t])
            if L.vx_bus_group_proof_bound(C.byref(cfg), one, 1, C.byref(need)) != 0:
                raise VxError(rc, "bus group: table %d (air %d, 2^%d rows) is not admitted: an unknown AIR, one without a logUp round of 4 challenges and one total, or rows out of range"
                              % (k, t[0], t[2]))
        raise VxError(rc, "bus group: no proof bound for these tables")
    return need.value


def bus_group_verify(blob, expect, cfg=None, outside=()):
    """Host-side check of a vx_bus_group_prove blob: expect = [(air_id, public inputs)] in bus order -- the verifier states its own AIR
    ids, the blob carries none --, outside = the messages [(t0, t1, t2, t3, tag, m)] of the party that is not a table (m: sent m,
    received P - m).  Raises VxError with the reason."""
    b = _words(blob)
    pubs = [np.ascontiguousarray(pub, dtype=np.uint64).reshape(-1) for _, pub in expect]
    arr = (BusExpectStruct * max(len(expect), 1))()
    for k, ((air_id, _), pub) in enumerate(zip(expect, pubs)):
        arr[k] = BusExpectStruct(int(air_id), pub.ctypes.data if pub.size else None, pub.size)
    o = _outside(outside)
    _host_verify("vx_bus_group_verify", cfg, b, b.size, arr, len(expect), o if o.size else None, o.shape[0])


def split_bus_group(blob):
    """-> the proofs of a vx_bus_group_prove blob, in bus order"""
    n = int(blob[1])
    out, off = [], BGRP_HDR + n
    for k in range(n):
        ln = int(blob[BGRP_HDR + k])
        out.append(blob[off: off + ln])
        off += ln
    return tuple(out)


ROT_HDR = 28  # words before the first proof in a rotate blob


def split_rotate_blob(blob):
    """-> (header-hash proof, current-set commitment proof, new-set commitment proof, Ed25519 proof, SHA-512 proof, epoch-end
    proof) of a vx_rotate_prove blob."""
    out, off = [], ROT_HDR
    for ln in (int(blob[16]), int(blob[17]), int(blob[18]), int(blob[19]), int(blob[24]), int(blob[27])):
        out.append(blob[off: off + ln])
        off += ln
    return tuple(out)


class Buffer:
    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        h = C.c_void_p()
        ctx._ck(ctx.L.vx_alloc(ctx.h, self.n, C.byref(h)))
        self.h = h

    def upload(self, arr, off=0):
        a = np.ascontiguousarray(arr).view(np.uint64).reshape(-1) if np.asarray(arr).dtype != np.uint64 else np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1)
        self.ctx._ck(self.ctx.L.vx_upload(self.ctx.h, self.h, off, _ptr(a), a.size))
        return self

    def download(self, n=None, off=0):
        n = self.n - off if n is None else n
        out = np.empty(n, dtype=np.uint64)
        self.ctx._ck(self.ctx.L.vx_download(self.ctx.h, self.h, off, _ptr(out), n))
        return out

    def devptr(self):
        return self.ctx.L.vx_buf_devptr(self.h)

    @classmethod
    def adopt(cls, ctx, handle):
        """A vx_buf* the library handed to a callback (vx_air_gen_aux_fn): usable, not owned."""
        b = cls.__new__(cls)
        b.ctx, b.h, b.borrowed = ctx, C.c_void_p(handle), True
        b.n = int(ctx.L.vx_buf_len(b.h))
        return b

    def free(self):
        if self.h and not getattr(self, "borrowed", False):
            self.ctx.L.vx_free(self.ctx.h, self.h)
        self.h = None


class Tree:
    def __init__(self, ctx, h, n_leaves, cap_height):
        self.ctx, self.h, self.n_leaves, self.cap_height = ctx, h, n_leaves, cap_height
        self.depth = n_leaves.bit_length() - 1 - cap_height

    def cap(self):
        out = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        self.ctx._ck(self.ctx.L.vx_merkle_cap(self.ctx.h, self.h, _ptr(out)))
        return out

    def open(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.empty((idx.size, self.depth, 4), dtype=np.uint64)
        self.ctx._ck(self.ctx.L.vx_merkle_open(self.ctx.h, self.h, _ptr(idx), idx.size, _ptr(out)))
        return out

    def leaf_digests(self):
        out = np.empty((self.n_leaves, 4), dtype=np.uint64)
        self.ctx._ck(self.ctx.L.vx_merkle_leaf_digests(self.ctx.h, self.h, _ptr(out)))
        return out

    def free(self):
        if self.h:
            self.ctx.L.vx_merkle_free(self.ctx.h, self.h)
            self.h = None


def table_streams_mode(table_streams, hw_queues):
    """The library's choice between a stream per table ("own") and one stream per proof ("shared") for the values of VX_TABLE_STREAMS and
    GPU_MAX_HW_QUEUES (strings, None = unset).  Host only.  (Bound here and not in load_library: an A/B library of an older build,
    VX_LIB_PATH, does not have it.)"""
    f = load_library().vx_table_streams_mode
    f.argtypes, f.restype = [C.c_char_p, C.c_char_p], C.c_int32
    a, b = (None if v is None else str(v).encode() for v in (table_streams, hw_queues))
    return ("own", "shared")[f(a, b)]


class Context:
    """One device + one stream (vx_ctx).  Raises VxError on any failure.  The circuit provers run their tables on side contexts behind it:
    with streams of their own or on this one's, as VX_TABLE_STREAMS says when the context is made (include/vx.h)."""

    def __init__(self, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.vx_ctx_create(device, C.byref(h))
        if rc != 0:
            raise VxError(rc, f"vx_ctx_create(device={device}) failed: no usable gfx950 device (no CPU fallback exists)")
        self.h = h

    def _ck(self, rc):
        if rc != 0:
            raise VxError(rc, self.L.vx_last_error(self.h).decode())

    @classmethod
    def adopt(cls, handle):
        """The vx_ctx* a callback was called with: usable, not owned."""
        c = cls.__new__(cls)
        c.L, c.h, c.borrowed = load_library(), C.c_void_p(handle), True
        return c

    def close(self):
        if self.h and not getattr(self, "borrowed", False):
            self.L.vx_ctx_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._ck(self.L.vx_sync(self.h))

    def timer_start(self):
        self._ck(self.L.vx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.L.vx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def alloc(self, n):
        return Buffer(self, n)

    # verifying on the GPU: the host verifiers with every Merkle opening checked in one launch (include/vx.h)
    def merkle_check(self, caps, log_leaves, tree_of, leaf_idx, leaves, siblings):
        """Checks a batch of Merkle openings on the device.  caps [n_trees][2^cap_height][4]; log_leaves [n_trees]; per claim its tree,
        its leaf index, its leaf row (any length >= 1) and its siblings [log_leaves - cap_height][4], leaf level first -- the layout
        of lib.stark_merkle_claims.  Returns None when every claim reaches its cap, else the smallest failing claim; VxError
        (VX_ERR_ARG) for claims out of range or non-canonical words."""
        cp = np.ascontiguousarray(caps, dtype=np.uint64)
        n_trees = len(log_leaves)
        cap_height = (cp.size // max(n_trees, 1) // 4).bit_length() - 1
        ll = np.ascontiguousarray(log_leaves, dtype=np.int32)
        tr, ix = _words(tree_of), _words(leaf_idx)
        ln = np.array([np.asarray(r).size for r in leaves], dtype=np.uint64)
        cat = lambda rows: np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1) for r in rows] + [np.zeros(0, np.uint64)]))
        lv, sb = cat(leaves), cat(siblings)
        bad = C.c_size_t(0)
        rc = self.L.vx_merkle_check(self.h, _ptr(cp), cap_height, _ptr(ll), n_trees, _ptr(tr), _ptr(ix), _ptr(ln), _ptr(lv), lv.size, _ptr(sb), sb.size, tr.size, C.byref(bad))
        if rc == -5:
            return bad.value
        self._ck(rc)
        return None

    def stark_verify(self, proof, cfg=None, expect_air=0, expect_public=None):
        """lib.stark_verify with the openings checked on this context's device: the same VxError, code and text."""
        stark_verify(proof, cfg, expect_air, expect_public, _symbol="vx_stark_verify_dev", _ctx=self.h)

    def header_range_verify(self, blob, max_headers, trusted_block, trusted_hash, target_block, out96, cfg=None, authority_set_hash=None, authority_set_id=0):
        """lib.header_range_verify with the openings of every table checked in one launch on this context's device."""
        header_range_verify(blob, max_headers, trusted_block, trusted_hash, target_block, out96, cfg, authority_set_hash, authority_set_id, _ctx=self.h)

    def rotate_verify(self, blob, authority_set_id, authority_set_hash, out32, cfg=None):
        """lib.rotate_verify with the openings of its six tables checked in one launch on this context's device."""
        rotate_verify(blob, authority_set_id, authority_set_hash, out32, cfg, _ctx=self.h)

    def from_host(self, arr):
        a = np.ascontiguousarray(arr)
        nwords = (a.nbytes + 7) // 8
        if a.dtype != np.uint64:
            raw = np.zeros(nwords * 8, dtype=np.uint8)
            raw[: a.nbytes] = a.view(np.uint8).reshape(-1)
            a = raw.view(np.uint64)
        return Buffer(self, max(nwords, 1)).upload(a.reshape(-1))

    def fill_random(self, buf, n, seed, off=0):
        self._ck(self.L.vx_fill_random(self.h, buf.h, off, n, seed))

    def copy(self, dst, src, n, dst_off=0, src_off=0):
        self._ck(self.L.vx_copy(self.h, dst.h, dst_off, src.h, src_off, n))

    # K1
    def field_op(self, name, a, b, out, n):
        f = getattr(self.L, "vx_field_batch_" + name)
        self._ck(f(self.h, a.h, out.h, n) if name == "inv" else f(self.h, a.h, b.h, out.h, n))

    def ext_mul(self, a, b, out, n):
        self._ck(self.L.vx_ext_batch_mul(self.h, a.h, b.h, out.h, n))

    # K2 / K3
    def ntt(self, buf, log_n, n_cols, inverse=False, shift=0, order=VX_ORDER_NATURAL, off=0, col_stride=None):
        cs = (1 << log_n) if col_stride is None else col_stride
        self._ck(self.L.vx_ntt(self.h, buf.h, off, log_n, n_cols, cs, int(inverse), shift, order))

    def lde(self, src, log_n, n_cols, rate_bits, dst, shift=7, src_kind=VX_LDE_SRC_VALUES, coeffs_out=None):
        self._ck(self.L.vx_lde(self.h, src.h, log_n, n_cols, rate_bits, shift, src_kind, dst.h, coeffs_out.h if coeffs_out else None))

    def lde_rows(self, lde, log_N, n_cols, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.empty((idx.size, n_cols), dtype=np.uint64)
        self._ck(self.L.vx_lde_rows(self.h, lde.h, log_N, n_cols, _ptr(idx), idx.size, _ptr(out)))
        return out

    # K4
    def poseidon(self, states_buf, n):
        self._ck(self.L.vx_poseidon_permute_batch(self.h, states_buf.h, n))

    def poseidon_air_trace(self, states_buf, n_perm, out=None):
        """The witness of PoseidonAir (air_library.poseidon_builder) for n_perm input states -> Buffer [48][32 * n_perm]."""
        out = out or self.alloc(48 * 32 * n_perm)
        self._ck(self.L.vx_poseidon_air_trace(self.h, states_buf.h, n_perm, out.h))
        return out

    def merkle_open_air_trace(self, tree, leaf_idx, log_n, out=None):
        """The witness of MerkleOpenAir for the openings leaf_idx of `tree` -> (Buffer [66][2^log_n], the 9 public inputs)."""
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        out = out or self.alloc(VX_MERKLE_OPEN_AIR_COLS << log_n)
        pub = np.zeros(9, dtype=np.uint64)
        self._ck(self.L.vx_merkle_open_air_trace(self.h, tree.h, _ptr(idx), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def _prove_blob(self, cfg, out, bound, bound_msg, prove):
        """The body of the aggregation provers: bound(cfg, need) sizes the blob when the caller gave no `out` (refused with
        bound_msg), prove(cfg, out, need) writes it -> the blob words.  A failed proof raises the context's error with the
        needed length as `.needed`."""
        cfg = cfg or self.stark_config()
        need = C.c_size_t(0)
        if out is None:
            rc = bound(C.byref(cfg), C.byref(need))
            if rc != 0:
                raise VxError(rc, bound_msg)
            out = np.empty(need.value, dtype=np.uint64)
        rc = prove(C.byref(cfg), out, C.byref(need))
        if rc != 0:
            e = VxError(rc, self.L.vx_last_error(self.h).decode())
            e.needed = need.value  # VX_ERR_BUFSZ: the words the blob needs
            raise e
        return out[: need.value]

    def merkle_openings_prove(self, tree, leaf_idx, cfg=None, out=None):
        """Proves the openings leaf_idx of `tree` in one MerkleOpenAir table -> blob words (lib.merkle_openings_verify checks it).
        out: a caller's uint64 buffer; when it is too small the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_merkle_openings_proof_bound(c, tree.n_leaves, idx.size, need),
                                "merkle openings: %d openings of a tree of %d leaves" % (idx.size, tree.n_leaves),
                                lambda c, o, need: self.L.vx_merkle_openings_prove(self.h, c, tree.h, _ptr(idx), idx.size, _ptr(o), o.size, need))

    def leaf_sponge_air_trace(self, data, n_leaves, leaf_len, layout, leaf_idx, log_n, off=0, out=None):
        """The witness of LeafSpongeAir for the rows leaf_idx of the leaves in `data` (as Context.merkle takes them)
        -> (Buffer [66][2^log_n], the 14 public inputs)."""
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        out = out or self.alloc(VX_LEAF_SPONGE_AIR_COLS << log_n)
        pub = np.zeros(14, dtype=np.uint64)
        self._ck(self.L.vx_leaf_sponge_air_trace(self.h, data.h, off, n_leaves, leaf_len, layout, _ptr(idx), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def merkle_rows_prove(self, tree, data, leaf_len, layout, leaf_idx, cfg=None, out=None, off=0):
        """Proves the openings leaf_idx of `tree` and hashes the opened rows of `data` (what the tree was built from) in two
        tables on one bus -> blob words (lib.merkle_rows_verify checks it).  out: a caller's uint64 buffer; when it is too small
        the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_merkle_rows_proof_bound(c, tree.n_leaves, leaf_len, idx.size, need),
                                "merkle rows: %d openings of %d words of a tree of %d leaves" % (idx.size, leaf_len, tree.n_leaves),
                                lambda c, o, need: self.L.vx_merkle_rows_prove(self.h, c, tree.h, data.h, off, leaf_len, layout, _ptr(idx), idx.size, _ptr(o), o.size, need))

    def fri_fold_air_trace(self, log_lde, betas, index, ev0, leaves, log_n, tree0=0, out=None):
        """The witness of FriFoldAir for the claims (index[i], ev0[i][2], leaves[i][NL][32]) under betas [NL][2]
        -> (Buffer [120][2^log_n], the 24 public inputs)."""
        be, _, idx, ev, lv = _fri_claims(betas, [0, 0], index, ev0, leaves)
        out = out or self.alloc(VX_FRI_FOLD_AIR_COLS << log_n)
        pub = np.zeros(24, dtype=np.uint64)
        self._ck(self.L.vx_fri_fold_air_trace(self.h, log_lde, _ptr(be), be.shape[0], tree0, _ptr(idx), _ptr(ev), _ptr(lv), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def fri_exit_air_trace(self, log_lde, n_layers, pow_bits, ord_pow, absorbed, values, final_poly, log_n, out=None):
        """The witness of FriExitAir (air_library.fri_exit_builder()): values = the proof-of-work response, then one index challenge
        per query -> (Buffer [21][2^log_n], the 12 public inputs).  VxError: VX_ERR_STATEMENT "proof of work invalid", VX_ERR_ARG
        for a non-canonical value or a shape the table does not hold."""
        vals, fp = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1), np.ascontiguousarray(final_poly, dtype=np.uint64).reshape(-1, 2)
        if vals.size < 2:
            raise ValueError("the proof-of-work response and at least one index challenge")
        own = out is None
        out = out or self.alloc(FRI_EXIT_AIR_COLS << log_n)
        pub = np.zeros(FRI_EXIT_PUBLIC, dtype=np.uint64)
        try:
            self._ck(self.L.vx_fri_exit_air_trace(self.h, log_lde, n_layers, pow_bits, int(ord_pow), int(absorbed), _ptr(vals), vals.size - 1, _ptr(fp), fp.shape[0], log_n, out.h, _ptr(pub)))
        except VxError:
            if own:
                out.free()
            raise
        return out, pub

    def fri_exits_tables(self, proof, cfg=None, ext_chal=None):
        """The three tables of an inner proof's exit group as bus_group_prove takes them, [(air_id, trace Buffer, log_n, public inputs)]
        for FriFoldAir, TranscriptAir, FriExitAir, every one with the group's statement digest as its last four public inputs, and
        the outside party's messages.  The three Buffers are the caller's to free."""
        cfg, fc, obs, chal, ord_pow, stmt, ops, logs = _fri_exits_statement(proof, cfg, ext_chal)
        NL = fc["betas"].shape[0]
        made = []  # allocated here and handed to the witness calls, so that a call that raises leaves nothing behind
        try:
            for cols, log_n in zip((VX_FRI_FOLD_AIR_COLS, VX_TRANSCRIPT_AIR_COLS, FRI_EXIT_AIR_COLS), logs):
                made.append(self.alloc(cols << log_n))
            ftr, fpub = self.fri_fold_air_trace(fc["log_lde"], fc["betas"], fc["index"], fc["ev0"], fc["leaves"], logs[0], out=made[0])
            ttr, _, _ = self.transcript_air_trace([ops], [obs], logs[1], out=made[1])
            etr, epub = self.fri_exit_air_trace(fc["log_lde"], NL, cfg.pow_bits, ord_pow, obs.size, chal[ord_pow:, 1], fc["final_poly"], logs[2], out=made[2])
        except Exception:
            for buf in made:
                buf.free()
            raise
        tables = [(VX_AIR_FRI_FOLD, ftr, logs[0], np.concatenate([fpub[:-4], stmt])), (VX_AIR_TRANSCRIPT, ttr, logs[1], stmt), (fri_exit_air_id(), etr, logs[2], np.concatenate([epub[:-4], stmt]))]
        return tables, fri_exits_outside(fc["log_lde"], ord_pow, obs, chal, fc["final_poly"], fc["index"], fc["ev0"], fc["leaves"]), cfg

    def fri_exits_prove(self, proof, cfg=None, ext_chal=None):
        """Proves the exit group of a vx_stark_prove proof: its fold chains (FriFoldAir), its transcript (TranscriptAir) and, between
        them on one bus, FriExitAir -- query indices, proof of work and the final polynomial at every query's point -> a bus-group
        blob (lib.fri_exits_verify checks it).  Composed from the exported claims, witnesses and the generic bus group."""
        tables, outside, cfg = self.fri_exits_tables(proof, cfg, ext_chal)
        try:
            return self.bus_group_prove(tables, cfg, outside)
        finally:
            for t in tables:
                t[1].free()

    def fri_fold_prove(self, log_lde, betas, final_poly, index, ev0, leaves, cfg=None, out=None):
        """Proves the fold chains of the claims in one FriFoldAir table -> blob words (lib.fri_fold_verify checks it).  The chains are
        folded natively first: VxError(VX_ERR_STATEMENT) names the query and layer that do not hold.  out: a caller's uint64 buffer;
        when it is too small the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        be, fp, idx, ev, lv = _fri_claims(betas, final_poly, index, ev0, leaves)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_fri_fold_proof_bound(c, log_lde, be.shape[0], idx.size, need),
                                "fri fold: bad shape or configuration (arity_bits 4, 1..8 layers, at least one index bit left, 1..2^20 queries)",
                                lambda c, o, need: self.L.vx_fri_fold_prove(self.h, c, log_lde, _ptr(be), be.shape[0], _ptr(fp), fp.shape[0], _ptr(idx), _ptr(ev), _ptr(lv), idx.size,
                                                                            _ptr(o), o.size, need))

    def fri_combine_air_trace(self, log_lde, rate_bits, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0, log_n, tree0=0, out=None):
        """The witness of FriCombineAir for the claims (index[i], rows[i][cm + ca + nq], ev0[i][2]) -> (Buffer [28][2^log_n], the 22
        public inputs)."""
        al, ze, ol, on, oq, idx, rw, ev = _combine_claims(cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0)
        out = out or self.alloc(VX_FRI_COMBINE_AIR_COLS << log_n)
        pub = np.zeros(22, dtype=np.uint64)
        self._ck(self.L.vx_fri_combine_air_trace(self.h, log_lde, rate_bits, cm, ca, nq, _ptr(al), _ptr(ze), _ptr(ol), _ptr(on), _ptr(oq), tree0, _ptr(idx), _ptr(rw), _ptr(ev), idx.size,
                                                 log_n, out.h, _ptr(pub)))
        return out, pub

    def fri_combine_prove(self, log_lde, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0, cfg=None, out=None):
        """Proves the FRI combination of the claims in one FriCombineAir table -> blob words (lib.fri_combine_verify checks it).  Every
        query is combined natively first: VxError(VX_ERR_STATEMENT) names the query whose ev_0 differs.  out: a caller's uint64
        buffer; when it is too small the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        al, ze, ol, on, oq, idx, rw, ev = _combine_claims(cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows, ev0)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_fri_combine_proof_bound(c, log_lde, cm, ca, nq, idx.size, need),
                                "fri combine: bad shape or configuration (log_lde 5..32, cm, nq >= 1, 1..2^20 queries, a table of at most 2^26 rows)",
                                lambda c, o, need: self.L.vx_fri_combine_prove(self.h, c, log_lde, cm, ca, nq, _ptr(al), _ptr(ze), _ptr(ol), _ptr(on), _ptr(oq), _ptr(idx), _ptr(rw), _ptr(ev),
                                                                               idx.size, _ptr(o), o.size, need))

    def fri_combine_fold_prove(self, log_lde, cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, betas, final_poly, index, rows, leaves, cfg=None, out=None):
        """Proves the FRI combination and the fold chains of the queries in two tables on one bus -> blob words
        (lib.fri_combine_fold_verify checks it).  ev_0 is computed here and closes between the tables.  The statement is checked
        natively first: VxError(VX_ERR_STATEMENT) names query and stage."""
        al, ze, ol, on, oq, idx, rw, _ = _combine_claims(cm, ca, nq, alpha, zeta, open_local, open_next, open_quot, index, rows)
        be, fp, _, _, lv = _fri_claims(betas, final_poly, index, np.zeros(2 * idx.size, dtype=np.uint64), leaves)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_fri_combine_fold_proof_bound(c, log_lde, cm, ca, nq, be.shape[0], idx.size, need),
                                "fri combine-fold: bad shape or configuration (arity_bits 4, 1..8 layers, cm, nq >= 1, 1..2^20 queries, tables of at most 2^26 rows)",
                                lambda c, o, need: self.L.vx_fri_combine_fold_prove(self.h, c, log_lde, cm, ca, nq, _ptr(al), _ptr(ze), _ptr(ol), _ptr(on), _ptr(oq), _ptr(be), be.shape[0],
                                                                                    _ptr(fp), fp.shape[0], _ptr(idx), _ptr(rw), _ptr(lv), idx.size, _ptr(o), o.size, need))

    def merkle_open_set_air_trace(self, trees, tree_of, leaf_idx, log_n, out=None):
        """The witness of MerkleOpenSetAir: opening i is leaf leaf_idx[i] of trees[tree_of[i]] -> (Buffer [72][2^log_n], the 4
        public inputs: the digest of the claims (tree, index, leaf digest))."""
        to = np.ascontiguousarray(tree_of, dtype=np.uint64).reshape(-1)
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        if to.size != idx.size:
            raise ValueError("one tree for every opening")
        th = (C.c_void_p * len(trees))(*[t.h for t in trees])
        out = out or self.alloc(VX_MERKLE_OPEN_SET_AIR_COLS << log_n)
        pub = np.zeros(4, dtype=np.uint64)
        self._ck(self.L.vx_merkle_open_set_air_trace(self.h, th, len(trees), _ptr(to), _ptr(idx), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def leaf_sponge_set_air_trace(self, evals, log_leaves, tree_of, leaf_idx, log_n, out=None):
        """The witness of LeafSpongeSetAir for leaves of FRI layers: tree t is the layer evals[t] of 2^(log_leaves[t] + 4) extension
        values in natural order, opening i is its leaf leaf_idx[i] for t = tree_of[i] -> (Buffer [67][2^log_n], the 14 public
        inputs: L = 32, B = 4, the tail flags, the digest of the claims (tree, index, row))."""
        to = np.ascontiguousarray(tree_of, dtype=np.uint64).reshape(-1)
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        if to.size != idx.size or len(evals) != len(log_leaves):
            raise ValueError("one tree for every opening, one log_leaves for every layer")
        eh = (C.c_void_p * len(evals))(*[e.h for e in evals])
        ll = (C.c_int * len(evals))(*[int(v) for v in log_leaves])
        out = out or self.alloc(VX_LEAF_SPONGE_SET_AIR_COLS << log_n)
        pub = np.zeros(14, dtype=np.uint64)
        self._ck(self.L.vx_leaf_sponge_set_air_trace(self.h, eh, ll, len(evals), _ptr(to), _ptr(idx), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def fri_queries_prove(self, log_lde, betas, final_poly, trees, evals, index, cfg=None, out=None):
        """Proves the FRI query phase of the queries `index`: trees[l] (fri_layer_tree, arity_bits 4) and evals[l] (the layer it was
        built from, natural order) for every fold layer -> blob words (lib.fri_queries_verify checks it).  Three tables on one bus:
        the openings, the leaf hashes, the fold chains.  The chains are folded natively first: VxError(VX_ERR_STATEMENT) names the
        query and layer that do not hold.  out: a caller's uint64 buffer; when it is too small the VxError (VX_ERR_BUFSZ) carries
        the needed length as `.needed`."""
        be = np.ascontiguousarray(betas, dtype=np.uint64).reshape(-1, 2)
        fp = np.ascontiguousarray(final_poly, dtype=np.uint64).reshape(-1, 2)
        idx = np.ascontiguousarray(index, dtype=np.uint64).reshape(-1)
        if len(trees) != be.shape[0] or len(evals) != be.shape[0]:
            raise ValueError("one tree and one layer for every beta")
        th = (C.c_void_p * len(trees))(*[t.h for t in trees])
        eh = (C.c_void_p * len(evals))(*[e.h for e in evals])
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_fri_queries_proof_bound(c, log_lde, be.shape[0], idx.size, need),
                                "fri queries: bad shape or configuration (arity_bits 4, 1..8 layers, at least one index bit left, 1..2^20 queries, tables of at most 2^26 rows)",
                                lambda c, o, need: self.L.vx_fri_queries_prove(self.h, c, log_lde, _ptr(be), be.shape[0], _ptr(fp), fp.shape[0], th, eh, _ptr(idx), idx.size,
                                                                               _ptr(o), o.size, need))

    def merkle_paths_air_trace(self, caps, log_leaves, tree_of, leaf_idx, leaf_digests, siblings, log_n, out=None):
        """The witness of MerkleOpenSetAir from authentication paths: tree t has 2^log_leaves[t] leaves (0: no such tree) and the cap
        caps[t][2^cap_height][4]; opening i enters with leaf_digests[i][4] and siblings[i] = the [log_leaves - cap_height][4] words of
        its path -> (Buffer [72][2^log_n], the 4 public inputs: the digest of the claims (tree, index, leaf digest))."""
        cp = np.ascontiguousarray(caps, dtype=np.uint64).reshape(len(log_leaves), -1, 4)
        cap_height = cp.shape[1].bit_length() - 1
        to = np.ascontiguousarray(tree_of, dtype=np.uint64).reshape(-1)
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        dg = np.ascontiguousarray(leaf_digests, dtype=np.uint64).reshape(-1)
        sb = np.concatenate([np.zeros(1, dtype=np.uint64)] + [np.ascontiguousarray(s, dtype=np.uint64).reshape(-1) for s in siblings])[1:]
        want = sum(4 * (int(log_leaves[int(t)]) - cap_height) for t in to if int(t) < len(log_leaves))
        if to.size != idx.size or dg.size != 4 * idx.size or cp.shape[1] != 1 << cap_height or sb.size != want:
            raise ValueError("one tree, one digest [4] and one path [log_leaves - cap_height][4] for every opening")
        sb = np.ascontiguousarray(np.concatenate([sb, np.zeros(1, dtype=np.uint64)]))  # (never empty)
        ll = (C.c_int * len(log_leaves))(*[int(v) for v in log_leaves])
        out = out or self.alloc(VX_MERKLE_OPEN_SET_AIR_COLS << log_n)
        pub = np.zeros(4, dtype=np.uint64)
        self._ck(self.L.vx_merkle_paths_air_trace(self.h, _ptr(cp), cap_height, ll, len(log_leaves), _ptr(to), _ptr(idx), _ptr(dg), _ptr(sb), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def leaf_sponge_rows_air_trace(self, tree_of, leaf_idx, rows, log_n, out=None):
        """The witness of LeafSpongeSetAir from rows handed over directly: opening i is the row rows[i][L] (L >= 5) of leaf leaf_idx[i]
        of tree tree_of[i] -> (Buffer [67][2^log_n], the 14 public inputs: L, B, the tail flags, the digest of the claims)."""
        to = np.ascontiguousarray(tree_of, dtype=np.uint64).reshape(-1)
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        rw = np.ascontiguousarray(rows, dtype=np.uint64).reshape(idx.size, -1)
        if to.size != idx.size:
            raise ValueError("one tree for every opening")
        out = out or self.alloc(VX_LEAF_SPONGE_SET_AIR_COLS << log_n)
        pub = np.zeros(14, dtype=np.uint64)
        self._ck(self.L.vx_leaf_sponge_rows_air_trace(self.h, rw.shape[1], _ptr(to), _ptr(idx), _ptr(rw), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def leaf_noop_air_trace(self, tree_of, leaf_idx, rows, log_n, out=None):
        """The witness of LeafNoopAir: opening i is the row rows[i] (1..4 words: its own digest) of leaf leaf_idx[i] of tree tree_of[i];
        the rows may differ in length -> (Buffer [11][2^log_n], the 4 public inputs: the digest of the claims)."""
        to = np.ascontiguousarray(tree_of, dtype=np.uint64).reshape(-1)
        idx = np.ascontiguousarray(leaf_idx, dtype=np.uint64).reshape(-1)
        if to.size != idx.size or len(rows) != idx.size:
            raise ValueError("one tree and one row for every opening")
        ln = np.array([len(r) for r in rows], dtype=np.uint64)
        rw = np.zeros((idx.size, 4), dtype=np.uint64)
        for i, r in enumerate(rows):
            rw[i, :min(len(r), 4)] = np.asarray(r, dtype=np.uint64)[:4]
        out = out or self.alloc(VX_LEAF_NOOP_AIR_COLS << log_n)
        pub = np.zeros(4, dtype=np.uint64)
        self._ck(self.L.vx_leaf_noop_air_trace(self.h, _ptr(to), _ptr(idx), _ptr(ln), _ptr(rw), idx.size, log_n, out.h, _ptr(pub)))
        return out, pub

    def _stark_group_prove(self, level, proof, cfg, ext_chal, out, refusal, bound_takes_chal=False):
        """the three levels of a proof's bus group share one prover signature; only the inner level's bound replays the head and takes ext_chal"""
        pr, ext = _words(proof), _words(ext_chal)
        ch = None if ext is None else _ptr(ext)
        bound, prove = getattr(self.L, f"vx_stark_{level}_proof_bound"), getattr(self.L, f"vx_stark_{level}_prove")
        return self._prove_blob(cfg, out, lambda c, need: bound(c, _ptr(pr), pr.size, ch, need) if bound_takes_chal else bound(c, _ptr(pr), pr.size, need),
                                f"stark {level}: {refusal}", lambda c, o, need: prove(self.h, c, _ptr(pr), pr.size, ch, _ptr(o), o.size, need))

    def stark_openings_prove(self, proof, cfg=None, ext_chal=None, out=None):
        """Proves the Merkle openings of the vx_stark_prove proof `proof` from the paths it carries -> blob words
        (lib.stark_openings_verify checks blob and proof together).  One openings table and one sponge table per leaf length above 4.
        The proof is verified on the way and every path walked natively first: VxError(VX_ERR_STATEMENT) names query and tree.
        out: a caller's uint64 buffer; when it is too small the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        return self._stark_group_prove("openings", proof, cfg, ext_chal, out, "not a proof of a known AIR under this configuration, or a shape without an openings group (more than 8 fold layers, a table above 2^26 rows)")

    def stark_queries_prove(self, proof, cfg=None, ext_chal=None, out=None):
        """Proves the whole query phase of the vx_stark_prove proof `proof` on one bus -> blob words (lib.stark_queries_verify checks
        blob and the proof's head together).  Five to seven tables: the openings, one sponge table per leaf length above 4, the no-op
        leaves, the FRI combination, the fold chains.  The proof is verified on the way and paths, combinations and folds are checked
        natively first: VxError(VX_ERR_STATEMENT) names query and tree or layer.  out: a caller's uint64 buffer; when it is too small
        the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        return self._stark_group_prove("queries", proof, cfg, ext_chal, out, "not a proof of a known AIR under this configuration, or a shape without a query-phase group (arity_bits other than 4, no fold layer or more than 8, a table above 2^26 rows)")

    def transcript_air_trace(self, ops, words, log_n, out=None):
        """The witness of TranscriptAir: chain c has the run lengths ops[c] = [observe count, challenge count, observe count, ...] and
        absorbs words[c] in order -> (Buffer [93][2^log_n], the 4 public inputs: the statement digest, the challenges the device drew
        per chain)."""
        if len(ops) != len(words):
            raise ValueError("one list of words for every chain")
        n_ops = (C.c_size_t * max(len(ops), 1))(*[len(o) for o in ops])
        op = np.ascontiguousarray([int(v) for o in ops for v in o] + [0], dtype=np.uint64)
        wd = np.ascontiguousarray([int(v) for w in words for v in w] + [0], dtype=np.uint64)
        drawn = [sum(int(v) for v in o[1::2]) for o in ops]
        chal = np.zeros(sum(drawn) + 1, dtype=np.uint64)
        out = out or self.alloc(VX_TRANSCRIPT_AIR_COLS << log_n)
        pub = np.zeros(4, dtype=np.uint64)
        self._ck(self.L.vx_transcript_air_trace(self.h, len(ops), n_ops, _ptr(op), _ptr(wd), wd.size - 1, log_n, out.h, _ptr(pub), _ptr(chal)))
        cut = np.cumsum([0] + drawn)
        return out, pub, [chal[cut[c]: cut[c + 1]].copy() for c in range(len(ops))]

    def stark_transcripts_prove(self, proofs, cfg=None, ext_chals=None, out=None):
        """Proves the Fiat-Shamir transcripts of the vx_stark_prove proofs `proofs` (each whole, or its head alone) in one TranscriptAir
        table -> blob words (lib.stark_transcripts_verify checks blob and proofs together).  ext_chals: per proof the external lookup
        challenges it was made under, or None.  Every proof is verified natively first: VxError(VX_ERR_STATEMENT) names the proof.
        out: a caller's uint64 buffer; when it is too small the VxError (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        pl = _ProofList(proofs, ext_chals)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_stark_transcripts_proof_bound(c, pl.ptrs, pl.lens, pl.n, pl.exts, need),
                                "stark transcripts: 1..64 proofs of known AIRs under this configuration, every one acceptable, in a table of at most 2^26 rows",
                                lambda c, o, need: self.L.vx_stark_transcripts_prove(self.h, c, pl.ptrs, pl.lens, pl.n, pl.exts, _ptr(o), o.size, need))

    def stark_inner_prove(self, proof, cfg=None, ext_chal=None, out=None):
        """Proves the query phase AND the Fiat-Shamir transcript of the vx_stark_prove proof `proof` on one bus -> blob words
        (lib.stark_inner_verify checks blob and the proof's head together).  Six to eight tables: those of stark_queries_prove, then
        the transcript.  The proof is verified on the way, by one replay, and paths, combinations and folds are checked natively first:
        VxError(VX_ERR_STATEMENT) names query and tree or layer.  out: a caller's uint64 buffer; when it is too small the VxError
        (VX_ERR_BUFSZ) carries the needed length as `.needed`."""
        return self._stark_group_prove("inner", proof, cfg, ext_chal, out, "not a proof of a known AIR under this configuration, its head is not acceptable, or a shape without a query-phase group (arity_bits other than 4, no fold layer or more than 8, a table above 2^26 rows)", True)

    def merkle(self, data, n_leaves, leaf_len, layout, cap_height, off=0):
        t = C.c_void_p()
        self._ck(self.L.vx_merkle_build(self.h, data.h, off, n_leaves, leaf_len, layout, cap_height, C.byref(t)))
        return Tree(self, t, n_leaves, cap_height)

    # K6
    def fri_fold(self, evals, log_n, arity_bits, beta, shift, out):
        b = np.ascontiguousarray(beta, dtype=np.uint64)
        self._ck(self.L.vx_fri_fold(self.h, evals.h, log_n, arity_bits, _ptr(b), shift, out.h))

    def fri_layer_tree(self, evals, log_n, arity_bits, cap_height):
        t = C.c_void_p()
        self._ck(self.L.vx_fri_layer_tree(self.h, evals.h, log_n, arity_bits, cap_height, C.byref(t)))
        return Tree(self, t, 1 << (log_n - arity_bits), cap_height)

    def fri_leaves(self, evals, log_n, arity_bits, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.empty((idx.size, 2 << arity_bits), dtype=np.uint64)
        self._ck(self.L.vx_fri_leaves(self.h, evals.h, log_n, arity_bits, _ptr(idx), idx.size, _ptr(out)))
        return out

    def fri_pow(self, state12, pos, bits):
        s = np.ascontiguousarray(state12, dtype=np.uint64)
        nonce = C.c_uint64()
        self._ck(self.L.vx_fri_pow(self.h, _ptr(s), pos, bits, C.byref(nonce)))
        return nonce.value

    # K5/K7: generic STARK prover
    def stark_config(self, **over):
        cfg = StarkConfig()
        self._ck(self.L.vx_stark_default_config(C.byref(cfg)))
        for k, v in over.items():
            setattr(cfg, k, v)
        return cfg

    def stark_prove(self, air_id, trace_buf, log_n, public_inputs, cfg=None):
        cfg = cfg or self.stark_config()
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        need = C.c_size_t(0)
        self._ck(self.L.vx_stark_proof_bound(air_id, C.byref(cfg), log_n, C.byref(need)))
        out = np.empty(need.value, dtype=np.uint64)
        self._ck(self.L.vx_stark_prove(self.h, air_id, C.byref(cfg), trace_buf.h, log_n, _ptr(pub), pub.size, _ptr(out), out.size, C.byref(need)))
        return out[: need.value]

    def bus_group_prove(self, tables, cfg=None, outside=(), out=None):
        """Proves tables = [(air_id, trace Buffer, log_n, public inputs)] together on one logUp bus, in that order, under shared lookup
        challenges -> blob words (lib.bus_group_verify checks it).  outside: the messages of the party that is not a table.  When every
        table has a message list the bus balance is checked on the device first: VX_ERR_STATEMENT names what has no partner."""
        arr, _keep = _bus_tables(tables)
        o = _outside(outside)
        cfg = cfg or self.stark_config()
        if out is None:
            need = C.c_size_t(0)  # (tables that have no bound are not admitted: the prover says why)
            rc = self.L.vx_bus_group_proof_bound(C.byref(cfg), arr, len(tables), C.byref(need))
            out = np.empty(need.value if rc == 0 else 1, dtype=np.uint64)
        return self._prove_blob(cfg, out, lambda c, need: self.L.vx_bus_group_proof_bound(c, arr, len(tables), need), "bus group: no proof bound for these tables",
                                lambda c, b, need: self.L.vx_bus_group_prove(self.h, c, arr, len(tables), _ptr(o) if o.size else None, o.shape[0], _ptr(b), b.size, need))

    def bus_group_check(self, tables, outside=()):
        """The bus balance of tables (as bus_group_prove takes them) and outside messages on the device, nothing proven: None when
        the bus closes, else a BusUnmatched (n_unmatched, table, message, row, net) naming the lowest message without a partner."""
        arr, _keep = _bus_tables(tables)
        o = _outside(outside)
        u = BusUnmatchedStruct()
        self._ck(self.L.vx_bus_group_check(self.h, arr, len(tables), _ptr(o) if o.size else None, o.shape[0], C.byref(u)))
        return None if u.n_unmatched == 0 else BusUnmatched(int(u.n_unmatched), int(u.table), int(u.message), int(u.row), int(u.net))

    def stark_aux_trace(self, air_id, trace_buf, log_n, challenges, n_aux_cols, public_inputs=(), out=None):
        """The auxiliary (logUp) columns of an AIR for given lookup challenges -> (Buffer [n_aux_cols][2^log_n], published values).
        out: a caller's Buffer of at least n_aux_cols << log_n words (the columns go to its start)."""
        ch = np.ascontiguousarray(challenges, dtype=np.uint64)
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = out or self.alloc(n_aux_cols << log_n)
        apub = np.zeros(8, dtype=np.uint64)
        self._ck(self.L.vx_stark_aux_trace(self.h, air_id, trace_buf.h, log_n, _ptr(pub) if pub.size else None, pub.size, _ptr(ch), ch.size, out.h, _ptr(apub)))
        return out, apub

    def header_range_prove(self, headers_buf, stride, sizes, max_headers, trusted_block, trusted_hash, target_block, cfg=None, out=None, just=None,
                           n_segments=1, shard=None):
        """HeaderRangeCircuit::prove for a chain resident in HBM -> (96-byte output, proof blob words).
        just: PackedJustification (or None to skip the justification check); n_segments: map segments of the hash-chain table;
        shard = (index, n_shards, exchange): prove only this shard's tables -- exchange(words) must return the element-wise sum
        over the shards of the uint64 array it is given (an all-reduce); the blob then holds the local proofs (lib.merge_blobs)."""
        cfg = cfg or self.stark_config()
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        th = np.frombuffer(bytes(trusted_hash), dtype=np.uint8).copy()
        chunks = int(((sizes.astype(np.int64) + 127) // 128).sum())
        need = C.c_size_t(0)
        self._ck(self.L.vx_header_range_proof_bound_ex(C.byref(cfg), chunks, just.struct.num_authorities if just is not None else 0, n_segments, C.byref(need)))
        if out is None or out.size < need.value:
            out = np.empty(need.value, dtype=np.uint64)
        out96 = np.zeros(96, dtype=np.uint8)
        xch, idx, n_shards = None, 0, 1
        if shard is not None:
            idx, n_shards, fn = shard
            errs = []

            def cb(_user, words, n_words):
                try:
                    a = np.ctypeslib.as_array(words, shape=(n_words,))
                    a[:] = fn(a.copy())
                    return 0
                except BaseException as e:  # noqa: BLE001 -- reported to the prover as a failed exchange
                    errs.append(e)
                    return -1

            xch = HrExchange(HrExchange._fields_[0][1](cb), None)
        rc = self.L.vx_header_range_prove_ex(self.h, headers_buf.h, stride, _ptr(sizes), sizes.size, max_headers, trusted_block, _ptr(th),
                                              target_block, C.byref(just.struct) if just is not None else None, C.byref(cfg), n_segments, idx, n_shards,
                                              C.byref(xch) if xch is not None else None, _ptr(out96), _ptr(out), out.size, C.byref(need))
        if shard is not None and errs:
            raise errs[0]
        self._ck(rc)
        return out96.tobytes(), out[: need.value]

    def verify_epoch_end_header(self, header_buf, num_authorities, start_position, new_pubkeys, max_authorities=300):
        pk = np.ascontiguousarray(np.frombuffer(b"".join(new_pubkeys), dtype=np.uint8)) if new_pubkeys else np.zeros(32, dtype=np.uint8)
        self._ck(self.L.vx_verify_epoch_end_header(self.h, header_buf.h, num_authorities, start_position, _ptr(pk), max_authorities))

    def rotate_prove(self, header_buf, header_size, epoch_end_block_number, num_authorities, start_position, new_pubkeys, just, cfg=None, out=None):
        """RotateCircuit::prove -> (32-byte new authority set hash, proof blob words)."""
        cfg = cfg or self.stark_config()
        pk = np.ascontiguousarray(np.frombuffer(b"".join(new_pubkeys), dtype=np.uint8))
        need = C.c_size_t(0)
        self._ck(self.L.vx_rotate_proof_bound(C.byref(cfg), max(1, (header_size + 127) // 128), max(1, just.struct.num_authorities), max(1, num_authorities), C.byref(need)))
        if out is None or out.size < need.value:
            out = np.empty(need.value, dtype=np.uint64)
        out32 = np.zeros(32, dtype=np.uint8)
        self._ck(self.L.vx_rotate_prove(self.h, header_buf.h, header_size, epoch_end_block_number, num_authorities, start_position, _ptr(pk),
                                        C.byref(just.struct), C.byref(cfg), _ptr(out32), _ptr(out), out.size, C.byref(need)))
        return out32.tobytes(), out[: need.value]

    def partial_products(self, wires_buf, sigmas_buf, log_n, n_routed, k_is, beta, gamma, chunk=8, out=None):
        """K9: Z and the partial products of the permutation argument -> Buffer [ceil(n_routed / chunk)][2^log_n] (column 0 = Z)."""
        m = (n_routed + chunk - 1) // chunk
        out = out or self.alloc(m << log_n)
        k = np.ascontiguousarray(k_is, dtype=np.uint64)
        self._ck(self.L.vx_partial_products(self.h, wires_buf.h, sigmas_buf.h, log_n, n_routed, _ptr(k), int(beta), int(gamma), chunk, out.h))
        return out

    def quotient_eval(self, air_id, rate_bits, trace_lde_buf, log_n, alphas, public_inputs, challenges=None, aux_public=None, out=None):
        """-> [2][N] quotient values on the coset for the two challenges.  With challenges / aux_public (both, possibly empty) the
        buffer holds the main columns then the auxiliary ones and any AIR is evaluated (vx_quotient_eval_aux).
        out: a caller's Buffer of at least 2 N words (the values go to its start; it is not freed)."""
        N = 1 << (log_n + rate_bits)
        own = out is None
        out = out or self.alloc(2 * N)
        al = np.ascontiguousarray(alphas, dtype=np.uint64)
        pub = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if challenges is None and aux_public is None:
            self._ck(self.L.vx_quotient_eval(self.h, air_id, rate_bits, trace_lde_buf.h, log_n, _ptr(al), _ptr(pub) if pub.size else None, pub.size, out.h))
        else:
            ch = np.ascontiguousarray(() if challenges is None else challenges, dtype=np.uint64)
            ap = np.ascontiguousarray(() if aux_public is None else aux_public, dtype=np.uint64)
            self._ck(self.L.vx_quotient_eval_aux(self.h, air_id, rate_bits, trace_lde_buf.h, log_n, _ptr(al), _ptr(pub) if pub.size else None, pub.size,
                                                 _ptr(ch) if ch.size else None, ch.size, _ptr(ap) if ap.size else None, ap.size, out.h))
        v = out.download(2 * N).reshape(2, N)
        if own:
            out.free()
        return v

    def gather_proofs(self, nccl_comm, world, blob_words):
        """All-gather equal-length proof blobs over RCCL (nccl_comm: a raw ncclComm_t as an integer / c_void_p)."""
        mine = np.ascontiguousarray(blob_words, dtype=np.uint64)
        out = np.empty(world * mine.size, dtype=np.uint64)
        self._ck(self.L.vx_gather_proofs(self.h, C.c_void_p(nccl_comm), world, _ptr(mine), mine.size, _ptr(out)))
        return out.reshape(world, mine.size)

    # K8 / statement
    def blake2b_256_batch(self, msgs_buf, stride, sizes):
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        out = np.empty((sizes.size, 32), dtype=np.uint8)
        self._ck(self.L.vx_blake2b_256_batch(self.h, msgs_buf.h, stride, _ptr(sizes), sizes.size, _ptr(out)))
        return out

    def sha256_pairs(self, pairs):
        p = np.ascontiguousarray(pairs, dtype=np.uint8).reshape(-1, 64)
        out = np.empty((p.shape[0], 32), dtype=np.uint8)
        self._ck(self.L.vx_sha256_pairs(self.h, _ptr(p), p.shape[0], _ptr(out)))
        return out

    def blake_chain_trace(self, headers_buf, stride, sizes, trusted_hash, first_block_number, log_n, trace_buf=None, tree_size=0, window=(0, 0), leaf_offset=0):
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        th = np.frombuffer(bytes(trusted_hash), dtype=np.uint8).copy()
        trace_buf = trace_buf or self.alloc(VX_BLAKE_AIR_COLS << log_n)
        pub = np.zeros(20, dtype=np.uint64)
        dig = np.zeros((sizes.size, 32), dtype=np.uint8)
        self._ck(self.L.vx_blake_chain_trace(self.h, headers_buf.h, stride, _ptr(sizes), sizes.size, _ptr(th), first_block_number, tree_size, window[0] if window[1] else leaf_offset, window[1], log_n,
                                             trace_buf.h, _ptr(pub), _ptr(dig)))
        return trace_buf, pub, dig

    def sha_chain_trace(self, pubkeys, log_n, trace_buf=None, signed=None, bus_on=0):
        """ShaChainAir trace -> (Buffer [414][2^log_n], the 10 public inputs, the commitment).  signed: the flags of the
        authorities whose keys go to the EdDSA table over the bus (bus_on)."""
        pk = np.ascontiguousarray(np.frombuffer(b"".join(pubkeys), dtype=np.uint8))
        trace_buf = trace_buf or self.alloc(VX_SHA_AIR_COLS << log_n)
        pub = np.zeros(10, dtype=np.uint64)
        com = np.zeros(32, dtype=np.uint8)
        sg = None if signed is None else np.ascontiguousarray(signed, dtype=np.uint8)
        self._ck(self.L.vx_sha_chain_trace(self.h, _ptr(pk), pk.size // 32, None if sg is None else _ptr(sg), bus_on, log_n, trace_buf.h, _ptr(pub), _ptr(com)))
        return trace_buf, pub, com.tobytes()

    def ed_trace(self, pubkeys, sigs, msg, signed, log_n, bus_on=0, trace_buf=None):
        """EdAir trace (the curve half of the conditional EdDSA verifications) -> (Buffer [838][2^log_n], public inputs)."""
        n = len(pubkeys)
        pk = np.ascontiguousarray(np.frombuffer(b"".join(pubkeys), dtype=np.uint8)) if n else None
        sg = np.ascontiguousarray(np.frombuffer(b"".join(sigs), dtype=np.uint8)) if n else None
        en = np.ascontiguousarray(signed, dtype=np.uint8) if n else None
        m = np.frombuffer(bytes(msg), dtype=np.uint8).copy()
        trace_buf = trace_buf or self.alloc(VX_ED_AIR_COLS << log_n)
        pub = np.zeros(2, dtype=np.uint64)
        self._ck(self.L.vx_ed_trace(self.h, _ptr(pk) if n else None, _ptr(sg) if n else None, _ptr(m), m.size, _ptr(en) if n else None, n, log_n, bus_on, trace_buf.h, _ptr(pub)))
        return trace_buf, pub

    def sha512_trace(self, pubkeys, sigs, msg, signed, log_n, bus_on=0, trace_buf=None):
        """Sha512Air trace (H = SHA-512(R || A || msg) per signed slot) -> (Buffer [801][2^log_n], public inputs)."""
        n = len(pubkeys)
        pk = np.ascontiguousarray(np.frombuffer(b"".join(pubkeys), dtype=np.uint8)) if n else None
        sg = np.ascontiguousarray(np.frombuffer(b"".join(sigs), dtype=np.uint8)) if n else None
        en = np.ascontiguousarray(signed, dtype=np.uint8) if n else None
        m = np.frombuffer(bytes(msg), dtype=np.uint8).copy()
        trace_buf = trace_buf or self.alloc(VX_SHA512_AIR_COLS << log_n)
        pub = np.zeros(15, dtype=np.uint64)
        self._ck(self.L.vx_sha512_trace(self.h, _ptr(pk) if n else None, _ptr(sg) if n else None, _ptr(m), m.size, _ptr(en) if n else None, n, log_n, bus_on, trace_buf.h, _ptr(pub)))
        return trace_buf, pub

    def epoch_end_trace(self, header_buf, start_position, num_authorities, bus_on=0, trace_buf=None):
        """EpochEndAir trace of the ScheduledChange log behind start_position -> (Buffer [52][512], public inputs, window length)."""
        trace_buf = trace_buf or self.alloc(VX_EPOCH_END_AIR_COLS << 9)
        pub = np.zeros(10, dtype=np.uint64)
        wlen = C.c_uint32(0)
        self._ck(self.L.vx_epoch_end_trace(self.h, header_buf.h, start_position, num_authorities, bus_on, trace_buf.h, _ptr(pub), C.byref(wlen)))
        return trace_buf, pub, wlen.value

    def ed25519_verify_batch(self, pubkeys, sigs, msg, enabled=None):
        pk = np.ascontiguousarray(np.frombuffer(b"".join(pubkeys), dtype=np.uint8))
        sg = np.ascontiguousarray(np.frombuffer(b"".join(sigs), dtype=np.uint8))
        n = pk.size // 32
        en = np.ones(n, dtype=np.uint8) if enabled is None else np.ascontiguousarray(enabled, dtype=np.uint8)
        m = np.frombuffer(bytes(msg), dtype=np.uint8).copy()
        ok = np.zeros(n, dtype=np.uint8)
        self._ck(self.L.vx_ed25519_verify_batch(self.h, _ptr(pk), _ptr(sg), _ptr(m), m.size, _ptr(en), n, _ptr(ok)))
        return ok

    def verify_simple_justification(self, block_number, block_hash, set_id, set_hash, just, max_authorities=None):
        """`just`: synth.Justification-like object (precommit, pubkeys, signatures, signed, num_authorities)."""
        n = len(just.pubkeys)
        mx = n if max_authorities is None else max_authorities
        pk = np.zeros(32 * mx, dtype=np.uint8)
        sg = np.zeros(64 * mx, dtype=np.uint8)
        en = np.zeros(mx, dtype=np.uint8)
        pk[: 32 * n] = np.frombuffer(b"".join(just.pubkeys), dtype=np.uint8)
        sg[: 64 * n] = np.frombuffer(b"".join(just.signatures), dtype=np.uint8)
        en[:n] = np.array(just.signed, dtype=np.uint8)
        bh = np.frombuffer(bytes(block_hash), dtype=np.uint8).copy()
        sh = np.frombuffer(bytes(set_hash), dtype=np.uint8).copy()
        pc = np.frombuffer(bytes(just.precommit), dtype=np.uint8).copy()
        self._ck(self.L.vx_verify_simple_justification(self.h, block_number, _ptr(bh), set_id, _ptr(sh), _ptr(pc), _ptr(pk), _ptr(sg), _ptr(en),
                                                       just.num_authorities, mx))

    def decode_headers(self, headers_buf, stride, sizes):
        """decode_header of every header -> dict(number, mode, ok, parent, state_root, data_root) of numpy arrays."""
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        n = sizes.size
        num, mode, ok = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        par, sr, dr = (np.zeros((n, 32), dtype=np.uint8) for _ in range(3))
        self._ck(self.L.vx_decode_header_batch(self.h, headers_buf.h, stride, _ptr(sizes), n, _ptr(num), _ptr(mode), _ptr(ok), _ptr(par), _ptr(sr), _ptr(dr)))
        return dict(number=num, mode=mode, ok=ok, parent=par, state_root=sr, data_root=dr)

    def decode_precommits(self, precommits):
        pc = np.ascontiguousarray(np.frombuffer(b"".join(bytes(p) for p in precommits), dtype=np.uint8))
        n = pc.size // 53
        ok, h = np.zeros(n, dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
        bn, rnd, sid = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        self._ck(self.L.vx_decode_precommit_batch(self.h, _ptr(pc), n, _ptr(ok), _ptr(h), _ptr(bn), _ptr(rnd), _ptr(sid)))
        return dict(ok=ok, hash=h, block_number=bn, round=rnd, set_id=sid)

    def verify_subchain(self, headers_buf, stride, sizes, max_headers, trusted_block, trusted_hash, target_block):
        sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        th = np.frombuffer(bytes(trusted_hash), dtype=np.uint8).copy()
        out = np.zeros(96, dtype=np.uint8)
        self._ck(self.L.vx_verify_subchain(self.h, headers_buf.h, stride, _ptr(sizes), sizes.size, max_headers, trusted_block, _ptr(th), target_block, _ptr(out)))
        return out.tobytes()
