"""ctypes binding of librsa_hip.so (C-ABI declared in include/rsa.h).

The HIP library is the product: there is no CPU or PyTorch fallback for device tensors.  If the shared
object is missing or cannot be loaded this module raises, and every operator that needs it fails loudly.
"""
from __future__ import annotations

import ctypes
import os

# PyTorch-ROCm bundles its own HIP runtime (soname libamdhip64.so.7).  It must be loaded BEFORE librsa_hip.so so
# that the library binds to the same runtime instance that owns torch's device context and streams; loading
# the system copy first leaves torch without a device on the GPU box.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librsa_hip.so")

RSA_BF16, RSA_FP16 = 0, 1
BLOCK = 128
BLOCKS = (64, 128)     # block sizes the library serves (64 through the _ex entry points, rsa.h 0.6.1)
HEADER_VERSION = 601   # RSA_HEADER_VERSION of include/rsa.h this ctypes mirror follows (rsa_abi_check)
GQA_PAIR_DEFAULT = 0   # the library's default of the tuning key k5_gqa_pair (grouped-query calls: 0 = one walk per query head)


class RsaError(RuntimeError):
    pass


class RsaLayout(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "B", "H", "D", "S", "NB_total", "NBv", "n_txt", "kv_valid", "pool_valid", "text_end_block",
        "first_frame_blocks", "q_text_valid", "kv_text_valid", "dtype")]


class RsaLayoutEx(ctypes.Structure):
    _fields_ = [("base", RsaLayout), ("block", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class RsaTensor4(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("stride_b", ctypes.c_int64), ("stride_h", ctypes.c_int64),
                ("stride_s", ctypes.c_int64)]


class RsaOut4(ctypes.Structure):
    _fields_ = RsaTensor4._fields_


BUFFER_NAMES = ("qbar", "aq", "kbar", "ak", "vbar", "scores", "unrel", "probs", "w", "R", "comp", "bitmask",
                "cols", "counts", "tpart")
TEXT_SPLIT = 32
TAIL_PIECES = 512
NUM_BUFFERS = len(BUFFER_NAMES)


class RsaBuffers(ctypes.Structure):
    # the 15 buffers, then the capacity of the last one in bytes (rsa.h 0.5.0: a non-NULL tpart must declare it)
    _fields_ = [(n, ctypes.c_void_p) for n in BUFFER_NAMES] + [("tpart_bytes", ctypes.c_size_t)]


class RsaFp8Operands(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("q8", "k8", "v8t", "scales")]


# Every prototype of include/rsa.h as name: (restype, argtypes), in the header's order, one type per parameter and no counted
# runs: an entry reads against its prototype parameter by parameter.  lib() applies the table in one loop.  int -> i32,
# int64_t -> i64, uint64_t -> u64, size_t -> sz, float -> f32, double -> f64, const char* -> cstr, rsa_tensor4 / rsa_out4 by value
# -> T4 / O4, a pointer to a struct or to a host size_t / int / int64_t / void* -> P(its mirror), every other pointer -> vp.
# tests/test_abi_cpu.py holds the table to the header, types included: one int for an int64_t shifts every later argument.
P = ctypes.POINTER
i32, i64, u64, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
f32, f64, cstr, vp = ctypes.c_float, ctypes.c_double, ctypes.c_char_p, ctypes.c_void_p
T4, O4 = RsaTensor4, RsaOut4
PROTOTYPES = {
    "rsa_version": (i32, []),
    "rsa_abi_check": (i32, [i32, sz, sz]),
    "rsa_set_shard_invariant": (i32, [i32]),
    "rsa_buffer_bytes": (i32, [P(RsaLayout), P(sz * NUM_BUFFERS), P(sz)]),
    "rsa_carve_workspace": (i32, [P(RsaLayout), vp, sz, P(RsaBuffers)]),
    "rsa_pool_stats": (i32, [P(RsaLayout), T4, T4, T4, P(RsaBuffers), vp]),
    "rsa_pooled_scores": (i32, [P(RsaLayout), T4, P(RsaBuffers), vp]),
    "rsa_select_mask": (i32, [P(RsaLayout), vp, i32, f32, P(RsaBuffers), vp]),
    "rsa_compensation": (i32, [P(RsaLayout), P(RsaBuffers), vp]),
    "rsa_block_sparse_fwd": (i32, [P(RsaLayout), T4, T4, T4, P(RsaBuffers), O4, vp]),
    "rsa_rectified_attention": (i32, [P(RsaLayout), T4, T4, T4, vp, i32, f32, vp, sz, O4, vp]),
    "rsa_dense_fwd": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, i32, i32, O4, vp]),
    "rsa_dense_causal_fwd": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, i32, i32, O4, vp]),
    "rsa_dense_masked_fwd": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, vp, i32, i64, i64, i64, i64, i32, O4, vp]),
    "rsa_dense_dropout_fwd": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, vp, i32, i64, i64, i64, i64, i32, i32, f32, u64, O4,
                                    vp]),
    "rsa_buffer_bytes_ex": (i32, [P(RsaLayoutEx), P(sz * NUM_BUFFERS), P(sz)]),
    "rsa_carve_workspace_ex": (i32, [P(RsaLayoutEx), vp, sz, P(RsaBuffers)]),
    "rsa_pool_stats_ex": (i32, [P(RsaLayoutEx), T4, T4, T4, P(RsaBuffers), vp]),
    "rsa_pooled_scores_ex": (i32, [P(RsaLayoutEx), T4, P(RsaBuffers), vp]),
    "rsa_select_mask_ex": (i32, [P(RsaLayoutEx), vp, i32, f32, P(RsaBuffers), vp]),
    "rsa_compensation_ex": (i32, [P(RsaLayoutEx), P(RsaBuffers), vp]),
    "rsa_block_sparse_fwd_ex": (i32, [P(RsaLayoutEx), T4, T4, T4, P(RsaBuffers), O4, vp]),
    "rsa_rectified_attention_ex": (i32, [P(RsaLayoutEx), T4, T4, T4, vp, i32, f32, vp, sz, O4, vp]),
    "rsa_block_mask_to_lists": (i32, [i32, i32, i32, i32, vp, i64, i64, i64, vp, vp, vp, vp]),
    "rsa_lists_to_block_mask": (i32, [i32, i32, i32, i32, vp, vp, vp]),
    "rsa_block_sparse_plain_fwd": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f64, T4, T4, T4, vp, vp, vp, sz, O4,
                                         vp]),
    "rsa_block_sparse_ranged_fwd": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f64, T4, T4, T4, vp, vp, vp, vp, i64,
                                          vp, sz, O4, vp]),
    "rsa_block_sparse_gqa_fwd": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, f64, T4, T4, T4, vp, vp, vp,
                                       vp, i64, vp, sz, O4, vp]),
    "rsa_block_select_bytes": (i32, [i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_select": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, T4, vp, i32, i32, i32, i32, i32, vp,
                               sz, vp, vp, vp, vp, vp]),
    "rsa_block_sparse_decode_bytes": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_sparse_decode": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4, vp, i64,
                                      i32, vp, vp, i32, vp, sz, O4, vp, vp]),
    "rsa_pool_keys": (i32, [i32, i32, i32, i32, i32, i32, i32, T4, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp]),
    "rsa_block_select_pooled_bytes": (i32, [i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_select_pooled": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, vp, vp, i32, i32, i32, i32, i32, i32,
                                      vp, sz, vp, vp, vp, vp, vp]),
    "rsa_kv8_append": (i32, [i32, i32, i32, i32, i32, i32, i32, T4, T4, O4, O4, vp, i64, i32, vp, i32, vp, i32, vp, vp, vp]),
    "rsa_block_sparse_decode_kv8": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4, vp,
                                          i64, i32, vp, vp, i32, vp, sz, O4, vp, vp, vp, vp]),
    "rsa_pool_keys_kv8": (i32, [i32, i32, i32, i32, i32, i32, T4, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp, vp]),
    "rsa_block_select_p_bytes": (i32, [i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_select_p": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, T4, vp, i32, i32, i32, i32, i32, vp,
                                 sz, vp, vp, vp, vp, i32, f32, vp, vp]),
    "rsa_block_select_pooled_p_bytes": (i32, [i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_select_pooled_p": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, vp, vp, i32, i32, i32, i32, i32, i32,
                                        vp, sz, vp, vp, vp, vp, i32, f32, vp, vp]),
    "rsa_select_from_mask": (i32, [P(RsaLayout), vp, i64, i64, i64, P(RsaBuffers), vp]),
    "rsa_select_from_mask_ex": (i32, [P(RsaLayoutEx), vp, i64, i64, i64, P(RsaBuffers), vp]),
    "rsa_rectified_attention_masked": (i32, [P(RsaLayout), T4, T4, T4, vp, i64, i64, i64, vp, sz, O4, vp]),
    "rsa_rectified_attention_masked_ex": (i32, [P(RsaLayoutEx), T4, T4, T4, vp, i64, i64, i64, vp, sz, O4, vp]),
    "rsa_estimate_pr_gain": (i32, [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "rsa_estimate_pr_gain_ex": (i32, [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "rsa_gilbert_mapping": (i32, [i32, i32, i32, cstr, vp, vp]),
    "rsa_gilbert_block_neighbors": (i32, [i32, i32, i32, i32, cstr, vp]),
    "rsa_permute_tokens": (i32, [i32, i32, i32, vp, i64, i64, vp, vp, i64, i64, vp]),
    "rsa_qk_norm_rope": (i32, [i32, i32, i32, i32, i32, T4, vp, f32, i32, vp, vp, i32, O4, vp]),
    "rsa_qk_layernorm_rope": (i32, [i32, i32, i32, i32, i32, T4, vp, vp, f32, vp, vp, i32, O4, vp]),
    "rsa_norm_rope_heads": (i32, [i32, i32, i32, i32, i32, vp, i64, i64, vp, f32, i32, i32, vp, vp, O4, vp]),
    "rsa_fp8_operand_bytes": (i32, [P(RsaLayout), P(sz * 4), P(sz)]),
    "rsa_carve_fp8_operands": (i32, [P(RsaLayout), vp, sz, P(RsaFp8Operands)]),
    "rsa_quantize_fp8": (i32, [P(RsaLayout), T4, T4, T4, P(RsaFp8Operands), vp]),
    "rsa_pool_stats_fp8": (i32, [P(RsaLayout), T4, T4, T4, P(RsaBuffers), P(RsaFp8Operands), vp]),
    "rsa_block_sparse_fwd_fp8": (i32, [P(RsaLayout), P(RsaFp8Operands), P(RsaBuffers), O4, vp]),
    "rsa_block_sparse_fwd_fp8pv": (i32, [P(RsaLayout), T4, T4, P(RsaFp8Operands), P(RsaBuffers), O4, vp]),
    "rsa_rectified_attention_fp8": (i32, [P(RsaLayout), T4, T4, T4, vp, i32, f32, vp, sz, vp, sz, O4, vp]),
    "rsa_rectified_attention_fp8pv": (i32, [P(RsaLayout), T4, T4, T4, vp, i32, f32, vp, sz, vp, sz, O4, vp]),
    "rsa_rel_l1": (i32, [vp, vp, i64, i32, vp, vp, vp]),
    "rsa_dense_fp8_bytes": (i32, [i32, i32, i32, i32, i32, P(sz)]),
    "rsa_dense_fwd_fp8": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, i32, i32, vp, sz, O4, vp]),
    "rsa_dense_causal_fwd_fp8": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, i32, i32, vp, sz, O4, vp]),
    "rsa_dense_fwd_fp8pv": (i32, [i32, i32, i32, i32, i32, i32, T4, T4, T4, i32, i32, i32, vp, sz, O4, vp]),
    "rsa_comm_unique_id": (i32, [vp]),
    "rsa_comm_create": (i32, [i32, i32, vp, P(vp)]),
    "rsa_comm_destroy": (i32, [vp]),
    "rsa_comm_count": (i32, [vp, P(i32)]),
    "rsa_allgather_heads": (i32, [vp, i32, vp, vp, vp, i64, i64, vp]),
    "rsa_p2p_state_bytes": (i32, []),
    "rsa_p2p_state_alloc": (i32, [P(vp)]),
    "rsa_p2p_state_free": (i32, [vp]),
    "rsa_p2p_state_timeout": (i32, [vp, P(i32)]),
    "rsa_allgather_heads_p2p": (i32, [i32, i32, vp, P(vp), P(vp), i64, i64, vp]),
    "rsa_ipc_export": (i32, [vp, vp]),
    "rsa_ipc_open": (i32, [vp, i32, P(vp)]),
    "rsa_ipc_close": (i32, [vp]),
    "rsa_ipc_offset": (i32, [vp, P(i64)]),
    "rsa_set_tuning": (i32, [cstr, i32]),
    "rsa_status_string": (cstr, [i32]),
    "rsa_last_hip_error": (cstr, []),
    # the bounds cache and the selection from it: additive and found by symbol, in front of the packed ones
    "rsa_pool_key_bounds": (i32, [i32, i32, i32, i32, i32, i32, i32, T4, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp]),
    "rsa_pool_key_bounds_kv8": (i32, [i32, i32, i32, i32, i32, i32, T4, vp, i64, i32, vp, i32, vp, i32, i32, vp, vp, vp]),
    "rsa_block_select_bound_bytes": (i32, [i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_select_bound": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, vp, vp, i32, i32, i32, i32, i32, i32, vp,
                                     sz, vp, vp, vp, vp, i32, f32, vp, vp, vp]),
    "rsa_block_select_bound_packed": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, vp, vp, i32, i32, i32, i32,
                                            i32, i32, vp, sz, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp]),
    # the packed entries: additive and found by symbol, in front of the ragged ones for the same reason
    "rsa_block_sparse_extend_packed_bytes": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, P(sz), P(i64)]),
    "rsa_block_sparse_extend_packed": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4, vp,
                                             i64, i32, vp, vp, i32, vp, sz, O4, vp, vp, vp]),
    "rsa_block_sparse_extend_packed_kv8": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4,
                                                 vp, i64, i32, vp, vp, i32, vp, sz, O4, vp, vp, vp, vp, vp]),
    "rsa_block_select_pooled_packed": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, vp, vp, i32, i32, i32, i32,
                                             i32, i32, vp, sz, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp]),
    "rsa_kv8_append_packed": (i32, [i32, i32, i32, i32, i32, i32, i32, T4, T4, O4, O4, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp]),
    # the ragged entries: additive and found by symbol like the extend entries, which stay the table's last three
    "rsa_block_sparse_extend_ragged": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4, vp,
                                             i64, i32, vp, vp, i32, vp, sz, O4, vp, vp, vp]),
    "rsa_block_sparse_extend_ragged_kv8": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4,
                                                 vp, i64, i32, vp, vp, i32, vp, sz, O4, vp, vp, vp, vp, vp]),
    "rsa_block_select_ragged": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, T4, vp, i32, i32, i32, i32, i32,
                                      vp, sz, vp, vp, vp, vp, i32, f32, vp, vp, vp]),
    "rsa_block_select_pooled_ragged": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, T4, vp, vp, i32, i32, i32, i32, i32,
                                             i32, vp, sz, vp, vp, vp, vp, i32, f32, vp, vp, vp]),
    # the merge of attention partials: additive and found by symbol, in front of the extend entries as well
    "rsa_merge_partials": (i32, [i32, i32, i32, i32, i32, i32, P(T4), P(vp), P(i64), vp, O4, vp, i64, i64, i64, vp]),
    # the block-sparse backward: additive and found by symbol, in front of the extend entries too
    "rsa_block_sparse_bwd_bytes": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_sparse_bwd": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, f64, T4, T4, T4, T4, T4, vp,
                                   vp, vp, vp, vp, sz, O4, O4, O4, vp]),
    "rsa_block_sparse_extend_bytes": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, P(sz)]),
    "rsa_block_sparse_extend": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4, vp, i64,
                                      i32, vp, vp, i32, vp, sz, O4, vp, vp]),
    "rsa_block_sparse_extend_kv8": (i32, [i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, f64, T4, T4, T4, vp,
                                          i64, i32, vp, vp, i32, vp, sz, O4, vp, vp, vp, vp]),
}
EXPORTED = tuple(PROTOTYPES)

_lib = None


def lib():
    """Load librsa_hip.so once; raise RsaError if it is not there (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RsaError(f"{LIB_PATH} not found: the HIP extension is not built "
                       f"(python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path")
    L = ctypes.CDLL(LIB_PATH)
    for name in ("rsa_version", "rsa_abi_check"):
        getattr(L, name).restype, getattr(L, name).argtypes = PROTOTYPES[name]
    if L.rsa_abi_check(HEADER_VERSION, ctypes.sizeof(RsaBuffers), ctypes.sizeof(RsaLayout)) != 0:
        raise RsaError(f"{LIB_PATH} (version {L.rsa_version()}) was built from another include/rsa.h than this package's "
                       f"ctypes mirror (header {HEADER_VERSION}, rsa_buffers {ctypes.sizeof(RsaBuffers)} B): rebuild it")
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    # kernel-variant switches for A/B runs and the variant tests; rsa_set_tuning works only under RSA_TUNING=1
    for key in ("k5_tsplit", "k3_prefix", "k3_long", "k4_split", "k5_rows256", "k5_static", "k5_gsync", "k5_gsync_ratio", "k5_text_last", "k5_tail_split", "k5_gqa_pair"):
        val = os.environ.get("RSA_" + key.upper())
        if val is not None:
            check_rc = L.rsa_set_tuning(key.encode(), int(val))
            if check_rc != 0:
                raise RsaError(f"RSA_{key.upper()} is set but rsa_set_tuning refused it (export RSA_TUNING=1)")
    _lib = L
    return L


def check(status: int, what: str):
    """Status code -> the exception types the reference raises: bad head_dim / dtype are
    AssertionError there (hunyuan :119-121); everything else is a RuntimeError subclass."""
    if status == 0:
        return
    msg = f"{what}: {lib().rsa_status_string(status).decode()} (rsa_status {status})"
    if status == -4:
        msg += f": {lib().rsa_last_hip_error().decode()}"
    if status == -2:
        raise AssertionError(msg)
    raise RsaError(msg)
