"""Block-sparse attention over caller-supplied block masks: the refusals, the host-side argument checks of the new C-ABI entries
(no launch happens: every call below fails its checks first) and the reference's import paths.  Runs without a GPU."""
import ctypes
import os

import pytest
import torch

VARIANTS = ("rectified_hunyuan_attn", "rectified_flux_attn", "rectified_wan21_attn", "rectified_cogvideo_attn")


def _qkv(B=1, H=2, Sq=256, Sk=256, D=64, dt=torch.bfloat16):
    return (torch.zeros(B, H, Sq, D, dtype=dt), torch.zeros(B, H, Sk, D, dtype=dt), torch.zeros(B, H, Sk, D, dtype=dt))


@pytest.mark.parametrize("variant", VARIANTS)
def test_reference_names_import_through_the_alias_package(variant):
    import importlib
    import inspect
    mod = importlib.import_module("rectified_spaattn." + variant)
    assert mod is importlib.import_module("rectified_spaattn_amd." + variant)
    from_ref = {}
    exec(f"from rectified_spaattn.{variant} import _triton_block_sparse_attention_onehot, "
         f"_build_block_index_with_importance_optimized", from_ref)
    sig = inspect.signature(from_ref["_triton_block_sparse_attention_onehot"])
    assert list(sig.parameters) == ["q", "k", "v", "seqlens", "block_mask", "sm_scale", "block_size_M", "block_size_N"]
    sig = inspect.signature(from_ref["_build_block_index_with_importance_optimized"])
    last = "first_frame_blocks" if variant == "rectified_wan21_attn" else "attenable"
    assert list(sig.parameters) == ["query", "key", "top_k", "block_size_M", "block_size_N", "text_start_block",
                                    "text_end_block", "num_blocks", "prob_threshold", "block_neighbor_list", last]


def test_package_exports_block_sparse_attention():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import block_sparse
    assert callable(rectified_spaattn_amd.block_sparse_attention)
    assert callable(block_sparse.block_sparse_attention)


@pytest.mark.parametrize("bs", [32, 96, 256])
def test_other_block_sizes_are_refused(bs):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv()
    m = torch.ones(1, 1, 2, 2, dtype=torch.bool)
    with pytest.raises(NotImplementedError):
        block_sparse_attention(q, k, v, m, block_size=bs)


def test_unequal_block_sizes_are_refused():
    from rectified_spaattn_amd.rectified_hunyuan_attn import (_build_block_index_with_importance_optimized,
                                                              _triton_block_sparse_attention_onehot)
    q, k, v = _qkv()
    m = torch.ones(1, 2, 2, 2, dtype=torch.bool)
    with pytest.raises(NotImplementedError):
        _triton_block_sparse_attention_onehot(q, k, v, torch.tensor([256]), m, 0.125, 128, 64)
    with pytest.raises(NotImplementedError):
        _build_block_index_with_importance_optimized(q, k, 1, 64, 128)


@pytest.mark.parametrize("case", ["mask_rows", "mask_cols", "mask_batch", "mask_heads", "mask_dtype", "mask_dim", "kv_shape",
                                  "v_shape", "dtype_mix", "fp32", "head_dim", "kv_len_range", "kv_len_count"])
def test_shape_and_dtype_mismatches_raise_value_error(case):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv(B=2, H=2, Sq=300, Sk=500)       # NQ = 3, NK <= 4 at block 128
    m = torch.ones(2, 2, 3, 4, dtype=torch.bool)
    kw = {}
    if case == "mask_rows":
        m = torch.ones(2, 2, 2, 4, dtype=torch.bool)
    elif case == "mask_cols":
        m = torch.ones(2, 2, 3, 5, dtype=torch.bool)
    elif case == "mask_batch":
        m = torch.ones(3, 2, 3, 4, dtype=torch.bool)
    elif case == "mask_heads":
        m = torch.ones(2, 3, 3, 4, dtype=torch.bool)
    elif case == "mask_dtype":
        m = torch.ones(2, 2, 3, 4, dtype=torch.float32)
    elif case == "mask_dim":
        m = torch.ones(2, 3, 4, dtype=torch.bool)
    elif case == "kv_shape":
        k = torch.zeros(2, 2, 500, 128, dtype=torch.bfloat16)
    elif case == "v_shape":
        v = torch.zeros(2, 2, 400, 64, dtype=torch.bfloat16)
    elif case == "dtype_mix":
        v = v.half()
    elif case == "fp32":
        q, k, v = q.float(), k.float(), v.float()
    elif case == "head_dim":
        q, k, v = _qkv(B=2, H=2, Sq=300, Sk=500, D=96)
    elif case == "kv_len_range":
        kw = dict(kv_len=[10, 501])
    elif case == "kv_len_count":
        kw = dict(kv_len=[10, 20, 30])
    with pytest.raises(ValueError):
        block_sparse_attention(q, k, v, m, **kw)


def test_more_key_blocks_than_the_kernel_walks_raise_value_error():
    from rectified_spaattn_amd import block_sparse, block_sparse_attention
    q, k, v = _qkv(Sq=64, Sk=8193 * 64)
    with pytest.raises(ValueError):
        block_sparse_attention(q, k, v, torch.ones(1, 1, 1, 8193, dtype=torch.bool), block_size=64)
    with pytest.raises(ValueError):
        block_sparse.block_mask_to_lists(torch.ones(1, 1, 1, 8193, dtype=torch.bool), 1, 1)


def test_cpu_tensors_raise_rsa_error():
    from rectified_spaattn_amd import _lib, block_sparse_attention
    q, k, v = _qkv()
    with pytest.raises(_lib.RsaError):
        block_sparse_attention(q, k, v, torch.ones(1, 2, 2, 2, dtype=torch.bool))
    from rectified_spaattn_amd.rectified_flux_attn import _build_block_index_with_importance_optimized
    with pytest.raises(_lib.RsaError):
        _build_block_index_with_importance_optimized(q, k, 1, attenable=0)


def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_cabi_mask_list_entries_check_their_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS = -1, -2
    p = ctypes.c_void_p(256)           # never dereferenced: every call below fails its host checks
    good = (1, 2, 3, 40, p, 0, 0, 40, p, p, p, None)
    assert L.rsa_block_mask_to_lists(*good[:4], None, *good[5:]) == BAD                  # no mask
    assert L.rsa_block_mask_to_lists(*good[:8], None, p, p, None) == BAD                  # no bitmask
    assert L.rsa_block_mask_to_lists(*good[:9], None, p, None) == BAD                     # no cols
    assert L.rsa_block_mask_to_lists(*good[:10], None, None) == BAD                       # no counts
    assert L.rsa_block_mask_to_lists(0, 2, 3, 40, *good[4:]) == BAD
    assert L.rsa_block_mask_to_lists(1, 2, 0, 40, *good[4:]) == BAD
    assert L.rsa_block_mask_to_lists(1, 2, 3, 0, *good[4:]) == BAD
    assert L.rsa_block_mask_to_lists(1, 2, 3, 8193, *good[4:]) == UNS                     # beyond K5's key-block limit
    assert L.rsa_block_mask_to_lists(1, 2, 3, 40, p, -1, 0, 40, p, p, p, None) == BAD     # negative stride
    assert L.rsa_block_mask_to_lists(1, 2, 3, 40, p, 0, 0, 40, ctypes.c_void_p(258), p, p, None) == BAD   # misaligned
    assert L.rsa_lists_to_block_mask(1, 2, 3, 40, None, p, None) == BAD
    assert L.rsa_lists_to_block_mask(1, 2, 3, 40, p, None, None) == BAD
    assert L.rsa_lists_to_block_mask(1, 2, 3, 9000, p, p, None) == UNS
    assert L.rsa_lists_to_block_mask(1, 0, 3, 40, p, p, None) == BAD


def test_cabi_plain_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 8 * 128 * 300, 128 * 300, 128)
    o = _lib.RsaOut4(4096, 8 * 128 * 300, 128, 8 * 128)
    p = ctypes.c_void_p(4096)

    def call(B=1, H=8, Sq=300, Sk=300, D=128, dt=0, blk=128, NQ=3, NK=3, kvv=300, sc=0.088, q=t, cols=p, counts=p, tp=None,
             tpb=0, out=o):
        return L.rsa_block_sparse_plain_fwd(B, H, Sq, Sk, D, dt, blk, NQ, NK, kvv, sc, q, t, t, cols, counts, tp, tpb, out, None)

    assert call(blk=96) == UNS
    assert call(D=96) == UNS
    assert call(dt=7) == UNS
    assert call(B=0) == BAD
    assert call(Sq=0) == BAD
    assert call(NQ=2) == BAD                       # NQ must be ceil(Sq / block)
    assert call(NK=4) == BAD                       # more key blocks than Sk has
    assert call(NK=0) == BAD
    assert call(kvv=0) == BAD
    assert call(kvv=301) == BAD
    assert call(sc=float("inf")) == BAD            # (a finite scale of either sign is accepted)
    assert call(sc=float("-inf")) == BAD
    assert call(sc=float("nan")) == BAD
    assert call(cols=None) == BAD
    assert call(counts=None) == BAD
    assert call(tp=p, tpb=0) == WS                 # a partial buffer without its capacity
    assert call(q=_lib.RsaTensor4(4100, 8 * 128 * 300, 128 * 300, 128)) == BAD    # misaligned q
    assert call(out=_lib.RsaOut4(4096, 8 * 128 * 300, 128, 1022)) == BAD         # output rows not 8-byte strided
    assert call(Sk=9000 * 128, NK=8193, kvv=9000 * 128) == UNS
