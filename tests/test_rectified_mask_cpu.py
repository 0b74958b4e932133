"""Rectified attention over a caller's block mask, without a GPU: the public keyword of every variant, the refusals that need no
device, and the host-side argument checks of the C entries (rsa_select_from_mask, rsa_rectified_attention_masked, _ex)."""
import ctypes
import inspect

import pytest
import torch

VARIANTS = ["rectified_hunyuan_attn", "rectified_flux_attn", "rectified_cogvideo_attn", "rectified_wan21_attn"]


@pytest.mark.parametrize("mod_name", VARIANTS)
def test_every_variant_takes_block_mask_as_its_last_keyword(mod_name):
    import importlib
    mod = importlib.import_module("rectified_spaattn_amd." + mod_name)
    for fn in (mod.block_sparse_attention_combined, mod.rectified_block_sparse_attention):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "block_mask" and params[-1].default is None, (mod_name, fn.__name__)


def test_wan22_re_exports_the_wan21_function():
    from rectified_spaattn_amd import rectified_wan21_attn, rectified_wan22_attn
    assert rectified_wan22_attn.rectified_block_sparse_attention is rectified_wan21_attn.rectified_block_sparse_attention
    assert "block_mask" in inspect.signature(rectified_wan22_attn.rectified_block_sparse_attention).parameters


def _hunyuan(B=2, H=3, S=1280, num_true=1224, D=128):
    from rectified_spaattn_amd.rectified_hunyuan_attn import rectified_block_sparse_attention
    q = torch.zeros(B, H, S, D, dtype=torch.bfloat16)
    cu = [0, num_true, S]
    return (lambda m, **kw: rectified_block_sparse_attention(q, q, q, None, 3, cu_seqlens_q=cu, cu_seqlens_kv=cu, block_mask=m,
                                                             **kw))


@pytest.mark.parametrize("shape,dtype", [
    ((2, 3, 8, 9), torch.bool),         # one key block short
    ((2, 3, 9, 10), torch.bool),        # one query block too many
    ((3, 3, 8, 10), torch.bool),        # batch axis neither B nor 1
    ((2, 2, 8, 10), torch.uint8),       # head axis neither H nor 1
    ((3, 8, 10), torch.bool),           # not 4-d
    ((2, 3, 8, 10), torch.float32),     # not bool / uint8
    ((2, 3, 8, 10), torch.int32),
])
def test_malformed_masks_raise_value_error_naming_the_expected_shape(shape, dtype):
    call = _hunyuan()   # NBv = 8, NB_total = 10
    with pytest.raises(ValueError, match=r"\[2\|1, 3\|1, 8, 10\]"):
        call(torch.zeros(shape, dtype=dtype))


def test_neighbour_list_and_first_frame_blocks_are_refused_with_a_mask():
    from rectified_spaattn_amd.rectified_wan21_attn import rectified_block_sparse_attention as wan
    call = _hunyuan()
    m = torch.ones(1, 1, 8, 10, dtype=torch.bool)
    with pytest.raises(ValueError, match="OR the neighbour blocks into the mask"):
        call(m, block_neighbor_list=torch.ones(8, 8, dtype=torch.bool))
    q = torch.zeros(1, 2, 1024, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="OR the first-frame square into the mask"):
        wan(q, q, q, None, 3, first_frame_blocks=2, block_mask=torch.ones(1, 1, 8, 8, dtype=torch.bool))


def test_cpu_tensors_with_a_valid_mask_raise_rsa_error():
    from rectified_spaattn_amd._lib import RsaError
    from rectified_spaattn_amd.rectified_wan21_attn import rectified_block_sparse_attention as wan
    for D in (128, 32):   # (32: through the zero-padded path)
        q = torch.zeros(1, 2, 1024, D, dtype=torch.bfloat16)
        with pytest.raises(RsaError):
            wan(q, q, q, None, None, p_remain_rates=None, block_mask=torch.ones(1, 2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RsaError):
        _hunyuan()(torch.ones(2, 1, 8, 10, dtype=torch.bool))


# ---- the C entries: every refusal below returns before a launch (no GPU here) ---------------------------------------------
FAKE = 1 << 20          # a 256-aligned address the host checks accept and nothing dereferences


def _buffers(**nulls):
    from rectified_spaattn_amd import _lib
    ptrs = [None if n in nulls else FAKE for n in _lib.BUFFER_NAMES]
    return _lib.RsaBuffers(*ptrs, 1 << 30)


def _layout(spec, D=128):
    return spec.to_c(1, 2, D, torch.bfloat16)


def test_select_from_mask_refuses_null_pointers_and_bad_strides():
    from rectified_spaattn_amd import _core, _lib
    L = _lib.lib()
    lay = ctypes.byref(_layout(_core.LayoutSpec.hunyuan(1280, 1224)))
    ok = ctypes.byref(_buffers())
    assert L.rsa_select_from_mask(lay, None, 0, 0, 10, ok, None) == -1                       # NULL mask
    for name in ("scores", "unrel", "probs", "w", "R", "bitmask", "cols", "counts"):
        assert L.rsa_select_from_mask(lay, FAKE, 0, 0, 10, ctypes.byref(_buffers(**{name: 1})), None) == -1, name
    assert L.rsa_select_from_mask(lay, FAKE, 0, 0, 10, None, None) == -1                     # NULL rsa_buffers
    assert L.rsa_select_from_mask(lay, FAKE, 0, 0, 0, ok, None) == -1                        # query stride 0
    assert L.rsa_select_from_mask(lay, FAKE, -1, 0, 10, ok, None) == -1                      # negative strides
    assert L.rsa_select_from_mask(lay, FAKE, 0, -80, 10, ok, None) == -1
    assert L.rsa_select_from_mask(lay, FAKE, 0, 0, -10, ok, None) == -1
    assert L.rsa_select_from_mask(None, FAKE, 0, 0, 10, ok, None) == -1                      # NULL layout


def test_select_from_mask_refuses_what_select_mask_refuses_with_the_same_code():
    from rectified_spaattn_amd import _core, _lib
    L = _lib.lib()
    ok = ctypes.byref(_buffers())
    # (only layouts both refuse: an accepted one would launch on the fake buffers)
    for spec, D, want in [(_core.LayoutSpec.wan(8193 * 128), 128, -2),          # more than 8 192 key blocks
                          (_core.LayoutSpec.hunyuan(1280, 1224), 96, -2)]:       # head dim without a kernel
        lay = ctypes.byref(_layout(spec, D))
        assert L.rsa_select_mask(lay, None, 3, 0.3, ok, None) == want
        assert L.rsa_select_from_mask(lay, FAKE, 0, 0, spec.NB_total, ok, None) == want, (spec, D)
    bad = _layout(_core.LayoutSpec.hunyuan(1280, 1224))
    bad.NB_total = 11
    assert L.rsa_select_from_mask(ctypes.byref(bad), FAKE, 0, 0, 11, ok, None) == \
        L.rsa_select_mask(ctypes.byref(bad), None, 3, 0.3, ok, None) == -1


def test_ex_forms_check_the_block_and_the_reserved_words():
    from rectified_spaattn_amd import _core, _lib
    L = _lib.lib()
    ok = ctypes.byref(_buffers())
    spec = _core.LayoutSpec.hunyuan(1280, 1224, block=64)
    lx = spec.to_c_ex(1, 2, 128, torch.bfloat16)
    assert L.rsa_select_from_mask_ex(ctypes.byref(lx), None, 0, 0, spec.NB_total, ok, None) == -1
    assert L.rsa_select_from_mask_ex(ctypes.byref(lx), FAKE, 0, 0, 0, ok, None) == -1
    lx.reserved[1] = 7
    assert L.rsa_select_from_mask_ex(ctypes.byref(lx), FAKE, 0, 0, spec.NB_total, ok, None) == -1
    lx.reserved[1] = 0
    lx.block = 96
    assert L.rsa_select_from_mask_ex(ctypes.byref(lx), FAKE, 0, 0, spec.NB_total, ok, None) == -2


def test_one_call_forms_check_the_mask_before_the_first_launch():
    from rectified_spaattn_amd import _core, _lib
    from rectified_spaattn_amd._lib import RsaOut4, RsaTensor4
    L = _lib.lib()
    spec = _core.LayoutSpec.hunyuan(1280, 1224)
    t = RsaTensor4(FAKE, 1280 * 2 * 128, 1280 * 128, 128)
    o = RsaOut4(FAKE, 1280 * 2 * 128, 128, 2 * 128)
    for lay, fn in [(_layout(spec), L.rsa_rectified_attention_masked),
                    (spec.to_c_ex(1, 2, 128, torch.bfloat16), L.rsa_rectified_attention_masked_ex),
                    (_core.LayoutSpec.hunyuan(1280, 1224, block=64).to_c_ex(1, 2, 128, torch.bfloat16),
                     L.rsa_rectified_attention_masked_ex)]:
        lp = ctypes.byref(lay)
        assert fn(lp, t, t, t, None, 0, 0, 10, FAKE, 1 << 40, o, None) == -1          # NULL mask
        assert fn(lp, t, t, t, FAKE, 0, 0, 0, FAKE, 1 << 40, o, None) == -1           # query stride 0
        assert fn(lp, t, t, t, FAKE, -5, 0, 10, FAKE, 1 << 40, o, None) == -1         # negative stride
        assert fn(lp, t, t, t, FAKE, 0, 0, 10, FAKE, 1024, o, None) == -3             # workspace too small
        assert fn(lp, t, t, t, FAKE, 0, 0, 10, None, 1 << 40, o, None) == -1          # no workspace
