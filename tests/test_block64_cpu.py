"""Host logic of the 64-token-block path (no GPU): LayoutSpec at block 64 against the numbers of the reference's own runs
(the op_b64_* fixtures' meta and array shapes), and the refusals that stay."""
import ast
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["b64_wan_pad_1450", "b64_hunyuan_1280", "b64_flux_1536", "b64_cogvideo_1058", "b64_wan_d64_1100",
         "b64_b2_hunyuan_1280", "b64_big_wan_16640"]


def _meta(name):
    z = np.load(os.path.join(GOLDEN, f"op_{name}.npz"))
    return ast.literal_eval(str(z["meta"])), tuple(z["one_hot_shape"]), z["probs"].shape


def _spec(meta):
    from rectified_spaattn_amd import _core
    var, S = meta["variant"], meta["S"]
    if var == "hunyuan":
        return _core.LayoutSpec.hunyuan(S, meta["num_true"], block=64)
    if var == "flux":
        return _core.LayoutSpec.flux(S, meta["text_length"], block=64)
    if var == "cogvideo":
        return _core.LayoutSpec.cogvideo(S, meta["text_length"], block=64)
    return _core.LayoutSpec.wan(S, meta.get("ffb", 0), block=64)


@pytest.mark.parametrize("name", CASES)
def test_layout_block64_matches_reference_shapes(name):
    meta, oh_shape, pr_shape = _meta(name)
    assert meta["block"] == 64 and meta["margin"] >= 1e-5
    spec = _spec(meta)
    assert spec.block == 64
    assert (spec.NBv, spec.NB_total) == oh_shape[-2:] == (meta["NBv"], meta["NB_total"])
    assert spec.L == pr_shape[-1] == meta["L"]
    assert spec.NB_total == (meta["S"] + 63) // 64
    if meta["variant"] == "hunyuan":
        assert spec.NB_total - spec.NBv == 256 // 64
        assert spec.text_end_block == (meta["num_true"] + 63) // 64
    if meta["variant"] == "flux":
        assert spec.NB_total - spec.NBv == meta["text_length"] // 64
    c = spec.to_c_ex(meta["B"], meta["H"], meta["D"], __import__("torch").bfloat16)
    assert c.block == 64 and c.base.NBv == spec.NBv and list(c.reserved) == [0, 0, 0]


def test_cogvideo_layout_valid_only_at_block64():
    """832 visual tokens + 226 text: a multiple of 64, not of 128."""
    from rectified_spaattn_amd import _core
    spec = _core.LayoutSpec.cogvideo(1058, 226, block=64)
    assert spec.NBv * 64 == 832
    with pytest.raises(ValueError):
        _core.LayoutSpec.cogvideo(1058, 226)


def test_block128_layout_unchanged():
    from rectified_spaattn_amd import _core
    for a, b in ((_core.LayoutSpec.hunyuan(1280, 1224), _core.LayoutSpec.hunyuan(1280, 1224, block=128)),
                 (_core.LayoutSpec.wan(1450, 2), _core.LayoutSpec.wan(1450, 2, block=128)),
                 (_core.LayoutSpec.flux(1536, 512), _core.LayoutSpec.flux(1536, 512, block=128))):
        assert a == b and a.block == 128


def test_block_refusals():
    from rectified_spaattn_amd import _core, _operator
    for bad in (32, 96, 256):
        with pytest.raises(NotImplementedError):
            _core.LayoutSpec.wan(1024, 0, block=bad)
    for bm, bn in ((64, 128), (128, 64), (32, 32), (256, 256)):
        with pytest.raises(NotImplementedError):
            _operator._check_blocks(bm, bn)
    assert _operator._check_blocks(64, 64) == 64 and _operator._check_blocks(128, 128) == 128


def test_abi_layout_ex_and_header_version():
    """rsa_layout_ex = rsa_layout + block + 3 reserved words; the ctypes mirror follows header 0.6.1, whose structs keep
    their 0.6.0 sizes (a 0.6.0 host passes rsa_abi_check)."""
    from rectified_spaattn_amd import _lib
    assert ctypes.sizeof(_lib.RsaLayoutEx) == ctypes.sizeof(_lib.RsaLayout) + 16
    assert _lib.HEADER_VERSION == 601 and _lib.HEADER_VERSION // 100 == 600 // 100
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "rsa.h")).read()
    assert "#define RSA_HEADER_VERSION 601" in hdr
    for fn in ("rsa_buffer_bytes_ex", "rsa_block_sparse_fwd_ex", "rsa_rectified_attention_ex", "rsa_estimate_pr_gain_ex"):
        assert fn in hdr and fn in _lib.EXPORTED


def test_library_abi_check_accepts_060_host():
    """Against the built library (when present): a host compiled against the 0.6.0 header still passes the check, and the
    _ex entry points refuse a block size other than 64 / 128 before touching anything."""
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    L = _lib.lib()
    assert L.rsa_version() == 601
    assert L.rsa_abi_check(600, ctypes.sizeof(_lib.RsaBuffers), ctypes.sizeof(_lib.RsaLayout)) == 0
    lay = _lib.RsaLayoutEx(_lib.RsaLayout(1, 1, 128, 1024, 32, 32, 0, 1024, 1024, 32, 0, 0, 1024, 0), 32)
    sizes = (ctypes.c_size_t * _lib.NUM_BUFFERS)()
    total = ctypes.c_size_t()
    assert L.rsa_buffer_bytes_ex(ctypes.byref(lay), ctypes.byref(sizes), ctypes.byref(total)) == -2
    lay.block = 64
    lay.base.NB_total = 16     # (1024 tokens are 16 blocks of 64, not 32)
    lay.base.NBv = 16
    lay.base.text_end_block = 16
    assert L.rsa_buffer_bytes_ex(ctypes.byref(lay), ctypes.byref(sizes), ctypes.byref(total)) == 0
    lay.base.NB_total = 8      # the 128-token count is inconsistent at block 64
    assert L.rsa_buffer_bytes_ex(ctypes.byref(lay), ctypes.byref(sizes), ctypes.byref(total)) == -1


def test_library_abi_check_refuses_other_struct_sizes():
    """rsa_abi_check still compares BOTH struct sizes and the major.minor of the header."""
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    L = _lib.lib()
    nb, nl = ctypes.sizeof(_lib.RsaBuffers), ctypes.sizeof(_lib.RsaLayout)
    assert L.rsa_abi_check(601, nb, nl) == 0
    assert L.rsa_abi_check(600, nb + 8, nl) == -2
    assert L.rsa_abi_check(600, nb - 8, nl) == -2
    assert L.rsa_abi_check(600, nb, nl + 4) == -2
    assert L.rsa_abi_check(500, nb, nl) == -2


def test_layout_ex_reserved_words_must_be_zero():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    L = _lib.lib()
    lay = _lib.RsaLayoutEx(_lib.RsaLayout(1, 1, 128, 1024, 16, 16, 0, 1024, 1024, 16, 0, 0, 1024, 0), 64)
    sizes = (ctypes.c_size_t * _lib.NUM_BUFFERS)()
    total = ctypes.c_size_t()
    assert L.rsa_buffer_bytes_ex(ctypes.byref(lay), ctypes.byref(sizes), ctypes.byref(total)) == 0
    for i in range(3):
        lay.reserved[i] = 1
        assert L.rsa_buffer_bytes_ex(ctypes.byref(lay), ctypes.byref(sizes), ctypes.byref(total)) == -1
        assert L.rsa_carve_workspace_ex(ctypes.byref(lay), None, 0, None) == -1
        lay.reserved[i] = 0
