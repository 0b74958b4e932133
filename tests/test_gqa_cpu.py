"""Grouped-query K/V heads of block_sparse_attention (k / v with Hkv < H heads) without a GPU: the Python refusals, the two small
rules the call is built on (which K/V head a query head reads; when two query heads can share a workgroup), and the new C entry's
presence and argument refusals (every call below fails its host checks: nothing is launched)."""
import ctypes
import os
import re

import pytest
import torch

ENTRY = "rsa_block_sparse_gqa_fwd"


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) ----------------------------------------
def _qkv(B=2, H=8, Hk=2, Hv=None, Sq=300, Sk=500, D=64, dt=torch.bfloat16):
    Hv = Hk if Hv is None else Hv
    return (torch.zeros(B, H, Sq, D, dtype=dt), torch.zeros(B, Hk, Sk, D, dtype=dt), torch.zeros(B, Hv, Sk, D, dtype=dt))


def _ones(heads, NQ=3, NK=4):
    return torch.ones(1, heads, NQ, NK, dtype=torch.bool)


@pytest.mark.parametrize("H,Hk", [(8, 3), (6, 4), (4, 8), (7, 2)])
def test_head_counts_that_do_not_divide_are_refused(H, Hk):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv(H=H, Hk=Hk)
    with pytest.raises(ValueError, match="Hkv"):
        block_sparse_attention(q, k, v, _ones(1))


@pytest.mark.parametrize("Hk,Hv", [(2, 4), (4, 2), (8, 1), (1, 8)])
def test_k_and_v_with_different_head_counts_are_refused(Hk, Hv):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv(Hk=Hk, Hv=Hv)
    with pytest.raises(ValueError, match="Hkv"):
        block_sparse_attention(q, k, v, _ones(1))


@pytest.mark.parametrize("heads", [4, 3, 16])
def test_a_mask_head_axis_outside_1_hkv_h_is_refused(heads):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv(H=8, Hk=2)
    with pytest.raises(ValueError, match="Hkv"):
        block_sparse_attention(q, k, v, _ones(heads))


@pytest.mark.parametrize("heads", [1, 2, 8])
@pytest.mark.parametrize("kw", [dict(), dict(causal=True), dict(block_size=64)], ids=["plain", "causal", "block64"])
def test_a_well_formed_grouped_call_on_cpu_tensors_reaches_the_device_check(heads, kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, block_sparse_attention
    q, k, v = _qkv(H=8, Hk=2)
    m = _ones(heads, 5, 8) if kw.get("block_size") == 64 else _ones(heads)
    with pytest.raises(_lib.RsaError):
        block_sparse_attention(q, k, v, m, **kw)


def test_ranges_stay_128_token_blocks_only():
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv()
    with pytest.raises(NotImplementedError, match="128"):
        block_sparse_attention(q, k, v, _ones(2, 5, 8), block_size=64, causal=True)


# ---- the two rules --------------------------------------------------------------------------------------------------------------
def test_head_map_is_repeat_interleave():
    from rectified_spaattn_amd.block_sparse import gqa_kv_head
    for H, Hkv in ((8, 1), (8, 2), (8, 4), (8, 8), (6, 2), (24, 12), (1, 1)):
        kv = torch.arange(Hkv).repeat_interleave(H // Hkv).tolist()
        assert [gqa_kv_head(h, H, Hkv) for h in range(H)] == kv
        if 1 < Hkv < H:     # (the other plausible map, h % Hkv, is a different one)
            assert kv != [h % Hkv for h in range(H)]
    for bad in ((0, 8, 3), (8, 8, 2), (-1, 8, 2), (0, 4, 8), (0, 8, 0)):
        with pytest.raises(ValueError, match="Hkv"):
            gqa_kv_head(*bad)


PAIR_TABLE = [  # (H, Hkv, Hl, block) -> two query heads per workgroup?
    ((8, 2, 2, 128), True),        # g = 4, the mask per K/V head
    ((8, 4, 4, 128), True),        # g = 2
    ((8, 4, 1, 128), True),        # one mask row for every head
    ((8, 1, 1, 128), True),        # MQA with an even number of heads
    ((24, 12, 12, 128), True),
    ((8, 2, 1, 128), True),
    ((8, 2, 4, 128), True),        # (lists finer than the K/V heads, still shared by neighbours)
    ((6, 2, 2, 128), False),       # g = 3: heads 2 and 3 read different K/V heads
    ((6, 2, 1, 128), False),
    ((3, 1, 1, 128), False),       # MQA with an odd number of heads
    ((8, 2, 8, 128), False),       # the mask per query head: the two heads walk different lists
    ((8, 4, 8, 128), False),
    ((8, 2, 2, 64), False),        # 64-token blocks run the 32-row kernel
    ((8, 1, 1, 64), False),
    ((8, 8, 8, 128), False),       # MHA
    ((8, 8, 1, 128), False),       # g = 1
]


@pytest.mark.parametrize("args,want", PAIR_TABLE, ids=["-".join(map(str, a)) for a, _ in PAIR_TABLE])
def test_pair_eligibility(args, want):
    from rectified_spaattn_amd.block_sparse import gqa_kv_head, gqa_pairable
    assert gqa_pairable(*args) is want
    H, Hkv, Hl, _ = args
    if want:        # what the rule stands for: heads 2p and 2p + 1 share their K/V head and their list head
        for p in range(H // 2):
            assert gqa_kv_head(2 * p, H, Hkv) == gqa_kv_head(2 * p + 1, H, Hkv)
            assert gqa_kv_head(2 * p, H, Hl) == gqa_kv_head(2 * p + 1, H, Hl)


@pytest.mark.parametrize("args", [(8, 3, 1, 128), (8, 2, 3, 128), (0, 1, 1, 128), (8, 0, 1, 128), (8, 2, 0, 128), (4, 8, 1, 128)])
def test_pair_eligibility_refuses_counts_that_do_not_divide(args):
    from rectified_spaattn_amd.block_sparse import gqa_pairable
    with pytest.raises(ValueError):
        gqa_pairable(*args)


# ---- the C entry ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entry_is_declared_listed_and_exported_and_the_version_stays():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", hdr)
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    assert ENTRY in _lib.EXPORTED
    _, L = _lib_or_skip()
    assert hasattr(L, ENTRY)
    assert L.rsa_version() == 601
    assert L.rsa_abi_check(601, ctypes.sizeof(_lib.RsaBuffers), ctypes.sizeof(_lib.RsaLayout)) == 0


def test_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 8 * 128 * 300, 128 * 300, 128)
    o = _lib.RsaOut4(4096, 8 * 128 * 300, 128, 8 * 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks

    def call(B=1, H=8, Hkv=2, Hl=2, Sq=300, Sk=300, D=128, dt=0, blk=128, NQ=3, NK=3, kvv=300, sc=0.088, q=t, cols=p, counts=p,
             lo=None, hi=None, sb=0, tp=None, tpb=0, out=o):
        return getattr(L, ENTRY)(B, H, Hkv, Hl, Sq, Sk, D, dt, blk, NQ, NK, kvv, sc, q, t, t, cols, counts, lo, hi, sb, tp, tpb, out,
                                 None)

    # the head counts: positive, and both divide H
    for kw in (dict(Hkv=0), dict(Hkv=-2), dict(Hl=0), dict(Hl=-1), dict(H=0), dict(H=-8), dict(Hkv=3), dict(Hkv=16), dict(Hl=3),
               dict(Hl=16), dict(H=6, Hkv=4, Hl=1), dict(H=6, Hkv=2, Hl=4)):
        assert call(**kw) == BAD, kw
        assert call(cols=None, **kw) == BAD
    # ranges: 128-token blocks only; the range arguments as the ranged entry takes them
    assert call(blk=64, NQ=5, NK=5, hi=p) == UNS
    assert call(blk=64, NQ=5, NK=5, lo=p, hi=p) == UNS
    assert call(hi=p, sb=-1) == BAD
    assert call(hi=ctypes.c_void_p(4098)) == BAD   # misaligned
    assert call(lo=ctypes.c_void_p(4097), hi=p) == BAD
    assert call(lo=p, hi=None) == BAD              # a lower limit alone
    # everything the plain entry refuses, with and without ranges, for a pairable and a non-pairable grouping
    for base in (dict(), dict(hi=p), dict(Hkv=8, Hl=1), dict(H=6, Hkv=2, Hl=2)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(D=96) == UNS
        assert c(dt=7) == UNS
        assert c(B=0) == BAD
        assert c(Sq=0) == BAD
        assert c(Sk=0) == BAD
        assert c(NQ=2) == BAD
        assert c(NK=4) == BAD
        assert c(NK=0) == BAD
        assert c(kvv=0) == BAD
        assert c(kvv=301) == BAD
        for bad in (float("inf"), float("-inf"), float("nan")):
            assert c(sc=bad) == BAD
        assert c(cols=None) == BAD
        assert c(counts=None) == BAD
        assert c(tp=p, tpb=0) == WS
        assert c(q=_lib.RsaTensor4(4100, 8 * 128 * 300, 128 * 300, 128)) == BAD
        assert c(out=_lib.RsaOut4(4096, 8 * 128 * 300, 128, 1022)) == BAD
        assert c(Sk=9000 * 128, NK=8193, kvv=9000 * 128) == UNS


def test_the_pair_switch_is_a_tuning_key():
    _lib, L = _lib_or_skip()
    try:
        assert L.rsa_set_tuning(b"k5_gqa_pair", 1) == 0
        assert L.rsa_set_tuning(b"k5_gqa_pair", 0) == 0
    finally:
        L.rsa_set_tuning(b"k5_gqa_pair", _lib.GQA_PAIR_DEFAULT)


def test_the_python_mirror_of_the_switchs_default_follows_the_library_source():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "rectified_spaattn_amd", "csrc", "rsa_attn.hip")).read()
    m = re.search(r"static int g_k5_gqa_pair = (\d+);", src)
    assert m and int(m.group(1)) == _lib.GQA_PAIR_DEFAULT
