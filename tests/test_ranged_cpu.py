"""Per-row key ranges of block_sparse_attention (causal=, window=, row_range=) without a GPU: the new C entry's presence and its
argument refusals (every call below fails its host checks: nothing is launched), the Python refusals, and the counting reference
of the visibility rule, which tests/test_gpu_ranged.py shares:

    row r of batch item b and head h sees key j  iff  block_mask[b, h, r // 128, j // 128]  and  lo[b, r] <= j < hi[b, r]
                                                      and  j < kv_len[b]  and  j < NK * 128
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

BLK = 128
ENTRY = "rsa_block_sparse_ranged_fwd"


# ---- the counting reference (numpy; nothing here touches the library) -----------------------------------------------------------
def window_ranges(Sq, lens, left, right):
    """lo, hi int64 [B, Sq] of flash-attn's window (left, right), -1 = unbounded, aligned bottom-right per batch item:
    row r sees keys r + off - left .. r + off + right with off = kv_len[b] - Sq."""
    r = np.arange(Sq, dtype=np.int64)[None, :]
    off = np.asarray(lens, np.int64)[:, None] - Sq
    lo = np.full((len(lens), Sq), np.iinfo(np.int64).min // 2) if left < 0 else r + off - left
    hi = np.full((len(lens), Sq), np.iinfo(np.int64).max // 2) if right < 0 else r + off + right + 1
    return lo, hi


def visible(mask, lo, hi, lens, Sq, Sk):
    """bool [B, H, Sq, Sk] of the rule in the module docstring.  mask bool [B|1, H|1, NQ, NK]; lo (None = no lower limit) and hi
    integer arrays [B|1, Sq]; lens B ints."""
    B = len(lens)
    m = np.broadcast_to(np.asarray(mask, bool), (B, mask.shape[1]) + tuple(mask.shape[2:]))
    NK = m.shape[-1]
    j = np.arange(Sk)
    r = np.arange(Sq)
    kept = np.zeros(m.shape[:2] + (Sq, Sk), bool)
    cols = j < NK * BLK
    kept[..., cols] = m[:, :, r // BLK][..., j[cols] // BLK]
    hi = np.broadcast_to(np.asarray(hi, np.int64), (B, Sq))
    vis = kept & (j[None, None, None, :] < hi[:, None, :, None])
    if lo is not None:
        lo = np.broadcast_to(np.asarray(lo, np.int64), (B, Sq))
        vis &= j[None, None, None, :] >= lo[:, None, :, None]
    vis &= j[None, None, None, :] < np.asarray(lens)[:, None, None, None]
    return vis


def plain_visible(mask, lens, Sq, Sk):
    """The plain call's rule, written on its own: the block's bit, j < kv_len[b], j < NK * 128."""
    B = len(lens)
    m = np.broadcast_to(np.asarray(mask, bool), (B, mask.shape[1]) + tuple(mask.shape[2:]))
    vis = np.zeros(m.shape[:2] + (Sq, Sk), bool)
    for b in range(B):
        for r in range(Sq):
            for jb in range(m.shape[-1]):
                if jb * BLK < min(lens[b], Sk):
                    vis[b, :, r, jb * BLK:min((jb + 1) * BLK, lens[b], Sk)] = m[b, :, r // BLK, jb][:, None]
    return vis


def _mask(seed, B, H, NQ, NK):
    return np.random.default_rng(seed).random((B, H, NQ, NK)) < 0.6


@pytest.mark.parametrize("Sq,Sk,lens", [(300, 300, [300, 300]), (200, 330, [330, 257]), (330, 200, [200, 131])])
def test_reference_identities(Sq, Sk, lens):
    """causal = window (-1, 0); window (-1, -1) = the plain rule; causal in closed form: j <= r + kv_len - Sq."""
    NQ, NK = -(-Sq // BLK), -(-Sk // BLK)
    m = _mask(Sq + Sk, 2, 2, NQ, NK)
    causal = visible(m, *window_ranges(Sq, lens, -1, 0), lens, Sq, Sk)
    r, j = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
    for b in range(2):
        closed = (j <= r + lens[b] - Sq) & (j < lens[b])
        assert np.array_equal(causal[b], plain_visible(m, lens, Sq, Sk)[b] & closed)
    assert np.array_equal(visible(m, *window_ranges(Sq, lens, -1, -1), lens, Sq, Sk), plain_visible(m, lens, Sq, Sk))
    # a window is the intersection of its two one-sided halves
    both = visible(m, *window_ranges(Sq, lens, 40, 9), lens, Sq, Sk)
    left = visible(m, *window_ranges(Sq, lens, 40, -1), lens, Sq, Sk)
    right = visible(m, *window_ranges(Sq, lens, -1, 9), lens, Sq, Sk)
    assert np.array_equal(both, left & right)
    # fewer mask columns than key blocks: keys past NK * 128 are never seen
    short = visible(m[..., :1], None, np.full((1, Sq), Sk), lens, Sq, Sk)
    assert not short[..., BLK:].any() and np.array_equal(short[..., :BLK], plain_visible(m[..., :1], lens, Sq, Sk)[..., :BLK])


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

    def call(B=1, H=8, Sq=300, Sk=300, D=128, dt=0, blk=128, NQ=3, NK=3, kvv=300, sc=0.088, q=t, cols=p, counts=p, lo=p, hi=p,
             sb=0, tp=None, tpb=0, out=o):
        return getattr(L, ENTRY)(B, H, Sq, Sk, D, dt, blk, NQ, NK, kvv, sc, q, t, t, cols, counts, lo, hi, sb, tp, tpb, out, None)

    # what the new arguments add
    assert call(blk=64, NQ=5, NK=5) == UNS         # the 32-row kernel has one scalar key limit, no per-row range
    assert call(blk=96) == UNS
    assert call(hi=None) == BAD
    assert call(lo=None, hi=None) == BAD
    assert call(sb=-1) == BAD
    assert call(sb=-300) == BAD
    assert call(hi=ctypes.c_void_p(4098)) == BAD   # misaligned
    assert call(lo=ctypes.c_void_p(4097)) == BAD
    # everything the plain entry refuses
    assert call(D=96) == UNS
    assert call(dt=7) == UNS
    assert call(B=0) == BAD
    assert call(H=0) == BAD
    assert call(Sq=0) == BAD
    assert call(Sk=0) == BAD
    assert call(NQ=2) == BAD
    assert call(NK=4) == BAD
    assert call(NK=0) == BAD
    assert call(kvv=0) == BAD
    assert call(kvv=301) == BAD
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert call(sc=bad) == BAD
    assert call(cols=None) == BAD
    assert call(counts=None) == BAD
    assert call(tp=p, tpb=0) == WS
    assert call(q=_lib.RsaTensor4(4100, 8 * 128 * 300, 128 * 300, 128)) == BAD
    assert call(out=_lib.RsaOut4(4096, 8 * 128 * 300, 128, 1022)) == BAD
    assert call(Sk=9000 * 128, NK=8193, kvv=9000 * 128) == UNS


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) ----------------------------------------
def _qkv(B=2, H=2, Sq=300, Sk=500, D=64, dt=torch.bfloat16):
    return (torch.zeros(B, H, Sq, D, dtype=dt), torch.zeros(B, H, Sk, D, dtype=dt), torch.zeros(B, H, Sk, D, dtype=dt))


def _rng(B=1, Sq=300, dtype=torch.int32, **kw):
    return torch.zeros(B, Sq, dtype=dtype, **kw)


@pytest.mark.parametrize("kw", [dict(causal=True, window=(3, 0)), dict(causal=True, row_range=(None, _rng())),
                                dict(window=(-1, 0), row_range=(None, _rng())),
                                dict(causal=True, window=(1, 1), row_range=(None, _rng()))],
                         ids=["causal+window", "causal+row_range", "window+row_range", "all"])
def test_more_than_one_kind_of_range_is_refused(kw):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv()
    with pytest.raises(ValueError, match="at most one"):
        block_sparse_attention(q, k, v, torch.ones(1, 1, 3, 4, dtype=torch.bool), **kw)


@pytest.mark.parametrize("kw", [dict(causal=True), dict(window=(5, 5)), dict(row_range=(None, _rng()))],
                         ids=["causal", "window", "row_range"])
def test_64_token_blocks_with_a_range_are_refused(kw):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv()
    with pytest.raises(NotImplementedError, match="128"):
        block_sparse_attention(q, k, v, torch.ones(1, 1, 5, 8, dtype=torch.bool), block_size=64, **kw)


@pytest.mark.parametrize("case", ["hi_dtype", "lo_dtype", "hi_rows", "hi_batch", "lo_shape", "hi_dim", "hi_none", "not_a_pair",
                                  "hi_device", "lo_device", "not_a_tensor"])
def test_malformed_row_ranges_raise_value_error(case):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv()           # B = 2, Sq = 300
    rr = dict(hi_dtype=(None, _rng(dtype=torch.int64)), lo_dtype=(_rng(dtype=torch.float32), _rng()),
              hi_rows=(None, _rng(Sq=299)), hi_batch=(None, _rng(B=3)), lo_shape=(_rng(B=2, Sq=301), _rng(B=2)),
              hi_dim=(None, torch.zeros(300, dtype=torch.int32)), hi_none=(_rng(), None), not_a_pair=_rng(),
              hi_device=(None, _rng(device="meta")), lo_device=(_rng(device="meta"), _rng()),
              not_a_tensor=(None, [0] * 300))[case]
    with pytest.raises(ValueError):
        block_sparse_attention(q, k, v, torch.ones(1, 1, 3, 4, dtype=torch.bool), row_range=rr)


@pytest.mark.parametrize("window", [(1,), (1, 2, 3), (-2, 0), (0, -5), (1.5, 0), "ab", 7])
def test_malformed_windows_raise_value_error(window):
    from rectified_spaattn_amd import block_sparse_attention
    q, k, v = _qkv()
    with pytest.raises(ValueError):
        block_sparse_attention(q, k, v, torch.ones(1, 1, 3, 4, dtype=torch.bool), window=window)


def test_a_well_formed_ranged_call_on_cpu_tensors_reaches_the_device_check():
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, block_sparse_attention
    q, k, v = _qkv()
    m = torch.ones(1, 1, 3, 4, dtype=torch.bool)
    for kw in (dict(causal=True), dict(window=(4680, 0)), dict(row_range=(_rng(), _rng(B=2))), dict(causal=True, kv_len=[500, 77])):
        with pytest.raises(_lib.RsaError):
            block_sparse_attention(q, k, v, m, **kw)
