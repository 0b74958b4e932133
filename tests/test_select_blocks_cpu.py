"""select_blocks (top-k block selection per K/V head) without a GPU: the numpy reference against its own
naive form, the Python refusals, and the C entry's presence and argument refusals (every call below fails its host checks:
nothing is launched)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import select_ref as ref

ENTRY, BYTES = "rsa_block_select", "rsa_block_select_bytes"


# ---- the reference: vectorised form = naive loop ---------------------------------------------------------------------------------
SHAPES = [  # (Sq, Sk, lens): ragged ends, Sq != Sk, off_b = len_b - Sq of both signs, a batch item whose first rows see nothing
    (200, 200, [200, 131]),
    (130, 450, [450, 300]),
    (450, 130, [130, 70]),
    (257, 330, [330, 1]),
]


@pytest.mark.parametrize("blk", [64, 128])
@pytest.mark.parametrize("Sq,Sk,lens", SHAPES, ids=[f"{a}x{b}" for a, b, _ in SHAPES])
def test_vectorised_reference_equals_the_naive_loop(Sq, Sk, lens, blk):
    """Tie-heavy integer scores (q, k in -1 .. 1, pooled over whole or half blocks at most of the rows): both forms of the kept
    set agree, and the count is min(max(top_k, |forced|), |visible|) in every row."""
    B, H, Hkv, D = 2, 4, 2, 8
    g = np.random.default_rng(Sq * 7 + Sk + blk)
    q = g.integers(-1, 2, (B, H, Sq, D)).astype(np.float64)
    k = g.integers(-1, 2, (B, Hkv, Sk, D)).astype(np.float64)
    k[:, :, :, 1:] = 0          # one live channel: few distinct scores
    NK = -(-Sk // blk)
    n = ties = 0
    for heads, causal in itertools.product(("kv", "q"), (False, True)):
        t = ref.scores(q, k, lens, blk, heads)
        t = np.round(t * 8) / 8     # (coarser still: many equal scores in a row)
        vis = ref.visible(Sq, Sk, lens, blk, causal)
        ties += int((np.diff(np.sort(t, axis=-1), axis=-1) == 0).sum())
        for kf, kl in itertools.product((0, 1, 2), (0, 1, 2)):
            frc = ref.forced(Sq, Sk, lens, blk, causal, kf, kl)
            assert not (frc & ~vis).any()
            for top_k in (0, 1, 3, NK, NK + 5):
                a = ref.kept_vectorised(t, vis, frc, top_k)
                b = ref.kept_naive(t, vis, frc, top_k)
                assert np.array_equal(a, b), (heads, causal, kf, kl, top_k)
                want = np.minimum(np.maximum(top_k, frc.sum(-1)), vis.sum(-1))
                assert np.array_equal(a.sum(-1), np.broadcast_to(want[:, None], a.shape[:3]))
                assert not (a & ~vis[:, None]).any() and (a | ~frc[:, None]).all()
                n += 1
    assert n == 2 * 2 * 9 * 5 and ties > 0


def test_reference_visible_blocks_are_the_causal_calls():
    """A block is visible iff some row of the query block sees some key of it under the attention call's rule:
    j < kv_len[b], and with causal j <= r + kv_len[b] - Sq (tests/test_ranged_cpu.py)."""
    for (Sq, Sk, lens), blk, causal in itertools.product(SHAPES, (64, 128), (False, True)):
        NQ, NK = -(-Sq // blk), -(-Sk // blk)
        r, j = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
        for b, n in enumerate(lens):
            seen = np.broadcast_to(j < n, (Sq, Sk)) & ((j <= r + n - Sq) if causal else True)
            pad = np.zeros((NQ * blk, NK * blk), bool)
            pad[:Sq, :Sk] = seen
            want = pad.reshape(NQ, blk, NK, blk).any(axis=(1, 3))
            assert np.array_equal(ref.visible(Sq, Sk, lens, blk, causal)[b], want), (Sq, Sk, blk, causal, b)


def test_reference_pooling_and_group_sum():
    g = np.random.default_rng(3)
    q, k = g.standard_normal((1, 4, 150, 8)), g.standard_normal((1, 2, 200, 8))
    t = ref.scores(q, k, [170], 64, "kv")
    tq = ref.scores(q, k, [170], 64, "q")
    assert t.shape == (1, 2, 3, 4) and tq.shape == (1, 4, 3, 4)
    assert np.allclose(t[0, 1], tq[0, 2] + tq[0, 3]) and np.allclose(t[0, 0], tq[0, 0] + tq[0, 1])
    # block 2 of the keys holds keys 128 .. 169 only, block 2 of the queries rows 128 .. 149; block 3 of the keys holds none
    want = q[0, 3, 128:150].mean(0) @ k[0, 1, 128:170].mean(0)
    assert np.isclose(tq[0, 3, 2, 2], want) and (t[..., 3] == 0).all()


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) -------------------------------------------
def _qk(B=2, H=8, Hkv=2, Sq=300, Sk=500, D=64, dt=torch.bfloat16, dtk=None):
    return torch.zeros(B, H, Sq, D, dtype=dt), torch.zeros(B, Hkv, Sk, D, dtype=dtk or dt)


def test_select_blocks_is_exported_from_the_package():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import block_sparse, select_blocks
    assert callable(select_blocks) and callable(block_sparse.select_blocks)
    assert "select_blocks" in dir(rectified_spaattn_amd)


@pytest.mark.parametrize("H,Hkv", [(8, 3), (6, 4), (4, 8), (7, 2)])
def test_head_counts_that_do_not_divide_are_refused(H, Hkv):
    from rectified_spaattn_amd import select_blocks
    with pytest.raises(ValueError, match="Hkv"):
        select_blocks(*_qk(H=H, Hkv=Hkv), 3)


@pytest.mark.parametrize("kw,exc,match", [
    (dict(block_size=96), NotImplementedError, "block_size"),
    (dict(block_size=32), NotImplementedError, "block_size"),
    (dict(mask_heads="all"), ValueError, "mask_heads"),
    (dict(keep_first=-1), ValueError, "keep_first"),
    (dict(keep_local=-2), ValueError, "keep_local"),
    (dict(keep_local=1.5), ValueError, "keep_local"),
    (dict(kv_len=501), ValueError, "kv_len"),
    (dict(kv_len=-1), ValueError, "kv_len"),
    (dict(kv_len=[1, 2, 3]), ValueError, "kv_len"),
])
def test_bad_keywords_are_refused(kw, exc, match):
    from rectified_spaattn_amd import select_blocks
    with pytest.raises(exc, match=match):
        select_blocks(*_qk(), 3, **kw)


def test_bad_operands_are_refused():
    from rectified_spaattn_amd import select_blocks
    q, k = _qk()
    with pytest.raises(ValueError, match="top_k"):
        select_blocks(q, k, -1)
    with pytest.raises(ValueError, match="top_k"):
        select_blocks(q, k, 2.0)
    with pytest.raises(ValueError, match="tensors"):
        select_blocks(q[0], k, 3)
    with pytest.raises(ValueError, match="match"):
        select_blocks(q, k[:1], 3)
    with pytest.raises(ValueError, match="match"):
        select_blocks(q, k[..., :32], 3)
    with pytest.raises(ValueError, match="dtype"):
        select_blocks(*_qk(dtk=torch.float16), 3)
    with pytest.raises(ValueError, match="dtype"):
        select_blocks(*_qk(dt=torch.float32), 3)
    with pytest.raises(ValueError, match="head dim"):
        select_blocks(*_qk(D=48), 3)
    with pytest.raises(ValueError, match="empty"):
        select_blocks(q[:, :, :0], k, 3)
    with pytest.raises(ValueError, match="key blocks"):
        select_blocks(*_qk(B=1, H=1, Hkv=1, Sq=64, Sk=8193 * 64, D=16), 3, block_size=64)


@pytest.mark.parametrize("kw", [dict(), dict(causal=True, keep_first=1, keep_local=1), dict(block_size=64, mask_heads="q"),
                                dict(kv_len=[500, 333], return_scores=True, as_lists=True)],
                         ids=["plain", "moba", "block64-q", "lens-lists"])
def test_a_well_formed_call_on_cpu_tensors_reaches_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, select_blocks
    with pytest.raises(_lib.RsaError):
        select_blocks(*_qk(), 3, **kw)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_declared_listed_and_exported_and_the_version_stays():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    for name in (ENTRY, BYTES):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        assert name in _lib.EXPORTED
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    _, L = _lib_or_skip()
    assert hasattr(L, ENTRY) and hasattr(L, BYTES)
    assert L.rsa_version() == 601
    assert L.rsa_abi_check(601, ctypes.sizeof(_lib.RsaBuffers), ctypes.sizeof(_lib.RsaLayout)) == 0


def test_workspace_size_query():
    _, L = _lib_or_skip()
    n = ctypes.c_size_t(0)
    assert L.rsa_block_select_bytes(2, 2, 8, 128, 3, 5, ctypes.byref(n)) == 0
    assert n.value == 4 * 128 * (2 * 8 * 3 + 2 * 2 * 5)        # the pooled query sums and the pooled keys, fp32
    assert L.rsa_block_select_bytes(2, 2, 8, 128, 3, 5, None) == -1
    assert L.rsa_block_select_bytes(0, 2, 8, 128, 3, 5, ctypes.byref(n)) == -1
    assert L.rsa_block_select_bytes(2, 2, 8, 128, 3, 0, ctypes.byref(n)) == -1
    assert L.rsa_block_select_bytes(2, 2, 8, 96, 3, 5, ctypes.byref(n)) == -2
    assert L.rsa_block_select_bytes(2, 2, 8, 128, 3, 8193, ctypes.byref(n)) == -2


def test_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 8 * 128 * 300, 128 * 300, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks
    big = 1 << 30

    def call(B=1, H=8, Hkv=2, Hl=2, Sq=300, Sk=300, D=128, dt=0, blk=128, NQ=3, NK=3, q=t, k=t, kv=None, kvv=300, causal=0,
             top_k=2, kf=0, kl=0, ws=p, wsb=big, bitmask=p, cols=p, counts=p, scores=None):
        return getattr(L, ENTRY)(B, H, Hkv, Hl, Sq, Sk, D, dt, blk, NQ, NK, q, k, kv, kvv, causal, top_k, kf, kl, ws, wsb, bitmask,
                                 cols, counts, scores, None)

    # the head counts: positive, Hkv divides H, Hl is Hkv or H
    for kw in (dict(H=0), dict(H=-8), dict(Hkv=0), dict(Hkv=-2), dict(Hl=0), dict(Hl=-1), dict(Hkv=3, Hl=3), dict(Hkv=16, Hl=16),
               dict(Hl=1), dict(Hl=4), dict(Hl=16), dict(H=6, Hkv=4, Hl=4)):
        assert call(**kw) == BAD, kw
    for base in (dict(), dict(Hl=8), dict(Hkv=8, Hl=8), dict(Hkv=1, Hl=1), dict(causal=1, kf=1, kl=1), dict(scores=p), dict(kv=p)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(blk=32) == UNS
        assert c(D=96) == UNS
        assert c(D=256) == UNS
        assert c(dt=7) == UNS
        assert c(B=0) == BAD
        assert c(Sq=0) == BAD
        assert c(Sk=0) == BAD
        assert c(Sq=-5) == BAD
        assert c(NQ=2) == BAD
        assert c(NQ=4) == BAD
        assert c(NK=4) == BAD
        assert c(NK=0) == BAD
        assert c(blk=64) == BAD                      # NQ / NK of 128-token blocks
        assert c(top_k=-1) == BAD
        assert c(kf=-1) == BAD
        assert c(kl=-1) == BAD
        assert c(ws=None) == BAD
        assert c(ws=ctypes.c_void_p(4104)) == BAD    # 16-byte alignment
        assert c(bitmask=None) == BAD
        assert c(cols=None) == BAD
        assert c(counts=None) == BAD
        assert c(cols=ctypes.c_void_p(4098)) == BAD
        assert c(scores=ctypes.c_void_p(4097)) == BAD
        assert c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(q=_lib.RsaTensor4(None, 8 * 128 * 300, 128 * 300, 128)) == BAD
        assert c(q=_lib.RsaTensor4(4100, 8 * 128 * 300, 128 * 300, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 8 * 128 * 300, 128 * 300, 132)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 8 * 128 * 300, 128 * 300, -128)) == BAD
        assert c(wsb=0) == WS
        assert c(Sk=8193 * 128, NK=8193, kvv=8193 * 128) == UNS
        assert c(Sk=8192 * 128, NK=8192, kvv=8192 * 128, wsb=0) == WS     # (the limit itself is served)
        if "kv" not in base:                         # the host limit: 0 .. Sk (a device limit is clamped on the device)
            assert c(kvv=-1) == BAD
            assert c(kvv=301) == BAD
    # the workspace: exactly what the query reports is enough for the checks, one byte less is not
    n = ctypes.c_size_t(0)
    assert L.rsa_block_select_bytes(1, 2, 2, 128, 3, 3, ctypes.byref(n)) == 0
    assert call(wsb=n.value - 1) == WS
    assert call(wsb=n.value, blk=96) == UNS
