"""pool_keys and select_blocks_pooled without a GPU: the numpy model of the cache against a naive per-block
loop, the Python refusals, and the C entries' presence and argument refusals (every call fails its host checks: nothing is
launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pooled_ref as ref
import select_ref

NAMES = ("rsa_pool_keys", "rsa_block_select_pooled_bytes", "rsa_block_select_pooled")


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _steps(b):
    """(old lengths, new lengths, start | None = the old lengths) for B = 2."""
    return [
        ([3, b // 2], [9, b - 1], None),                    # appends that stay inside a block
        ([b - 7, 2 * b - 1], [b, 2 * b], None),             # ... that fill it exactly
        ([b - 1, 3 * b], [b + 1, 3 * b + 4], None),         # ... that cross into the next
        ([2 * b - 1, b - 3], [3 * b + 1, 2 * b + 2], None),   # ... that cross two (an Sq-sized append)
        ([b + 5, 2 * b + 9], [b + 5, 2 * b + 9], "len"),    # start = len: the ragged tail alone
        ([2 * b, b], [2 * b, b], "len"),                    # ... and no ragged tail: nothing
        ([b + 5, 9], [b + 5, 9], [b + 6, 5 * b]),           # start > len: nothing
        ([2 * b + 5, 4 * b], [b + 3, 3 * b - 1], "len"),    # truncation, then start = kv_len
        ([b + 5, 2 * b], [0, 0], None),                     # len = 0
        ([0, 0], [0, 5 * b + 60], None),                    # from nothing to everything
    ]


@pytest.mark.parametrize("blk", [64, 128])
def test_model_is_the_naive_loop(blk):
    B, Hkv, D = 2, 2, 4
    Sk = 5 * blk + 60
    NK = -(-Sk // blk)
    k = np.random.default_rng(blk).standard_normal((B, Hkv, Sk, D))
    nothing = 0
    for n, (old, new, start) in enumerate(_steps(blk)):
        starts = old if start is None else (new if start == "len" else start)
        cache, first = ref.make(k, old, blk, fill=-7.0)
        assert np.array_equal(first, np.arange(NK)[None] * blk < np.asarray(old)[:, None])
        k2 = k.copy()
        for b in range(B):                                  # an append rewrites [old, new); a truncation leaves garbage behind
            k2[b, :, min(old[b], new[b]):] = np.random.default_rng(n + b).standard_normal((Hkv, Sk - min(old[b], new[b]), D))
        got, wrote = ref.update(cache, k2, new, starts, blk)
        for b in range(B):
            lo, hi = starts[b] // blk, -(-new[b] // blk)
            for j in range(NK):
                inside = starts[b] <= new[b] and lo <= j < hi
                assert wrote[b, j] == inside, (n, b, j)
                if not inside:
                    assert np.array_equal(got[b, :, j], cache[b, :, j]), (n, b, j)        # untouched, the sentinel included
                    continue
                want = ref.block_naive(k2, b, j, new[b], blk)
                assert want is not None and np.allclose(got[b, :, j], want, rtol=1e-13, atol=1e-14), (n, b, j)
            # what an update must leave behind: below ceil(new / blk) the cache of a fresh pooling at the new lengths
            if start is None and new[b] >= old[b]:
                fresh = select_ref.pooled(k2, new, blk)
                assert np.array_equal(got[b, :, :hi], fresh[b, :, :hi]), (n, b)
        nothing += int(not wrote.any())
    assert nothing >= 3


def test_written_ranges():
    b = 128
    assert list(ref.written(0, 0, b)) == [] and list(ref.written(0, 1, b)) == [0] and list(ref.written(0, 700, b)) == list(range(6))
    assert list(ref.written(127, 128, b)) == [0] and list(ref.written(127, 129, b)) == [0, 1]
    assert list(ref.written(255, 385, b)) == [1, 2, 3]
    assert list(ref.written(128, 128, b)) == [] and list(ref.written(133, 133, b)) == [1]
    assert list(ref.written(134, 133, b)) == [] and list(ref.written(256, 133, b)) == []


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) -------------------------------------------
def _k(B=2, Hkv=2, Sk=700, D=64, dt=torch.bfloat16):
    return torch.zeros(B, Hkv, Sk, D, dtype=dt)


def _cache(B=2, Hkv=2, NK=6, D=64):
    return torch.zeros(B, Hkv, NK, D, dtype=torch.float32)


def test_both_are_exported_from_the_package():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import block_sparse, pool_keys, select_blocks_pooled
    assert callable(pool_keys) and callable(block_sparse.pool_keys)
    assert callable(select_blocks_pooled) and callable(block_sparse.select_blocks_pooled)
    assert {"pool_keys", "select_blocks_pooled"} <= set(dir(rectified_spaattn_amd))


def test_pool_keys_refusals():
    from rectified_spaattn_amd import pool_keys
    k = _k()
    with pytest.raises(NotImplementedError, match="block_size"):
        pool_keys(k, block_size=96)
    with pytest.raises(ValueError, match="tensor"):
        pool_keys(k[0])
    with pytest.raises(ValueError, match="dtype"):
        pool_keys(k.float())
    with pytest.raises(ValueError, match="head dim"):
        pool_keys(_k(D=48))
    with pytest.raises(ValueError, match="empty"):
        pool_keys(k[:, :, :0])
    with pytest.raises(ValueError, match="at most 8192"):
        pool_keys(torch.zeros(1, 1, 8193 * 64, 16, dtype=torch.bfloat16), block_size=64)
    for kv_len in (701, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="kv_len"):
            pool_keys(k, kv_len=kv_len)
    for start in (701, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="start"):
            pool_keys(k, start=start, out=_cache())
    with pytest.raises(ValueError, match="out: required"):
        pool_keys(k, start=5)
    for bad in (_cache().double(), _cache(NK=5), _cache(Hkv=1), _cache(D=128), _cache()[..., ::2], [0.0]):
        with pytest.raises(ValueError, match="out"):
            pool_keys(k, out=bad)
    for w in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="workgroups_per_head"):
            pool_keys(k, workgroups_per_head=w)
    # the paged form: the table's type and rank, pools of block_size rows
    pool = torch.zeros(9, 2, 128, 64, dtype=torch.bfloat16)
    for table in (torch.zeros(2, 6, dtype=torch.int64), torch.zeros(12, dtype=torch.int32), [[0] * 6] * 2):
        with pytest.raises(ValueError, match="block_table"):
            pool_keys(pool, block_table=table)
    with pytest.raises(ValueError, match="page pool"):
        pool_keys(pool[:, :, :64], block_table=torch.zeros(2, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="at most 8192"):
        pool_keys(pool, block_table=torch.zeros(1, 8193, dtype=torch.int32))
    with pytest.raises(ValueError, match="out"):
        pool_keys(pool, block_table=torch.zeros(2, 6, dtype=torch.int32), out=_cache(NK=7))
    # a cache is never copied: strides that would need a copy are refused
    with pytest.raises(ValueError, match="not copied"):
        pool_keys(k.transpose(2, 3).contiguous().transpose(2, 3))


def test_select_blocks_pooled_refusals():
    from rectified_spaattn_amd import select_blocks_pooled as sel
    q, pk = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16), _cache()
    with pytest.raises(NotImplementedError, match="block_size"):
        sel(q, pk, 2, block_size=96)
    with pytest.raises(ValueError, match="mask_heads"):
        sel(q, pk, 2, mask_heads="all")
    for name in ("top_k", "keep_first", "keep_local"):
        for bad in (-1, 1.5, True):
            with pytest.raises(ValueError, match=name):
                sel(q, pk, **{"top_k": 2, name: bad})
    for bad in (0, -1, 257, 1.5, True):
        with pytest.raises(ValueError, match="score_splits"):
            sel(q, pk, 2, score_splits=bad)
    with pytest.raises(ValueError, match="tensor"):
        sel(q[0], pk, 2)
    with pytest.raises(ValueError, match="tensor"):
        sel(q, pk[0], 2)
    with pytest.raises(ValueError, match="Hkv"):
        sel(q, _cache(Hkv=3), 2)
    with pytest.raises(ValueError, match="match"):
        sel(q, _cache(B=1), 2)
    with pytest.raises(ValueError, match="match"):
        sel(q, _cache(D=128), 2)
    with pytest.raises(ValueError, match="dtype"):
        sel(q.float(), pk, 2)
    with pytest.raises(ValueError, match="float32"):
        sel(q, pk.bfloat16(), 2)
    with pytest.raises(ValueError, match="contiguous"):
        sel(q, torch.zeros(2, 6, 2, 64).transpose(1, 2), 2)
    with pytest.raises(ValueError, match="head dim"):
        sel(torch.zeros(2, 8, 1, 48, dtype=torch.bfloat16), _cache(D=48), 2)
    with pytest.raises(ValueError, match="empty"):
        sel(q[:, :, :0], pk, 2)
    with pytest.raises(ValueError, match="at most 8192"):
        sel(torch.zeros(1, 1, 1, 16, dtype=torch.bfloat16), torch.zeros(1, 1, 8193, 16), 2)
    for kv_len in (6 * 128 + 1, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="kv_len"):
            sel(q, pk, 2, kv_len=kv_len)


@pytest.mark.parametrize("kw", [dict(), dict(kv_len=[700, 333], start=[650, 333], out=True), dict(block_size=64, workgroups_per_head=3),
                                dict(paged=True)], ids=["plain", "update", "block64-hint", "paged"])
def test_a_well_formed_pool_keys_call_on_cpu_tensors_reaches_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, pool_keys
    kw = dict(kw)
    k = _k()
    if kw.pop("out", False):
        kw["out"] = _cache()
    if kw.pop("paged", False):
        k = torch.zeros(15, 2, 128, 64, dtype=torch.bfloat16)
        kw["block_table"] = torch.zeros(2, 6, dtype=torch.int32)
    with pytest.raises(_lib.RsaError):
        pool_keys(k, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(causal=True, kv_len=[700, 333], keep_first=1, keep_local=1, return_scores=True),
                                dict(mask_heads="q", as_lists=True, score_splits=7)], ids=["plain", "causal-lens", "q-lists-splits"])
def test_a_well_formed_selection_on_cpu_tensors_reaches_the_device_check(kw):
    from rectified_spaattn_amd import _lib, select_blocks_pooled as sel
    with pytest.raises(_lib.RsaError):
        sel(torch.zeros(2, 8, 3, 64, dtype=torch.float16), _cache(), 2, **kw)


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
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTED, name
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    _, L = _lib_or_skip()
    assert all(hasattr(L, name) for name in NAMES)
    assert L.rsa_version() == 601


def test_workspace_size_query():
    _, L = _lib_or_skip()
    n = ctypes.c_size_t(0)

    def size(B, Hkv, Hl, D, NQ, NK):
        st = L.rsa_block_select_pooled_bytes(B, Hkv, Hl, D, NQ, NK, ctypes.byref(n))
        return n.value if st == 0 else st
    # per list row: the pooled query (D floats) and the row's ordered keys (NK words); no pooled keys
    assert size(2, 2, 2, 128, 1, 6) == 4 * (128 + 6) * 4
    assert size(1, 8, 32, 128, 1, 1024) == 32 * (128 + 1024) * 4
    assert size(3, 2, 2, 16, 5, 8192) == 30 * (16 + 8192) * 4
    assert L.rsa_block_select_pooled_bytes(2, 2, 2, 128, 1, 6, None) == -1
    for bad in ((0, 2, 2, 128, 1, 6), (2, 0, 2, 128, 1, 6), (2, 2, 0, 128, 1, 6), (2, 2, 2, 128, 0, 6), (2, 2, 2, 128, 1, 0)):
        assert size(*bad) == -1, bad
    for uns in ((2, 2, 2, 96, 1, 6), (2, 2, 2, 8, 1, 6), (2, 2, 2, 128, 1, 8193)):
        assert size(*uns) == -2, uns


def test_pool_keys_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS = -1, -2
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks

    def call(B=2, Hkv=2, Sk=700, D=128, dt=0, blk=128, NK=6, k=t, table=None, tsb=6, pages=0, kv=None, kvv=700, st=None, stv=0,
             wph=0, out=p):
        return L.rsa_pool_keys(B, Hkv, Sk, D, dt, blk, NK, k, table, tsb, pages, kv, kvv, st, stv, wph, out, None)

    for base in (dict(), dict(kv=p), dict(st=p), dict(kv=p, st=p), dict(table=p, pages=20, Sk=768), dict(wph=3), dict(stv=650)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(blk=32) == UNS
        assert c(D=96) == UNS
        assert c(D=8) == UNS
        assert c(dt=7) == UNS
        assert c(Sk=8193 * 128, NK=8193) == UNS
        assert c(B=0) == BAD
        assert c(Hkv=0) == BAD
        assert c(Hkv=-2) == BAD
        assert c(Sk=0) == BAD
        assert c(NK=0) == BAD
        assert c(NK=7) == BAD                        # not ceil(Sk / block)
        assert c(NK=5) == BAD
        assert c(blk=64, NK=6) == BAD
        assert c(wph=-1) == BAD
        assert c(out=None) == BAD
        assert c(out=ctypes.c_void_p(4104)) == BAD   # 16-byte alignment: the selection reads 16 bytes a lane
        assert c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(st=ctypes.c_void_p(4097)) == BAD
        assert c(table=ctypes.c_void_p(4098), pages=20) == BAD
        assert c(table=p, pages=0) == BAD
        assert c(table=p, pages=-3) == BAD
        assert c(table=p, pages=20, tsb=-6) == BAD
        assert c(k=_lib.RsaTensor4(None, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4100, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        if "kv" not in base:                         # the host limits: 0 .. Sk (a device limit is clamped on the device)
            assert c(kvv=-1) == BAD
            assert c(kvv=base.get("Sk", 700) + 1) == BAD
        if "st" not in base:
            assert c(stv=-1) == BAD
            assert c(stv=base.get("Sk", 700) + 1) == BAD


def test_selection_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)
    big = 1 << 30

    def call(B=2, H=8, Hkv=2, Hl=2, Sq=1, D=128, dt=0, blk=128, NQ=1, NK=6, q=t, pk=p, kv=None, kvv=700, causal=0, top_k=2, kf=0,
             kl=0, splits=0, ws=p, wsb=big, bitmask=p, cols=p, counts=p, scores=None):
        return L.rsa_block_select_pooled(B, H, Hkv, Hl, Sq, D, dt, blk, NQ, NK, q, pk, kv, kvv, causal, top_k, kf, kl, splits, ws,
                                         wsb, bitmask, cols, counts, scores, None)

    for kw in (dict(H=0), dict(Hkv=0), dict(Hl=0), dict(Hkv=3, Hl=3), dict(Hl=4), dict(Hl=1), dict(H=6, Hkv=4, Hl=4)):
        assert call(**kw) == BAD, kw
    for base in (dict(), dict(Hl=8), dict(causal=1, Sq=300, NQ=3), dict(scores=p), dict(kv=p), dict(splits=1), dict(splits=64)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(D=96) == UNS
        assert c(D=8) == UNS
        assert c(dt=7) == UNS
        assert c(NK=8193) == UNS
        assert c(B=0) == BAD
        assert c(Sq=0) == BAD
        assert c(Sq=-5) == BAD
        assert c(NK=0) == BAD
        assert c(NQ=base.get("NQ", 1) + 1) == BAD    # not ceil(Sq / block)
        assert c(top_k=-1) == BAD
        assert c(kf=-1) == BAD
        assert c(kl=-1) == BAD
        assert c(splits=-1) == BAD
        assert c(splits=257) == BAD
        assert c(ws=None) == BAD
        assert c(ws=ctypes.c_void_p(4104)) == BAD
        assert c(pk=None) == BAD
        assert c(pk=ctypes.c_void_p(4104)) == BAD
        assert c(bitmask=None) == BAD
        assert c(cols=None) == BAD
        assert c(counts=None) == BAD
        assert c(cols=ctypes.c_void_p(4098)) == BAD
        assert c(scores=ctypes.c_void_p(4098)) == BAD
        assert c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(q=_lib.RsaTensor4(None, 8 * 128, 128, 128)) == BAD
        assert c(q=_lib.RsaTensor4(4100, 8 * 128, 128, 128)) == BAD
        assert c(q=_lib.RsaTensor4(4096, 8 * 128, 128, 132)) == BAD
        assert c(q=_lib.RsaTensor4(4096, 8 * 128, 128, -128)) == BAD
        assert c(wsb=0) == WS
        assert c(NK=8192, wsb=0) == WS               # (the limit itself is served)
        if "kv" not in base:                         # the host limit: 0 .. NK * block
            assert c(kvv=-1) == BAD
            assert c(kvv=6 * 128 + 1) == BAD
            assert c(kvv=6 * 128, wsb=0) == WS
    n = ctypes.c_size_t(0)
    assert L.rsa_block_select_pooled_bytes(2, 2, 2, 128, 1, 6, ctypes.byref(n)) == 0
    assert call(wsb=n.value - 1) == WS
    assert call(wsb=n.value, blk=96) == UNS
