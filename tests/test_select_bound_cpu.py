"""pool_key_bounds and select_blocks_bound without a GPU: the numpy model against naive loops, the
property that defines the score (no key of a block scores above the block), the needle the mean criterion drops and the bound
keeps, constant blocks (bound = mean), the Python refusals, and the C entries' presence and argument refusals (every call fails
its host checks: nothing is launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bound_ref as ref
import select_p_ref
import select_ref

NAMES = ("rsa_pool_key_bounds", "rsa_pool_key_bounds_kv8", "rsa_block_select_bound_bytes", "rsa_block_select_bound",
         "rsa_block_select_bound_packed")


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _naive_bounds(k, lens, blk):
    B, Hkv, Sk, D = k.shape
    NK = -(-Sk // blk)
    out = np.zeros((B, Hkv, NK, 2, D))
    for b in range(B):
        for h in range(Hkv):
            for j in range(NK):
                rows = [r for r in range(j * blk, min((j + 1) * blk, Sk)) if r < lens[b]]
                for d in range(D):
                    if rows:
                        mn = mx = k[b, h, rows[0], d]
                        for r in rows[1:]:
                            mn, mx = min(mn, k[b, h, r, d]), max(mx, k[b, h, r, d])
                        out[b, h, j, 0, d], out[b, h, j, 1, d] = mn, mx
    return out


def _naive_scores(q, bnd, blk, heads):
    B, H, Sq, D = q.shape
    Hkv, NK = bnd.shape[1], bnd.shape[2]
    Hl = Hkv if heads == "kv" else H
    gl, NQ = H // Hl, -(-Sq // blk)
    t = np.zeros((B, Hl, NQ, NK))
    for b in range(B):
        for hl in range(Hl):
            for i in range(NQ):
                rows = range(i * blk, min((i + 1) * blk, Sq))
                qs = np.zeros(D)
                for u in range(gl):
                    qs += sum(q[b, hl * gl + u, r] for r in rows) / len(rows)
                hk = hl // (Hl // Hkv)
                for j in range(NK):
                    t[b, hl, i, j] = sum(max(qs[d] * bnd[b, hk, j, 0, d], qs[d] * bnd[b, hk, j, 1, d]) for d in range(D))
    return t


@pytest.mark.parametrize("blk", [64, 128])
def test_model_is_the_naive_loop(blk):
    B, H, Hkv, D = 2, 4, 2, 5
    Sk, Sq = 3 * blk + 17, blk + 9
    lens = [Sk, blk + 1]
    rng = np.random.default_rng(blk)
    q, k = rng.standard_normal((B, H, Sq, D)), rng.standard_normal((B, Hkv, Sk, D))
    bnd = ref.bounds(k, lens, blk)
    assert bnd.shape == (B, Hkv, 4, 2, D) and np.array_equal(bnd, _naive_bounds(k, lens, blk))
    assert not bnd[1, :, 2:].any() and (bnd[:, :, :, 0] <= bnd[:, :, :, 1]).all()
    for heads in ("kv", "q"):
        t = ref.scores(q, bnd, blk, heads)
        assert np.allclose(t, _naive_scores(q, bnd, blk, heads), rtol=1e-13, atol=1e-13)
        M = ref.magnitude(q, bnd, blk, heads)
        assert (np.abs(t) <= M * (1 + 1e-12)).all()
    # the naive and the vectorised selection agree, top-k and top-p
    for kw in (dict(top_k=2, causal=True, keep_first=1), dict(top_k=3, top_p=0.7, keep_local=1, mask_heads="q")):
        a, b = ref.select(q, k, blk=blk, lens=lens, **kw), ref.select(q, k, blk=blk, lens=lens, naive=True, **kw)
        assert np.array_equal(a["mask"], b["mask"]) and a["mask"].any()


def test_update_writes_pooled_ref_s_blocks():
    blk, B, Hkv, D = 64, 2, 2, 3
    Sk = 5 * blk
    k = np.random.default_rng(1).standard_normal((B, Hkv, Sk, D))
    old, new = [blk - 1, 2 * blk + 5], [blk + 1, 2 * blk + 5]
    cache, first = ref.update(np.full((B, Hkv, 5, 2, D), -7.0), k, old, [0, 0], blk)
    assert first.tolist() == [[True, False, False, False, False], [True, True, True, False, False]]
    got, wrote = ref.update(cache, k, new, [old[0], new[1]], blk)
    assert wrote.tolist() == [[True, True, False, False, False], [False, False, True, False, False]]
    fresh = ref.bounds(k, new, blk)
    assert np.array_equal(got[0, :, :2], fresh[0, :, :2]) and np.array_equal(got[1, :, :3], fresh[1, :, :3])
    assert (got[0, :, 2:] == -7.0).all() and (got[1, :, 3:] == -7.0).all()


@pytest.mark.parametrize("blk,heads,causal", [(64, "kv", False), (128, "q", True), (64, "q", False), (128, "kv", True)])
def test_no_key_of_a_visible_block_scores_above_the_block(blk, heads, causal):
    """The defining property, in fp64: t >= max over the block's keys below kv_len of qs . k."""
    B, H, Hkv, D = 2, 4, 2, 16
    Sk, Sq = 4 * blk + 31, 2 * blk + 5
    lens = [Sk, 2 * blk + 7]
    rng = np.random.default_rng(blk + len(heads))
    q, k = rng.standard_normal((B, H, Sq, D)), rng.standard_normal((B, Hkv, Sk, D))
    r = ref.select(q, k, 2, blk=blk, lens=lens, causal=causal, mask_heads=heads)
    qs = ref.pooled_query(q, blk, heads, Hkv)
    Hl = qs.shape[1]
    seen = tight = 0
    for b in range(B):
        for hl in range(Hl):
            dots = qs[b, hl] @ k[b, hl // (Hl // Hkv)].T                # [NQ, Sk]
            for i in range(qs.shape[2]):
                for j in range(-(-Sk // blk)):
                    if r["vis"][b, i, j]:
                        best = dots[i, j * blk:min((j + 1) * blk, lens[b])].max()
                        assert r["t"][b, hl, i, j] >= best - 1e-12 * ref.magnitude(q, ref.bounds(k, lens, blk), blk, heads)[b, hl, i, j]
                        seen += 1
                        tight += int(r["t"][b, hl, i, j] > best + 1e-9)
    assert seen > 20 and tight > 0


@pytest.mark.parametrize("blk", [64, 128])
def test_the_needle_is_dropped_by_the_mean_and_kept_by_the_bound(blk):
    B, H, Hkv, D, NK = 2, 4, 2, 16, 6
    needle = [3, 5]
    q, k = ref.needle_inputs(B, H, Hkv, D, blk, NK, needle, 5)
    assert np.array_equal(q, np.round(q)) and np.array_equal(k, np.round(k))
    mean = select_ref.select(q, k, 1, blk=blk)
    bound = ref.select(q, k, 1, blk=blk)
    g = H // Hkv
    for b in range(B):
        others = [j for j in range(NK) if j != needle[b]]
        tm, tb = mean["t"][b, :, 0], bound["t"][b, :, 0]       # [Hl, NK]
        assert (tm[:, [needle[b]]] < tm[:, others]).all()       # below every other block's mean score
        assert (tm[:, needle[b]] == (4 - 2 * (blk - 1)) * D * g / blk).all()
        assert (tb[:, needle[b]] == 4 * D * g).all() and (tb[:, others] <= 2 * D * g).all()
        assert not mean["mask"][b, :, 0, needle[b]].any() and mean["mask"][b, :, 0, 0].all()
        assert bound["mask"][b, :, 0, needle[b]].all()
    assert (mean["mask"].sum(-1) == 1).all() and (bound["mask"].sum(-1) == 1).all()


@pytest.mark.parametrize("heads,causal", [("kv", True), ("q", False)])
def test_constant_blocks_give_the_mean_selection(heads, causal):
    """Every key of a block identical: mn = mx = the mean, so the bound is the mean score."""
    blk, B, H, Hkv, D, NK = 64, 2, 4, 2, 8, 7
    rng = np.random.default_rng(3)
    Sk = NK * blk - 20
    q = rng.integers(-2, 3, (B, H, 2 * blk, D)).astype(np.float64)
    k = np.repeat(rng.integers(-2, 3, (B, Hkv, NK, D)).astype(np.float64), blk, axis=2)[:, :, :Sk]
    lens = [Sk, 3 * blk + 9]
    kw = dict(blk=blk, lens=lens, causal=causal, keep_first=1, keep_local=1, mask_heads=heads)
    a, b = ref.select(q, k, 3, **kw), select_ref.select(q, k, 3, **kw)
    assert np.array_equal(a["t"], b["t"]) and np.array_equal(a["mask"], b["mask"]) and np.isfinite(a["t"]).any()
    ap = ref.select(q, k, 5, top_p=0.8, **kw)
    bp = select_p_ref.select(q, k, 5, 0.8, **kw)
    assert np.array_equal(ap["mask"], bp["mask"]) and np.array_equal(ap["mass"], bp["mass"])


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) -------------------------------------------
def _k(B=2, Hkv=2, Sk=700, D=64, dt=torch.bfloat16):
    return torch.zeros(B, Hkv, Sk, D, dtype=dt)


def _cache(B=2, Hkv=2, NK=6, D=64):
    return torch.zeros(B, Hkv, NK, 2, D, dtype=torch.float32)


def test_both_are_exported_from_the_package():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import block_sparse, pool_key_bounds, select_blocks_bound
    assert callable(pool_key_bounds) and callable(block_sparse.pool_key_bounds)
    assert callable(select_blocks_bound) and callable(block_sparse.select_blocks_bound)
    assert {"pool_key_bounds", "select_blocks_bound"} <= set(dir(rectified_spaattn_amd))


def test_pool_key_bounds_refusals():
    from rectified_spaattn_amd import pool_key_bounds
    k = _k()
    with pytest.raises(NotImplementedError, match="pool_key_bounds.*block_size"):
        pool_key_bounds(k, block_size=96)
    with pytest.raises(ValueError, match="tensor"):
        pool_key_bounds(k[0])
    with pytest.raises(ValueError, match="dtype"):
        pool_key_bounds(k.float())
    with pytest.raises(ValueError, match="head dim"):
        pool_key_bounds(_k(D=48))
    with pytest.raises(ValueError, match="kv_len"):
        pool_key_bounds(k, kv_len=701)
    with pytest.raises(ValueError, match="out: required"):
        pool_key_bounds(k, start=5)
    # out: fp32, contiguous, the 5-d shape -- the message names it; the 4-d cache of pool_keys is refused
    mean_cache = torch.zeros(2, 2, 6, 64)
    for bad in (_cache().double(), _cache(NK=5), _cache(D=128), _cache()[..., ::2], mean_cache, torch.zeros(2, 2, 6, 3, 64), [0.0]):
        with pytest.raises(ValueError, match=r"out: a contiguous float32 tensor \[2, 2, 6, 2, 64\]"):
            pool_key_bounds(k, out=bad)
    for w in (0, -1, True):
        with pytest.raises(ValueError, match="workgroups_per_head"):
            pool_key_bounds(k, workgroups_per_head=w)
    # scales belong to an e4m3 cache, and an e4m3 cache needs one
    with pytest.raises(ValueError, match="k_scale.*float8_e4m3fn cache"):
        pool_key_bounds(k, k_scale=0.5)
    k8 = torch.zeros(2, 2, 700, 64, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="k_scale: required"):
        pool_key_bounds(k8)
    with pytest.raises(NotImplementedError, match="e4m3"):
        pool_key_bounds(torch.zeros(2, 2, 700, 32, dtype=torch.float8_e4m3fn), k_scale=1.0)
    pool = torch.zeros(9, 2, 128, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block_table"):
        pool_key_bounds(pool, block_table=torch.zeros(2, 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="not copied"):
        pool_key_bounds(k.transpose(2, 3).contiguous().transpose(2, 3))


def test_a_misaligned_cache_is_refused(monkeypatch):
    """The alignment checks stand behind the device check: CPU tensors pass for device ones here, and nothing is launched."""
    from rectified_spaattn_amd import _core, pool_key_bounds, select_blocks_bound
    monkeypatch.setattr(_core, "_require_device", lambda *ts: None)
    flat = torch.zeros(2 * 2 * 6 * 2 * 64 + 4, dtype=torch.float32)
    off = 1 if flat.data_ptr() % 16 == 0 else 0
    shifted = flat[off:off + 2 * 2 * 6 * 2 * 64].view(2, 2, 6, 2, 64)
    assert shifted.data_ptr() % 16 and shifted.is_contiguous()
    with pytest.raises(ValueError, match="out: 16-byte aligned"):
        pool_key_bounds(_k(), out=shifted)
    with pytest.raises(ValueError, match="key_bounds: 16-byte aligned"):
        select_blocks_bound(torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16), shifted, 2)


def test_select_blocks_bound_refusals():
    from rectified_spaattn_amd import select_blocks_bound as sel, select_blocks_pooled
    q, kb = torch.zeros(2, 8, 1, 64, dtype=torch.bfloat16), _cache()
    shape = r"\[B, Hkv, NK, 2, D\]"
    # the wrong cache rank, for each of the two select functions
    with pytest.raises(ValueError, match="key_bounds.*" + shape + ".*pool_keys belongs to select_blocks_pooled"):
        sel(q, torch.zeros(2, 2, 6, 64), 2)
    with pytest.raises(ValueError, match=r"pooled_k \[B, Hkv, NK, D\].*select_blocks_bound"):
        select_blocks_pooled(q, kb, 2)
    for bad in (kb.bfloat16(), kb.double(), torch.zeros(2, 2, 6, 3, 64), kb[..., ::2], kb.transpose(1, 2), kb[0], [0.0]):
        with pytest.raises(ValueError, match="key_bounds: a contiguous float32 tensor " + shape):
            sel(q, bad, 2)
    with pytest.raises(NotImplementedError, match="select_blocks_bound.*block_size"):
        sel(q, kb, 2, block_size=96)
    with pytest.raises(ValueError, match="mask_heads"):
        sel(q, kb, 2, mask_heads="all")
    for name in ("top_k", "keep_first", "keep_local"):
        with pytest.raises(ValueError, match=name):
            sel(q, kb, **{"top_k": 2, name: -1})
    for bad in (0, 257, True):
        with pytest.raises(ValueError, match="score_splits"):
            sel(q, kb, 2, score_splits=bad)
    with pytest.raises(ValueError, match="tensor"):
        sel(q[0], kb, 2)
    with pytest.raises(ValueError, match="Hkv"):
        sel(q, _cache(Hkv=3), 2)
    with pytest.raises(ValueError, match="match"):
        sel(q, _cache(B=1), 2)
    with pytest.raises(ValueError, match="match"):
        sel(q, _cache(D=128), 2)
    with pytest.raises(ValueError, match="dtype"):
        sel(q.float(), kb, 2)
    with pytest.raises(ValueError, match="at most 8192"):
        sel(torch.zeros(1, 1, 1, 16, dtype=torch.bfloat16), torch.zeros(1, 1, 8193, 2, 16), 2)
    for kv_len in (6 * 128 + 1, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="kv_len"):
            sel(q, kb, 2, kv_len=kv_len)
    with pytest.raises(ValueError, match="top_p"):
        sel(q, kb, 2, top_p=1.5)
    with pytest.raises(ValueError, match="score_scale"):
        sel(q, kb, 2, score_scale=1.0)
    with pytest.raises(ValueError, match="return_mass"):
        sel(q, kb, 2, return_mass=True)
    with pytest.raises(ValueError, match="q_len"):
        sel(q, kb, 2, q_len=[1, 2])
    cu = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="max_q_len"):
        sel(q, kb, 2, max_q_len=1)
    with pytest.raises(ValueError, match="packed"):
        sel(q, kb, 2, cu_seqlens_q=cu, max_q_len=1)
    with pytest.raises(ValueError, match="max_q_len"):
        sel(torch.zeros(5, 8, 64, dtype=torch.bfloat16), kb, 2, cu_seqlens_q=cu)
    with pytest.raises(ValueError, match="q_len belongs"):
        sel(torch.zeros(5, 8, 64, dtype=torch.bfloat16), kb, 2, cu_seqlens_q=cu, max_q_len=2, q_len=[1, 1])


@pytest.mark.parametrize("kw", [dict(), dict(causal=True, kv_len=[700, 333], keep_first=1, keep_local=1, return_scores=True),
                                dict(mask_heads="q", as_lists=True, score_splits=7), dict(top_p=0.9, return_mass=True),
                                dict(q_len=[1, 0]), dict(packed=True)],
                         ids=["plain", "causal-lens", "q-lists-splits", "top-p", "ragged", "packed"])
def test_well_formed_calls_on_cpu_tensors_reach_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, pool_key_bounds, select_blocks_bound as sel
    kw = dict(kw)
    q = torch.zeros(2, 8, 3, 64, dtype=torch.float16)
    if kw.pop("packed", False):
        q = torch.zeros(5, 8, 64, dtype=torch.float16)
        kw.update(cu_seqlens_q=torch.tensor([0, 3, 5], dtype=torch.int32), max_q_len=3)
    with pytest.raises(_lib.RsaError):
        sel(q, _cache(), 2, **kw)
    with pytest.raises(_lib.RsaError):
        pool_key_bounds(_k(), kv_len=[700, 333], start=[650, 333], out=_cache())
    with pytest.raises(_lib.RsaError):
        pool_key_bounds(torch.zeros(2, 2, 700, 64, dtype=torch.float8_e4m3fn), k_scale=0.5)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_declared_listed_in_the_header_s_order_and_exported():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTED, name
    order = [n for n in re.findall(r"\bint\s+(rsa_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)) if n in NAMES]
    assert [n for n in _lib.PROTOTYPES if n in NAMES] == order == list(NAMES)
    P = _lib.PROTOTYPES
    assert P["rsa_pool_key_bounds"] == P["rsa_pool_keys"] and P["rsa_pool_key_bounds_kv8"] == P["rsa_pool_keys_kv8"]
    assert P["rsa_block_select_bound_bytes"] == P["rsa_block_select_pooled_bytes"]
    assert P["rsa_block_select_bound"] == P["rsa_block_select_pooled_ragged"]
    assert P["rsa_block_select_bound_packed"] == P["rsa_block_select_pooled_packed"]
    assert _lib.EXPORTED[-3:] == ("rsa_block_sparse_extend_bytes", "rsa_block_sparse_extend", "rsa_block_sparse_extend_kv8")
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    _, L = _lib_or_skip()
    assert all(hasattr(L, name) for name in NAMES) and L.rsa_version() == 601


def test_workspace_size_query_is_the_pooled_one():
    _, L = _lib_or_skip()
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for args in ((2, 2, 2, 128, 1, 6), (1, 8, 32, 128, 1, 1024), (3, 2, 2, 16, 5, 8192)):
        assert L.rsa_block_select_bound_bytes(*args, ctypes.byref(n)) == 0
        assert L.rsa_block_select_pooled_bytes(*args, ctypes.byref(m)) == 0
        B, _, Hl, D, NQ, NK = args
        assert n.value == m.value == B * Hl * NQ * (D + NK) * 4
    assert L.rsa_block_select_bound_bytes(2, 2, 2, 128, 1, 6, None) == -1
    assert L.rsa_block_select_bound_bytes(2, 0, 2, 128, 1, 6, ctypes.byref(n)) == -1
    assert L.rsa_block_select_bound_bytes(2, 2, 2, 96, 1, 6, ctypes.byref(n)) == -2
    assert L.rsa_block_select_bound_bytes(2, 2, 2, 128, 1, 8193, ctypes.byref(n)) == -2


@pytest.mark.parametrize("kv8", [False, True], ids=["2-byte", "e4m3"])
def test_pool_key_bounds_entries_check_their_arguments(kv8):
    """Before any launch, with rsa_pool_keys' statuses: each call is made to both entries."""
    _lib, L = _lib_or_skip()
    BAD, UNS = -1, -2
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks

    def call(B=2, Hkv=2, Sk=700, D=128, dt=0, blk=128, NK=6, k=t, table=None, tsb=6, pages=0, kv=None, kvv=700, st=None, stv=0,
             wph=0, out=p, ks=p):
        if kv8:
            args = (B, Hkv, Sk, D, blk, NK, k, table, tsb, pages, kv, kvv, st, stv, wph, out, ks, None)
            got, want = L.rsa_pool_key_bounds_kv8(*args), L.rsa_pool_keys_kv8(*args)
        else:
            args = (B, Hkv, Sk, D, dt, blk, NK, k, table, tsb, pages, kv, kvv, st, stv, wph, out, None)
            got, want = L.rsa_pool_key_bounds(*args), L.rsa_pool_keys(*args)
        assert got == want, (args, got, want)
        return got

    for base in (dict(), dict(kv=p, st=p), dict(table=p, pages=20, Sk=768), dict(stv=650)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(D=96) == UNS
        assert c(D=8) == UNS
        assert (c(D=32) if kv8 else c(dt=7)) == UNS  # (an e4m3 cache serves head dims 64 / 128; it has no dtype)
        assert c(Sk=8193 * 128, NK=8193) == UNS
        assert c(B=0) == BAD
        assert c(Hkv=0) == BAD
        assert c(Sk=0) == BAD
        assert c(NK=0) == BAD
        assert c(NK=7) == BAD                        # not ceil(Sk / block)
        assert c(blk=64, NK=6) == BAD
        assert c(wph=-1) == BAD
        assert c(out=None) == BAD
        assert c(out=ctypes.c_void_p(4104)) == BAD   # 16-byte alignment: the selection reads 16 bytes a lane
        assert c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(st=ctypes.c_void_p(4097)) == BAD
        assert c(table=ctypes.c_void_p(4098), pages=20) == BAD
        assert c(table=p, pages=0) == BAD
        assert c(table=p, pages=20, tsb=-6) == BAD
        assert c(k=_lib.RsaTensor4(None, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4100, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        if kv8:
            assert c(ks=None) == BAD
            assert c(ks=ctypes.c_void_p(4098)) == BAD
        if "kv" not in base:                         # the host limits: 0 .. Sk
            assert c(kvv=-1) == BAD
            assert c(kvv=base.get("Sk", 700) + 1) == BAD
            assert c(stv=-1) == BAD
            assert c(stv=base.get("Sk", 700) + 1) == BAD


@pytest.mark.parametrize("packed", [False, True], ids=["ragged-list", "packed-list"])
def test_selection_entries_check_their_arguments(packed):
    """Before any launch, with rsa_block_select_pooled's statuses in its order: each call is made to the pooled entry of the same
    argument list too, and where two things are wrong both answer alike."""
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)
    big = 1 << 30

    def call(B=2, H=8, Hkv=2, Hl=2, Sq=1, D=128, dt=0, blk=128, NQ=1, NK=6, q=t, pk=p, kv=None, kvv=700, causal=0, top_k=2, kf=0,
             kl=0, splits=0, ws=p, wsb=big, bitmask=p, cols=p, counts=p, scores=None, p16=-1, c=0.0, mass=None, ql=None, T=5,
             cu=p, items=p):
        head = (B, H, Hkv, Hl, Sq, D, dt, blk, NQ, NK, q, pk, kv, kvv, causal, top_k, kf, kl, splits, ws, wsb, bitmask, cols, counts,
                scores, p16, c, mass)
        if packed:
            args = (T,) + head + (cu, items, None)
            got, want = L.rsa_block_select_bound_packed(*args), L.rsa_block_select_pooled_packed(*args)
        else:
            args = head + (ql, None)
            got, want = L.rsa_block_select_bound(*args), L.rsa_block_select_pooled_ragged(*args)
        assert got == want, (args, got, want)
        return got

    for kw in (dict(H=0), dict(Hkv=0), dict(Hl=0), dict(Hkv=3, Hl=3), dict(Hl=4), dict(Hl=1), dict(H=6, Hkv=4, Hl=4)):
        assert call(**kw) == BAD, kw
    for base in (dict(), dict(Hl=8), dict(causal=1, Sq=300, NQ=3, T=700), dict(scores=p), dict(kv=p), dict(splits=1), dict(splits=64),
                 dict(p16=32768, c=1.0, mass=p)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(D=96) == UNS
        assert c(D=8) == UNS
        assert c(dt=7) == UNS
        assert c(NK=8193) == UNS
        assert c(B=0) == BAD
        assert c(Sq=0) == BAD
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
        assert c(wsb=0) == WS
        assert c(NK=8192, wsb=0) == WS               # (the limit itself is served)
        # wrong in two ways: the earlier check decides, as in the pooled entry
        assert c(blk=96, B=0) == BAD and c(blk=96, D=96) == UNS and c(D=96, top_k=-1) == UNS and c(NK=8193, ws=None) == UNS
        assert c(pk=None, wsb=0) == BAD
        if "p16" in base:
            assert c(p16=65537) == BAD
            assert c(c=0.0) == BAD
            assert c(mass=ctypes.c_void_p(4098)) == BAD
        if packed:
            assert c(T=0) == BAD
            assert c(cu=None) == BAD
            assert c(items=ctypes.c_void_p(4098)) == BAD
            assert c(Sq=base.get("T", 5) + 1, NQ=-(-(base.get("T", 5) + 1) // 128)) == BAD       # M above T
        else:
            assert c(ql=ctypes.c_void_p(4098)) == BAD
            assert c(ql=p, wsb=0) == WS
        if "kv" not in base:                         # the host limit: 0 .. NK * block
            assert c(kvv=-1) == BAD
            assert c(kvv=6 * 128 + 1) == BAD
            assert c(kvv=6 * 128, wsb=0) == WS
    n = ctypes.c_size_t(0)
    assert L.rsa_block_select_bound_bytes(2, 2, 2, 128, 1, 6, ctypes.byref(n)) == 0
    assert call(wsb=n.value - 1) == WS
    assert call(wsb=n.value, blk=96) == UNS
