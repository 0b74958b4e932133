"""pool_keys and select_blocks_pooled on the MI355X (rsa_pool_keys, rsa_block_select_pooled).

    selection      select_blocks_pooled(q, pool_keys(k, kv_len=L), kv_len=L) = select_blocks(q, k, kv_len=L), byte for byte (mask,
                   lists, scores), for every score_splits
    cache          against fp64 (tests/pooled_ref.py): bit-equal on small integers over power-of-two counts; on random normal data
                   over ragged counts within 4 (b + 1) 2^-24 mean|k_d| per channel -- four times the fp32 bound of a sum of b
                   terms and one division (section 5.11's convention)
    updates        incremental = from scratch, byte for byte, and nothing outside the written range moves
    paged          = contiguous, byte for byte; NaN beyond the limits stays where it is; device limits are not read on the host
    one graph      pool_keys -> select_blocks_pooled -> block_sparse_decode captured once, replayed on changed contents
"""
import itertools

import numpy as np
import pytest
import torch

import pooled_ref as ref
import select_ref
from test_gpu_decode import _pool
from test_gpu_select_blocks import KEEPS_TOPK, _top_k

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SK = 700                            # 6 blocks of 128, 11 of 64, a ragged last block
SENTINEL = -12345.6787109375        # (an fp32 value no pooled key takes)
SPLITS = (None, 1, 2, 7, 64)


def _randn(shape, dt, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32).to(DT[dt])


def _bits(t):
    return t.view(torch.uint8) if t.dtype == torch.bool else t.view(torch.int32)


def _same_lists(a, b, what):
    assert set(a) == set(b) == {"bitmask", "cols", "counts"}
    for name in ("bitmask", "counts"):
        assert a[name].dtype == torch.int32 and a[name].shape == b[name].shape and torch.equal(a[name], b[name]), (name, what)
    live = torch.arange(a["cols"].shape[-1], device=DEV)[None, None, :] < b["counts"][..., None]
    assert a["cols"].shape == b["cols"].shape
    assert torch.equal(torch.where(live, a["cols"], 0), torch.where(live, b["cols"], 0)), ("cols", what)


def _same_scores(a, b, what):
    assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), ("scores", what)


# ---- 1. the selection from the cache = select_blocks, byte for byte ----------------------------------------------------------------
CASES = [(dt, D, blk) for dt in DT for D in (16, 64, 128) for blk in (64, 128)]
HEAD_FORMS = list(itertools.product((4, 2, 1), ("kv", "q"), (False, True)))       # Hkv, mask_heads, causal: 12


def _one_shape(dt, D, blk, NK, Sq, Hkv, heads, causal, triple, seed, B=2, H=4, splits=SPLITS):
    from rectified_spaattn_amd import pool_keys, select_blocks, select_blocks_pooled
    Sk = (NK - 1) * blk + blk // 2 + 3
    lens = [Sk, max(Sk - 2 * blk - 17, 5)][:B]
    q, k = _randn((B, H, Sq, D), dt, seed), _randn((B, Hkv, Sk, D), dt, seed + 1)
    kf, kl, tk = triple
    kw = dict(block_size=blk, kv_len=lens, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads)
    what = (dt, D, blk, NK, Sq, Hkv, heads, causal, triple)
    want_lists, want_t = select_blocks(q, k, _top_k(tk, NK), as_lists=True, return_scores=True, **kw)
    cache = pool_keys(k, block_size=blk, kv_len=lens)
    assert cache.dtype == torch.float32 and cache.shape == (B, Hkv, NK, D) and cache.is_contiguous()
    for s in splits:
        lists, t = select_blocks_pooled(q, cache, _top_k(tk, NK), as_lists=True, return_scores=True, score_splits=s, **kw)
        _same_lists(lists, want_lists, what + (s,))
        _same_scores(t, want_t, what + (s,))
    mask = select_blocks_pooled(q, cache, _top_k(tk, NK), **kw)
    want_mask = select_blocks(q, k, _top_k(tk, NK), **kw)
    assert mask.dtype == torch.bool and mask.shape == want_mask.shape and torch.equal(mask, want_mask), what
    return int(want_lists["counts"].sum()), int(torch.isfinite(want_t).sum())


@pytest.mark.parametrize("dt,D,blk", CASES, ids=[f"{a}-D{b}-b{c}" for a, b, c in CASES])
def test_selection_from_the_cache_equals_select_blocks(dt, D, blk):
    """B = 2 with a limit per item, H = 4.  Twelve shapes (NK in 3, 70, 300 x Sq in 1, 3, block, 2.5 blocks); the twelve (Hkv,
    mask_heads, causal) forms and the 45 (keep_first, keep_local, top_k) triples take turns over them, shifted per case."""
    n = CASES.index((dt, D, blk))
    kept = seen = 0
    for m, (NK, Sq) in enumerate(itertools.product((3, 70, 300), (1, 3, blk, 2 * blk + blk // 2))):
        Hkv, heads, causal = HEAD_FORMS[(m + 5 * n) % 12]
        triple = KEEPS_TOPK[(12 * n + m + 7 * (n // 4)) % len(KEEPS_TOPK)]
        a, b = _one_shape(dt, D, blk, NK, Sq, Hkv, heads, causal, triple, 1000 * n + 10 * m)
        kept, seen = kept + a, seen + b
    assert kept > 0 and seen > kept


def test_every_head_form_meets_every_shape_and_every_triple_is_used():
    forms, triples = set(), set()
    for n in range(len(CASES)):
        for m in range(12):
            forms.add((m, (m + 5 * n) % 12))
            triples.add((12 * n + m + 7 * (n // 4)) % len(KEEPS_TOPK))
    assert len(forms) == 144 and len(triples) == len(KEEPS_TOPK)


def test_selection_at_the_key_block_limit():
    """NK = 8192 blocks of 64, B = H = 1, D = 16."""
    for Sq, causal, triple in ((1, True, (1, 2, 90)), (130, False, (0, 0, 4000))):
        kept, _ = _one_shape("bf16", 16, 64, 8192, Sq, 1, "kv", causal, triple, 31 + Sq, B=1, H=1)
        assert kept >= 90


# ---- 2. the cache against fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,blk", CASES, ids=[f"{a}-D{b}-b{c}" for a, b, c in CASES])
def test_cache_against_fp64(dt, D, blk):
    from rectified_spaattn_amd import pool_keys
    B, Hkv = 2, 3
    # exact: integers -2 .. 2, every valid-key count a power of two
    Sk = 5 * blk + blk // 2
    lens = [Sk, 3 * blk + blk // 4]
    ki = np.random.default_rng(D + blk).integers(-2, 3, (B, Hkv, Sk, D))
    k = torch.from_numpy(ki).to(DEV, DT[dt])
    NK = -(-Sk // blk)
    out = torch.full((B, Hkv, NK, D), SENTINEL, dtype=torch.float32, device=DEV)
    got = pool_keys(k, block_size=blk, kv_len=lens, out=out)
    assert got is out
    want, wrote = ref.make(ki.astype(np.float64), lens, blk, fill=SENTINEL)
    assert wrote.sum() == 6 + 4
    want32 = torch.from_numpy(want.astype(np.float32))
    assert np.array_equal(want32.double().numpy(), want), "the reference's means are not fp32 values"
    assert torch.equal(_bits(got.cpu()), _bits(want32))         # (the sentinel beyond ceil(len / b) included)
    # rounding: random normal data, ragged counts
    lens = [SK, 333]
    k = _randn((B, Hkv, SK, D), dt, D + blk)
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
    k64 = k.double().cpu().numpy()
    got = pool_keys(k, block_size=blk, kv_len=lens).cpu().numpy().astype(np.float64)
    want, wrote = ref.make(np.nan_to_num(k64), lens, blk, fill=0.0)
    tol = 4 * (blk + 1) * 2.0 ** -24 * select_ref.pooled(np.abs(np.nan_to_num(k64)), lens, blk)
    live = np.broadcast_to(wrote[:, None, :, None], got.shape)
    err = np.abs(np.where(live, got - want, 0.0))
    print(f"{dt} D{D} b{blk}: error / tol max {float((err[live] / tol[live]).max()):.3f}")
    assert np.isfinite(got[live]).all() and (err <= tol)[live].all()


# ---- 3. incremental = from scratch -------------------------------------------------------------------------------------------------
def _update_cases(b):
    """(old, new, start = "old" | "len") per batch item; every case meets item 0 and, shifted by one, item 1."""
    return [(b - 1, b, "old"), (b - 1, b + 1, "old"), (2 * b - 1, 3 * b + 1, "old"), (b, b, "old"), (2 * b + 5, b + 3, "len")]


@pytest.mark.parametrize("blk", [64, 128])
@pytest.mark.parametrize("form", ["list", "device"])
def test_incremental_update_equals_pooling_from_scratch(blk, form):
    from rectified_spaattn_amd import pool_keys
    B, Hkv, D, dt = 2, 2, 64, "bf16"
    NK = -(-SK // blk)
    cases = _update_cases(blk)
    full = _randn((B, Hkv, SK, D), dt, blk)
    nothing = 0
    for n in range(len(cases)):
        per = [cases[n], cases[(n + 1) % len(cases)]]
        old, new = [c[0] for c in per], [c[1] for c in per]
        starts = [c[0] if c[2] == "old" else c[1] for c in per]
        k = full.clone()
        for b in range(B):
            k[b, :, old[b]:] = float("nan")
        cache = pool_keys(k, block_size=blk, kv_len=old, out=torch.full((B, Hkv, NK, D), SENTINEL, dtype=torch.float32, device=DEV))
        for b in range(B):          # the append (or the truncation), in place
            k[b, :, old[b]:new[b]] = full[b, :, old[b]:new[b]]
            k[b, :, new[b]:] = float("nan")
        fresh = pool_keys(k, block_size=blk, kv_len=new, out=torch.full((B, Hkv, NK, D), SENTINEL, dtype=torch.float32, device=DEV))
        wrote = torch.zeros(B, NK, dtype=torch.bool)
        for b in range(B):
            wrote[b, list(ref.written(starts[b], new[b], blk))] = True
        nothing += int(not wrote[0].any())
        inside = wrote[:, None, :, None].expand(B, Hkv, NK, D).to(DEV)
        as_arg = (lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)) if form == "device" else list
        results = []
        for wph in (None, 1, 2, 5):
            # 1. the cache as it stood: below ceil(new / b) it becomes the fresh one
            c1 = pool_keys(k, block_size=blk, kv_len=as_arg(new), start=as_arg(starts), out=cache.clone(), workgroups_per_head=wph)
            for b in range(B):
                hi = -(-new[b] // blk)
                assert torch.equal(_bits(c1[b, :, :hi]), _bits(fresh[b, :, :hi])), (n, b, wph)
            assert torch.equal(_bits(c1[~inside]), _bits(cache[~inside])), (n, wph)
            # 2. a sentinel outside the expected range survives bit for bit
            c2 = torch.where(inside, cache, torch.full_like(cache, SENTINEL))
            c2 = pool_keys(k, block_size=blk, kv_len=as_arg(new), start=as_arg(starts), out=c2, workgroups_per_head=wph)
            assert bool((c2[~inside] == SENTINEL).all()), (n, wph)
            assert torch.equal(_bits(c2[inside]), _bits(fresh[inside])) and bool(torch.isfinite(c2[inside]).all()), (n, wph)
            results.append(c2)
        assert all(torch.equal(_bits(r), _bits(results[0])) for r in results)
    assert nothing >= 1         # (b -> b: nothing is written)


# ---- 4. paged = contiguous ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,blk,bad", [("bf16", 128, 128, "P+5"), ("fp16", 64, 64, -1), ("bf16", 16, 64, "P+5")])
def test_paged_equals_contiguous(dt, D, blk, bad):
    from rectified_spaattn_amd import pool_keys
    B, Hkv = 2, 2
    NK = -(-SK // blk)
    lens = [SK, 333]
    k = _randn((B, Hkv, SK, D), dt, D)
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
    want = pool_keys(k, block_size=blk, kv_len=lens, out=torch.full((B, Hkv, NK, D), SENTINEL, dtype=torch.float32, device=DEV))
    kp, _, table, P = _pool(k, k, blk, lens, D + blk, bad=bad)
    fill = lambda: torch.full((B, Hkv, NK, D), SENTINEL, dtype=torch.float32, device=DEV)       # noqa: E731
    got = pool_keys(kp, block_size=blk, kv_len=lens, block_table=table, out=fill())
    assert torch.equal(_bits(got), _bits(want)) and bool((got[1, :, -(-333 // blk):] == SENTINEL).all())
    assert bool(torch.isfinite(got[0]).all())
    # an update through the table, device limits
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)       # noqa: E731
    got = pool_keys(kp, block_size=blk, kv_len=dev(lens), start=dev([blk + 1, 333]), block_table=table, out=fill())
    assert torch.equal(_bits(got[0, :, 1:]), _bits(want[0, :, 1:])) and bool((got[0, :, 0] == SENTINEL).all())
    last = 332 // blk
    assert torch.equal(_bits(got[1, :, last]), _bits(want[1, :, last])) and bool((got[1, :, :last] == SENTINEL).all())
    # an out-of-range entry of a written block: zeros, and nothing else moves
    for entry in (P + 5, -1, P, 2 ** 31 - 1):
        t2 = table.clone()
        t2[0, 1] = entry
        got = pool_keys(kp, block_size=blk, kv_len=lens, block_table=t2, out=fill())
        assert bool((got[0, :, 1] == 0).all())
        got[0, :, 1] = want[0, :, 1]
        assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("H,Hkv,D,blk", [(8, 2, 128, 128), (4, 1, 16, 64)])
def test_views_of_one_fused_projection_run_without_a_copy(monkeypatch, H, Hkv, D, blk):
    from rectified_spaattn_amd import _core, pool_keys
    B = 2
    buf = _randn((B, SK, (H + 2 * Hkv) * D), "bf16", H + D)
    k = buf[..., H * D:(H + Hkv) * D].view(B, SK, Hkv, D).permute(0, 2, 1, 3)
    assert not k.is_contiguous()
    seen = []
    t4 = _core._t4
    monkeypatch.setattr(_core, "_t4", lambda t: (seen.append(t.data_ptr()), t4(t))[1])
    got = pool_keys(k, block_size=blk, kv_len=[SK, 333], out=torch.zeros(B, Hkv, -(-SK // blk), D, device=DEV))
    assert seen == [k.data_ptr()]
    want = pool_keys(k.contiguous(), block_size=blk, kv_len=[SK, 333], out=torch.zeros(B, Hkv, -(-SK // blk), D, device=DEV))
    assert torch.equal(_bits(got), _bits(want)) and bool(got.any())


# ---- 5. NaN containment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk,splits", [(128, 1), (64, 7)])
def test_nan_beyond_the_limits_is_never_read(blk, splits):
    from rectified_spaattn_amd import pool_keys, select_blocks_pooled
    B, H, Hkv, D, dt = 2, 4, 2, 64, "fp16"
    NK = -(-SK // blk)
    lens = [SK - 70, 333]
    q, clean_k = _randn((B, H, 3, D), dt, blk), _randn((B, Hkv, SK, D), dt, blk + 1)
    dirty_k = clean_k.clone()
    for b, n in enumerate(lens):
        clean_k[b, :, n:] = 0
        dirty_k[b, :, n:] = float("nan")
    clean = pool_keys(clean_k, block_size=blk, kv_len=lens, out=torch.zeros(B, Hkv, NK, D, device=DEV))
    dirty = pool_keys(dirty_k, block_size=blk, kv_len=lens, out=torch.full((B, Hkv, NK, D), float("nan"), device=DEV))
    for b, n in enumerate(lens):
        hi = -(-n // blk)
        assert torch.equal(_bits(dirty[b, :, :hi]), _bits(clean[b, :, :hi])) and bool(torch.isfinite(dirty[b, :, :hi]).all())
        assert hi < NK and bool(torch.isnan(dirty[b, :, hi:]).all())
    kw = dict(block_size=blk, kv_len=lens, causal=True, keep_first=1, as_lists=True, return_scores=True, score_splits=splits)
    lists, t = select_blocks_pooled(q, dirty, 3, **kw)
    want_lists, want_t = select_blocks_pooled(q, clean, 3, **kw)
    _same_lists(lists, want_lists, blk)
    _same_scores(t, want_t, blk)
    assert not bool(torch.isnan(t).any()) and bool(torch.isfinite(t).any()) and int(lists["counts"].min()) == 3


# ---- 6. limits on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [(torch.int32, 3), (torch.int64, 3), (torch.int64, 1)])
def test_device_limits_give_the_ints_result_and_are_not_read_on_the_host(monkeypatch, dtype, n):
    from rectified_spaattn_amd import pool_keys, select_blocks_pooled
    B, H, Hkv, D = 3, 4, 2, 128
    q, k = _randn((B, H, 3, D), "bf16", 9), _randn((B, Hkv, SK, D), "bf16", 10)
    lens, starts = ([700, 333, 517], [640, 333, 380]) if n == 3 else ([517], [380])
    one = lambda v: v if n == 3 else v[0]       # noqa: E731
    fill = lambda: torch.full((B, Hkv, 6, D), SENTINEL, dtype=torch.float32, device=DEV)       # noqa: E731
    kw = dict(causal=True, keep_first=1, keep_local=1, return_scores=True)
    host_cache = pool_keys(k, kv_len=one(lens), start=one(starts), out=fill())
    full_cache = pool_keys(k, kv_len=one(lens))
    on_host = select_blocks_pooled(q, full_cache, 3, kv_len=one(lens), **kw)
    kv, st = torch.tensor(lens, dtype=dtype, device=DEV), torch.tensor(starts, dtype=dtype, device=DEV)
    out = fill()
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("a device limit was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dev_cache = pool_keys(k, kv_len=kv, start=st, out=out)
        on_device = select_blocks_pooled(q, full_cache, 3, kv_len=kv, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    assert torch.equal(_bits(dev_cache), _bits(host_cache))
    assert bool((host_cache == SENTINEL).any()) and not bool((host_cache == SENTINEL).all())
    for a, b in zip(on_device, on_host):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(on_host[0].any()) and not bool(on_host[0].all())
    # a device limit beyond the capacity is clamped, a negative one is 0
    wild = pool_keys(k, kv_len=torch.tensor([10 ** 6], device=DEV), start=torch.tensor([-5], device=DEV), out=fill())
    assert torch.equal(_bits(wild), _bits(pool_keys(k)))


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    from rectified_spaattn_amd import pool_keys, select_blocks_pooled
    q, k = _randn((2, 8, 200, 128), "bf16", 21), _randn((2, 2, 9000, 128), "bf16", 22)
    caches = [pool_keys(k, kv_len=[9000, 4444], out=torch.zeros(2, 2, 71, 128, device=DEV)) for _ in range(2)]
    assert torch.equal(_bits(caches[0]), _bits(caches[1]))
    for s in (None, 1, 4):
        outs = [select_blocks_pooled(q, caches[0], 7, kv_len=[9000, 4444], causal=True, keep_local=1, return_scores=True, score_splits=s)
                for _ in range(2)]
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        assert bool(outs[0][0].any())


# ---- 8. one graph for the decode step ------------------------------------------------------------------------------------------------
def test_one_graph_for_the_three_calls_of_a_decode_step():
    """pool_keys(start = prev), select_blocks_pooled(as_lists) and block_sparse_decode(block_table, return_lse) captured together
    on a side stream; then, in place, one more key per item (item 0's opens a new block), kv_len and prev bumped, a page moved.
    The replay equals the eager three calls, and select_blocks on the gathered contiguous K feeding block_sparse_decode."""
    from rectified_spaattn_amd import block_sparse_decode, pool_keys, select_blocks, select_blocks_pooled
    B, H, Hkv, Sq, D, blk = 2, 8, 2, 1, 128, 128
    NK = -(-SK // blk)
    lens = [512, 333]           # item 0's next key opens a new block (the fifth), item 1's lands in the page that moves
    q = _randn((B, H, Sq, D), "bf16", 5)
    k, v = _randn((B, Hkv, SK, D), "bf16", 6), _randn((B, Hkv, SK, D), "bf16", 7)
    new_k, new_v = k[:, :, 600].clone(), v[:, :, 600].clone()
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    kp, vp, table, P = _pool(k, v, blk, [SK, SK], 11)       # (every block has a page: the new keys have somewhere to go)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    prev = kv_len.clone()
    cache = pool_keys(kp, kv_len=kv_len, block_table=table, out=torch.full((B, Hkv, NK, D), float("nan"), device=DEV))
    sel_kw = dict(kv_len=kv_len, causal=True, keep_first=1, keep_local=1, as_lists=True)
    dec_kw = dict(kv_len=kv_len, causal=True, block_table=table, return_lse=True)

    def step(cache):
        pool_keys(kp, kv_len=kv_len, start=prev, block_table=table, out=cache)
        lists = select_blocks_pooled(q, cache, 3, **sel_kw)
        return (lists,) + block_sparse_decode(q, kp, vp, lists, **dec_kw)

    def by_select_blocks():
        kc, vc = (p[table.long()].permute(0, 2, 1, 3, 4).reshape(B, Hkv, NK * blk, D) for p in (kp, vp))
        lists = select_blocks(q, kc, 3, **sel_kw)
        return (lists,) + block_sparse_decode(q, kc, vc, lists, kv_len=kv_len, causal=True, return_lse=True)

    def same(a, b):
        _same_lists(a[0], b[0], "graph")
        assert torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(cache.clone())             # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step(cache)
    graph.replay()
    torch.cuda.synchronize()
    same(got, step(cache.clone()))
    same(got, by_select_blocks())
    before = got[1].clone()
    # the step: one more key per batch item, in place
    prev.copy_(kv_len)
    for b in range(B):
        j, r = lens[b] // blk, lens[b] % blk
        kp[table[b, j].item(), :, r] = new_k[b]
        vp[table[b, j].item(), :, r] = new_v[b]
    kv_len += 1
    spare = sorted(set(range(P)) - set(table.reshape(-1).tolist()))[0]
    kp[spare], vp[spare] = kp[table[1, 2].item()].clone(), vp[table[1, 2].item()].clone()
    kp[table[1, 2].item()], vp[table[1, 2].item()] = float("nan"), float("nan")
    table[1, 2] = spare
    stale = cache.clone()
    graph.replay()
    torch.cuda.synchronize()
    same(got, step(stale))
    same(got, by_select_blocks())
    assert torch.equal(_bits(cache[0, :, :5]), _bits(pool_keys(kp, kv_len=kv_len, block_table=table)[0, :, :5]))
    assert not torch.equal(got[1], before) and bool(torch.isfinite(got[1].float()).all())
    assert int(got[0]["counts"].min()) == 3
