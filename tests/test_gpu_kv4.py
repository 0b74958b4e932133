"""The MXFP4 K/V cache on the device: append_kv_mxfp4, block_sparse_decode and pool_keys over e2m1 codes
with one e8m0 scale byte per 32 channels: the writer's bytes against tests/kv4_ref.py, decode and pool_keys byte-equal to the 2-byte
calls on the dequantised cache, a written cache against fp64, the step in one graph.  Shapes are the decode tests': capacity 700,
B = 2, H = 4 over Hkv = 2; codes and scales beyond kv_len[b] and in spare pages are 0xFF."""
import numpy as np
import pytest
import torch

import decode_ref as ref
import kv4_ref as kv4
import kv8_ref
from test_gpu_decode import LSE_TOL, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SK = ref.SK
B, H, HKV = 2, 4, 2
LENS = [SK, 333]
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = 0xA5
FORMS = [(dt, D, paged) for dt in ("bf16", "fp16") for D in (64, 128) for paged in (False, True)]
IDS = [f"{dt}-D{D}-{'paged' if p else 'contig'}" for dt, D, p in FORMS]


def _blk(D, paged):         # both block sizes at both head dims over the eight forms
    return 64 if (D == 64) != paged else 128


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    view = torch.uint8 if a.element_size() == 1 else torch.int16 if a.element_size() == 2 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def _random_cache(D, seed, lens=LENS):
    """Random code bytes, random scale bytes over the writer's whole range, 0xFF beyond kv_len[b]: [kc, ks, vc, vs]."""
    rng = np.random.default_rng(seed)
    arrays = [rng.integers(0, 256, (B, HKV, SK, D // 2), dtype=np.uint8), rng.integers(114, 141, (B, HKV, SK, D // 32), dtype=np.uint8),
              rng.integers(0, 256, (B, HKV, SK, D // 2), dtype=np.uint8), rng.integers(114, 141, (B, HKV, SK, D // 32), dtype=np.uint8)]
    for a in arrays:
        for b, n in enumerate(lens):
            a[b, :, n:] = kv4.FILL
    return arrays


def _dequantised(arrays, dt):
    return [torch.from_numpy(kv4.dequant(arrays[i], arrays[i + 1])).to(DEV, TDT[dt]) for i in (0, 2)]


# ---- 1. the writer -------------------------------------------------------------------------------------------------------------------
EDGES = np.array([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -0.0, 0.0, -1e-3, 7.9,
                  -7.5, 6.0, -6.0, np.nan, 0.5, 1.0, 1.5, 2.0, 3.0, 0.24, 0.76, 5.1, 4.9], np.float32)


def _new_rows(T, D, dt, seed):
    """Random rows over the exponent range; in the first group of the first tokens the named edges: ties and saturation under
    e = -5, 0, 5, +-Inf, both clamp ends (fp16 subnormals among them), an all-NaN group."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HKV, T, D, generator=g) * torch.exp2(torch.randint(-18, 17, (B, HKV, T, D // 32, 1), generator=g).float()).expand(
        B, HKV, T, D // 32, 32).reshape(B, HKV, T, D)
    rows = [EDGES * 2.0 ** -5, EDGES, EDGES * 2.0 ** 5, np.where(np.arange(32) % 3 == 0, np.inf, EDGES * 1000) * np.where(np.arange(32) % 2, -1, 1),
            EDGES * 2.0 ** -14, EDGES * 2.0 ** 13, np.full(32, np.nan)]
    for t, r in enumerate(rows[:T]):
        x[:, :, t, :32] = torch.from_numpy(np.asarray(r, np.float32))
    return x.to(TDT[dt])


def _writes(blk):
    """(start per item, n_new per item | None, T, limits on the device)."""
    return [([5, 70], None, 7, False), ([blk - 3, 2 * blk - 3], None, 7, False), ([blk - 3, 2 * blk - 3], None, blk + 10, False),
            ([0, 130], [2, 0], 7, False), ([0, 0], None, blk, True), ([SK - 2, SK], None, 7, False), ([690, 3], [40, 1], 40, True)]


@pytest.mark.parametrize("dt,D,paged", FORMS, ids=IDS)
def test_writer_bytes_placement_and_untouched_sentinel(dt, D, paged):
    from rectified_spaattn_amd import append_kv_mxfp4
    blk = _blk(D, paged)
    NK = -(-SK // blk)
    table, tab, lead = None, None, (B, HKV, SK)
    if paged:
        P = B * NK + 2
        table = np.random.default_rng(blk + D).permutation(P)[:B * NK].reshape(B, NK).astype(np.int32)
        table[0, 2], table[1, 1] = -1, P + 5            # two blocks without a page: their rows are dropped
        tab, lead = _dev(table), (P, HKV, blk)
    model = [np.full(lead + (last,), SENTINEL, np.uint8) for last in (D // 2, D // 32, D // 2, D // 32)]
    caches = [_dev(m) for m in model]
    placed = 0
    for i, (start, n_new, T, on_device) in enumerate(_writes(blk)):
        news = [_new_rows(T, D, dt, 10 * i + s) for s in (1, 2)]
        counts = [T, T] if n_new is None else n_new
        as_arg = (lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)) if on_device else (lambda v: v)      # noqa: E731
        kw = dict(start=as_arg(start), n_new=None if n_new is None else as_arg(n_new), block_size=blk, block_table=tab)
        for again in range(2 if i == 3 else 1):         # (the call again: the same bytes)
            append_kv_mxfp4(news[0].to(DEV), news[1].to(DEV), *caches, **kw)
        want = kv4.quantize(news[0]) + kv4.quantize(news[1])
        for j in range(4):
            model[j], wrote = kv8_ref.append(model[j], want[j], start, counts, blk, table)
            assert np.array_equal(caches[j].cpu().numpy(), model[j]), (i, "kc ks vc vs".split()[j])
        placed += int(wrote.sum())
    assert 0 < placed and (model[0] == SENTINEL).mean() > 0.3       # (the sentinel survives everywhere else)
    assert {114, 140} <= set(np.unique(model[1]).tolist())           # both clamp ends were written


@pytest.mark.parametrize("writer", ["e4m3", "mxfp4"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_both_writers_place_across_a_page_edge_under_device_limits(writer, dt, D):
    """B = 2, Hkv = 2, T = 3, two 64-token pages per item: item 0 starts at 62 and straddles the page edge, its second page's entry
    is P (out of range: that token is dropped); item 1 starts at 126 with n_new = 2 on the device, and its third token would lie
    beyond the capacity.  Every byte of codes and scales against the model, the sentinel everywhere else."""
    from rectified_spaattn_amd import append_kv_e4m3, append_kv_mxfp4
    T, blk, P, start, n_new = 3, 64, 5, [62, 126], [3, 2]
    table = np.array([[3, P], [0, 4]], np.int32)
    news = [_new_rows(T, D, dt, s) for s in (1, 2)]
    if writer == "e4m3":
        pair = (np.array([0.37, 4.0], np.float32), np.array([2.3, 0.11], np.float32))
        want, lasts = [kv8_ref.quantize(x, s) for x, s in zip(news, pair)], (D, D)
        call = lambda *c, **kw: append_kv_e4m3(*c[:2], *(t.view(torch.float8_e4m3fn) for t in c[2:]), **kw,     # noqa: E731
                                               k_scale=_dev(pair[0]), v_scale=_dev(pair[1]))
    else:
        want, lasts, call = kv4.quantize(news[0]) + kv4.quantize(news[1]), (D // 2, D // 32, D // 2, D // 32), append_kv_mxfp4
    caches = [_dev(np.full((P, HKV, blk, last), SENTINEL, np.uint8)) for last in lasts]
    kw = dict(start=torch.tensor(start, dtype=torch.int32, device=DEV), n_new=torch.tensor(n_new, dtype=torch.int32, device=DEV),
              block_size=blk, block_table=_dev(table))
    call(news[0].to(DEV), news[1].to(DEV), *caches, **kw)
    for j, (cache, new) in enumerate(zip(caches, want)):
        model, wrote = kv8_ref.append(np.full(cache.shape, SENTINEL, np.uint8), new, start, n_new, blk, table)
        assert np.array_equal(cache.cpu().numpy(), model), j
        assert int(wrote[:, 0, :, 0].sum()) == 4 and not wrote[[1, 2]].any()      # 62, 63 of item 0 and 126, 127 of item 1; no other page


# ---- 2. decode: the bytes of the 2-byte call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,paged", FORMS, ids=IDS)
def test_decode_gives_the_bytes_of_the_two_byte_call_on_the_dequantised_cache(dt, D, paged):
    from rectified_spaattn_amd import block_sparse_decode as dec
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    blk = _blk(D, paged)
    NK = -(-SK // blk)
    arrays = _random_cache(D, D + paged)
    kd, vd = _dequantised(arrays, dt)
    if paged:       # garbage table entries where no key is, 0xFF in every spare byte
        arrays, table, _ = kv4.paged(arrays, blk, LENS, D, bad=-1 if dt == "bf16" else 10 ** 6)
    kc, ks, vc, vs = (_dev(a) for a in arrays)
    g = torch.Generator().manual_seed(D)
    for Sq in (1, 4):
        q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
        for causal in (False, True):
            for Hl, as_lists, bps in ((HKV, False, None), (H, True, None), (1, False, 2)):     # (2 blocks a split: several splits)
                mask = (torch.rand(B, Hl, 1, NK, generator=g) < 0.6).to(DEV)
                mask[..., 0] = True
                kw = dict(kv_len=LENS, block_size=blk, causal=causal, return_lse=True, blocks_per_split=bps)
                want = dec(q, kd, vd, mask, **kw)
                if paged:
                    kw["block_table"] = _dev(table)
                got = dec(q, kc, vc, block_mask_to_lists(mask, B, Hl) if as_lists else mask, k_block_scale=ks, v_block_scale=vs, **kw)
                assert _same(got[0], want[0]) and _same(got[1], want[1]), (Sq, causal, Hl)
                assert bool(torch.isfinite(got[0].float()).all()) and bool(got[0].any())
    again = dec(q, kc.view(torch.float4_e2m1fn_x2), vc.view(torch.float4_e2m1fn_x2), mask, k_block_scale=ks.view(torch.float8_e8m0fnu),
                v_block_scale=vs.view(torch.float8_e8m0fnu), **kw)
    assert _same(again[0], want[0]) and _same(again[1], want[1])      # the typed views are the same bytes; two calls, the same result


# ---- 3. a cache the writer wrote, against fp64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D", [("bf16", 128), ("fp16", 64)])
def test_written_cache_against_fp64_over_the_dequantised_operands(dt, D):
    """The tolerances of the same comparison over an e4m3 cache (tests/test_gpu_kv8.py), which are the plain call's."""
    from rectified_spaattn_amd import append_kv_mxfp4, block_sparse_decode as dec
    blk, Sq = 128, 4
    g = torch.Generator().manual_seed(D)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
    kf, vf = (torch.randn(B, HKV, SK, D, generator=g).to(torch.bfloat16) for _ in range(2))
    caches = [_dev(np.full((B, HKV, SK, last), kv4.FILL, np.uint8)) for last in (D // 2, D // 32, D // 2, D // 32)]
    append_kv_mxfp4(kf.to(DEV, TDT[dt]), vf.to(DEV, TDT[dt]), *caches, start=0, n_new=LENS)
    mask = (torch.rand(B, HKV, 1, -(-SK // blk), generator=g) < 0.6).to(DEV)
    mask[..., 0] = True
    out, lse = dec(q, caches[0], caches[2], mask, kv_len=LENS, causal=True, return_lse=True, k_block_scale=caches[1], v_block_scale=caches[3])
    kc, ks, vc, vs = (c.cpu().numpy() for c in caches)
    kd, vd = kv4.dequant(kc, ks), kv4.dequant(vc, vs)
    qn, sm = q.float().cpu().numpy(), D ** -0.5
    seen = ref.visible(mask.cpu().numpy(), LENS, Sq, SK, blk, H, True)
    want, _ = ref.attention(ref.scores2(qn, kd, sm), seen, vd)
    _, lse_hat = ref.attention(ref.scores2(qn, kd, sm, dt), seen, vd)
    exact, _ = ref.attention(ref.scores2(qn, kf.double().numpy(), sm), seen, vf.double().numpy())
    got, got_lse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    err, fmt = np.abs(got - want), np.abs(got - exact)
    d_hat = float(np.abs(got_lse - lse_hat).max())
    print(f"{dt} D{D}: out max {err.max():.3e} mean {err.mean():.3e}; lse {d_hat:.3e} (bound {LSE_TOL[dt]:.3e}); vs attention over the "
          f"un-quantised K / V (the format's, not gated): max {fmt.max():.3e} mean {fmt.mean():.3e}")
    assert seen.any(-1).all() and np.isfinite(got).all()
    assert err.max() < TOL[dt][0] and err.mean() < TOL[dt][1] and d_hat <= LSE_TOL[dt]


# ---- 4. pool_keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,paged", FORMS[:4], ids=IDS[:4])
def test_pool_keys_equals_the_two_byte_pool_incremental_and_zeros(dt, D, paged):
    from rectified_spaattn_amd import pool_keys
    blk = _blk(D, paged)
    NK = -(-SK // blk)
    arrays = _random_cache(D, 7 * D + paged)
    kd, _ = _dequantised(arrays, dt)
    fill = lambda: torch.full((B, HKV, NK, D), float("nan"), dtype=torch.float32, device=DEV)       # noqa: E731
    want = pool_keys(kd, block_size=blk, kv_len=LENS, out=fill())
    kw = dict(block_size=blk)
    if paged:
        arrays, table, P = kv4.paged(arrays, blk, LENS, D, bad=-1)
        kw["block_table"] = _dev(table)
    kc, ks = _dev(arrays[0]), _dev(arrays[1])
    got = pool_keys(kc, kv_len=LENS, out=fill(), k_block_scale=ks, **kw)
    assert _same(got, want) and bool(torch.isfinite(got[0]).all()) and bool(torch.isnan(got[1, :, -(-333 // blk):]).all())
    # incremental = from scratch: the cache of shorter limits, updated from them on the device, for several workgroup counts
    old = [blk + 1, 200]
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)       # noqa: E731
    stale = pool_keys(kc, kv_len=old, out=fill(), k_block_scale=ks, **kw)
    for wph in (None, 1, 3):
        upd = pool_keys(kc, kv_len=dev(LENS), start=dev(old), out=stale.clone(), k_block_scale=ks, workgroups_per_head=wph, **kw)
        assert _same(upd, want), wph
    assert not _same(stale, want)
    if paged:       # an out-of-range entry of a written block gives zeros
        t2 = kw["block_table"].clone()
        t2[0, 1] = P + 5
        z = pool_keys(kc, kv_len=LENS, out=fill(), k_block_scale=ks, block_size=blk, block_table=t2)
        assert bool((z[0, :, 1] == 0).all()) and _same(z[1], want[1]) and _same(z[0, :, 2:], want[0, :, 2:])


# ---- 5. one step, one graph --------------------------------------------------------------------------------------------------------------
def test_one_graph_for_the_four_calls_of_a_decode_step():
    """append_kv_mxfp4(start = prev) -> pool_keys(start = prev, out = pooled) -> select_blocks_pooled -> block_sparse_decode over a
    paged MXFP4 cache, captured on a side stream.  Replayed after another token (item 0's opens a block) and bumped device limits
    it equals the eager calls, three times."""
    from rectified_spaattn_amd import append_kv_mxfp4, block_sparse_decode, pool_keys, select_blocks_pooled
    Hq, Sq, D, blk, dt = 8, 1, 128, 128, torch.bfloat16
    NK = -(-SK // blk)
    lens = [511, 332]           # the step's token lands at 511 / 332; the next one opens item 0's fifth block
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, Hq, Sq, D, generator=g).to(DEV, dt)
    kf, vf = (torch.randn(B, HKV, SK, D, generator=g).to(dt) for _ in range(2))
    P = B * NK + 3
    table = torch.randperm(P, generator=g)[:B * NK].reshape(B, NK).to(torch.int32).to(DEV)
    caches = [_dev(np.full((P, HKV, blk, last), kv4.FILL, np.uint8)) for last in (D // 2, D // 32, D // 2, D // 32)]
    append_kv_mxfp4(kf.to(DEV), vf.to(DEV), *caches, start=0, n_new=lens, block_table=table)        # the prefill is the same call
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    prev = kv_len.clone()
    pooled = pool_keys(caches[0], kv_len=kv_len, block_table=table, k_block_scale=caches[1],
                       out=torch.full((B, HKV, NK, D), float("nan"), device=DEV))
    tok_k, tok_v = (torch.empty(B, HKV, 1, D, dtype=dt, device=DEV) for _ in range(2))
    sel_kw = dict(kv_len=kv_len, causal=True, keep_first=1, keep_local=1, as_lists=True)

    def feed(pos):              # the token of position pos[b], and the device limits after it
        for b in range(B):
            tok_k[b, :, 0], tok_v[b, :, 0] = kf[b, :, pos[b]].to(DEV), vf[b, :, pos[b]].to(DEV)
        prev.copy_(torch.tensor(pos, dtype=torch.int32))
        kv_len.copy_(prev + 1)

    def step(pooled, kc, ks, vc, vs):
        append_kv_mxfp4(tok_k, tok_v, kc, ks, vc, vs, start=prev, block_table=table)
        pool_keys(kc, kv_len=kv_len, start=prev, block_table=table, k_block_scale=ks, out=pooled)
        lists = select_blocks_pooled(q, pooled, 3, **sel_kw)
        return (lists,) + block_sparse_decode(q, kc, vc, lists, kv_len=kv_len, causal=True, return_lse=True, block_table=table,
                                              k_block_scale=ks, v_block_scale=vs)

    def same(a, b):
        assert torch.equal(a[0]["bitmask"], b[0]["bitmask"]) and torch.equal(a[0]["counts"], b[0]["counts"])
        assert _same(a[1], b[1]) and _same(a[2], b[2])

    feed(lens)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(pooled.clone(), *[c.clone() for c in caches])        # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step(pooled, *caches)
    before = None
    for pos in (lens, [n + 1 for n in lens], [n + 2 for n in lens]):
        feed(pos)
        stale = [pooled.clone()] + [c.clone() for c in caches]
        graph.replay()
        torch.cuda.synchronize()
        same(got, step(*stale))
        assert all(_same(a, b) for a, b in zip(stale, [pooled] + caches))
        assert before is None or not torch.equal(got[1], before)
        before = got[1].clone()
    opened = caches[0][table[0, 4].item(), :, 0]
    assert bool((opened != kv4.FILL).any()) and bool((caches[0][table[0, 4].item(), :, 2] == kv4.FILL).all())
    assert bool(torch.isfinite(got[1].float()).all()) and int(got[0]["counts"].min()) == 3
