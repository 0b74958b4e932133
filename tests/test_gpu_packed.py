"""The packed calls on the device: block_sparse_extend / select_blocks_pooled(cu_seqlens_q=, max_q_len=) and
append_kv_e4m3(cu_seqlens=) over T = 300 rows that hold B = 4 items, capacity 700, NaN in the cache beyond kv_len[b] and in q's rows
outside every item.
  1. extend against fp64 attention over the rule of tests/packed_ref.py, within test_gpu_decode's TOL / LSE_TOL; rows outside every
     item and rows without a visible key exactly 0 / -inf
  2. extend byte for byte: item b's rows = block_sparse_extend on its slice and = the q_len= call on the padded copy, at an equal
     explicit blocks_per_split; paged = contiguous, lists = mask, a second call, e4m3 = the dequantised 2-byte cache; M = 1 = decode
  3. exact visibility witnesses on packed batches; malformed cu_seqlens_q = the sanitised rule, every row written
  4. selection = the q_len= call on the padded copy; append = the padded append
  5. the whole step on a paged e4m3 cache: packed = per item, nothing read on the host, one captured graph that follows cu_seqlens_q"""
import ctypes

import numpy as np
import pytest
import torch

import extend_ref as eref
import kv8_ref as kv8
import packed_ref as ref
import ragged_ref as rref
import test_gpu_decode as tgd
import test_gpu_kv8 as tg8
from rectified_spaattn_amd import block_sparse_extend as ext

pytestmark = pytest.mark.gpu
DEV = tgd.DEV
B, T, SK = ref.B, ref.T, ref.SK
TDT, TOL, LSE_TOL = tgd.TDT, tgd.TOL, tgd.LSE_TOL
COMBOS = ref.gpu_combos()


def _id(c):
    return (f"H{c['H']}kv{c['Hkv']}-D{c['D']}-{c['dt']}-b{c['blk']}-m{c['axis']}-l{c['lset']}-kv{'dev' if c['kv_dev'] else 'host'}-"
            f"{'causal' if c['causal'] else 'full'}-s{c['bps']}-{c['cache']}")


def _hl(c):
    return {"H": c["H"], "Hkv": c["Hkv"], "1": 1}[c["axis"]]


def test_combos_cover_every_axis_for_every_grouping():
    assert len(COMBOS) == 60
    for H, Hkv in eref.GROUPS:
        mine = [c for c in COMBOS if (c["H"], c["Hkv"]) == (H, Hkv)]
        for key, n in (("D", 1 if H == 72 else 2), ("dt", 2), ("blk", 2), ("axis", 3), ("causal", 2), ("lset", 3), ("kv_dev", 2),
                       ("cache", 3)):
            assert len({c[key] for c in mine}) == n, (H, Hkv, key)
        assert {c["bps"] for c in mine} >= {None, 1, 2} and any(c["bps"] == -(-SK // c["blk"]) for c in mine)


def _same(a, b):
    return all(tg8._same(x, y) for x, y in zip(a, b))


def _cu(cu):
    return torch.tensor(cu, dtype=torch.int32, device=DEV)


def _packed(qpad, s, ns, fill=float("nan")):
    """[B, H, M, D] -> [T, H, D]: item b's rows at s_b .., `fill` in the rows of no item."""
    out = torch.full((T, qpad.shape[1], qpad.shape[3]), fill, dtype=qpad.dtype, device=qpad.device)
    for b, n in enumerate(ns):
        out[s[b]:s[b] + n] = qpad[b, :, :n].transpose(0, 1)
    return out


def _item(pair, s, b, n):
    """Rows of item b of packed (out [T, H, D], lse [T, H]) in the padded call's layout: ([1, H, n, D], [1, H, n])."""
    out, lse = pair
    return out[s[b]:s[b] + n].transpose(0, 1)[None].contiguous(), lse[s[b]:s[b] + n].t()[None].contiguous()


@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_against_fp64_and_byte_for_byte(c):
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists, extend_default_split, packed_row_groups
    H, Hkv, D, blk, dt, Hl = c["H"], c["Hkv"], c["D"], c["blk"], c["dt"], _hl(c)
    lengths, M, gap = ref.LSETS[c["lset"]]
    cu = ref.cu_of(lengths, gap)
    s, ns = ref.sanitise(cu, T, M)
    NQ, NK = -(-M // blk), -(-SK // blk)
    lens = ref.combo_lens(c)
    g = torch.Generator().manual_seed(c["seed"])
    qpad = torch.randn(B, H, M, D, generator=g).to(DEV, TDT[dt])
    for b, n in enumerate(ns):
        qpad[b, :, n:] = float("nan")
    q = _packed(qpad, s, ns)
    kf, vf = (torch.randn(B, Hkv, SK, D, generator=g) for _ in range(2))
    pair = kv8.pow2_scales(Hkv, c["seed"])
    kc, vc, kd, vd = tg8._quantised(kf.numpy(), vf.numpy(), pair, lens, dt)
    ks, vs = tg8._scales(pair)
    if c["cache"] == "e4m3-paged":      # the 2-byte cache of this turn: what the codes hold
        k, v = kd, vd
    else:
        k, v = kf.to(DEV, TDT[dt]), vf.to(DEV, TDT[dt])
        tgd._nan_tail(k, v, lens)
    mask = (torch.rand(B, Hl, NQ, NK, generator=g) < 0.5).to(DEV)
    mask[:, ::2, :, 0] = True
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV) if c["kv_dev"] else list(lens)
    kw = dict(kv_len=kv_len, block_size=blk, causal=c["causal"], blocks_per_split=c["bps"], return_lse=True)
    pk = dict(cu_seqlens_q=_cu(cu), max_q_len=M)
    out, lse = base = ext(q, k, v, mask, **pk, **kw)
    torch.cuda.synchronize()
    assert out.shape == (T, H, D) and out.dtype == TDT[dt] and lse.shape == (T, H) and lse.dtype == torch.float32
    # the turn's cache form gives the contiguous call's bytes (garbage table entries where no key is)
    if c["cache"] == "bf16-paged":
        kp, vp, table, _ = tgd._pool(k, v, blk, lens, c["seed"], bad=-1 if c["seed"] % 2 else "P+5")
        assert _same(ext(q, kp, vp, mask, **pk, **dict(kw, block_table=table)), base)
    elif c["cache"] == "e4m3-paged":
        kp8, vp8, table8, _ = tg8._pool8(kc, vc, blk, lens, c["seed"], bad=-1)
        assert _same(ext(q, tg8._dev8(kp8), tg8._dev8(vp8), mask, k_scale=ks, v_scale=vs, **pk,
                         **dict(kw, block_table=torch.from_numpy(table8).to(DEV))), base)
    else:
        assert _same(ext(q, tg8._dev8(kc), tg8._dev8(vc), mask, k_scale=ks, v_scale=vs, **pk, **kw), ext(q, kd, vd, mask, **pk, **kw))

    # 1. against fp64 attention over the rule, item by item; the rows of no item exactly 0 / -inf
    item, _ = ref.row_items(cu, T, M)
    dead = torch.from_numpy(item < 0).to(DEV)
    assert not out[dead].any() and bool(torch.isneginf(lse[dead]).all()) and int(dead.sum()) == T - sum(ns) > 0
    mask_n = mask.cpu().numpy()
    sm = D ** -0.5
    worst = [0.0, 0.0, 0.0]
    for b, n in enumerate(ns):
        if n == 0:
            continue
        o1, l1 = _item(base, s, b, n)
        got, got_lse = o1.float().cpu().numpy().astype(np.float64), l1.cpu().numpy().astype(np.float64)
        qn = qpad[b:b + 1, :, :n].float().cpu().numpy()
        kn, vn = (t[b:b + 1].float().cpu().numpy() for t in (k, v))
        seen = rref.visible(mask_n[b:b + 1, :, :ref.live_blocks(n, blk)], lens[b:b + 1], [n], n, SK, blk, H, c["causal"])
        want, _ = rref.attention(qn, kn, vn, seen, sm)
        _, lse_hat = rref.attention(qn, kn, vn, seen, sm, dt)
        has = seen.any(-1)
        err = np.abs(got - want)
        assert np.isfinite(got).all() and (got[~has] == 0).all() and np.isneginf(got_lse[~has]).all()
        assert np.isfinite(got_lse[has]).all()
        d_hat = float(np.abs(got_lse[has] - lse_hat[has]).max()) if has.any() else 0.0
        worst = [max(worst[0], float(err.max())), max(worst[1], float(err.mean())), max(worst[2], d_hat)]
    print(f"{_id(c)}: out max {worst[0]:.3e} mean (worst item) {worst[1]:.3e}; lse vs quantised {worst[2]:.3e} (bound {LSE_TOL[dt]:.3e})")
    assert worst[0] < TOL[dt][0] and worst[1] < TOL[dt][1] and worst[2] <= LSE_TOL[dt]

    # 2. byte for byte at the packed call's split size: the extend call on each item's slice, the q_len= call on the padded copy
    C = c["bps"] or extend_default_split(packed_row_groups(T, B, H, Hkv, Hl, M, blk)["groups"], NK)
    kwC = dict(kw, blocks_per_split=C)
    padded = ext(qpad, k, v, mask, q_len=list(ns), **kwC)
    for b, n in enumerate(ns):
        if n == 0:
            continue
        nq = ref.live_blocks(n, blk)
        mine = _item(base, s, b, n)
        alone = ext(q[s[b]:s[b] + n].transpose(0, 1)[None], k[b:b + 1], v[b:b + 1], mask[b:b + 1, :, :nq], **dict(kwC, kv_len=[lens[b]]))
        assert _same(alone, mine), (b, n)
        assert _same(tuple(t[b:b + 1, :, :n].contiguous() for t in padded), mine), (b, n)
    # the lists dict (garbage in the rows of query blocks without a row) = the mask; a second call
    lists = block_mask_to_lists(mask, B, Hl)
    lists = dict(cols=lists["cols"], counts=lists["counts"])
    for b, n in enumerate(ns):
        lists["cols"].view(B, Hl, NQ, NK)[b, :, ref.live_blocks(n, blk):] = -7
        lists["counts"].view(B, Hl, NQ)[b, :, ref.live_blocks(n, blk):] = NK + 5
    assert _same(ext(q, k, v, lists, **pk, **kw), base)
    assert _same(ext(q, k, v, mask, **pk, **kw), base)
    # a strided q (a view of a fused projection [T, (H + 2 Hkv) D]) is read where it lies, with the same bytes
    fused = torch.full((T, (H + 2 * Hkv) * D), float("nan"), dtype=q.dtype, device=DEV)
    qv = fused[:, :H * D].view(T, H, D)
    qv.copy_(q)
    assert _same(ext(qv, k, v, mask, **pk, **kw), base)


@pytest.mark.parametrize("dt,D,blk,kv8_cache", [("bf16", 128, 128, False), ("fp16", 64, 64, True)])
def test_one_row_items_are_the_decode_call(dt, D, blk, kv8_cache):
    """Length set (1, 1, 1, 1) with M = 1: qg = 1, the one-row-tile kernels, block_sparse_decode's bytes at blocks_per_split = 8."""
    from rectified_spaattn_amd import block_sparse_decode
    H, Hkv = 8, 2
    lengths, M, gap = ref.LSETS[1]
    cu = ref.cu_of(lengths, gap)
    s, ns = ref.sanitise(cu, T, M)
    NK = -(-SK // blk)
    lens = [SK, 40, 333, 129]
    g = torch.Generator().manual_seed(77)
    q4 = torch.randn(B, H, 1, D, generator=g).to(DEV, TDT[dt])
    kf, vf = (torch.randn(B, Hkv, SK, D, generator=g) for _ in range(2))
    mask = (torch.rand(B, Hkv, 1, NK, generator=g) < 0.6).to(DEV)
    mask[..., 0] = True
    kw = dict(kv_len=lens, block_size=blk, causal=True, blocks_per_split=8, return_lse=True)
    if kv8_cache:
        pair = kv8.pow2_scales(Hkv, 5)
        kc, vc, _, _ = tg8._quantised(kf.numpy(), vf.numpy(), pair, lens, dt)
        k, v = tg8._dev8(kc), tg8._dev8(vc)
        kw.update(zip(("k_scale", "v_scale"), tg8._scales(pair)))
    else:
        k, v = kf.to(DEV, TDT[dt]), vf.to(DEV, TDT[dt])
        tgd._nan_tail(k, v, lens)
    want = block_sparse_decode(q4, k, v, mask, **kw)
    got = ext(_packed(q4, s, ns), k, v, mask, cu_seqlens_q=_cu(cu), max_q_len=1, **kw)
    for b in range(B):
        assert _same(_item(got, s, b, 1), tuple(t[b:b + 1] for t in want)), b
    assert bool(got[0][s[0]:s[-1]].any())


# ---- 3. exact visibility, malformed cu_seqlens_q -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.WITNESS_CASES, ids=lambda c: c["id"])
def test_exact_visibility(c):
    """Zero scores, V of 0 / 1: every output element is a count over the visible keys divided by their number; the probes sit either
    side of each item's own causal diagonal at its first and last row -- which also tells item b's first row from item b - 1's
    last -- and of kv_len[b].  The bound is test_gpu_extend's; exactly 0 where the reference is 0, every row of no item among them."""
    inp = ref.witness_inputs(c)
    want, lse_want = ref.witness_reference(c, inp)
    q, k, v = (torch.from_numpy(inp[n]).to(DEV, TDT[c["dt"]]) for n in ("q", "k", "v"))
    item, _ = ref.row_items(c["cu"], T, c["M"])
    q[torch.from_numpy(item < 0).to(DEV)] = float("nan")
    tgd._nan_tail(k, v, c["lens"])
    out, lse = ext(q, k, v, torch.from_numpy(inp["mask"]).to(DEV), kv_len=list(c["lens"]), cu_seqlens_q=_cu(c["cu"]), max_q_len=c["M"],
                   sm_scale=inp["sm_scale"], block_size=c["blk"], causal=c["causal"], blocks_per_split=c["C"], return_lse=True)
    got, lse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    ok, worst = eref.within(got, want, c["dt"])
    print(f"{c['id']}: worst {worst:.3f} tolerances")
    assert ok, worst
    has = np.isfinite(lse_want)
    assert np.isneginf(lse[~has]).all() and np.isfinite(lse[has]).all()


@pytest.mark.parametrize("kind", ref.MALFORMED)
def test_malformed_cu_seqlens_only_decides_which_rows_come_out_empty(kind):
    """The C entry on an out / lse pre-filled with NaN: every row is written, and the result is the sanitised rule's."""
    from rectified_spaattn_amd import _core, _lib
    from rectified_spaattn_amd.block_sparse import RsaOut4, _t3, block_mask_to_lists
    cu, M = ref.malformed(kind)
    s, ns = ref.sanitise(cu, T, M)
    H, Hkv, D, blk, dt = 8, 2, 64, 64, "bf16"
    NQ, NK = -(-M // blk), -(-SK // blk)
    lens = [SK, 340, 333, 129]
    g = torch.Generator().manual_seed(len(kind))
    q = torch.randn(T, H, D, generator=g).to(DEV, TDT[dt])
    item, _ = ref.row_items(cu, T, M)
    q[torch.from_numpy(item < 0).to(DEV)] = float("nan")
    k, v = (torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[dt]) for _ in range(2))
    tgd._nan_tail(k, v, lens)
    mask = (torch.rand(B, Hkv, NQ, NK, generator=g) < 0.5).to(DEV)
    mask[..., 0] = True
    lists = block_mask_to_lists(mask, B, Hkv)
    out = torch.full((T, H, D), float("nan"), dtype=TDT[dt], device=DEV)
    lse = torch.full((T, H), float("nan"), dtype=torch.float32, device=DEV)
    L = _lib.lib()
    need = ctypes.c_size_t(0)
    _lib.check(L.rsa_block_sparse_extend_packed_bytes(T, B, H, Hkv, Hkv, M, D, blk, NK, 2, ctypes.byref(need), None), "bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    cu_dev = _cu(cu)
    # (kv_len on the device: the host form takes one limit for every item)
    kv_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    _lib.check(L.rsa_block_sparse_extend_packed(T, B, H, Hkv, Hkv, M, SK, D, _core.dtype_code(q.dtype), blk, NK, kv_dev.data_ptr(), SK, 1,
                                                D ** -0.5, _t3(q), _core._t4(k), _core._t4(v), None, 0, 0, lists["cols"].data_ptr(),
                                                lists["counts"].data_ptr(), 2, ws.data_ptr(), need.value,
                                                RsaOut4(out.data_ptr(), 0, out.stride(1), out.stride(0)), lse.data_ptr(),
                                                cu_dev.data_ptr(), _core._stream()), "rsa_block_sparse_extend_packed")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and not bool(torch.isnan(lse).any())         # every row was written
    dead = torch.from_numpy(item < 0).to(DEV)
    assert not out[dead].any() and bool(torch.isneginf(lse[dead]).all()) and int(dead.sum()) > 0
    want, lse_want = ref.attention(q.float().cpu().numpy(), k.float().cpu().numpy(), v.float().cpu().numpy(), cu, T, M,
                                   mask.cpu().numpy(), lens, blk, True, D ** -0.5)
    got = out.float().cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    assert err.max() < TOL[dt][0] and err.mean() < TOL[dt][1]
    assert np.array_equal(np.isneginf(lse.cpu().numpy()), np.isneginf(lse_want))
    # and the Python call gives the same bytes
    again = ext(q, k, v, mask, kv_len=lens, cu_seqlens_q=cu_dev, max_q_len=M, block_size=blk, causal=True, blocks_per_split=2,
                return_lse=True)
    assert _same(again, (out, lse))


# ---- 4. selection, append --------------------------------------------------------------------------------------------------------------
SEL_CASES = [dict(blk=128, D=128, dt="bf16", top_k=3, top_p=None, forced=True, lset=0),
             dict(blk=64, D=64, dt="fp16", top_k=4, top_p=None, forced=False, lset=2),
             dict(blk=128, D=64, dt="fp16", top_k=2, top_p=None, forced=False, lset=1),
             dict(blk=64, D=128, dt="bf16", top_k=6, top_p=0.5, forced=False, lset=0),
             dict(blk=128, D=128, dt="fp16", top_k=4, top_p=0.7, forced=True, lset=2),
             dict(blk=64, D=64, dt="bf16", top_k=8, top_p=0.9, forced=True, lset=1)]


@pytest.mark.parametrize("c", SEL_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_selection_is_the_ragged_selection_on_the_padded_copy(c):
    from rectified_spaattn_amd import pool_keys, select_blocks_pooled
    H, Hkv, D, blk = 8, 2, c["D"], c["blk"]
    lengths, M, gap = ref.LSETS[c["lset"]]
    cu = ref.cu_of(lengths, gap)
    s, ns = ref.sanitise(cu, T, M)
    lens = [SK, 40, 333, 129]
    g = torch.Generator().manual_seed(60 + c["lset"])
    qpad = torch.randn(B, H, M, D, generator=g).to(DEV, TDT[c["dt"]])
    for b, n in enumerate(ns):
        qpad[b, :, n:] = float("nan")
    q = _packed(qpad, s, ns)
    k = torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[c["dt"]])
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
    kw = dict(block_size=blk, causal=True, keep_first=int(c["forced"]), keep_local=int(c["forced"]), as_lists=True, return_scores=True)
    if c["top_p"] is not None:
        kw.update(top_p=c["top_p"], return_mass=True)
    pooled = pool_keys(k, block_size=blk, kv_len=lens)
    want = select_blocks_pooled(qpad, pooled, c["top_k"], kv_len=lens, q_len=list(ns), **kw)
    pk = dict(cu_seqlens_q=_cu(cu), max_q_len=M)
    got = select_blocks_pooled(q, pooled, c["top_k"], kv_len=lens, **pk, **kw)
    tg8._same_lists(got[0], want[0])
    assert all(tg8._same(x, y) for x, y in zip(got[1:], want[1:])) and int(got[0]["counts"].sum()) > 0
    for splits in (1, 2, 4):
        spread = select_blocks_pooled(q, pooled, c["top_k"], kv_len=lens, score_splits=splits, **pk, **kw)
        tg8._same_lists(spread[0], want[0])
        assert all(tg8._same(x, y) for x, y in zip(spread[1:], want[1:])), splits
    as_mask = select_blocks_pooled(q, pooled, c["top_k"], kv_len=lens, **pk, **dict(kw, as_lists=False))[0]
    assert as_mask.shape == (B, Hkv, -(-M // blk), -(-SK // blk)) and int(as_mask.sum()) == int(got[0]["counts"].sum())


@pytest.mark.parametrize("paged,dt,D,lset", [(True, "bf16", 128, 0), (False, "fp16", 64, 2), (True, "fp16", 64, 1)])
def test_append_places_the_bytes_of_the_padded_append(paged, dt, D, lset):
    from rectified_spaattn_amd import append_kv_e4m3
    Hkv, blk = 2, 128
    lengths, M, gap = ref.LSETS[lset]
    cu = ref.cu_of(lengths, gap)
    s, ns = ref.sanitise(cu, T, T)
    NK = -(-SK // blk)
    start = [100, 640, 0, 333]          # item 1's tokens run past the capacity (dropped)
    g = torch.Generator().manual_seed(9 + lset)
    kpad, vpad = (torch.randn(B, Hkv, M, D, generator=g).to(DEV, TDT[dt]) for _ in range(2))
    kn, vn = _packed(kpad, s, ns), _packed(vpad, s, ns)
    scales = dict(k_scale=torch.tensor([0.5, 2.0], device=DEV), v_scale=0.25)
    SENT = 0x5A
    if paged:
        P = B * NK + 2
        table = torch.randperm(P, generator=g)[:B * NK].reshape(B, NK).to(torch.int32).to(DEV)
        table[3, 3] = -1                # no page: dropped
        shape, kwt = (P, Hkv, blk, D), dict(block_table=table, block_size=blk)
    else:
        shape, kwt = (B, Hkv, SK, D), dict(block_size=blk)
    caches = [torch.full(shape, SENT, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(4)]
    append_kv_e4m3(kpad, vpad, caches[0], caches[1], start=start, n_new=list(ns), **scales, **kwt)
    append_kv_e4m3(kn, vn, caches[2], caches[3], start=torch.tensor(start, device=DEV), cu_seqlens=_cu(cu), **scales, **kwt)
    torch.cuda.synchronize()
    assert tg8._same(caches[2], caches[0]) and tg8._same(caches[3], caches[1])
    touched = int((caches[2].view(torch.uint8) != SENT).sum())
    assert 0 < touched <= sum(ns) * Hkv * D      # the sentinel stays everywhere else (a placed code may equal it by chance)


# ---- 5. the whole step -----------------------------------------------------------------------------------------------------------------
class _Step:
    """append_kv_e4m3(cu_seqlens) -> pool_keys(start = prev) -> select_blocks_pooled(cu_seqlens_q) -> block_sparse_extend(cu_seqlens_q)
    over a paged e4m3 cache; T = 200 rows hold B = 4 items of at most M = 130 rows, 128-token blocks."""
    H, Hkv, T, M, D, blk, dt = 8, 2, 200, 130, 128, 128, torch.bfloat16

    def __init__(self, seed):
        self.NK = -(-SK // self.blk)
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(self.T, self.H, self.D, generator=g).to(DEV, self.dt)
        self.kf, self.vf = (torch.randn(B, self.Hkv, SK, self.D, generator=g).to(self.dt) for _ in range(2))
        self.pair = kv8.pow2_scales(self.Hkv, 3)
        self.ks, self.vs = tg8._scales(self.pair)
        self.P = B * self.NK + 3
        self.table = torch.randperm(self.P, generator=g)[:B * self.NK].reshape(B, self.NK).to(torch.int32).to(DEV)
        self.kp, self.vp = (tg8._dev8(np.full((self.P, self.Hkv, self.blk, self.D), kv8.NAN_CODE, np.uint8)) for _ in range(2))
        self.pooled = torch.full((B, self.Hkv, self.NK, self.D), float("nan"), device=DEV)
        self.new_k, self.new_v = (torch.zeros(self.T, self.Hkv, self.D, dtype=self.dt, device=DEV) for _ in range(2))
        self.prev = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.cu = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=DEV)

    def prefill(self, prev):
        from rectified_spaattn_amd import append_kv_e4m3, pool_keys
        append_kv_e4m3(self.kf.to(DEV), self.vf.to(DEV), self.kp, self.vp, start=0, n_new=prev, k_scale=self.ks, v_scale=self.vs,
                       block_table=self.table)
        pool_keys(self.kp, kv_len=prev, block_table=self.table, k_scale=self.ks, out=self.pooled)

    def feed(self, prev, ns, gap=2):
        """Item b's chunk: tokens prev[b] .. prev[b] + ns[b] of its sequence at rows cu[b] .., NaN in the rows of no item."""
        cu = ref.cu_of(ns, gap)
        assert cu[-1] <= self.T and max(ns) <= self.M
        self.new_k.fill_(float("nan"))
        self.new_v.fill_(float("nan"))
        for b, (p, n) in enumerate(zip(prev, ns)):
            self.new_k[cu[b]:cu[b] + n] = self.kf[b, :, p:p + n].transpose(0, 1).to(DEV)
            self.new_v[cu[b]:cu[b] + n] = self.vf[b, :, p:p + n].transpose(0, 1).to(DEV)
        self.prev.copy_(torch.tensor(prev, dtype=torch.int32))
        self.cu.copy_(torch.tensor(cu, dtype=torch.int32))
        self.kv_len.copy_(self.prev + torch.tensor(ns, dtype=torch.int32, device=DEV))
        return cu

    def run(self, pooled, kp, vp):
        from rectified_spaattn_amd import append_kv_e4m3, pool_keys, select_blocks_pooled
        kw8 = dict(k_scale=self.ks, v_scale=self.vs, block_table=self.table)
        append_kv_e4m3(self.new_k, self.new_v, kp, vp, start=self.prev, cu_seqlens=self.cu, **kw8)
        pool_keys(kp, kv_len=self.kv_len, start=self.prev, block_table=self.table, k_scale=self.ks, out=pooled)
        lists = select_blocks_pooled(self.q, pooled, 3, kv_len=self.kv_len, cu_seqlens_q=self.cu, max_q_len=self.M, causal=True,
                                     keep_first=1, keep_local=1, as_lists=True)
        return (lists,) + ext(self.q, kp, vp, lists, kv_len=self.kv_len, cu_seqlens_q=self.cu, max_q_len=self.M, causal=True,
                              blocks_per_split=2, return_lse=True, **kw8)

    def item(self, stale, b, p, n, row0):
        """The step of item b alone through the padded calls (no q_len, no cu_seqlens) on copies of the stale caches."""
        from rectified_spaattn_amd import append_kv_e4m3, pool_keys, select_blocks_pooled
        pooled, kp, vp = (t.clone() for t in stale)
        table = self.table[b:b + 1]
        kw8 = dict(k_scale=self.ks, v_scale=self.vs, block_table=table)
        rows = slice(row0, row0 + n)
        k4, v4, q4 = (t[rows].transpose(0, 1)[None] for t in (self.new_k, self.new_v, self.q))
        append_kv_e4m3(k4, v4, kp, vp, start=[p], **kw8)
        pool_keys(kp, kv_len=[p + n], start=[p], block_table=table, k_scale=self.ks, out=pooled[b:b + 1])
        lists = select_blocks_pooled(q4, pooled[b:b + 1], 3, kv_len=[p + n], causal=True, keep_first=1, keep_local=1, as_lists=True)
        return (lists,) + ext(q4, kp, vp, lists, kv_len=[p + n], causal=True, blocks_per_split=2, return_lse=True, **kw8)

    def check_against_items(self, got, stale, prev, ns, cu):
        lists, out, lse = got
        NQ = -(-self.M // self.blk)
        counts = lists["counts"].view(B, self.Hkv, NQ)
        cols = lists["cols"].view(B, self.Hkv, NQ, self.NK)
        item, _ = ref.row_items(cu, self.T, self.M)
        dead = torch.from_numpy(item < 0).to(DEV)
        assert not out[dead].any() and bool(torch.isneginf(lse[dead]).all())
        for b, n in enumerate(ns):
            nq = ref.live_blocks(n, self.blk)
            assert not counts[b, :, nq:].any()
            if n == 0:
                continue
            l1, o1, s1 = self.item(stale, b, prev[b], n, cu[b])
            assert _same((o1, s1), _item((out, lse), cu, b, n)), b
            assert torch.equal(l1["counts"].view(self.Hkv, nq), counts[b, :, :nq])
            live = torch.arange(self.NK, device=DEV)[None, None, :] < counts[b, :, :nq, None]
            assert torch.equal(torch.where(live, l1["cols"].view(self.Hkv, nq, self.NK), 0), torch.where(live, cols[b, :, :nq], 0))


def test_the_whole_step_equals_the_per_item_steps_and_reads_nothing_on_the_host(monkeypatch):
    prev, ns = [200, 333, 511, 0], [130, 40, 1, 0]
    s = _Step(7)
    s.prefill(prev)
    cu = s.feed(prev, ns)
    stale = (s.pooled.clone(), s.kp.clone(), s.vp.clone())
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("a device value was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = s.run(s.pooled, s.kp, s.vp)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    s.check_against_items(got, stale, prev, ns, cu)
    assert bool(got[1][cu[0]].any()) and bool(torch.isfinite(got[1].float()).all())


def test_one_graph_for_the_packed_step_follows_cu_seqlens():
    prev, ns = [200, 333, 511, 0], [130, 40, 1, 5]
    s = _Step(11)
    s.prefill(prev)
    cu = s.feed(prev, ns)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.run(s.pooled.clone(), s.kp.clone(), s.vp.clone())        # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    stale = (s.pooled.clone(), s.kp.clone(), s.vp.clone())
    with torch.cuda.graph(graph, stream=side):
        got = s.run(s.pooled, s.kp, s.vp)
    graph.replay()
    torch.cuda.synchronize()
    s.check_against_items(got, stale, prev, ns, cu)
    before = got[1].clone()
    # the next step: the one-row item grows to 129 rows, the chunk becomes a decode item; the limits changed on the device, the
    # cache grown by the first step, a page moved
    prev = [p + n for p, n in zip(prev, ns)]
    ns = [1, 0, 129, 64]
    cu = s.feed(prev, ns, gap=0)
    spare = sorted(set(range(s.P)) - set(s.table.reshape(-1).tolist()))[0]
    moved = s.table[1, 2].item()
    for pool in (s.kp, s.vp):
        pool.view(torch.uint8)[spare] = pool.view(torch.uint8)[moved].clone()
        pool.view(torch.uint8)[moved] = kv8.NAN_CODE
    s.table[1, 2] = spare
    stale = (s.pooled.clone(), s.kp.clone(), s.vp.clone())
    graph.replay()
    torch.cuda.synchronize()
    s.check_against_items(got, stale, prev, ns, cu)
    eager = s.run(*stale)
    tg8._same_lists(got[0], eager[0])
    assert _same(got[1:], eager[1:])
    assert not torch.equal(got[1], before) and bool(torch.isfinite(got[1].float()).all())
