"""block_sparse_extend on the device: against fp64 attention over the rule of tests/extend_ref.py, the
log-sum-exp, paged = contiguous, lists = mask, e4m3 = the dequantised 2-byte cache, block_sparse_decode on its ground and the
call itself per query block, all byte for byte; the exact witnesses (visibility: zero scores; weights: integer scores) over more
than one query block and row group; a captured graph replayed on changed contents.  decode's scale: capacity Sk = 700 (6 blocks
of 128, 11 of 64, a ragged last one), B = 2, the cache past kv_len[b] NaN in every case."""
import numpy as np
import pytest
import torch

import extend_ref as ref
import kv8_ref as kv8
import test_gpu_decode as tgd
import test_gpu_kv8 as tg8
from rectified_spaattn_amd import block_sparse_extend as ext

pytestmark = pytest.mark.gpu
DEV = tgd.DEV
SK = ref.SK
TDT, TOL, LSE_TOL, LENS = tgd.TDT, tgd.TOL, tgd.LSE_TOL, tgd.LENS
SQS = (1, 8, 65, 128, 129, 300)


def _combos():
    """Parameters take turns over the product: every value of every axis meets every head grouping."""
    out = []
    for gi, (H, Hkv) in enumerate(ref.GROUPS):
        for i in range(12):
            blk = (128, 64)[(i // 4) % 2]
            out.append(dict(H=H, Hkv=Hkv, Sq=SQS[(i + gi) % 6], D=64 if H == 72 else (64, 128)[i % 2], dt=("bf16", "fp16")[(i // 2) % 2],
                            blk=blk, axis=("H", "Hkv", "1")[(i + i // 3) % 3], lens=tuple(LENS)[(i + 2 * gi) % 6],
                            causal=bool((i // 3) % 2), bps=(None, 1, 2, -(-SK // blk))[(i + gi) % 4], seed=1000 * gi + i))
    return out


COMBOS = _combos()


def _id(c):
    return (f"H{c['H']}kv{c['Hkv']}-Sq{c['Sq']}-D{c['D']}-{c['dt']}-b{c['blk']}-m{c['axis']}-{c['lens']}-"
            f"{'causal' if c['causal'] else 'full'}-s{c['bps']}")


def _hl(c):
    return {"H": c["H"], "Hkv": c["Hkv"], "1": 1}[c["axis"]]


def test_combos_cover_every_axis_for_every_grouping():
    for H, Hkv in ref.GROUPS:
        mine = [c for c in COMBOS if (c["H"], c["Hkv"]) == (H, Hkv)]
        for key, n in (("Sq", 6), ("D", 1 if H == 72 else 2), ("dt", 2), ("blk", 2), ("axis", 3), ("lens", 6), ("causal", 2)):
            assert len({c[key] for c in mine}) == n, (H, Hkv, key)
        assert {c["bps"] for c in mine} >= {None, 1, 2}
        assert any(c["bps"] == -(-SK // c["blk"]) for c in mine)
    units = {c["H"] // max(_hl(c), c["Hkv"]) for c in COMBOS}
    assert 72 in units and 1 in units
    served = [c for c in COMBOS if _decode_serves(c)]
    assert len(served) >= 8 and {c["Sq"] for c in served} >= {1, 8}


def _decode_serves(c):
    return c["Sq"] <= c["blk"] and c["Sq"] * (c["H"] // max(_hl(c), c["Hkv"])) <= 64 and c["bps"] is not None


def _same(a, b):
    return all(tg8._same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_against_fp64_and_byte_for_byte(c):
    from rectified_spaattn_amd import block_sparse_decode as dec
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists, extend_default_split, extend_row_groups
    B, H, Hkv, Sq, D, blk, dt, Hl = 2, c["H"], c["Hkv"], c["Sq"], c["D"], c["blk"], c["dt"], _hl(c)
    NQ, NK = -(-Sq // blk), -(-SK // blk)
    lens = LENS[c["lens"]]
    g = torch.Generator().manual_seed(c["seed"])
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
    kf, vf = (torch.randn(B, Hkv, SK, D, generator=g) for _ in range(2))
    k, v = kf.to(DEV, TDT[dt]), vf.to(DEV, TDT[dt])
    tgd._nan_tail(k, v, lens)
    mask = (torch.rand(B, Hl, NQ, NK, generator=g) < 0.5).to(DEV)
    mask[:, ::2, :, 0] = True       # (every other list head keeps the first block: the short caches are not all empty rows)
    kw = dict(kv_len=tgd._kv_arg(c["lens"], lens), block_size=blk, causal=c["causal"], blocks_per_split=c["bps"], return_lse=True)
    out, lse = ext(q, k, v, mask, **kw)
    torch.cuda.synchronize()
    assert out.shape == (B, H, Sq, D) and out.dtype == TDT[dt] and lse.shape == (B, H, Sq) and lse.dtype == torch.float32

    # 1. against fp64 attention over the rule; the log-sum-exp on the operands the kernel multiplies; empty rows exactly 0 / -inf
    qn, kn, vn = (t.float().cpu().numpy() for t in (q, k, v))
    seen = ref.visible(mask.cpu().numpy(), lens, Sq, SK, blk, H, c["causal"])
    sm = D ** -0.5
    want, lse64 = ref.attention(ref.scores2(qn, kn, sm), seen, vn)
    _, lse_hat = ref.attention(ref.scores2(qn, kn, sm, dt), seen, vn)
    got, got_lse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    has = seen.any(-1)
    err = np.abs(got - want)
    d_hat = float(np.abs(got_lse[has] - lse_hat[has]).max()) if has.any() else 0.0
    d_64 = float(np.abs(got_lse[has] - lse64[has]).max()) if has.any() else 0.0
    print(f"{_id(c)}: out max {err.max():.3e} mean {err.mean():.3e}; lse vs quantised {d_hat:.3e} (bound {LSE_TOL[dt]:.3e}), "
          f"vs fp64 {d_64:.3e} (not gated); empty rows {int((~has).sum())} of {has.size}")
    assert np.isfinite(got).all()
    assert err.max() < TOL[dt][0] and err.mean() < TOL[dt][1]
    assert (got[~has] == 0).all() and np.isneginf(got_lse[~has]).all()
    assert np.isfinite(got_lse[has]).all() and d_hat <= LSE_TOL[dt]

    # 2. paged = contiguous (garbage -1 / P + 5 in the table where no key is); the lists dict = the mask; a second call
    kp, vp, table, P = tgd._pool(k, v, blk, lens, c["seed"], bad=-1 if c["seed"] % 2 else "P+5")
    kwp = dict(kw, kv_len=list(lens) if kw["kv_len"] is None else kw["kv_len"], block_table=table)
    assert _same(ext(q, kp, vp, mask, **kwp), (out, lse))
    lists = block_mask_to_lists(mask, B, Hl)
    assert lists["cols"].shape == (B * Hl, NQ, NK)
    assert _same(ext(q, k, v, dict(cols=lists["cols"], counts=lists["counts"]), **kw), (out, lse))
    assert _same(ext(q, k, v, mask, **kw), (out, lse))
    # ... and with power-of-two scales the e4m3 cache = the 2-byte call on the dequantised cache
    pair = kv8.pow2_scales(Hkv, c["seed"])
    kc, vc, kd, vd = tg8._quantised(kf.numpy(), vf.numpy(), pair, lens, dt)
    ks, vs = tg8._scales(pair)
    want8 = ext(q, kd, vd, mask, **kw)
    assert _same(ext(q, tg8._dev8(kc), tg8._dev8(vc), mask, k_scale=ks, v_scale=vs, **kw), want8)
    if c["seed"] % 3 == 0:
        kp8, vp8, table8, _ = tg8._pool8(kc, vc, blk, lens, c["seed"], bad=-1)
        kwp8 = dict(kwp, block_table=torch.from_numpy(table8).to(DEV))
        assert _same(ext(q, tg8._dev8(kp8), tg8._dev8(vp8), mask, k_scale=ks, v_scale=vs, **kwp8), want8)

    # 3. block_sparse_decode wherever it serves the shape, at an equal explicit blocks_per_split
    if _decode_serves(c):
        assert _same(dec(q, k, v, mask, **kw), (out, lse))
        assert _same(dec(q, kp, vp, lists, **kwp), (out, lse))

    # 4. itself per query block: the rows of query block i = the first block of the call on q[:, :, i * block:] and mask[:, :, i:]
    # (causal and kv_len fixed: the absolute limits do not move).  The split size is pinned: the default follows the row groups.
    C = c["bps"] or extend_default_split(extend_row_groups(B, H, Hkv, Hl, Sq, blk)["groups"], NK)
    for i in range(1, NQ):
        o_i, l_i = ext(q[:, :, i * blk:], k, v, mask[:, :, i:], **dict(kw, blocks_per_split=C))
        rows = slice(i * blk, min((i + 1) * blk, Sq))
        assert _same((o_i[:, :, :blk].contiguous(), l_i[:, :, :blk].contiguous()),
                     (out[:, :, rows].contiguous(), lse[:, :, rows].contiguous())), i


def test_device_kv_len_is_not_read_on_the_host(monkeypatch):
    B, H, Hkv, Sq, D, Sk = 2, 4, 2, 130, 64, 389
    g = torch.Generator().manual_seed(17)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Sk, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    mask = torch.ones(1, 1, 2, 4, dtype=torch.bool, device=DEV)
    kw = dict(block_size=128, causal=True, return_lse=True)
    on_host = ext(q, k, v, mask, kv_len=[389, 131], **kw)
    kv = torch.tensor([5000, 131], dtype=torch.int64, device=DEV)       # (clamped to Sk on the device)
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("kv_len was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        on_device = ext(q, k, v, mask, kv_len=kv, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    assert _same(on_device, on_host)
    assert bool(on_host[0].any()) and not torch.equal(on_host[0][0], on_host[0][1])


def test_graph_replay_on_changed_contents():
    """One call with Sq = 129 captured on a side stream with a device kv_len, the lists and a table; then one more key is written
    into the cache in place, kv_len is bumped, the lists change and a page moves; the replay equals the eager call on the new
    contents."""
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, Sq, D, blk, dt = 2, 8, 2, 129, 128, 128, "bf16"
    NQ, NK = 2, -(-SK // blk)
    lens = [511, 333]           # item 0's next key opens a new block
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
    k, v = (torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[dt]) for _ in range(2))
    new_k, new_v = k[:, :, 600].clone(), v[:, :, 600].clone()
    tgd._nan_tail(k, v, lens)
    kp, vp, table, P = tgd._pool(k, v, blk, [SK, SK], 11)       # (every block has a page: the new keys have somewhere to go)
    mask = (torch.rand(B, Hkv, NQ, NK, generator=g) < 0.6).to(DEV)
    mask[:, :, :, 4] = True
    made = block_mask_to_lists(mask, B, Hkv)
    lists = dict(cols=made["cols"], counts=made["counts"])
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(kv_len=kv_len, block_size=blk, causal=True, block_table=table, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext(q, kp, vp, lists, **kw)       # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out_g, lse_g = ext(q, kp, vp, lists, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(ext(q, kp, vp, mask, **kw), (out_g, lse_g))
    before = out_g.clone()
    for b in range(B):
        j, r = lens[b] // blk, lens[b] % blk
        kp[table[b, j].item(), :, r] = new_k[b]
        vp[table[b, j].item(), :, r] = new_v[b]
    kv_len += 1
    mask[:, :, 1, 0] ^= True
    mask[0, :, :, 3] ^= True
    again = block_mask_to_lists(mask, B, Hkv)
    lists["cols"].copy_(again["cols"])
    lists["counts"].copy_(again["counts"])
    spare = sorted(set(range(P)) - set(table.reshape(-1).tolist()))[0]
    kp[spare], vp[spare] = kp[table[1, 1].item()].clone(), vp[table[1, 1].item()].clone()
    kp[table[1, 1].item()], vp[table[1, 1].item()] = float("nan"), float("nan")
    table[1, 1] = spare
    graph.replay()
    torch.cuda.synchronize()
    assert _same(ext(q, kp, vp, mask, **kw), (out_g, lse_g))
    assert not torch.equal(out_g, before) and torch.isfinite(out_g.float()).all()


def _run_case(c, inp):
    q, k, v = (torch.from_numpy(inp[n]).to(DEV, TDT[c["dt"]]) for n in ("q", "k", "v"))
    tgd._nan_tail(k, v, c["lens"])
    mask = torch.from_numpy(inp["mask"]).to(DEV)
    out, lse = ext(q, k, v, mask, kv_len=list(c["lens"]), sm_scale=inp["sm_scale"], block_size=c["blk"], causal=c["causal"],
                   blocks_per_split=c["C"], return_lse=True)
    return out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("c", ref.VIS_CASES, ids=lambda c: c["id"])
def test_exact_visibility(c):
    """Zero scores, V of 0 / 1: every output element is a count over the visible keys divided by their number.  Every merge
    factor is 1, so the bound of decode's exact tests holds across splits: |got - ref| <= ULP |ref| + FLOOR max|ref|, 0 where the
    reference is 0.  The probes sit either side of kv_len, of the causal limits of the first and last row of every query block and
    of the rows either side of every row-group boundary, at the edges of a dropped block and at split starts."""
    inp = ref.vis_inputs(c)
    want, lse_want, _ = ref.case_reference(c, inp)
    got, lse = _run_case(c, inp)
    ok, worst = ref.within(got, want, c["dt"])
    print(f"{c['id']}: worst {worst:.3f} tolerances")
    assert ok, worst
    has = np.isfinite(lse_want)
    assert np.isneginf(lse[~has]).all() and np.isfinite(lse[has]).all()


@pytest.mark.parametrize("c", ref.WEIGHT_CASES, ids=lambda c: c["id"])
def test_exact_weights(c):
    """Integer scores in the kernel's units over two query blocks and more: every exp2, every rescale and every merge factor is a
    power of two and every sum is exact in fp32 (the budget is asserted), so out meets visibility's bound and the log-sum-exp is
    within 2^-21 max(1, |ref|) of ln 2 * log2(sum 2^n), as in decode's test."""
    inp = ref.weight_inputs(c)
    total, spread = ref.weight_budget(c, inp)
    assert total < 2.0 ** 24 and spread <= ref.dref.SPREAD and inp["mask"].shape[2] >= 2
    want, lse_want, _ = ref.case_reference(c, inp)
    got, lse = _run_case(c, inp)
    ok, worst = ref.within(got, want, c["dt"])
    has = np.isfinite(lse_want)
    d = np.abs(lse[has] - lse_want[has]) / np.maximum(1.0, np.abs(lse_want[has]))
    print(f"{c['id']}: worst {worst:.3f} tolerances; lse {float(d.max()) * 2 ** 21 if has.any() else 0:.3f} x 2^-21")
    assert ok, worst
    assert np.isneginf(lse[~has]).all()
    assert (d <= 2.0 ** -21).all()
