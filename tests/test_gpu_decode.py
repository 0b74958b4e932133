"""block_sparse_decode on the device: against fp64 attention over the rule of tests/decode_ref.py, the
log-sum-exp, paged = contiguous and lists = mask byte for byte, a captured graph replayed on changed contents, and the exact
witnesses (visibility: zero scores; weights: integer scores).  Capacity Sk = 700 (6 blocks of 128, 11 of 64, a ragged last one),
B = 2; the cache past kv_len[b] is NaN in every case."""
import numpy as np
import pytest
import torch

import decode_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SK = ref.SK
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"bf16": (2e-2, 2e-3), "fp16": (2e-3, 2e-4)}          # the plain call's (tests/test_gpu_block_mask.py)
LSE_TOL = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
LENS = {"none": [SK, SK], "list": [SK, 333], "short": [129, 2], "dev": [SK, 333], "dev64": [129, 2], "zero": [0, 450]}


def _combos():
    """Parameters take turns over the product: every value of every axis meets every head grouping."""
    out = []
    for gi, (H, Hkv) in enumerate(ref.GROUPS):
        for i in range(12):
            blk = (128, 64)[(i // 4) % 2]
            out.append(dict(H=H, Hkv=Hkv, Sq=(1, 3, 8)[i % 3], D=(64, 128)[i % 2], dt=("bf16", "fp16")[(i // 2) % 2], blk=blk,
                            axis=("H", "Hkv", "1")[(i + i // 3) % 3], lens=tuple(LENS)[(i + gi) % 6], causal=bool((i // 3) % 2),
                            bps=(None, 1, 2, -(-SK // blk))[(i + gi) % 4], seed=1000 * gi + i))
    return out


COMBOS = _combos()


def _id(c):
    return (f"H{c['H']}kv{c['Hkv']}-Sq{c['Sq']}-D{c['D']}-{c['dt']}-b{c['blk']}-m{c['axis']}-{c['lens']}-"
            f"{'causal' if c['causal'] else 'full'}-s{c['bps']}")


def test_combos_cover_every_axis_for_every_grouping():
    for H, Hkv in ref.GROUPS:
        mine = [c for c in COMBOS if (c["H"], c["Hkv"]) == (H, Hkv)]
        for key, n in (("Sq", 3), ("D", 2), ("dt", 2), ("blk", 2), ("axis", 3), ("lens", 6), ("causal", 2)):
            assert len({c[key] for c in mine}) == n, (H, Hkv, key)
        assert {c["bps"] for c in mine} >= {None, 1, 2}
        assert any(c["bps"] == -(-SK // c["blk"]) for c in mine)


def _nan_tail(k, v, lens):
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")


def _kv_arg(form, lens):
    if form == "none":
        return None
    if form in ("dev", "dev64"):
        return torch.tensor(lens, dtype=torch.int64 if form == "dev64" else torch.int32, device=DEV)
    return list(lens)


def _pool(k, v, blk, lens, seed, bad=-1):
    """The cache in pages: B * NK + 3 pages placed by a random permutation, the spare ones and the ragged tails full of NaN;
    table entries past ceil(kv_len[b] / block) are garbage (`bad`)."""
    B, Hkv, Sk, D = k.shape
    NK = -(-Sk // blk)
    P = B * NK + 3
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed)).tolist()
    kp = torch.full((P, Hkv, blk, D), float("nan"), dtype=k.dtype, device=k.device)
    vp = kp.clone()
    table = torch.full((B, NK), P + 5 if bad == "P+5" else bad, dtype=torch.int32)
    for b in range(B):
        for j in range(NK):
            if j * blk >= lens[b]:
                continue
            pg = perm[b * NK + j]
            rows = min(blk, Sk - j * blk)
            kp[pg, :, :rows] = k[b, :, j * blk:j * blk + rows]
            vp[pg, :, :rows] = v[b, :, j * blk:j * blk + rows]
            table[b, j] = pg
    return kp, vp, table.to(k.device), P


def _hl(c):
    return {"H": c["H"], "Hkv": c["Hkv"], "1": 1}[c["axis"]]


@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_against_fp64_lse_paged_and_lists(c):
    from rectified_spaattn_amd import block_sparse_decode as dec
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, Sq, D, blk, dt = 2, c["H"], c["Hkv"], c["Sq"], c["D"], c["blk"], c["dt"]
    NK = -(-SK // blk)
    lens = LENS[c["lens"]]
    g = torch.Generator().manual_seed(c["seed"])
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
    k, v = (torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[dt]) for _ in range(2))
    _nan_tail(k, v, lens)
    mask = (torch.rand(B, _hl(c), 1, NK, generator=g) < 0.5).to(DEV)
    mask[:, ::2, 0, 0] = True       # (every other list head keeps the first block: the short caches are not all empty rows)
    kw = dict(kv_len=_kv_arg(c["lens"], lens), block_size=blk, causal=c["causal"], blocks_per_split=c["bps"], return_lse=True)
    out, lse = dec(q, k, v, mask, **kw)
    torch.cuda.synchronize()

    # 1. against fp64 attention over the rule; 2. the log-sum-exp on the operands the kernel multiplies
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
          f"vs fp64 {d_64:.3e} (not gated); empty rows {int((~has).sum())}")
    assert np.isfinite(got).all()
    assert err.max() < TOL[dt][0] and err.mean() < TOL[dt][1]
    assert (got[~has] == 0).all() and np.isneginf(got_lse[~has]).all()
    assert np.isfinite(got_lse[has]).all() and d_hat <= LSE_TOL[dt]

    # 3. paged = contiguous, byte for byte (garbage -1 / P + 5 in the table where no key is)
    kp, vp, table, P = _pool(k, v, blk, lens, c["seed"], bad=-1 if c["seed"] % 2 else "P+5")
    kwp = dict(kw, kv_len=list(lens) if kw["kv_len"] is None else kw["kv_len"], block_table=table)
    out_p, lse_p = dec(q, kp, vp, mask, **kwp)
    assert torch.equal(out_p, out) and torch.equal(lse_p, lse)

    # 4. the lists dict = the mask, byte for byte; two calls give the same bytes
    lists = block_mask_to_lists(mask, B, _hl(c))
    out_l, lse_l = dec(q, k, v, lists, **kw)
    assert torch.equal(out_l, out) and torch.equal(lse_l, lse)
    out_2, lse_2 = dec(q, k, v, mask, **kw)
    assert torch.equal(out_2, out) and torch.equal(lse_2, lse)


@pytest.mark.parametrize("blk,bad", [(128, "P+5"), (64, "-1")])
def test_an_out_of_range_entry_is_a_cleared_mask_bit(blk, bad):
    """A kept, visible block whose table entry (or whose entry of a caller's lists) is out of range contributes no key.  The
    block is the LAST entry of its list: every other entry then keeps its place in the walk, so the summation order -- and with
    it every byte -- is that of the call with the bit cleared."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, Sq, D, dt = 2, 8, 2, 3, 128, "bf16"
    NK = -(-SK // blk)
    lens = [SK, 333]
    g = torch.Generator().manual_seed(blk)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
    k, v = (torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[dt]) for _ in range(2))
    _nan_tail(k, v, lens)
    mask = (torch.rand(B, Hkv, 1, NK, generator=g) < 0.5).to(DEV)
    mask[0, :, 0, NK - 1] = True
    cleared = mask.clone()
    cleared[0, :, 0, NK - 1] = False
    for bps in (None, 1, 2):
        kw = dict(kv_len=lens, block_size=blk, causal=True, blocks_per_split=bps, return_lse=True)
        want = dec(q, k, v, cleared, **kw)
        kp, vp, table, P = _pool(k, v, blk, lens, 7)
        table[0, NK - 1] = P + 5 if bad == "P+5" else -1
        got = dec(q, kp, vp, mask, block_table=table, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        lists = block_mask_to_lists(mask, B, Hkv)
        cols, counts = lists["cols"].clone(), lists["counts"]
        for row in range(Hkv):      # batch item 0: the last entry of each list row
            cols[row, 0, int(counts[row, 0]) - 1] = NK + 3 if bad == "P+5" else -1
        got = dec(q, k, v, dict(cols=cols, counts=counts), **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(want[0], dec(q, k, v, mask, **kw)[0])       # (the block did matter)


def test_strided_views_and_a_batch_broadcast_mask_give_the_same_bytes():
    """q, k, v as [B, S, H, D] views (nothing is copied for k / v) and a mask with a batch axis of 1."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    B, H, Hkv, Sq, D, blk = 2, 8, 2, 3, 64, 64
    NK = -(-SK // blk)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, torch.float16)
    k, v = (torch.randn(B, Hkv, SK, D, generator=g).to(DEV, torch.float16) for _ in range(2))
    mask1 = (torch.rand(1, Hkv, 1, NK, generator=g) < 0.5).to(DEV)
    kw = dict(kv_len=[SK, 333], block_size=blk, causal=True, return_lse=True)
    want = dec(q, k, v, mask1.expand(B, Hkv, 1, NK).contiguous(), **kw)
    views = [t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k, v)]
    assert not views[1].is_contiguous()
    got = dec(*views, mask1, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("dtype,n", [(torch.int32, 2), (torch.int64, 2), (torch.int64, 1)])
def test_device_kv_len_gives_the_ints_result_and_is_not_read_on_the_host(monkeypatch, dtype, n):
    from rectified_spaattn_amd import block_sparse_decode as dec
    B, H, Hkv, Sq, D, Sk = 2, 4, 2, 2, 64, 389
    g = torch.Generator().manual_seed(17)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, torch.bfloat16)
    k, v = (torch.randn(B, Hkv, Sk, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    mask = torch.ones(1, 1, 1, 4, dtype=torch.bool, device=DEV)
    lens = [389, 130] if n == 2 else [130]
    kw = dict(block_size=128, causal=True, return_lse=True)
    on_host = dec(q, k, v, mask, kv_len=lens if n == 2 else lens[0], **kw)
    kv = torch.tensor(lens, dtype=dtype, device=DEV)
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("kv_len was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        on_device = dec(q, k, v, mask, kv_len=kv, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    for a, b in zip(on_device, on_host):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))
    out = on_host[0]
    assert bool(out.any()) and not torch.equal(out[0], out[1])


def test_graph_replay_on_changed_contents():
    """One call captured on a side stream with a device kv_len, a mask tensor and a table; then one more key is written into the
    cache in place, kv_len is bumped, mask bits flip and a page moves; the replay equals the eager call on the new contents."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    B, H, Hkv, Sq, D, blk, dt = 2, 8, 2, 1, 128, 128, "bf16"
    NK = -(-SK // blk)
    lens = [511, 333]           # item 0's next key opens a new block
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[dt])
    k, v = (torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[dt]) for _ in range(2))
    new_k, new_v = k[:, :, 600].clone(), v[:, :, 600].clone()
    _nan_tail(k, v, lens)
    kp, vp, table, P = _pool(k, v, blk, [SK, SK], 11)       # (every block has a page: the new keys have somewhere to go)
    mask = (torch.rand(B, Hkv, 1, NK, generator=g) < 0.6).to(DEV)
    mask[:, :, 0, 4] = True
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(kv_len=kv_len, block_size=blk, causal=True, block_table=table, return_lse=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec(q, kp, vp, mask, **kw)       # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out_g, lse_g = dec(q, kp, vp, mask, **kw)
    graph.replay()
    torch.cuda.synchronize()
    first = dec(q, kp, vp, mask, **kw)
    assert torch.equal(out_g, first[0]) and torch.equal(lse_g, first[1])
    before = out_g.clone()
    # the step: one more key per batch item, in place
    for b in range(B):
        j, r = lens[b] // blk, lens[b] % blk
        kp[table[b, j].item(), :, r] = new_k[b]
        vp[table[b, j].item(), :, r] = new_v[b]
    kv_len += 1
    mask[:, :, 0, 0] ^= True
    mask[0, :, 0, 3] ^= True
    spare = sorted(set(range(P)) - set(table.reshape(-1).tolist()))[0]
    kp[spare], vp[spare] = kp[table[1, 1].item()].clone(), vp[table[1, 1].item()].clone()
    kp[table[1, 1].item()], vp[table[1, 1].item()] = float("nan"), float("nan")
    table[1, 1] = spare
    graph.replay()
    torch.cuda.synchronize()
    eager = dec(q, kp, vp, mask, **kw)
    assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1])
    assert not torch.equal(out_g, before) and torch.isfinite(out_g.float()).all()


def _run_case(c, inp):
    from rectified_spaattn_amd import block_sparse_decode as dec
    q, k, v = (torch.from_numpy(inp[n]).to(DEV, TDT[c["dt"]]) for n in ("q", "k", "v"))
    _nan_tail(k, v, c["lens"])
    mask = torch.from_numpy(inp["mask"]).to(DEV)
    out, lse = dec(q, k, v, mask, kv_len=list(c["lens"]), sm_scale=inp["sm_scale"], block_size=c["blk"], causal=c["causal"],
                   blocks_per_split=c["C"], return_lse=True)
    return out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("c", ref.VIS_CASES, ids=lambda c: c["id"])
def test_exact_visibility(c):
    """Zero scores, V of 0 / 1: every output element is a count over the visible keys divided by their number.  Every merge
    factor is 1, so the bound holds across splits: |got - ref| <= ULP |ref| + FLOOR max|ref|, 0 where the reference is 0."""
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
    """Integer scores in the kernel's units: every exp2, every rescale and every merge factor is a power of two and every sum is
    exact in fp32 (the budget is asserted), so out meets visibility's bound and the log-sum-exp is within 2^-21 max(1, |ref|) of
    ln 2 * log2(sum 2^n): four fp32 ulps for one log2, one add and one multiply (the accuracy of the hardware log2 is assumed)."""
    inp = ref.weight_inputs(c)
    total, spread = ref.weight_budget(c, inp)
    assert total < 2.0 ** 24 and spread <= ref.SPREAD
    want, lse_want, _ = ref.case_reference(c, inp)
    got, lse = _run_case(c, inp)
    ok, worst = ref.within(got, want, c["dt"])
    has = np.isfinite(lse_want)
    d = np.abs(lse[has] - lse_want[has]) / np.maximum(1.0, np.abs(lse_want[has]))
    print(f"{c['id']}: worst {worst:.3f} tolerances; lse {float(d.max()) * 2 ** 21 if has.any() else 0:.3f} x 2^-21")
    assert ok, worst
    assert np.isneginf(lse[~has]).all()
    assert (d <= 2.0 ** -21).all()
