"""The ragged calls on the device: block_sparse_extend(q_len=) and select_blocks(_pooled)(q_len=) over a
batch of B = 4 items padded to Sq = 300 rows, capacity 700, NaN in the cache beyond kv_len[b] and in q beyond q_len[b].
  1. extend against fp64 attention over the rule of tests/ragged_ref.py, within test_gpu_decode's TOL / LSE_TOL; rows >= q_len[b]
     and rows without a visible key exactly 0 / -inf
  2. extend byte for byte: item b's live rows = the existing call on the truncated item; paged = contiguous, lists = mask, a second
     call, e4m3 = the dequantised 2-byte cache, q_len = [Sq] * B = no q_len
  3. selection byte for byte against the existing call on the truncated item, top-k and top-p; empty blocks beyond; select_blocks =
     select_blocks_pooled
  4. the exact visibility witnesses on a ragged batch
  5. the whole step on a paged e4m3 cache: batched = per item, the device q_len never read on the host, one captured graph
     replayed after q_len, kv_len, the cache and the table changed in place"""
import numpy as np
import pytest
import torch

import extend_ref as eref
import kv8_ref as kv8
import ragged_ref as ref
import test_gpu_decode as tgd
import test_gpu_kv8 as tg8
from rectified_spaattn_amd import block_sparse_extend as ext

pytestmark = pytest.mark.gpu
DEV = tgd.DEV
B, SQ, SK = ref.B, ref.SQ, ref.SK
TDT, TOL, LSE_TOL = tgd.TDT, tgd.TOL, tgd.LSE_TOL
COMBOS = ref.gpu_combos()


def _id(c):
    return (f"H{c['H']}kv{c['Hkv']}-D{c['D']}-{c['dt']}-b{c['blk']}-m{c['axis']}-q{c['qset']}{'dev' if c['q_dev'] else 'host'}-"
            f"kv{'dev' if c['kv_dev'] else 'host'}-{'causal' if c['causal'] else 'full'}-s{c['bps']}")


def _hl(c):
    return {"H": c["H"], "Hkv": c["Hkv"], "1": 1}[c["axis"]]


def test_combos_cover_every_axis_for_every_grouping():
    for H, Hkv in eref.GROUPS:
        mine = [c for c in COMBOS if (c["H"], c["Hkv"]) == (H, Hkv)]
        for key, n in (("D", 1 if H == 72 else 2), ("dt", 2), ("blk", 2), ("axis", 3), ("causal", 2), ("qset", 3), ("q_dev", 2),
                       ("kv_dev", 2)):
            assert len({c[key] for c in mine}) == n, (H, Hkv, key)
        assert {c["bps"] for c in mine} >= {None, 1, 2}
        assert any(c["bps"] == -(-SK // c["blk"]) for c in mine)
        assert all(c["q_dev"] for c in mine if c["qset"] == 2)      # the unclamped values travel as a device tensor
    units = {c["H"] // max(_hl(c), c["Hkv"]) for c in COMBOS}
    assert 72 in units and 1 in units
    # the lengths, held against each combo's own row groups (qg rows of a query block) and block size: for every grouping and block
    # size some combo has lengths either side of a group boundary inside the chunk (n > 0 ends a group; n - 1 or n + 1), and some
    # combo a length one row into a further query block (n > block, n % block == 1).  The two prescribed sets do not each hold both:
    # (300, 129, 1, 0) has 129 without 128, (64, 65, 128, 128) no length one row into a second block of 128; the device set
    # (128, 129, 300, 0 after the clamp) holds both at every group width and block size.
    from rectified_spaattn_amd.block_sparse import extend_row_groups

    def boundary(c):
        qg = extend_row_groups(B, c["H"], c["Hkv"], _hl(c), SQ, c["blk"])["qg"]
        ns = set(ref.clamp(ref.combo_qlens(c), SQ))
        return any(n > 0 and n % c["blk"] % qg == 0 and ({n - 1, n + 1} & ns) for n in ns)     # (groups never straddle blocks)

    def into_next(c):
        return any(n > c["blk"] and n % c["blk"] == 1 for n in ref.clamp(ref.combo_qlens(c), SQ))
    for H, Hkv in eref.GROUPS:
        for blk in (64, 128):
            mine = [c for c in COMBOS if (c["H"], c["Hkv"], c["blk"]) == (H, Hkv, blk)]
            assert any(boundary(c) for c in mine) and any(into_next(c) for c in mine), (H, Hkv, blk)
    assert all(boundary(c) and into_next(c) for c in COMBOS if c["qset"] == 2)
    assert any(boundary(c) and c["H"] == c["Hkv"] and c["axis"] != "1" and c["qset"] == 1 for c in COMBOS)      # 64 / 65 rows at gu = 1


def _limit_arg(vals, on_device, seed):
    if not on_device:
        return list(vals)
    return torch.tensor(vals, dtype=torch.int64 if seed % 2 else torch.int32, device=DEV)


def _same(a, b):
    return all(tg8._same(x, y) for x, y in zip(a, b))


def _rows(pair, b, n):
    return tuple(t[b:b + 1, :, :n].contiguous() for t in pair)


@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_against_fp64_and_byte_for_byte(c):
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists, extend_default_split, extend_row_groups
    H, Hkv, D, blk, dt, Hl = c["H"], c["Hkv"], c["D"], c["blk"], c["dt"], _hl(c)
    NQ, NK = -(-SQ // blk), -(-SK // blk)
    raw = ref.combo_qlens(c)
    ns = ref.clamp(raw, SQ)
    lens = ref.combo_lens(c, ns)
    g = torch.Generator().manual_seed(c["seed"])
    q = torch.randn(B, H, SQ, D, generator=g).to(DEV, TDT[dt])
    for b, n in enumerate(ns):
        q[b, :, n:] = float("nan")
    kf, vf = (torch.randn(B, Hkv, SK, D, generator=g) for _ in range(2))
    k, v = kf.to(DEV, TDT[dt]), vf.to(DEV, TDT[dt])
    tgd._nan_tail(k, v, lens)
    mask = (torch.rand(B, Hl, NQ, NK, generator=g) < 0.5).to(DEV)
    mask[:, ::2, :, 0] = True
    kw = dict(kv_len=_limit_arg(lens, c["kv_dev"], c["seed"]), block_size=blk, causal=c["causal"], blocks_per_split=c["bps"],
              return_lse=True)
    q_len = _limit_arg(raw, c["q_dev"], c["seed"] // 2)
    out, lse = ext(q, k, v, mask, q_len=q_len, **kw)
    torch.cuda.synchronize()
    assert out.shape == (B, H, SQ, D) and out.dtype == TDT[dt] and lse.shape == (B, H, SQ) and lse.dtype == torch.float32

    # 1. against fp64 attention over the rule, item by item (the 72-head unit is 15M scores an item)
    mask_n = mask.cpu().numpy()
    sm = D ** -0.5
    worst = [0.0, 0.0, 0.0]
    for b, n in enumerate(ns):
        got = out[b:b + 1].float().cpu().numpy().astype(np.float64)
        got_lse = lse[b:b + 1].cpu().numpy().astype(np.float64)
        assert (got[:, :, n:] == 0).all() and np.isneginf(got_lse[:, :, n:]).all(), b
        if n == 0:
            continue
        qn, kn, vn = (t[b:b + 1].float().cpu().numpy() for t in (q, k, v))
        seen = ref.visible(mask_n[b:b + 1], lens[b:b + 1], [n], SQ, SK, blk, H, c["causal"])
        want, _ = ref.attention(qn, kn, vn, seen, sm)
        _, lse_hat = ref.attention(qn, kn, vn, seen, sm, dt)
        has = seen.any(-1)
        err = np.abs(got - want)
        assert np.isfinite(got).all()
        assert (got[~has] == 0).all() and np.isneginf(got_lse[~has]).all()
        assert np.isfinite(got_lse[has]).all()
        d_hat = float(np.abs(got_lse[has] - lse_hat[has]).max()) if has.any() else 0.0
        worst = [max(worst[0], float(err.max())), max(worst[1], float(err[:, :, :n].mean())), max(worst[2], d_hat)]
    print(f"{_id(c)}: out max {worst[0]:.3e} mean (live rows, worst item) {worst[1]:.3e}; lse vs quantised {worst[2]:.3e} "
          f"(bound {LSE_TOL[dt]:.3e})")
    assert worst[0] < TOL[dt][0] and worst[1] < TOL[dt][1] and worst[2] <= LSE_TOL[dt]

    # 2. byte for byte: item b's live rows = the existing call on the truncated item, at the padded call's split size
    C = c["bps"] or extend_default_split(extend_row_groups(B, H, Hkv, Hl, SQ, blk)["groups"], NK)
    for b, n in enumerate(ns):
        if n == 0:
            continue
        nq = ref.live_blocks(n, blk)
        alone = ext(q[b:b + 1, :, :n], k[b:b + 1], v[b:b + 1], mask[b:b + 1, :, :nq], **dict(kw, kv_len=[lens[b]], blocks_per_split=C))
        assert _same(alone, _rows((out, lse), b, n)), (b, n)
    # paged = contiguous (garbage table entries where no key is); the lists dict = the mask; a second call
    kp, vp, table, P = tgd._pool(k, v, blk, lens, c["seed"], bad=-1 if c["seed"] % 2 else "P+5")
    assert _same(ext(q, kp, vp, mask, q_len=q_len, **dict(kw, block_table=table)), (out, lse))
    lists = block_mask_to_lists(mask, B, Hl)
    lists = dict(cols=lists["cols"], counts=lists["counts"])
    for b, n in enumerate(ns):      # list rows of query blocks without a row are never read: garbage there
        lists["cols"].view(B, Hl, NQ, NK)[b, :, ref.live_blocks(n, blk):] = -7
        lists["counts"].view(B, Hl, NQ)[b, :, ref.live_blocks(n, blk):] = NK + 5
    assert _same(ext(q, k, v, lists, q_len=q_len, **kw), (out, lse))
    assert _same(ext(q, k, v, mask, q_len=q_len, **kw), (out, lse))
    # e4m3 with power-of-two scales = the 2-byte call on the dequantised cache
    pair = kv8.pow2_scales(Hkv, c["seed"])
    kc, vc, kd, vd = tg8._quantised(kf.numpy(), vf.numpy(), pair, lens, dt)
    ks, vs = tg8._scales(pair)
    want8 = ext(q, kd, vd, mask, q_len=q_len, **kw)
    assert _same(ext(q, tg8._dev8(kc), tg8._dev8(vc), mask, q_len=q_len, k_scale=ks, v_scale=vs, **kw), want8)
    if c["seed"] % 3 == 0:
        kp8, vp8, table8, _ = tg8._pool8(kc, vc, blk, lens, c["seed"], bad=-1)
        assert _same(ext(q, tg8._dev8(kp8), tg8._dev8(vp8), mask, q_len=q_len, k_scale=ks, v_scale=vs,
                         **dict(kw, block_table=torch.from_numpy(table8).to(DEV))), want8)
    # q_len = [Sq] * B = the call without q_len (on a q without NaN)
    qz = torch.nan_to_num(q)
    plain = ext(qz, k, v, mask, **kw)
    assert _same(ext(qz, k, v, mask, q_len=[SQ] * B, **kw), plain)
    assert _same(ext(qz, k, v, mask, q_len=torch.full((B,), SQ + 9, dtype=torch.int32, device=DEV), **kw), plain)


# ---- 3. the selection ------------------------------------------------------------------------------------------------------------------
SEL_CASES = [dict(blk=128, D=128, dt="bf16", top_k=3, top_p=None, forced=True, qset=0),
             dict(blk=64, D=64, dt="fp16", top_k=4, top_p=None, forced=False, qset=1),
             dict(blk=128, D=64, dt="fp16", top_k=2, top_p=None, forced=False, qset=2),
             dict(blk=64, D=128, dt="bf16", top_k=5, top_p=None, forced=True, qset=2),
             dict(blk=128, D=128, dt="fp16", top_k=4, top_p=0.7, forced=True, qset=1),
             dict(blk=64, D=64, dt="bf16", top_k=6, top_p=0.5, forced=False, qset=0),
             dict(blk=64, D=128, dt="fp16", top_k=8, top_p=0.9, forced=True, qset=2),
             dict(blk=128, D=64, dt="bf16", top_k=3, top_p=0.3, forced=False, qset=1)]


@pytest.mark.parametrize("c", SEL_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_selection_is_the_truncated_selection_byte_for_byte(c):
    from rectified_spaattn_amd import pool_keys, select_blocks, select_blocks_pooled
    H, Hkv, D, blk = 8, 2, c["D"], c["blk"]
    NQ, NK = -(-SQ // blk), -(-SK // blk)
    raw = (ref.QLENS + (ref.RAW_QLEN,))[c["qset"]]
    ns = ref.clamp(raw, SQ)
    lens = [SK, 40, 333, 129]
    g = torch.Generator().manual_seed(40 + c["qset"])
    q = torch.randn(B, H, SQ, D, generator=g).to(DEV, TDT[c["dt"]])
    for b, n in enumerate(ns):
        q[b, :, n:] = float("nan")
    k = torch.randn(B, Hkv, SK, D, generator=g).to(DEV, TDT[c["dt"]])
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
    q_len = torch.tensor(raw, dtype=torch.int32, device=DEV) if c["qset"] == 2 else list(raw)
    kw = dict(block_size=blk, causal=True, keep_first=int(c["forced"]), keep_local=int(c["forced"]), as_lists=True, return_scores=True)
    if c["top_p"] is not None:
        kw.update(top_p=c["top_p"], return_mass=True)
    pooled = pool_keys(k, block_size=blk, kv_len=lens)
    got = select_blocks_pooled(q, pooled, c["top_k"], kv_len=lens, q_len=q_len, **kw)
    lists, scores = got[0], got[1]
    mass = got[2] if c["top_p"] is not None else None
    Hl = Hkv
    bit = lists["bitmask"].view(B, Hl, NQ, -1)
    cols, counts = lists["cols"].view(B, Hl, NQ, NK), lists["counts"].view(B, Hl, NQ)
    kept = 0
    for b, n in enumerate(ns):
        nq = ref.live_blocks(n, blk)
        # the blocks without a row: empty
        assert not bit[b, :, nq:].any() and not counts[b, :, nq:].any() and bool(torch.isneginf(scores[b, :, nq:]).all())
        assert mass is None or not mass[b, :, nq:].any()
        if n == 0:
            continue
        want = select_blocks_pooled(q[b:b + 1, :, :n], pooled[b:b + 1], c["top_k"], kv_len=[lens[b]], **kw)
        wl = want[0]
        assert torch.equal(bit[b, :, :nq], wl["bitmask"].view(Hl, nq, -1)), b
        assert torch.equal(counts[b, :, :nq], wl["counts"].view(Hl, nq)), b
        live = torch.arange(NK, device=DEV)[None, None, :] < counts[b, :, :nq, None]
        assert torch.equal(torch.where(live, cols[b, :, :nq], 0), torch.where(live, wl["cols"].view(Hl, nq, NK), 0)), b
        assert tg8._same(scores[b:b + 1, :, :nq].contiguous(), want[1]), b
        if mass is not None:
            assert tg8._same(mass[b:b + 1, :, :nq].contiguous(), want[2]), b
        kept += int(counts[b, :, :nq].sum())
    assert kept > 0
    # the score pass spread over workgroups of its own (these shapes default to one: the select workgroup scores) gives the same bytes
    for splits in (2, 4):
        spread = select_blocks_pooled(q, pooled, c["top_k"], kv_len=lens, q_len=q_len, score_splits=splits, **kw)
        tg8._same_lists(spread[0], lists)
        assert all(tg8._same(x, y) for x, y in zip(spread[1:], got[1:])), splits
    # select_blocks gives the bytes of select_blocks_pooled
    again = select_blocks(q, k, c["top_k"], kv_len=lens, q_len=q_len, **kw)
    tg8._same_lists(again[0], lists)
    assert all(tg8._same(x, y) for x, y in zip(again[1:], got[1:]))
    # the mask form, and q_len = Sq is the call without it
    as_mask = select_blocks_pooled(q, pooled, c["top_k"], kv_len=lens, q_len=q_len, **dict(kw, as_lists=False))[0]
    assert as_mask.shape == (B, Hl, NQ, NK) and int(as_mask.sum()) == int(counts.sum())
    qz = torch.nan_to_num(q)
    full = select_blocks_pooled(qz, pooled, c["top_k"], kv_len=lens, **kw)
    same = select_blocks_pooled(qz, pooled, c["top_k"], kv_len=lens, q_len=SQ, **kw)
    dev_full = select_blocks_pooled(qz, pooled, c["top_k"], kv_len=lens, q_len=torch.tensor([SQ + 3], device=DEV), **kw)
    for other in (same, dev_full):
        tg8._same_lists(other[0], full[0])
        assert all(tg8._same(x, y) for x, y in zip(other[1:], full[1:]))


# ---- 4. exact visibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.WITNESS_CASES, ids=lambda c: c["id"])
def test_exact_visibility(c):
    """Zero scores, V of 0 / 1: every output element is a count over the visible keys divided by their number; the probes sit either
    side of each item's own causal diagonal at its first and last live row.  The bound is test_gpu_extend's: |got - ref| <=
    ULP |ref| + FLOOR max|ref|, exactly 0 where the reference is 0 -- every row at or beyond q_len[b] among them."""
    inp = ref.witness_inputs(c)
    want, lse_want = ref.witness_reference(c, inp)
    q, k, v = (torch.from_numpy(inp[n]).to(DEV, TDT[c["dt"]]) for n in ("q", "k", "v"))
    for b, n in enumerate(c["q_lens"]):
        q[b, :, n:] = float("nan")
    tgd._nan_tail(k, v, c["lens"])
    raw = ref.combo_qlens(c)
    q_len = torch.tensor(raw, dtype=torch.int64, device=DEV) if c["qset"] == 2 else list(raw)
    out, lse = ext(q, k, v, torch.from_numpy(inp["mask"]).to(DEV), kv_len=list(c["lens"]), q_len=q_len, sm_scale=inp["sm_scale"],
                   block_size=c["blk"], causal=c["causal"], blocks_per_split=c["C"], return_lse=True)
    got, lse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    ok, worst = eref.within(got, want, c["dt"])
    print(f"{c['id']}: worst {worst:.3f} tolerances")
    assert ok, worst
    has = np.isfinite(lse_want)
    assert np.isneginf(lse[~has]).all() and np.isfinite(lse[has]).all()


# ---- 5. the whole step -----------------------------------------------------------------------------------------------------------------
class _Step:
    """append_kv_e4m3(n_new = q_len) -> pool_keys(start = prev) -> select_blocks_pooled(as_lists, q_len) -> block_sparse_extend(q_len)
    over a paged e4m3 cache; B = 4 items padded to Sq = 130 rows of 128-token blocks."""
    H, Hkv, Sq, D, blk, dt = 8, 2, 130, 128, 128, torch.bfloat16

    def __init__(self, seed):
        self.NK = -(-SK // self.blk)
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(B, self.H, self.Sq, self.D, generator=g).to(DEV, self.dt)
        self.kf, self.vf = (torch.randn(B, self.Hkv, SK, self.D, generator=g).to(self.dt) for _ in range(2))
        self.pair = kv8.pow2_scales(self.Hkv, 3)
        self.ks, self.vs = tg8._scales(self.pair)
        self.P = B * self.NK + 3
        self.table = torch.randperm(self.P, generator=g)[:B * self.NK].reshape(B, self.NK).to(torch.int32).to(DEV)
        self.kp, self.vp = (tg8._dev8(np.full((self.P, self.Hkv, self.blk, self.D), kv8.NAN_CODE, np.uint8)) for _ in range(2))
        self.pooled = torch.full((B, self.Hkv, self.NK, self.D), float("nan"), device=DEV)
        self.new_k, self.new_v = (torch.zeros(B, self.Hkv, self.Sq, self.D, dtype=self.dt, device=DEV) for _ in range(2))
        self.prev = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.q_len = torch.zeros(B, dtype=torch.int32, device=DEV)
        self.kv_len = torch.zeros(B, dtype=torch.int32, device=DEV)

    def prefill(self, prev):
        from rectified_spaattn_amd import append_kv_e4m3, pool_keys
        append_kv_e4m3(self.kf.to(DEV), self.vf.to(DEV), self.kp, self.vp, start=0, n_new=prev, k_scale=self.ks, v_scale=self.vs,
                       block_table=self.table)
        pool_keys(self.kp, kv_len=prev, block_table=self.table, k_scale=self.ks, out=self.pooled)

    def feed(self, prev, ns):
        """The chunk of item b: tokens prev[b] .. prev[b] + ns[b] of its sequence, NaN behind them (in q's padding rows too)."""
        self.new_k.fill_(float("nan"))
        self.new_v.fill_(float("nan"))
        for b, (p, n) in enumerate(zip(prev, ns)):
            self.new_k[b, :, :n], self.new_v[b, :, :n] = self.kf[b, :, p:p + n].to(DEV), self.vf[b, :, p:p + n].to(DEV)
        self.prev.copy_(torch.tensor(prev, dtype=torch.int32))
        self.q_len.copy_(torch.tensor(ns, dtype=torch.int32))
        self.kv_len.copy_(self.prev + self.q_len)

    def run(self, pooled, kp, vp, items=slice(None), rows=None, limits=None):
        """The four calls on the batch items `items` (their first `rows` rows; limits: (prev, q_len, kv_len) in any form)."""
        from rectified_spaattn_amd import append_kv_e4m3, pool_keys, select_blocks_pooled
        prev, q_len, kv_len = limits or (self.prev, self.q_len, self.kv_len)
        rows = slice(None) if rows is None else slice(0, rows)
        table, q = self.table[items], self.q[items, :, rows]
        kw8 = dict(k_scale=self.ks, v_scale=self.vs, block_table=table)
        append_kv_e4m3(self.new_k[items, :, rows], self.new_v[items, :, rows], kp, vp, start=prev, n_new=q_len, **kw8)
        pool_keys(kp, kv_len=kv_len, start=prev, block_table=table, k_scale=self.ks, out=pooled[items])
        lists = select_blocks_pooled(q, pooled[items], 3, kv_len=kv_len, q_len=q_len, causal=True, keep_first=1, keep_local=1,
                                     as_lists=True)
        return (lists,) + ext(q, kp, vp, lists, kv_len=kv_len, q_len=q_len, causal=True, blocks_per_split=2, return_lse=True, **kw8)

    def check_against_items(self, got, stale, prev, ns):
        """The batched step = the step of every item alone on its truncated chunk (the existing calls: no q_len)."""
        lists, out, lse = got
        NQ = -(-self.Sq // self.blk)
        counts = lists["counts"].view(B, self.Hkv, NQ)
        cols = lists["cols"].view(B, self.Hkv, NQ, self.NK)
        for b, n in enumerate(ns):
            assert not out[b, :, n:].any() and bool(torch.isneginf(lse[b, :, n:]).all())
            nq = ref.live_blocks(n, self.blk)
            assert not counts[b, :, nq:].any()
            if n == 0:
                continue
            pooled, kp, vp = (t.clone() for t in stale)
            l1, o1, s1 = self.run(pooled, kp, vp, slice(b, b + 1), n, ([prev[b]], None, [prev[b] + n]))
            assert tg8._same(o1, out[b:b + 1, :, :n].contiguous()) and tg8._same(s1, lse[b:b + 1, :, :n].contiguous()), b
            assert torch.equal(l1["counts"].view(self.Hkv, nq), counts[b, :, :nq])
            live = torch.arange(self.NK, device=DEV)[None, None, :] < counts[b, :, :nq, None]
            assert torch.equal(torch.where(live, l1["cols"].view(self.Hkv, nq, self.NK), 0), torch.where(live, cols[b, :, :nq], 0))


def test_the_whole_step_equals_the_per_item_steps_and_reads_no_length_on_the_host(monkeypatch):
    prev, ns = [200, 333, 511, 0], [130, 40, 1, 0]
    s = _Step(7)
    s.prefill(prev)
    s.feed(prev, ns)
    stale = (s.pooled.clone(), s.kp.clone(), s.vp.clone())
    on_host = s.run(*(t.clone() for t in stale), limits=(prev, ns, [p + n for p, n in zip(prev, ns)]))
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("a device length was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = s.run(s.pooled, s.kp, s.vp)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    tg8._same_lists(got[0], on_host[0])
    assert _same(got[1:], on_host[1:])
    s.check_against_items(got, stale, prev, ns)
    assert bool(got[1][0].any()) and bool(torch.isfinite(got[1].float()).all())


def test_one_graph_for_the_ragged_step_follows_the_lengths():
    prev, ns = [200, 333, 511, 0], [130, 40, 1, 5]
    s = _Step(11)
    s.prefill(prev)
    s.feed(prev, ns)
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
    s.check_against_items(got, stale, prev, ns)
    before = got[1].clone()
    # the next step: other chunk lengths (the decode item becomes a chunk, the chunk a decode item), the limits changed on the
    # device, the cache grown by the first step, a page moved
    prev = [p + n for p, n in zip(prev, ns)]
    ns = [1, 0, 129, 64]
    s.feed(prev, ns)
    spare = sorted(set(range(s.P)) - set(s.table.reshape(-1).tolist()))[0]
    moved = s.table[1, 2].item()
    for pool in (s.kp, s.vp):
        pool.view(torch.uint8)[spare] = pool.view(torch.uint8)[moved].clone()
        pool.view(torch.uint8)[moved] = kv8.NAN_CODE
    s.table[1, 2] = spare
    stale = (s.pooled.clone(), s.kp.clone(), s.vp.clone())
    graph.replay()
    torch.cuda.synchronize()
    s.check_against_items(got, stale, prev, ns)
    eager = s.run(*stale)
    tg8._same_lists(got[0], eager[0])
    assert _same(got[1:], eager[1:])
    assert not torch.equal(got[1], before) and bool(torch.isfinite(got[1].float()).all())
