"""select_blocks on the MI355X (rsa_block_select: the pooling pass and the score-and-select pass) against
the fp64 reference of tests/select_ref.py.

    exact class      small integers pooled over power-of-two counts: every fp32 sum and division is exact, so the mask and the
                     scores equal the reference's bit for bit, ties included
    rounding class   random normal inputs over ragged counts: the count and the forced / visible sets hold exactly, the choice
                     and the scores within tol = 2^-14 M, M = sum |q| mean x |k| mean of the block pair -- four times the fp32
                     bound (b + D + g) 2^-24 M <= 2^-15.9 M of b-term pooling sums, a D-term dot product and a g-term group sum
"""
import itertools

import numpy as np
import pytest
import torch

import select_ref as ref
import test_ranged_cpu as rule
from test_gpu_gqa import TOL, _attend, _expand_heads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
KEEPS_TOPK = [(kf, kl, tk) for kf in (0, 1, 2) for kl in (0, 1, 2) for tk in (0, 1, 3, "NK", "NK+5")]      # 45


def _ints(shape, seed):
    """Integers -2 .. 2 (exact in bf16 and fp16) -> (device tensor maker, float64 numpy)."""
    a = np.random.default_rng(seed).integers(-2, 3, shape)
    return a, a.astype(np.float64)


def _top_k(tk, NK):
    return {"NK": NK, "NK+5": NK + 5}.get(tk, tk)


def _assert_exact_sums(q64, k64, lens, blk, heads):
    """Every partial sum of every score is a multiple of 1 / (count_q count_k) >= 2^-14 below M: exact in fp32 iff M < 2^10."""
    M = ref.magnitude(q64, k64, lens, blk, heads)
    assert M.max() < 2.0 ** 10 * (128 / blk) ** 2, M.max()


def _check_exact(q, k, q64, k64, lens, blk, heads, causal, combos, kv_len):
    from rectified_spaattn_amd import select_blocks
    t64 = None
    for n, (kf, kl, tk) in enumerate(combos):
        NK = -(-k.shape[2] // blk)
        r = ref.select(q64, k64, _top_k(tk, NK), blk=blk, lens=lens, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads)
        kw = dict(block_size=blk, kv_len=kv_len, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads)
        what = (tuple(q.shape), tuple(k.shape), lens, blk, heads, causal, kf, kl, tk)
        if n == 0:
            mask, t = select_blocks(q, k, _top_k(tk, NK), return_scores=True, **kw)
            t64 = r["t"]
            assert t.dtype == torch.float32 and t.shape == t64.shape
            want = torch.from_numpy(t64.astype(np.float32))
            assert np.array_equal(want.double().numpy(), t64), "the reference's scores are not fp32 values"
            assert torch.equal(t.cpu().view(torch.int32), want.view(torch.int32)), what
        else:
            mask = select_blocks(q, k, _top_k(tk, NK), **kw)
        assert mask.dtype == torch.bool and mask.shape == r["mask"].shape
        assert torch.equal(mask.cpu(), torch.from_numpy(r["mask"])), what
    return t64


# ---- 1. the exact class ----------------------------------------------------------------------------------------------------------
def _small_shapes(b):
    """(Sq, Sk, lens): every block's row count and valid-key count a power of two."""
    return [
        (2 * b + b // 2, 2 * b + b // 2, [2 * b + b // 2, b + b // 4]),           # NK = 3: one ballot step
        (5 * b + b // 2, 5 * b + b // 2, [5 * b + b // 2, 3 * b + b // 4]),       # Sq = Sk
        (2 * b, 8 * b + b // 4, [8 * b + b // 4, 4 * b + b // 2]),                # few rows against many keys: off_b > 0
        (5 * b + b // 2, 5 * b + b // 2, [2 * b + b // 2, b // 4]),               # Sq > len_b: row blocks that see nothing
    ]


EXACT = [(dt, D, blk) for dt in DT for D in (16, 64, 128) for blk in (64, 128)]


@pytest.mark.parametrize("dt,D,blk", EXACT, ids=[f"{a}-D{b}-b{c}" for a, b, c in EXACT])
def test_exact_class_small_rows(dt, D, blk):
    """B = 2 with a key limit per item, H = 4 over Hkv = 4, 2, 1, both mask_heads, causal on and off, the kv_len forms taking turns;
    the 45 (keep_first, keep_local, top_k) triples go round over the 48 configurations, nine each."""
    B, H = 2, 4
    turn = itertools.cycle(range(len(KEEPS_TOPK)))
    kv_forms = itertools.cycle(("list", "tensor"))
    blind = 0
    for s, (Sq, Sk, lens) in enumerate(_small_shapes(blk)):
        for Hkv in (4, 2, 1):
            qi, q64 = _ints((B, H, Sq, D), 100 * s + Hkv + D)
            ki, k64 = _ints((B, Hkv, Sk, D), 100 * s + Hkv + D + 50)
            q, k = (torch.from_numpy(a).to(DEV, DT[dt]) for a in (qi, ki))
            for heads in ("kv", "q"):
                _assert_exact_sums(q64, k64, lens, blk, heads)
                for causal in (False, True):
                    combos = [KEEPS_TOPK[next(turn)] for _ in range(9)]
                    kv = lens if next(kv_forms) == "list" else torch.tensor(lens, dtype=torch.int32, device=DEV)
                    t64 = _check_exact(q, k, q64, k64, lens, blk, heads, causal, combos, kv)
                    blind += int(np.isinf(t64).all(-1).sum())
                    assert np.isfinite(t64).any()
    assert blind > 0        # (the last shape, causal: whole row blocks without a visible block, count 0)


MANY = [("bf16", 64, 64, 70), ("fp16", 16, 64, 300), ("bf16", 16, 128, 70)]


@pytest.mark.parametrize("dt,D,blk,NK", MANY, ids=[f"{a}-D{b}-b{c}-NK{d}" for a, b, c, d in MANY])
def test_exact_class_more_blocks_than_a_ballot_step_and_than_threads(dt, D, blk, NK):
    B, H, Hkv = 2, 4, 2
    Sk = (NK - 1) * blk + blk // 2
    lens = [Sk, (NK - 6) * blk + blk // 4]
    for Sq in (Sk, 2 * blk):
        qi, q64 = _ints((B, H, Sq, D), NK + Sq)
        ki, k64 = _ints((B, Hkv, Sk, D), NK + Sq + 1)
        q, k = (torch.from_numpy(a).to(DEV, DT[dt]) for a in (qi, ki))
        for heads, causal in (("kv", True), ("q", False)) if Sq == Sk else (("kv", False), ("q", True)):
            _assert_exact_sums(q64, k64, lens, blk, heads)
            combos = [(1, 1, 3), (0, 0, 1), (2, 2, "NK"), (0, 2, "NK+5"), (1, 0, 0), (0, 0, 65), (0, 1, NK - 7)]
            _check_exact(q, k, q64, k64, lens, blk, heads, causal, combos, lens)


def test_exact_class_at_the_key_block_limit():
    """NK = 8192 blocks of 64, B = H = 1, D = 16: 16 MB of K, 32 KB of scores in LDS."""
    blk, NK, D = 64, 8192, 16
    Sk, Sq = (NK - 1) * blk + blk // 2, 2 * blk
    qi, q64 = _ints((1, 1, Sq, D), 1)
    ki, k64 = _ints((1, 1, Sk, D), 2)
    q, k = (torch.from_numpy(a).to(DEV, torch.bfloat16) for a in (qi, ki))
    _assert_exact_sums(q64, k64, [Sk], blk, "kv")
    _check_exact(q, k, q64, k64, [Sk], blk, "kv", True, [(1, 2, 90), (0, 0, 4000), (0, 0, "NK+5")], None)
    _check_exact(q, k, q64, k64, [Sk - 3 * blk], blk, "q", False, [(0, 1, 1)], Sk - 3 * blk)


# ---- 2. the rounding class -------------------------------------------------------------------------------------------------------
ROUND = [(dt, D, blk) for dt in DT for D in (16, 128) for blk in (64, 128)] + [("bf16", 32, 128), ("fp16", 64, 64)]


def _normal(B, H, Hkv, Sq, Sk, D, dt, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, DT[dt])
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(DEV, DT[dt])
    return q, k, q.double().cpu().numpy(), k.double().cpu().numpy()


@pytest.mark.parametrize("dt,D,blk", ROUND, ids=[f"{a}-D{b}-b{c}" for a, b, c in ROUND])
def test_rounding_class_every_row(dt, D, blk):
    from rectified_spaattn_amd import select_blocks
    B, H = 2, 4
    rows = 0
    for (Sq, Sk, lens), Hkv in (((300, 1500, [1500, 1333]), 2), ((1210, 1210, [1210, 777]), 1), ((1100, 1000, [1000, 333]), 4)):
        q, k, q64, k64 = _normal(B, H, Hkv, Sq, Sk, D, dt, Sq + Sk + D + blk)
        NK = -(-Sk // blk)
        for heads, causal, kf, kl, top_k in (("kv", True, 1, 1, 3), ("q", False, 0, 2, 4), ("kv", False, 0, 0, 2),
                                             ("q", True, 2, 0, 1), ("kv", True, 0, 1, NK // 2)):
            r = ref.select(q64, k64, top_k, blk=blk, lens=lens, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads)
            tol = 2.0 ** -14 * ref.magnitude(q64, k64, lens, blk, heads)
            mask, t = select_blocks(q, k, top_k, block_size=blk, kv_len=lens, causal=causal, keep_first=kf, keep_local=kl,
                                    mask_heads=heads, return_scores=True)
            kept, got = mask.cpu().numpy(), t.double().cpu().numpy()
            vis, frc = (np.broadcast_to(a[:, None], kept.shape) for a in (r["vis"], r["frc"]))
            what = (Sq, Sk, heads, causal, kf, kl, top_k)
            # exactly: kept within visible, forced within kept, the count
            assert not (kept & ~vis).any() and not (frc & ~kept).any(), what
            nf, nv = frc.sum(-1), vis.sum(-1)
            assert np.array_equal(kept.sum(-1), np.minimum(np.maximum(top_k, nf), nv)), what
            # the scores
            assert np.array_equal(np.isneginf(got), ~vis), what
            err = np.abs(np.where(vis, got - np.where(vis, r["t"], 0.0), 0.0))
            print(f"{what}: score error / tol max {float((err[vis] / np.maximum(tol[vis], 1e-300)).max()):.3f}")
            assert (err <= tol)[vis].all(), what
            # the choice: theta = the reference's (top_k - |forced|)-th best unforced score
            cand = vis & ~frc
            need = np.maximum(top_k - nf, 0)
            srt = -np.sort(-np.where(cand, r["t"], -np.inf), axis=-1)
            theta = np.take_along_axis(srt, np.clip(need - 1, 0, NK - 1)[..., None], axis=-1)
            theta = np.where((need == 0)[..., None], np.inf, theta)
            t_ref = np.where(vis, r["t"], 0.0)
            assert (t_ref >= theta - tol)[kept & cand].all(), what
            assert (t_ref <= theta + tol)[vis & ~kept].all(), what
            rows += kept[..., 0].size
            assert bool((nv == 0).any()) == (causal and Sq - min(lens) >= blk)
    assert rows > 0


# ---- 3. lists --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk,heads", [(128, "kv"), (64, "q")])
def test_lists_are_what_the_mask_converts_to(blk, heads):
    from rectified_spaattn_amd import select_blocks
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, D = 2, 4, 2, 64
    q, k, _, _ = _normal(B, H, Hkv, 700, 9000, D, "bf16", 5)
    kw = dict(block_size=blk, kv_len=[9000, 1500], causal=True, keep_first=1, keep_local=2, mask_heads=heads)
    mask = select_blocks(q, k, 40, **kw)
    lists = select_blocks(q, k, 40, as_lists=True, **kw)
    Hl = Hkv if heads == "kv" else H
    want = block_mask_to_lists(mask, B, Hl)
    assert set(lists) == {"bitmask", "cols", "counts"}
    for name in ("bitmask", "counts"):
        assert lists[name].dtype == torch.int32 and lists[name].shape == want[name].shape
        assert torch.equal(lists[name], want[name]), name
    NK = mask.shape[-1]
    live = torch.arange(NK, device=DEV)[None, None, :] < want["counts"][..., None]
    assert lists["cols"].shape == want["cols"].shape
    assert torch.equal(torch.where(live, lists["cols"], 0), torch.where(live, want["cols"], 0))
    assert int(want["counts"].max()) == 40 and int(want["counts"].min()) < 40
    lists2, t = select_blocks(q, k, 40, as_lists=True, return_scores=True, **kw)
    assert torch.equal(lists2["bitmask"], lists["bitmask"]) and t.shape == mask.shape


# ---- 4. kv_len on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [(torch.int32, 3), (torch.int64, 3), (torch.int64, 1)])
def test_device_kv_len_gives_the_ints_result_and_is_not_read_on_the_host(monkeypatch, dtype, n):
    from rectified_spaattn_amd import select_blocks
    B, H, Hkv, D = 3, 4, 2, 128
    q, k, _, _ = _normal(B, H, Hkv, 640, 900, D, "bf16", 9)
    lens = [900, 333, 517] if n == 3 else [517]
    kw = dict(causal=True, keep_first=1, keep_local=1, return_scores=True)
    on_host = select_blocks(q, k, 3, kv_len=lens if n == 3 else lens[0], **kw)
    kv = torch.tensor(lens, dtype=dtype, device=DEV)
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("kv_len was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        on_device = select_blocks(q, k, 3, kv_len=kv, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    for a, b in zip(on_device, on_host):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))
    assert bool(on_host[0].any()) and not bool(on_host[0].all())


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    from rectified_spaattn_amd import select_blocks
    q, k, _, _ = _normal(2, 8, 2, 3000, 5000, 128, "bf16", 21)
    outs = [select_blocks(q, k, 7, kv_len=[5000, 4444], causal=True, keep_local=1, return_scores=True) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert bool(outs[0][0].any())


# ---- 6. the fused-projection layout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,D", [(8, 2, 128), (6, 2, 64), (4, 1, 16)])
def test_views_of_one_fused_projection_run_without_a_copy(monkeypatch, H, Hkv, D):
    from rectified_spaattn_amd import _core, select_blocks
    B, S = 2, 700
    g = torch.Generator().manual_seed(H + Hkv + D)
    buf = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).to(DEV, torch.bfloat16)
    q = buf[..., :H * D].view(B, S, H, D).permute(0, 2, 1, 3)
    k = buf[..., H * D:(H + Hkv) * D].view(B, S, Hkv, D).permute(0, 2, 1, 3)
    seen = []
    as_bhsd = _core._as_bhsd
    monkeypatch.setattr(_core, "_as_bhsd", lambda t: (seen.append((t.data_ptr(), as_bhsd(t).data_ptr())), as_bhsd(t))[1])
    kw = dict(causal=True, keep_first=1, return_scores=True)
    mask, t = select_blocks(q, k, 2, **kw)
    assert [a for a, _ in seen] == [q.data_ptr(), k.data_ptr()] and all(a == b for a, b in seen), seen
    want, tw = select_blocks(q.contiguous(), k.contiguous(), 2, **kw)
    assert torch.equal(mask, want) and torch.equal(t.view(torch.int32), tw.view(torch.int32))
    assert bool(mask.any()) and not bool(mask.all())


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------
def test_selected_mask_drives_causal_attention_against_fp64():
    """MoBA-style: the first block, the diagonal block and the best of the rest (three in all), then causal attention over the
    selection, held to fp64 attention over exactly the keys the semantics make visible."""
    from rectified_spaattn_amd import block_sparse_attention, select_blocks
    B, H, Hkv, D, S = 2, 4, 2, 128, 5 * 128 + 40
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(B, h, S, D, generator=g).to(DEV, dt) for h in (H, Hkv, Hkv))
    q64, k64, v64 = q.double().cpu(), k.double().cpu(), v.double().cpu()
    lens = [S] * B
    mask = select_blocks(q, k, 3, causal=True, keep_first=1, keep_local=1)
    r = ref.select(q64.numpy(), k64.numpy(), 3, blk=128, lens=lens, causal=True, keep_first=1, keep_local=1)
    assert mask.shape == (B, Hkv, 6, 6) and torch.equal(mask.cpu(), torch.from_numpy(r["mask"]))
    counts = r["mask"].sum(-1)
    assert np.array_equal(counts[0, 0], [1, 2, 3, 3, 3, 3])
    out = block_sparse_attention(q, k, v, mask, causal=True)
    lo, hi = rule.window_ranges(S, lens, -1, 0)
    seen = rule.visible(_expand_heads(r["mask"], H), lo, hi, lens, S, S)
    right = torch.arange(H) // (H // Hkv)
    scores = torch.matmul(q64, k64[:, right].transpose(-1, -2)) * D ** -0.5
    want = _attend(scores, v64[:, right], seen)
    err = (out.double().cpu() - want).abs()
    mx, mean = TOL[dt]
    print(f"max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
    assert torch.isfinite(out.float()).all() and err.max() <= mx and err.mean() <= mean
    assert seen.any(-1).all()
