"""select_blocks_observed on the device: the scores against tests/observed_ref.py, exact visibility at
zero queries, the selection against the project's reference select on the device's own scores, the same bytes from every call, and
the point of the criterion.  Sk = 2 block + 37: every shape has a ragged last block."""
import itertools

import numpy as np
import pytest
import torch

import observed_ref as oref
import select_p_ref as pref
import select_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = dict(bf16=torch.bfloat16, fp16=torch.float16)
TOL = 2.0 ** -9     # the worst case of a fixed-order fp32 sum of at most 2^15 positive terms; covers the logit error < 2^-13


def _inputs(seed, B, H, Hkv, W, Sk, D, dt="bf16"):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, D, generator=gen).to(DT[dt]).to(DEV), torch.randn(B, Hkv, Sk, D, generator=gen).to(DT[dt]).to(DEV)


def _hide(k, lens, blk, paged):
    """NaN in every key at or beyond lens[b]; paged: a shuffled table into a pool of three pages more than it names, all NaN."""
    k = k.clone()
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
    if not paged:
        return k, None
    B, Hkv, Sk, D = k.shape
    NK = -(-Sk // blk)
    perm = torch.randperm(B * NK + 3, generator=torch.Generator().manual_seed(9))
    table = perm[:B * NK].view(B, NK).to(torch.int32)
    pool = torch.full((B * NK + 3, Hkv, blk, D), float("nan"), dtype=k.dtype, device=DEV)
    kp = torch.nn.functional.pad(k, (0, 0, 0, NK * blk - Sk), value=float("nan"))
    pool[table.reshape(-1).long().to(DEV)] = kp.view(B, Hkv, NK, blk, D).transpose(1, 2).reshape(B * NK, Hkv, blk, D)
    return pool, table.to(DEV)


def _check(t, P, Sk, lens, blk):
    t, want = t.cpu().numpy().astype(np.float64), oref.scores(P, Sk, lens, blk)
    vis = np.isfinite(want)
    assert np.array_equal(np.isneginf(t), ~vis)
    err = np.abs(np.exp(t[vis] - want[vis]) - 1.0).max()
    assert err <= TOL, f"max |exp(t) / P - 1| = {err:.3e} (bar {TOL:.3e})"


BASE = [dict(dt=dt, D=D, blk=blk, causal=causal) for dt, D, blk, causal in itertools.product(DT, (64, 128), (64, 128), (False, True))]
EXTRA = [dict(B=2, **kw) for kw in (dict(W=1), dict(W=16, heads="q"), dict(W=64), dict(g=1, heads="q"), dict(g=8), dict(paged=True),
                                    dict(short=True))]


@pytest.mark.parametrize("case", BASE + EXTRA, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_scores_against_fp64(case):
    """W = 17: a full row tile and one live row; g = 8: two head passes; extra: kv_len = [Sk, block + 5] (short: 9 < W) on the device."""
    from rectified_spaattn_amd import select_blocks_observed
    c = dict(dict(dt="bf16", D=128, blk=128, causal=True, B=1, W=17, g=4, heads="kv", paged=False, short=False), **case)
    blk, B, W = c["blk"], c["B"], c["W"]
    Sk = 2 * blk + 37
    lens = [Sk] if B == 1 else [Sk, 9 if c["short"] else blk + 5]
    q, k = _inputs(3, B, 2 * c["g"], 2, W, Sk, c["D"], c["dt"])
    P = oref.mass(q.double().cpu().numpy(), k.double().cpu().numpy(), lens, blk, c["causal"], None, c["heads"])
    kk, table = _hide(k, lens, blk, c["paged"])
    kv = None if B == 1 else torch.tensor(lens, dtype=torch.int32, device=DEV)
    _, t = select_blocks_observed(q, kk, 2, block_size=blk, kv_len=kv, causal=c["causal"], mask_heads=c["heads"], block_table=table,
                                  return_scores=True)
    _check(t, P, Sk, lens, blk)


@pytest.mark.parametrize("causal,W", itertools.product((False, True), (5, 64)))
def test_zero_queries_give_the_share_of_visible_keys(causal, W):
    """P[jb] = heads x sum over the rows of visible_keys(r, jb) / visible_keys(r); kv_len one below, at, one above a block edge."""
    from rectified_spaattn_amd import select_blocks_observed
    blk, H, Sk = 64, 2, 2 * 64 + 37
    lens = [2 * blk - 1, 2 * blk, 2 * blk + 1]
    q, k = _inputs(4, 3, H, 1, W, Sk, 64)
    P = np.zeros((3, 1, 3))
    for b, n in enumerate(lens):
        for r in range(W):
            n_r = max(min(n, r + n - W + 1), 0) if causal else n
            for jb in range(3):
                P[b, 0, jb] += H * min(max(min(n_r, (jb + 1) * blk) - jb * blk, 0), blk) / max(n_r, 1)
    _, t = select_blocks_observed(torch.zeros_like(q), _hide(k, lens, blk, False)[0], 2, block_size=blk, kv_len=lens, causal=causal,
                                  return_scores=True)
    _check(t, P, Sk, lens, blk)


@pytest.mark.parametrize("blk,heads", [(128, "kv"), (64, "q")])
def test_selection_is_the_reference_select_on_the_device_scores(blk, heads):
    from rectified_spaattn_amd import block_sparse_decode, select_blocks_observed
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, W, D, NK = 2, 8, 2, 17, 128, 9
    Sk, Hl = NK * blk, Hkv if heads == "kv" else H
    lens = [Sk - 3, 5 * blk + 5]
    q, k = _inputs(5, B, H, Hkv, W, Sk, D)
    pool, table = _hide(k, lens, blk, True)
    kw = dict(block_size=blk, kv_len=lens, causal=True, keep_first=1, keep_local=1, mask_heads=heads, block_table=table)
    lists, t = select_blocks_observed(q, pool, 4, as_lists=True, return_scores=True, **kw)
    mask = select_blocks_observed(q, pool, 4, **kw)
    t64 = t.cpu().numpy().astype(np.float64)
    vis, frc = ref.visible(W, Sk, lens, blk, True), ref.forced(W, Sk, lens, blk, True, 1, 1)
    want = ref.kept_vectorised(t64, vis, frc, 4)
    assert np.array_equal(mask.cpu().numpy(), want) and mask.shape == (B, Hl, 1, NK)
    for name, x in block_mask_to_lists(torch.from_numpy(want).to(DEV), B, Hl).items():
        live = torch.arange(NK, device=DEV) < lists["counts"][..., None] if name == "cols" else 1      # (cols: the first counts entries)
        assert torch.equal(lists[name] * live, x * live), name
    shape = dict(blk=blk, lens=lens, causal=True, keep_first=1, keep_local=1, mask_heads=heads)      # top-p: integer weights, exact
    mask_p, t_p, mass = select_blocks_observed(q, pool, 7, top_p=0.6, return_scores=True, return_mass=True, **kw)
    own = pref.select(np.empty((B, H, W, D)), np.empty((B, Hkv, Sk, D)), 7, 0.6, score_scale=1.0, t=t64, **shape)
    assert torch.equal(t_p, t) and np.array_equal(mask_p.cpu().numpy(), own["mask"]) and np.array_equal(mass.cpu().numpy(), own["mass"])
    if heads == "kv":       # the lists drive decode over the same paged cache
        out = block_sparse_decode(q[:, :, -1:], pool, pool.nan_to_num(0.0), lists, kv_len=lens, block_size=blk, causal=True,
                                  block_table=table)
        assert bool(torch.isfinite(out.float()).all())


def test_every_call_gives_the_same_bytes():
    from rectified_spaattn_amd import select_blocks_observed
    B, blk, NK = 2, 128, 9
    q, k = _inputs(6, B, 8, 2, 33, NK * blk - 50, 128)
    kv = torch.tensor([NK * blk - 50, 700], dtype=torch.int32, device=DEV)

    def call(splits=None):
        mask, t, mass = select_blocks_observed(q, k, 3, kv_len=kv, causal=True, top_p=0.9, return_scores=True, return_mass=True,
                                               score_splits=splits)
        return [mask.view(torch.uint8), t.view(torch.int32), mass.view(torch.int32)]
    first = call()
    for other in (call(), call(1), call(3)):
        assert all(torch.equal(a, b) for a, b in zip(first, other))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        call()      # (the allocator's pool of the side stream is warm before the capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            held = call()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, held))


def test_one_aligned_key_per_row_wins_where_the_pooled_mean_loses():
    """Each row of head 0 has one key aligned with it (8 x the row: a logit ~ 90) in block 5 among unit-normal keys: kept at top_k = 1.
    select_blocks (mean pooling) ranks the block below the median on the same tensors.  The block's other keys are shifted by
    -2 c s / (block - W), s = the sum of head 0's rows (the needles alone would pull the block's mean towards s): its mean is
    -c s / block plus noise, its pooled score ~ -c D / block = -8 against a noise of standard deviation < 1."""
    from rectified_spaattn_amd import select_blocks, select_blocks_observed
    B, H, Hkv, W, D, blk, NK, at, c = 1, 4, 1, 17, 128, 128, 11, 5, 8.0
    q, k = _inputs(7, B, H, Hkv, W, NK * blk, D)
    rows = q[0, 0].float()
    block = k[0, 0, at * blk:(at + 1) * blk].float() - 2.0 * c / (blk - W) * rows.sum(0)
    block[3 * torch.arange(W, device=DEV)] = c * rows
    k[0, 0, at * blk:(at + 1) * blk] = block.to(k.dtype)
    mask = select_blocks_observed(q, k, 1)
    assert mask[0, 0, 0].nonzero().flatten().tolist() == [at]
    _, t = select_blocks(q, k, 1, return_scores=True)
    assert int((t[0, 0, 0] > t[0, 0, 0, at]).sum()) > NK // 2
