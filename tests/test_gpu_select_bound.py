"""pool_key_bounds and select_blocks_bound on the MI355X (rsa_pool_key_bounds, rsa_block_select_bound)
against tests/bound_ref.py.

    cache            min and max are exact: equal by value to numpy's over the stored keys, for every workgroups_per_head; an
                     update writes pooled_ref.written's blocks and no other byte; paged = contiguous; e4m3 = the dequantised cache
    exact class      integers -2 .. 2 over power-of-two row counts: every product and partial sum of a score is a multiple of
                     1 / rows below 2^10 (128 / block)^2, exact in fp32 -- scores and masks equal the reference's bit for bit
    rounding class   random normal data: scores within 2^-14 M, M = sum_d |qs_d| max(|mn_d|, |mx_d|) (section 5.11's rule: the sum
                     has the mean score's D terms and one rounding more per term), the sets exactly, the choice within the cut
    one body         every score_splits the same bytes; top_p = 1 at c = 1 is top-k; top_p = 0.9 against select_p_ref
    tied to old code constant blocks give select_blocks_pooled's bytes; the needle is dropped there and kept here
    ragged, packed   = the per-item calls; one graph for the decode step
"""
import itertools

import numpy as np
import pytest
import torch

import bound_ref as ref
import kv8_ref as kv8
import pooled_ref
import select_p_ref as pref
import select_ref
from test_gpu_decode import _pool
from test_gpu_pooled_keys import _bits, _same_lists, _same_scores
from test_gpu_select_blocks import KEEPS_TOPK, _ints, _small_shapes, _top_k

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -12345.6787109375        # (an fp32 value no bound takes)


def _randn(shape, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV, DT[dt])


def _np_bounds(k, lens, blk, fill):
    """numpy min / max of the stored values of k (a device tensor; NaN beyond the limits is never looked at) -> fp32 tensor
    [B, Hkv, NK, 2, D] with `fill` in the blocks without a key."""
    k64 = k.double().cpu().numpy()
    B, Hkv, Sk, D = k64.shape
    NK = -(-Sk // blk)
    want = ref.bounds(k64, lens, blk)
    for b in range(B):
        want[b, :, -(-lens[b] // blk):] = fill
    assert np.isfinite(want).all()
    return torch.from_numpy(want.astype(np.float32))


def _full(shape, value):
    return torch.full(shape, value, dtype=torch.float32, device=DEV)


# ---- 1. the cache, exact by value ----------------------------------------------------------------------------------------------------
CACHE = [(dt, D, blk) for dt in DT for D in (16, 64, 128) for blk in (64, 128)]


@pytest.mark.parametrize("dt,D,blk", CACHE, ids=[f"{a}-D{b}-b{c}" for a, b, c in CACHE])
def test_cache_is_numpy_min_and_max_by_value(dt, D, blk):
    from rectified_spaattn_amd import pool_key_bounds
    B, Hkv, NK = 2, 2, 5
    Sk = NK * blk
    k = _randn((B, Hkv, Sk, D), dt, D + blk)
    # the tail block at 1 key, at blk / 4 + 3 keys, full
    for n, lens in enumerate(([3 * blk + 1, blk + blk // 4 + 3], [5 * blk, 1], [2 * blk, 4 * blk + blk // 4 + 3])):
        dirty = k.clone()
        for b, ln in enumerate(lens):
            dirty[b, :, ln:] = float("nan")
        want = _np_bounds(dirty, lens, blk, SENTINEL)
        got = []
        for wph, form in ((None, "list"), (1, "device"), (2, "list"), (NK, "device")):
            kv = lens if form == "list" else torch.tensor(lens, dtype=torch.int32, device=DEV)
            out = pool_key_bounds(dirty, block_size=blk, kv_len=kv, out=_full((B, Hkv, NK, 2, D), SENTINEL), workgroups_per_head=wph)
            assert out.dtype == torch.float32 and out.shape == (B, Hkv, NK, 2, D) and out.is_contiguous()
            assert torch.equal(out.cpu(), want), (n, wph, form)         # by value: -0 equals +0
            got.append(out)
        assert all(torch.equal(_bits(g), _bits(got[0])) for g in got)
        assert bool((want[:, :, :, 0] <= want[:, :, :, 1]).all()) and bool((want[:, :, 0, 0] < want[:, :, 0, 1]).any())
    fresh = pool_key_bounds(k, block_size=blk)
    assert fresh.shape == (B, Hkv, NK, 2, D) and torch.equal(fresh.cpu(), _np_bounds(k, [Sk, Sk], blk, 0.0))


# ---- 2. incremental updates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [64, 128])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_incremental_update_writes_its_blocks_and_nothing_else(paged, blk):
    """A cache full of NaN; a prefill, an append across a block edge, a rollback (start = kv_len).  Paged: a permuted table, spare
    pages full of NaN, and one entry of a written block outside [0, P): zeros, min and max alike."""
    from rectified_spaattn_amd import pool_key_bounds
    B, Hkv, D, NK, dt = 2, 2, 64, 5, "bf16"
    Sk = NK * blk
    full = _randn((B, Hkv, Sk, D), dt, blk + int(paged))
    steps = [([blk + blk // 2, 2 * blk + 5], [0, 0]),                           # prefill
             ([2 * blk + 3, 2 * blk + 9], [blk + blk // 2, 2 * blk + 5]),       # append: item 0 crosses a block edge
             ([blk + 7, 2 * blk + 2], [blk + 7, 2 * blk + 2])]                   # rollback: the ragged tail block alone
    cache = _full((B, Hkv, NK, 2, D), float("nan"))
    model = np.full((B, Hkv, NK, 2, D), np.nan)
    as_dev = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)       # noqa: E731
    for n, (lens, starts) in enumerate(steps):
        k = full.clone()
        for b, ln in enumerate(lens):
            k[b, :, ln:] = float("nan")
        k64 = k.double().cpu().numpy()
        if paged:
            src, _, table, P = _pool(k, k, blk, [Sk] * B, 17 + blk)
            table[0, 1] = P + 5
            k64[0, :, blk:2 * blk] = 0.0            # what the bad entry stands for
            kw = dict(block_table=table)
        else:
            src, kw = k, dict()
        model, wrote = ref.update(model, k64, lens, starts, blk)
        assert [list(np.flatnonzero(w)) for w in wrote] == [list(pooled_ref.written(s, ln, blk)) for s, ln in zip(starts, lens)]
        before = cache.clone()
        form = (lambda v: v) if n % 2 else as_dev
        got = pool_key_bounds(src, block_size=blk, kv_len=form(lens), start=form(starts) if n else None, out=cache, **kw)
        assert got is cache
        inside = torch.from_numpy(wrote)[:, None, :, None, None].expand(B, Hkv, NK, 2, D).to(DEV)
        assert torch.equal(_bits(cache[~inside]), _bits(before[~inside])), n          # every other element keeps its bytes
        want = torch.from_numpy(model.astype(np.float32))
        assert torch.equal(cache[inside].cpu(), want[inside.cpu()]) and bool(torch.isfinite(cache[inside]).all()), n
        fresh = pool_key_bounds(src, block_size=blk, kv_len=lens, **kw)                # a full call on the visible prefix
        for b, ln in enumerate(lens):
            hi = -(-ln // blk)
            assert torch.equal(_bits(cache[b, :, :hi]), _bits(fresh[b, :, :hi])), (n, b)
        assert int(wrote.sum()) in ([5], [3], [2])[n]
    if paged:
        assert not bool(cache[0, :, 1].any()) and bool(cache[1, :, 1].any())
    assert bool(torch.isnan(cache[:, :, 3:]).all())


# ---- 3. e4m3 -------------------------------------------------------------------------------------------------------------------------
E4M3_CASES = [(64, 64, False), (128, 128, True), (128, 64, True), (64, 128, False)]


@pytest.mark.parametrize("D,blk,paged", E4M3_CASES)
def test_e4m3_cache_is_the_two_byte_cache_of_the_dequantised_keys(D, blk, paged):
    """Codes written by append_kv_e4m3 under scales 2^e, a different e per head (the four cases go through -2 .. 2)."""
    from rectified_spaattn_amd import append_kv_e4m3, pool_key_bounds
    B, Hkv, NK = 2, 2, 5
    Sk = NK * blk
    lens = [4 * blk + 1, blk + blk // 4 + 3]
    n = E4M3_CASES.index((D, blk, paged))
    ks = torch.tensor([2.0 ** ((2 * n + h) % 5 - 2) for h in range(Hkv)], dtype=torch.float32, device=DEV)
    vs = torch.tensor([2.0 ** ((2 * n + h + 1) % 5 - 2) for h in range(Hkv)], dtype=torch.float32, device=DEV)
    kf = _randn((B, Hkv, Sk, D), "bf16", D) * 3
    if paged:
        P = B * NK + 3
        table = torch.randperm(P, generator=torch.Generator().manual_seed(blk))[:B * NK].reshape(B, NK).to(torch.int32).to(DEV)
        shape, kwt = (P, Hkv, blk, D), dict(block_table=table)
    else:
        shape, kwt = (B, Hkv, Sk, D), dict()
    k8, v8 = (torch.full(shape, kv8.NAN_CODE, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(2))
    append_kv_e4m3(kf, kf, k8, v8, start=0, n_new=lens, k_scale=ks, v_scale=vs, block_size=blk, **kwt)
    codes = k8.view(torch.uint8).cpu().numpy()
    assert (codes == kv8.NAN_CODE).any()
    kd = torch.from_numpy(kv8.dequant(codes, ks.cpu().numpy())).to(DEV, torch.bfloat16)      # (2^e scales: exact in bf16)
    got = pool_key_bounds(k8, block_size=blk, kv_len=lens, k_scale=ks, out=_full((B, Hkv, NK, 2, D), SENTINEL), **kwt)
    want = pool_key_bounds(kd, block_size=blk, kv_len=lens, out=_full((B, Hkv, NK, 2, D), SENTINEL), **kwt)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert bool((got[1, :, 2:] == SENTINEL).all()) and bool((got[0, :, :4, 0] < got[0, :, :4, 1]).all())
    assert float(ks[0]) != float(ks[1])


# ---- 4. the exact class ----------------------------------------------------------------------------------------------------------------
def _check_exact(q, k, q64, k64, lens, blk, heads, causal, combos, kv_len, **extra):
    """Scores bit for bit (first combo) and masks, ties included, against bound_ref; the reference's bounds, scores and sets are
    computed once."""
    from rectified_spaattn_amd import pool_key_bounds, select_blocks_bound
    B, _, Sq, _ = q.shape
    Sk = k.shape[2]
    NK = -(-Sk // blk)
    bnd64 = ref.bounds(k64, lens, blk)
    M = ref.magnitude(q64, bnd64, blk, heads)
    assert M.max() < 2.0 ** 10 * (128 / blk) ** 2, M.max()         # every partial sum is exact
    t64 = ref.scores(q64, bnd64, blk, heads)
    vis = select_ref.visible(Sq, Sk, lens, blk, causal)
    cache = pool_key_bounds(k, block_size=blk, kv_len=kv_len)
    for b, ln in enumerate(lens):
        cache[b, :, -(-ln // blk):] = float("nan")                  # beyond the visible prefix: never read
    for n, (kf, kl, tk) in enumerate(combos):
        frc = select_ref.forced(Sq, Sk, lens, blk, causal, kf, kl)
        want = select_ref.kept_vectorised(t64, vis, frc, _top_k(tk, NK))
        kw = dict(block_size=blk, kv_len=kv_len, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads, **extra)
        what = (tuple(q.shape), tuple(k.shape), lens, blk, heads, causal, kf, kl, tk)
        if n == 0:
            mask, t = select_blocks_bound(q, cache, _top_k(tk, NK), return_scores=True, **kw)
            tw = np.where(vis[:, None], t64, -np.inf)
            want32 = torch.from_numpy(tw.astype(np.float32))
            assert np.array_equal(want32.double().numpy(), tw), "the reference's scores are not fp32 values"
            assert t.dtype == torch.float32 and torch.equal(_bits(t.cpu()), _bits(want32)), what
        else:
            mask = select_blocks_bound(q, cache, _top_k(tk, NK), **kw)
        assert mask.dtype == torch.bool and mask.shape == want.shape and torch.equal(mask.cpu(), torch.from_numpy(want)), what
    return np.where(vis[:, None], t64, -np.inf)


EXACT = [(D, blk) for D in (16, 64, 128) for blk in (64, 128)]


@pytest.mark.parametrize("D,blk", EXACT, ids=[f"D{a}-b{b}" for a, b in EXACT])
def test_exact_class_small_rows(D, blk):
    """B = 2 with a key limit per item, H = 4 over Hkv = 4, 2, 1, both mask_heads, causal on and off, the kv_len forms and the
    dtypes taking turns; the 45 (keep_first, keep_local, top_k) triples go round over the 48 configurations, nine each."""
    B, H = 2, 4
    turn = itertools.cycle(range(len(KEEPS_TOPK)))
    kv_forms = itertools.cycle(("list", "tensor"))
    blind = ties = 0
    for s, (Sq, Sk, lens) in enumerate(_small_shapes(blk)):
        for Hkv in (4, 2, 1):
            dt = ("bf16", "fp16")[(s + Hkv + EXACT.index((D, blk))) % 2]
            qi, q64 = _ints((B, H, Sq, D), 100 * s + Hkv + D)
            ki, k64 = _ints((B, Hkv, Sk, D), 100 * s + Hkv + D + 50)
            q, k = (torch.from_numpy(a).to(DEV, DT[dt]) for a in (qi, ki))
            for heads in ("kv", "q"):
                for causal in (False, True):
                    combos = [KEEPS_TOPK[next(turn)] for _ in range(9)]
                    kv = lens if next(kv_forms) == "list" else torch.tensor(lens, dtype=torch.int32, device=DEV)
                    t = _check_exact(q, k, q64, k64, lens, blk, heads, causal, combos, kv)
                    blind += int(np.isinf(t).all(-1).sum())
                    fin = np.where(np.isfinite(t), t, np.nan)
                    ties += int((np.diff(np.sort(fin, axis=-1), axis=-1) == 0).sum())
                    assert np.isfinite(t).any()
    assert blind > 0 and ties > 0


MANY = [("bf16", 64, 64, 70), ("fp16", 16, 64, 300)]


@pytest.mark.parametrize("dt,D,blk,NK", MANY, ids=[f"{a}-D{b}-b{c}-NK{d}" for a, b, c, d in MANY])
def test_exact_class_more_blocks_than_a_ballot_step_and_than_threads(dt, D, blk, NK):
    B, H, Hkv = 2, 4, 2
    Sk = (NK - 1) * blk + blk // 2
    lens = [Sk, (NK - 6) * blk + blk // 4]
    for Sq, splits in ((Sk, None), (2 * blk, 1)):
        qi, q64 = _ints((B, H, Sq, D), NK + Sq)
        ki, k64 = _ints((B, Hkv, Sk, D), NK + Sq + 1)
        q, k = (torch.from_numpy(a).to(DEV, DT[dt]) for a in (qi, ki))
        for heads, causal in (("kv", True), ("q", False)) if Sq == Sk else (("kv", False), ("q", True)):
            combos = [(1, 1, 3), (0, 0, 1), (2, 2, "NK"), (0, 2, "NK+5"), (1, 0, 0), (0, 0, 65), (0, 1, NK - 7)]
            _check_exact(q, k, q64, k64, lens, blk, heads, causal, combos, lens, score_splits=splits)


# ---- 5. the rounding class -----------------------------------------------------------------------------------------------------------
ROUND = [("bf16", 16, 64), ("fp16", 128, 64), ("fp16", 16, 128), ("bf16", 128, 128)]


@pytest.mark.parametrize("dt,D,blk", ROUND, ids=[f"{a}-D{b}-b{c}" for a, b, c in ROUND])
def test_rounding_class_every_row(dt, D, blk):
    from rectified_spaattn_amd import pool_key_bounds, select_blocks_bound
    B, H = 2, 4
    rows = 0
    for (Sq, Sk, lens), Hkv in (((300, 1500, [1500, 1333]), 2), ((1210, 1210, [1210, 777]), 1), ((1100, 1000, [1000, 333]), 4)):
        q, k = _randn((B, H, Sq, D), dt, Sq + Sk + D + blk), _randn((B, Hkv, Sk, D), dt, Sq + Sk + D + blk + 1)
        q64, k64 = q.double().cpu().numpy(), k.double().cpu().numpy()
        NK = -(-Sk // blk)
        cache = pool_key_bounds(k, block_size=blk, kv_len=lens)
        bnd64 = ref.bounds(k64, lens, blk)
        for heads, causal, kf, kl, top_k in (("kv", True, 1, 1, 3), ("q", False, 0, 2, 4), ("kv", False, 0, 0, 2),
                                             ("q", True, 2, 0, 1), ("kv", True, 0, 1, NK // 2)):
            t64 = ref.scores(q64, bnd64, blk, heads)
            tol = 2.0 ** -14 * ref.magnitude(q64, bnd64, blk, heads)
            vis1, frc1 = select_ref.visible(Sq, Sk, lens, blk, causal), select_ref.forced(Sq, Sk, lens, blk, causal, kf, kl)
            mask, t = select_blocks_bound(q, cache, top_k, block_size=blk, kv_len=lens, causal=causal, keep_first=kf, keep_local=kl,
                                          mask_heads=heads, return_scores=True)
            kept, got = mask.cpu().numpy(), t.double().cpu().numpy()
            vis, frc = (np.broadcast_to(a[:, None], kept.shape) for a in (vis1, frc1))
            what = (Sq, Sk, heads, causal, kf, kl, top_k)
            # exactly: kept within visible, forced within kept, the count
            assert not (kept & ~vis).any() and not (frc & ~kept).any(), what
            nf, nv = frc.sum(-1), vis.sum(-1)
            assert np.array_equal(kept.sum(-1), np.minimum(np.maximum(top_k, nf), nv)), what
            # the scores
            assert np.array_equal(np.isneginf(got), ~vis), what
            err = np.abs(np.where(vis, got - np.where(vis, t64, 0.0), 0.0))
            print(f"{what}: score error / tol max {float((err[vis] / np.maximum(tol[vis], 1e-300)).max()):.3f}")
            assert (err <= tol)[vis].all(), what
            # the choice: theta = the reference's (top_k - |forced|)-th best unforced score
            cand = vis & ~frc
            need = np.maximum(top_k - nf, 0)
            srt = -np.sort(-np.where(cand, t64, -np.inf), axis=-1)
            theta = np.take_along_axis(srt, np.clip(need - 1, 0, NK - 1)[..., None], axis=-1)
            theta = np.where((need == 0)[..., None], np.inf, theta)
            t_ref = np.where(vis, t64, 0.0)
            assert (t_ref >= theta - tol)[kept & cand].all(), what
            assert (t_ref <= theta + tol)[vis & ~kept].all(), what
            rows += kept[..., 0].size
    assert rows > 0


# ---- 6. one body -----------------------------------------------------------------------------------------------------------------------
def _select_all(q, cache, top_k, **kw):
    from rectified_spaattn_amd import select_blocks_bound
    return select_blocks_bound(q, cache, top_k, as_lists=True, return_scores=True, **kw)


@pytest.mark.parametrize("dt,D,blk,NK,Sq", [("bf16", 128, 128, 70, 1), ("fp16", 64, 64, 300, 150), ("bf16", 16, 64, 3, 3)])
def test_every_score_splits_gives_the_same_bytes(dt, D, blk, NK, Sq):
    from rectified_spaattn_amd import pool_key_bounds, select_blocks_bound
    B, H, Hkv = 2, 4, 2
    Sk = (NK - 1) * blk + blk // 2 + 3
    lens = [Sk, max(Sk - 2 * blk - 17, 5)]
    q, k = _randn((B, H, Sq, D), dt, NK), _randn((B, Hkv, Sk, D), dt, NK + 1)
    cache = pool_key_bounds(k, block_size=blk, kv_len=lens)
    for kw in (dict(causal=True, keep_first=1, keep_local=1), dict(mask_heads="q", top_p=0.8, return_mass=True)):
        kw.update(block_size=blk, kv_len=lens)
        want = _select_all(q, cache, 5, score_splits=1, **kw)
        for s in (4, None, 1):
            got = _select_all(q, cache, 5, score_splits=s, **kw)
            _same_lists(got[0], want[0], (s, kw))
            for a, b in zip(got[1:], want[1:]):
                _same_scores(a, b, (s, kw))
        masks = [select_blocks_bound(q, cache, 5, score_splits=s, **kw) for s in (1, 4, None)]
        masks = [m[0] if isinstance(m, tuple) else m for m in masks]
        assert all(m.dtype == torch.bool and torch.equal(m, masks[0]) for m in masks)
        assert int(masks[0].sum()) == int(want[0]["counts"].sum()) > 0


@pytest.mark.parametrize("blk,NK,Hkv,heads,causal,Sq", [(64, 70, 2, "q", True, 64), (128, 300, 1, "kv", False, 1), (64, 3, 4, "kv", True, 1)])
def test_top_p_one_at_unit_scale_is_top_k(blk, NK, Hkv, heads, causal, Sq):
    """select_p_ref.plateau_inputs: at c = 1 every visible block weighs at least 2^6, so top_p = 1 keeps what the cap allows."""
    from rectified_spaattn_amd import pool_key_bounds
    B, H, D = 2, 4, 16
    Sk = (NK - 1) * blk + blk // 2 + 3
    lens = [Sk, max(Sk - 2 * blk - 17, 5)]
    q64, k64 = pref.plateau_inputs(B, H, Hkv, Sq, Sk, D, blk, heads, 300 + NK)
    q, k = (torch.from_numpy(a).to(DEV, torch.bfloat16) for a in (q64, k64))
    cache = pool_key_bounds(k, block_size=blk, kv_len=lens)
    for tk, kf, kl in pref.PLATEAU_BUDGETS:
        kw = dict(block_size=blk, kv_len=lens, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads)
        want = _select_all(q, cache, pref.exact_top_k(tk, NK), **kw)
        got = _select_all(q, cache, pref.exact_top_k(tk, NK), top_p=1.0, score_scale=pref.SCALE_EXACT, **kw)
        _same_lists(got[0], want[0], (tk, kf, kl))
        _same_scores(got[1], want[1], (tk, kf, kl))
    assert int(want[0]["counts"].max()) >= 1


@pytest.mark.parametrize("case", [pref.exact_cases()[m] for m in (1, 2, 6, 10)], ids=lambda c: f"NK{c['NK']}-b{c['blk']}-D{c['D']}")
def test_top_p_with_mass_against_the_reference_on_the_exact_class(case):
    """select_p_ref.exact_inputs with the keys spread inside each block: one key of block j holds level_j in channel 0 and the
    others less (q is positive there and 0 elsewhere, where the keys are random), so t = (1 + i % 2) level_j is the bound and not
    the mean; at c = 1 every weight is a power of two."""
    from rectified_spaattn_amd import pool_key_bounds, select_blocks_bound
    c = case
    B, H, Hkv, Sq, Sk, D, blk, NK = c["B"], c["H"], c["Hkv"], c["Sq"], c["Sk"], c["D"], c["blk"], c["NK"]
    q64, k64 = pref.exact_inputs(B, H, Hkv, Sq, Sk, D, blk, c["heads"], c["seed"])
    rng = np.random.default_rng(c["seed"])
    k64[..., 1:] = rng.integers(-2, 3, k64[..., 1:].shape)
    drop = rng.integers(1, 4, k64.shape[:3]).astype(np.float64)
    for b in range(B):
        for j in range(NK):
            drop[b, :, min(j * blk + (j * 5) % blk, min((j + 1) * blk, c["lens"][b], Sk) - 1)] = 0      # the block's maximum stays
    k64[..., 0] -= drop
    q, k = (torch.from_numpy(a).to(DEV, DT[c["dt"]]) for a in (q64, k64))
    assert np.array_equal(k.double().cpu().numpy(), k64)
    cache = pool_key_bounds(k, block_size=blk, kv_len=c["lens"])
    for top_p, tk, kf, kl in ((0.9, "NK", 0, 0), (0.9, 8, 1, 1), (0.5, "NK", 0, 0)):
        top_k = pref.exact_top_k(tk, NK)
        r = ref.select(q64, k64, top_k, blk=blk, lens=c["lens"], causal=c["causal"], keep_first=kf, keep_local=kl,
                       mask_heads=c["heads"], top_p=top_p, score_scale=pref.SCALE_EXACT)
        kw = dict(block_size=blk, kv_len=c["lens"], causal=c["causal"], keep_first=kf, keep_local=kl, mask_heads=c["heads"],
                  top_p=top_p, score_scale=pref.SCALE_EXACT, return_mass=True)
        mask, t, mass = select_blocks_bound(q, cache, top_k, return_scores=True, **kw)
        want_t = torch.from_numpy(r["t"].astype(np.float32))
        assert torch.equal(_bits(t.cpu()), _bits(want_t)), (top_p, tk)
        assert torch.equal(mask.cpu(), torch.from_numpy(r["mask"])), (top_p, tk)
        assert torch.equal(_bits(mass.cpu()), _bits(torch.from_numpy(r["mass"]))), (top_p, tk)
        assert 0 < int(mask.sum()) < mask.numel() and bool((mass > 0).any())


# ---- 7. constant blocks: the bytes of select_blocks_pooled ------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,blk,Hkv,heads", [("bf16", 128, 128, 2, "kv"), ("fp16", 16, 64, 1, "q"), ("bf16", 64, 64, 4, "kv")])
def test_constant_blocks_give_the_bytes_of_select_blocks_pooled(dt, D, blk, Hkv, heads):
    from rectified_spaattn_amd import pool_key_bounds, pool_keys, select_blocks_pooled
    B, H, NK = 2, 4, 9
    Sk = NK * blk - blk // 2
    lens = [Sk, 3 * blk + blk // 4]
    rng = np.random.default_rng(D + blk)
    k = torch.from_numpy(np.repeat(rng.integers(-2, 3, (B, Hkv, NK, D)), blk, axis=2)[:, :, :Sk]).to(DEV, DT[dt])
    for Sq in (1, 2 * blk):
        q = torch.from_numpy(rng.integers(-2, 3, (B, H, Sq, D))).to(DEV, DT[dt])
        bounds, means = pool_key_bounds(k, block_size=blk, kv_len=lens), pool_keys(k, block_size=blk, kv_len=lens)
        for b, ln in enumerate(lens):
            hi = -(-ln // blk)
            assert torch.equal(bounds[b, :, :hi, 0], means[b, :, :hi]) and torch.equal(bounds[b, :, :hi, 1], means[b, :, :hi])
        for kw in (dict(causal=True, keep_first=1, keep_local=1), dict(top_p=0.7, return_mass=True), dict(score_splits=1)):
            kw.update(block_size=blk, kv_len=lens, mask_heads=heads, as_lists=True, return_scores=True)
            got = _select_all(q, bounds, 3, **{n: v for n, v in kw.items() if n not in ("as_lists", "return_scores")})
            want = select_blocks_pooled(q, means, 3, **kw)
            _same_lists(got[0], want[0], (Sq, kw))
            for a, b in zip(got[1:], want[1:]):
                _same_scores(a, b, (Sq, kw))
            assert int(got[0]["counts"].sum()) > 0 and bool(torch.isfinite(got[1]).any())


# ---- 8. the needle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D,blk", [("bf16", 128, 128), ("fp16", 64, 64), ("bf16", 16, 128)])
def test_the_needle_is_dropped_by_the_mean_and_kept_by_the_bound(dt, D, blk):
    from rectified_spaattn_amd import pool_key_bounds, pool_keys, select_blocks_bound, select_blocks_pooled
    B, H, Hkv, NK = 2, 4, 2, 6
    needle = [3, 5]
    q64, k64 = ref.needle_inputs(B, H, Hkv, D, blk, NK, needle, D + blk)
    q, k = (torch.from_numpy(a).to(DEV, DT[dt]) for a in (q64, k64))
    by_mean = select_blocks_pooled(q, pool_keys(k, block_size=blk), 1, block_size=blk)
    by_bound, t = select_blocks_bound(q, pool_key_bounds(k, block_size=blk), 1, block_size=blk, return_scores=True)
    assert by_mean.shape == by_bound.shape == (B, Hkv, 1, NK)
    assert bool((by_mean.sum(-1) == 1).all()) and bool((by_bound.sum(-1) == 1).all())
    for b in range(B):
        assert not bool(by_mean[b, :, 0, needle[b]].any()) and bool(by_mean[b, :, 0, 0].all())
        assert bool(by_bound[b, :, 0, needle[b]].all())
        assert bool((t[b, :, 0, needle[b]] == 4 * D * (H // Hkv)).all())
    r = ref.select(q64, k64, 1, blk=blk)
    assert torch.equal(by_bound.cpu(), torch.from_numpy(r["mask"])) and torch.equal(t.double().cpu(), torch.from_numpy(r["t"]))


# ---- 9. ragged and packed ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_p", [None, 0.7], ids=["top-k", "top-p"])
def test_ragged_and_packed_rows_equal_the_per_item_calls(top_p):
    """q_len with a zero-row item and a one-row item; the same items packed behind cu_seqlens_q / max_q_len."""
    from rectified_spaattn_amd import pool_key_bounds, select_blocks_bound
    B, H, Hkv, D, blk, NK, M = 4, 8, 2, 128, 128, 6, 150
    ns = [150, 0, 1, 40]
    lens = [700, 40, 333, 129]
    qpad = _randn((B, H, M, D), "bf16", 3)
    for b, n in enumerate(ns):
        qpad[b, :, n:] = float("nan")
    k = _randn((B, Hkv, NK * blk, D), "bf16", 4)
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
    cache = pool_key_bounds(k, kv_len=lens, out=_full((B, Hkv, NK, 2, D), float("nan")))
    kw = dict(causal=True, keep_first=1, keep_local=1, as_lists=True, return_scores=True)
    if top_p is not None:
        kw.update(top_p=top_p, return_mass=True)
    NQ = -(-M // blk)
    ragged = select_blocks_bound(qpad, cache, 3, kv_len=lens, q_len=torch.tensor(ns, dtype=torch.int32, device=DEV), **kw)
    cu = [0] + list(np.cumsum(ns))
    q = torch.cat([qpad[b, :, :n].transpose(0, 1) for b, n in enumerate(ns)]).contiguous()
    assert q.shape == (sum(ns), H, D)
    packed = select_blocks_bound(q, cache, 3, kv_len=lens, cu_seqlens_q=torch.tensor(cu, dtype=torch.int32, device=DEV),
                                 max_q_len=M, **kw)
    _same_lists(packed[0], ragged[0], "packed")
    for a, b in zip(packed[1:], ragged[1:]):
        _same_scores(a, b, "packed")
    counts = ragged[0]["counts"].view(B, Hkv, NQ)
    cols = ragged[0]["cols"].view(B, Hkv, NQ, NK)
    bitmask = ragged[0]["bitmask"].view(B, Hkv, NQ, -1)
    for b, n in enumerate(ns):
        nq = -(-n // blk)
        assert not bool(counts[b, :, nq:].any()) and not bool(bitmask[b, :, nq:].any())
        assert bool(torch.isneginf(ragged[1][b, :, nq:]).all())
        if top_p is not None:
            assert not bool(ragged[2][b, :, nq:].any())
        if n == 0:
            continue
        one = select_blocks_bound(qpad[b:b + 1, :, :n], cache[b:b + 1], 3, kv_len=[lens[b]], **kw)
        assert torch.equal(one[0]["counts"].view(Hkv, nq), counts[b, :, :nq]), b
        assert torch.equal(one[0]["bitmask"].view(Hkv, nq, -1), bitmask[b, :, :nq]), b
        live = torch.arange(NK, device=DEV)[None, None, :] < counts[b, :, :nq, None]
        assert torch.equal(torch.where(live, one[0]["cols"].view(Hkv, nq, NK), 0), torch.where(live, cols[b, :, :nq], 0)), b
        for a, r in zip(one[1:], ragged[1:]):
            assert torch.equal(_bits(a[0]), _bits(r[b, :, :nq])), b
    assert int(counts.sum()) > 0


# ---- 10. one graph for the decode step -------------------------------------------------------------------------------------------------
def test_one_graph_for_the_three_calls_of_a_decode_step():
    """pool_key_bounds(start = prev), select_blocks_bound(as_lists) and block_sparse_decode(block_table, return_lse) captured
    together on one stream; then, in place, one more key per item (item 0's opens a new block) and kv_len and prev bumped on the
    device.  The replay equals the eager three calls."""
    from rectified_spaattn_amd import block_sparse_decode, pool_key_bounds, select_blocks_bound
    B, H, Hkv, Sq, D, blk, SK = 2, 8, 2, 1, 128, 128, 700
    NK = -(-SK // blk)
    lens = [512, 333]           # item 0's next key opens a new block (the fifth)
    q = _randn((B, H, Sq, D), "bf16", 5)
    k, v = _randn((B, Hkv, SK, D), "bf16", 6), _randn((B, Hkv, SK, D), "bf16", 7)
    new_k, new_v = k[:, :, 600].clone(), v[:, :, 600].clone()
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    kp, vp, table, P = _pool(k, v, blk, [SK, SK], 11)       # (every block has a page: the new keys have somewhere to go)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    prev = kv_len.clone()
    cache = pool_key_bounds(kp, kv_len=kv_len, block_table=table, out=_full((B, Hkv, NK, 2, D), float("nan")))
    sel_kw = dict(kv_len=kv_len, causal=True, keep_first=1, keep_local=1, as_lists=True)
    dec_kw = dict(kv_len=kv_len, causal=True, block_table=table, return_lse=True)

    def step(cache):
        pool_key_bounds(kp, kv_len=kv_len, start=prev, block_table=table, out=cache)
        lists = select_blocks_bound(q, cache, 3, **sel_kw)
        return (lists,) + block_sparse_decode(q, kp, vp, lists, **dec_kw)

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
    before = got[1].clone()
    # the step: one more key per batch item, in place
    prev.copy_(kv_len)
    for b in range(B):
        j, r = lens[b] // blk, lens[b] % blk
        kp[table[b, j].item(), :, r] = new_k[b]
        vp[table[b, j].item(), :, r] = new_v[b]
    kv_len += 1
    stale = cache.clone()
    graph.replay()
    torch.cuda.synchronize()
    same(got, step(stale))
    fresh = pool_key_bounds(kp, kv_len=kv_len, block_table=table)
    assert torch.equal(_bits(cache[0, :, :5]), _bits(fresh[0, :, :5])) and torch.equal(_bits(cache[1, :, :3]), _bits(fresh[1, :, :3]))
    assert bool(torch.isnan(cache[1, :, 3:]).all())
    assert not torch.equal(got[1], before) and bool(torch.isfinite(got[1].float()).all())
    assert int(got[0]["counts"].min()) == 3
