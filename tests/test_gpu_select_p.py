"""The top-p selection on the MI355X (rsa_block_select_p, rsa_block_select_pooled_p) against the reference of
tests/select_p_ref.py.

    exact class      q and k of select_p_ref.exact_inputs: every pooled sum is exact, t takes small integers, and with
                     score_scale = ln 2 (c == 1.0f) every weight is a power of two or 0.  Mask, cols, counts, scores and mass
                     equal the reference bit for bit.  tests/test_select_p_cpu.py counts, on the reference, the cases these
                     inputs hold (exact landings, plateaus across the cut, forced blocks that pass the target, a cap that binds
                     and one that does not, zero tails at top_p = 1, top_p = 0) and shows that six mutants each change one.
    rounding class   random normal inputs over ragged counts: set relations exactly, the ranking within section 5.11's score
                     tolerance, the kept fraction within an epsilon derived below (_epsilon) from the fixed point and that
                     tolerance.
    byte for byte    the pooled call against the plain one, lists against mask, call against call, a device kv_len, one graph;
                     top_p = 1 over rows without a zero weight against top-k, whose contract it then is.
    end to end       the top-p lists drive block_sparse_decode (paged, log-sum-exp), the mask block_sparse_attention(causal).
"""
import numpy as np
import pytest
import torch

import decode_ref
import select_p_ref as pref
import select_ref as ref
import test_ranged_cpu as rule
from test_gpu_decode import LSE_TOL, _pool
from test_gpu_gqa import TOL, _attend, _expand_heads
from test_gpu_pooled_keys import _bits, _randn, _same_lists, _same_scores

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CASES = pref.exact_cases()


def _id(c):
    return (f"NK{c['NK']}-Sq{c['Sq']}-{c['dt']}-D{c['D']}-b{c['blk']}-kv{c['Hkv']}-{c['heads']}-"
            f"{'causal' if c['causal'] else 'full'}")


# ---- 1. the exact class ----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_every_axis():
    for key, n in (("NK", 3), ("Sq", 4), ("dt", 2), ("D", 3), ("blk", 2), ("Hkv", 3), ("heads", 2), ("causal", 2)):
        assert len({c[key] for c in CASES}) == n, key
    assert len({(c["Hkv"], c["heads"], c["causal"]) for c in CASES}) == 12
    assert {c["Sq"] for c in CASES} >= {1, 3}


def _check_exact(q64, k64, c, params, kv_len, call=None):
    """Every parameter set on one input: lists, scores (first set) and mass against the reference, bit for bit."""
    from rectified_spaattn_amd import select_blocks
    from rectified_spaattn_amd.block_sparse import lists_to_block_mask
    B, Hkv, H, blk, NK = c["B"], c["Hkv"], c["H"], c["blk"], c["NK"]
    Hl = Hkv if c["heads"] == "kv" else H
    q, k = (torch.from_numpy(a).to(DEV, DT[c["dt"]]) for a in (q64, k64))
    assert np.array_equal(q.double().cpu().numpy(), q64) and np.array_equal(k.double().cpu().numpy(), k64)
    t64 = ref.scores(q64, k64, c["lens"], blk, c["heads"])
    call = call or (lambda *a, **kw: select_blocks(q, k, *a, **kw))
    kept_rows = 0
    for n, (top_p, tk, kf, kl) in enumerate(params):
        top_k = pref.exact_top_k(tk, NK)
        kw = dict(block_size=blk, kv_len=kv_len, causal=c["causal"], keep_first=kf, keep_local=kl, mask_heads=c["heads"])
        r = pref.select(q64, k64, top_k, top_p, score_scale=pref.SCALE_EXACT, blk=blk, lens=c["lens"], t=t64, **{
            k_: v for k_, v in kw.items() if k_ not in ("block_size", "kv_len")})
        what = (_id(c), top_p, tk, kf, kl)
        lists, t, mass = call(top_k, top_p=top_p, score_scale=pref.SCALE_EXACT, as_lists=True, return_scores=True,
                              return_mass=True, **kw)
        NQ = r["mask"].shape[2]
        if n == 0:
            want = torch.from_numpy(r["t"].astype(np.float32))
            assert np.array_equal(want.double().numpy(), r["t"]), "the reference's scores are not fp32 values"
            assert t.shape == want.shape and torch.equal(_bits(t.cpu()), _bits(want)), what
        mask = lists_to_block_mask(lists["bitmask"], B, Hl, NQ, NK).view(torch.bool).cpu().numpy()
        assert np.array_equal(mask, r["mask"]), (what, np.argwhere(mask != r["mask"])[:4].tolist())
        cnt = r["mask"].sum(-1)
        assert np.array_equal(lists["counts"].cpu().numpy().reshape(cnt.shape), cnt), what
        cols = lists["cols"].cpu().numpy().reshape(B, Hl, NQ, NK)
        live = np.arange(NK) < cnt[..., None]
        want_cols = np.zeros_like(cols)
        want_cols[live] = np.nonzero(r["mask"])[3]      # (np.nonzero is row-major: ascending columns row after row)
        assert np.array_equal(np.where(live, cols, 0), want_cols), what
        assert mass.dtype == torch.float32 and mass.shape == (B, Hl, NQ)
        assert np.array_equal(mass.cpu().numpy().view(np.uint32), r["mass"].view(np.uint32)), what
        kept_rows += int((cnt > 0).sum())
    return kept_rows


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_exact_class(c):
    q64, k64 = pref.exact_inputs(c["B"], c["H"], c["Hkv"], c["Sq"], c["Sk"], c["D"], c["blk"], c["heads"], c["seed"])
    kv = c["lens"] if c["seed"] % 2 else torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    assert _check_exact(q64, k64, c, pref.EXACT_PARAMS, kv) > 0


@pytest.mark.parametrize("shift,Sq,causal", [(2, 1, True), (1, 130, False)], ids=["zero-tail", "plateau"])
def test_exact_class_at_the_key_block_limit(shift, Sq, causal):
    """NK = 8192 blocks of 64, B = H = 1, D = 16: thousands of unit weights behind the head of the zero-tail profile, and the
    plateau profile's tail of 2^-8 .. 2^-12; 32 KB of keys in LDS."""
    blk, NK, D = 64, 8192, 16
    Sk = (NK - 1) * blk + blk // 2
    c = dict(B=1, H=1, Hkv=1, Sq=Sq, Sk=Sk, D=D, blk=blk, NK=NK, lens=[Sk], heads="kv", causal=causal, dt="bf16", seed=5)
    q64, k64 = pref.exact_inputs(1, 1, 1, Sq, Sk, D, blk, "kv", 5, shift=shift)
    params = [(1.0, "NK+5", 0, 1), (0.9, 90, 1, 2), (0.999, 5000, 0, 0)]
    assert _check_exact(q64, k64, c, params, None) > 0


# ---- 2. the rounding class -------------------------------------------------------------------------------------------------------
def _epsilon(c64, delta, n_vis):
    """The slack of the two mass statements, from the fixed point and the score tolerance alone.

    The device's score t^ is within delta = max_j 2^-14 M_j of t (section 5.11), so (t^_j - t^_max) is within 2 delta of
    (t_j - t_max).  The fp32 subtraction, the product with c = float32(c64) and c's own rounding are a relative error theta,
    |theta| <= 2^-22, of a_j; 2^18 (w^(1 + theta) - w) <= 2^18 2^-22 ln 2 max(|a| 2^-|a|) < 2^-5 for w = 2^a <= 1.  v_exp_f32 is
    within one ulp and the fp32 product and sum with 0.5 round once each: a factor (1 + 2^-21) covers them.  The floor moves the
    value by at most 0.5.  With U_j = 2^18 w_j the ideal weight and rho = 2^(2 c delta) (1 + 2^-21) - 1 (rho < 1/2 asserted):
        |u_j - U_j| <= 0.5 + 2^-4 + rho U_j
    The kernel keeps sum_kept u >= (total_u P16) / 2^16, and the kept prefix without its last block sums to < that + 1, with
    |P16 / 2^16 - top_p| <= 2^-17 and S = sum_visible U >= 2^18 (the best block has w = 1).  Dividing through,
        K / S >= top_p - eps   and   K' / S < top_p + eps,   eps = (2 rho + (1.125 n_vis + 1) / 2^18) / (1 - rho) + 2^-17."""
    rho = 2.0 ** (2.0 * c64 * delta) * (1.0 + 2.0 ** -21) - 1.0
    assert (rho < 0.5).all()
    return (2.0 * rho + (1.125 * n_vis + 1.0) / 2.0 ** 18) / (1.0 - rho) + 2.0 ** -17


ROUND = [("bf16", 128, 128), ("fp16", 16, 64), ("bf16", 64, 64), ("fp16", 128, 128)]


@pytest.mark.parametrize("dt,D,blk", ROUND, ids=[f"{a}-D{b}-b{c}" for a, b, c in ROUND])
def test_rounding_class_every_row(dt, D, blk):
    from rectified_spaattn_amd import select_blocks
    B, H = 2, 4
    rows = bound = free = 0
    worst = -1.0
    for (Sq, Sk, lens), Hkv in (((300, 1500, [1500, 1333]), 2), ((1210, 1210, [1210, 777]), 1)):
        g = torch.Generator().manual_seed(Sq + Sk + D + blk)
        q = torch.randn(B, H, Sq, D, generator=g).to(DEV, DT[dt])
        k = torch.randn(B, Hkv, Sk, D, generator=g).to(DEV, DT[dt])
        q64, k64 = q.double().cpu().numpy(), k.double().cpu().numpy()
        NK = -(-Sk // blk)
        for heads, causal, kf, kl, top_k in (("kv", True, 1, 1, NK), ("q", False, 0, 2, 6), ("kv", False, 0, 0, NK // 2)):
            Hl = Hkv if heads == "kv" else H
            t64 = ref.scores(q64, k64, lens, blk, heads)
            tol = 2.0 ** -14 * ref.magnitude(q64, k64, lens, blk, heads)
            vis3, frc3 = ref.visible(Sq, Sk, lens, blk, causal), ref.forced(Sq, Sk, lens, blk, causal, kf, kl)
            vis, frc = (np.broadcast_to(a[:, None], t64.shape) for a in (vis3, frc3))
            nv, nf = vis.sum(-1), frc.sum(-1)
            delta = np.where(vis, tol, 0.0).max(-1)
            tmax = np.where(vis, t64, -np.inf).max(-1, keepdims=True)
            for mult in (1.0, 4.0):
                scale = mult * pref.default_scale(H, Hl, D)
                c64 = scale * pref.LOG2_E
                with np.errstate(invalid="ignore"):
                    U = np.where(vis, np.exp2((t64 - tmax) * c64), 0.0)
                S = U.sum(-1)
                eps = _epsilon(c64, delta, nv)
                for top_p in (0.5, 0.9, 0.99):
                    mask, t, mass = select_blocks(q, k, top_k, block_size=blk, kv_len=lens, causal=causal, keep_first=kf,
                                                  keep_local=kl, mask_heads=heads, return_scores=True, top_p=top_p,
                                                  score_scale=None if mult == 1.0 else scale, return_mass=True)
                    kept, got = mask.cpu().numpy(), t.double().cpu().numpy()
                    what = (Sq, Sk, heads, causal, kf, kl, top_k, mult, top_p)
                    # exactly: forced within kept within visible; ascending columns are the mask's own (lists = mask, below)
                    assert not (kept & ~vis).any() and not (frc & ~kept).any(), what
                    ku = kept & ~frc
                    n_k = np.maximum(min(top_k, NK) - nf, 0)
                    assert (ku.sum(-1) <= n_k).all(), what
                    assert np.array_equal(np.isneginf(got), ~vis), what
                    assert (np.abs(np.where(vis, got - np.where(vis, t64, 0.0), 0.0)) <= tol)[vis].all(), what
                    # the ranking: no kept unforced block below a dropped one by more than the score tolerance
                    lo_kept = np.where(ku, t64 + tol, np.inf).min(-1)
                    hi_drop = np.where(vis & ~kept, t64 - tol, -np.inf).max(-1)
                    assert (lo_kept >= hi_drop).all(), what
                    # the mass, in fp64 weights of the fp64 scores
                    live = nv > 0
                    with np.errstate(invalid="ignore", divide="ignore"):
                        frac = np.where(kept, U, 0.0).sum(-1) / S
                        capped = ku.sum(-1) == n_k
                        low = (frac >= top_p - eps) | capped | ~live
                        assert low.all(), (what, float((top_p - frac)[~low].max()), float(eps[~low].min()))
                        # without the lowest-ranked kept unforced block (by the device's own scores, the higher j among equals)
                        worst_t = np.where(ku, got, np.inf).min(-1, keepdims=True)
                        last = NK - 1 - np.argmax((ku & (got == worst_t))[..., ::-1], axis=-1)
                        less = frac - np.take_along_axis(U, last[..., None], axis=-1)[..., 0] / S
                        has = ku.any(-1) & live
                        assert (less < top_p + eps)[has].all(), (what, float((less - top_p)[has].max()))
                        worst = max(worst, float(np.where(has, (less - top_p) / eps, -1).max()),
                                    float(np.where(live & ~capped, (top_p - frac) / eps, -1).max()))
                        # the returned mass is the integer ratio: within the same epsilon of the ideal fraction
                        assert (np.abs(mass.double().cpu().numpy() - frac) <= eps)[live].all(), what
                    assert (mass.cpu().numpy()[~live] == 0).all()
                    rows += int(live.sum())
                    bound += int((capped & live).sum())
                    free += int((~capped & live).sum())
    print(f"{dt} D{D} b{blk}: rows {rows}, cap bound {bound}, free {free}, worst (mass - top_p) / eps {worst:.3f}")
    assert bound > 0 and free > 0


# ---- 3. byte for byte ------------------------------------------------------------------------------------------------------------
POOLED = [("bf16", 128, 128, 70, 1, 2, "kv", True), ("fp16", 16, 64, 300, 3, 1, "q", False), ("bf16", 64, 64, 3, 160, 4, "kv", True),
          ("fp16", 64, 128, 300, 1, 2, "q", True)]


@pytest.mark.parametrize("dt,D,blk,NK,Sq,Hkv,heads,causal", POOLED, ids=[f"{a}-D{b}-b{c}-NK{d}-Sq{e}" for a, b, c, d, e, *_ in POOLED])
def test_selection_from_the_cache_equals_select_blocks(dt, D, blk, NK, Sq, Hkv, heads, causal):
    from rectified_spaattn_amd import pool_keys, select_blocks, select_blocks_pooled
    B, H = 2, 4
    Sk = (NK - 1) * blk + blk // 2 + 3
    lens = [Sk, max(Sk - 2 * blk - 17, 5)]
    q, k = _randn((B, H, Sq, D), dt, NK + Sq), _randn((B, Hkv, Sk, D), dt, NK + Sq + 1)
    cache = pool_keys(k, block_size=blk, kv_len=lens)
    kept = 0
    for top_p, top_k, kf, kl, scale in ((0.9, NK, 1, 1, None), (0.5, 5, 0, 2, 0.5), (1.0, NK + 5, 0, 0, None), (0.0, 3, 2, 1, None)):
        kw = dict(block_size=blk, kv_len=lens, causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads, top_p=top_p,
                  score_scale=scale, return_scores=True, return_mass=True)
        want = select_blocks(q, k, top_k, as_lists=True, **kw)
        what = (dt, D, blk, NK, Sq, top_p, top_k)
        for s in (None, 1, 7, 64):
            got = select_blocks_pooled(q, cache, top_k, as_lists=True, score_splits=s, **kw)
            _same_lists(got[0], want[0], what + (s,))
            _same_scores(got[1], want[1], what + (s,))
            assert torch.equal(_bits(got[2]), _bits(want[2])), what + (s,)
        m1, m2 = select_blocks_pooled(q, cache, top_k, **kw)[0], select_blocks(q, k, top_k, **kw)[0]
        assert m1.dtype == torch.bool and torch.equal(m1, m2)
        kept += int(want[0]["counts"].sum())
    assert kept > 0


# (blk, NK, (Hkv, mask_heads), causal, Sq in blocks, dtype) out of select_p_ref.plateau_cases: every value of every axis
COINCIDE = [(64, 3, (4, "kv"), False, 0, "bf16"), (128, 70, (2, "q"), True, 1, "fp16"), (64, 300, (1, "kv"), True, 0, "fp16"),
            (128, 3, (2, "q"), False, 1, "bf16"), (64, 70, (1, "kv"), False, 1, "bf16"), (128, 300, (4, "kv"), True, 0, "fp16")]


@pytest.mark.parametrize("blk,NK,form,causal,sq_blocks,dt", COINCIDE,
                         ids=[f"b{a}-NK{b}-kv{c[0]}-{c[1]}-{'causal' if d else 'full'}-Sq{e}-{f}" for a, b, c, d, e, f in COINCIDE])
def test_top_p_one_over_nonzero_weights_equals_top_k_byte_for_byte(blk, NK, form, causal, sq_blocks, dt):
    """Both select kernels on inputs where their contracts coincide (tests/test_select_p_cpu.py: top_p = 1, every visible weight
    >= 1): mask, bitmask, counts, live cols and scores are the same bytes, from q and k and from the cache, scored in the select
    workgroup (score_splits = 1) and loaded from the score pass (4)."""
    from rectified_spaattn_amd import pool_keys, select_blocks, select_blocks_pooled
    (Hkv, heads), Sq = form, sq_blocks * blk or 1
    c = next(c for c in pref.plateau_cases() if (c["blk"], c["NK"], c["Hkv"], c["heads"], c["causal"], c["Sq"]) ==
             (blk, NK, Hkv, heads, causal, Sq))
    q64, k64 = pref.plateau_inputs(c["B"], c["H"], Hkv, Sq, c["Sk"], c["D"], blk, heads, c["seed"])
    q, k = (torch.from_numpy(a).to(DEV, DT[dt]) for a in (q64, k64))
    assert np.array_equal(q.double().cpu().numpy(), q64) and np.array_equal(k.double().cpu().numpy(), k64)
    cache = pool_keys(k, block_size=blk, kv_len=c["lens"])
    calls = [lambda *a, **kw: select_blocks(q, k, *a, **kw)] + [
        lambda *a, s=s, **kw: select_blocks_pooled(q, cache, *a, score_splits=s, **kw) for s in (1, 4)]
    kept = dropped = 0
    for tk, kf, kl in pref.PLATEAU_BUDGETS:
        top_k = pref.exact_top_k(tk, NK)
        kw = dict(block_size=blk, kv_len=c["lens"], causal=causal, keep_first=kf, keep_local=kl, mask_heads=heads, return_scores=True)
        for n, call in enumerate(calls):
            what = (tk, kf, kl, n)
            by_k, by_p = call(top_k, as_lists=True, **kw), call(top_k, as_lists=True, top_p=1.0, score_scale=pref.SCALE_EXACT, **kw)
            _same_lists(by_p[0], by_k[0], what)
            _same_scores(by_p[1], by_k[1], what)
            m_k, m_p = call(top_k, **kw), call(top_k, top_p=1.0, score_scale=pref.SCALE_EXACT, **kw)
            assert m_k[0].dtype == torch.bool and torch.equal(_bits(m_p[0]), _bits(m_k[0])), what
            _same_scores(m_p[1], m_k[1], what)
            assert int(m_k[0].sum()) == int(by_k[0]["counts"].sum()), what
            kept += int(m_k[0].sum())
            dropped += int((~m_k[0] & torch.isfinite(m_k[1])).sum())
    assert kept > 0 and dropped > 0


def test_selection_from_the_cache_at_the_key_block_limit():
    from rectified_spaattn_amd import pool_keys, select_blocks, select_blocks_pooled
    blk, NK, D = 64, 8192, 16
    Sk = (NK - 1) * blk + 7
    q, k = _randn((1, 2, 1, D), "bf16", 3), _randn((1, 1, Sk, D), "bf16", 4)
    cache = pool_keys(k, block_size=blk)
    kw = dict(block_size=blk, causal=True, keep_first=1, keep_local=2, top_p=0.6, score_scale=1.0, as_lists=True, return_mass=True)
    want, got = select_blocks(q, k, 4000, **kw), select_blocks_pooled(q, cache, 4000, **kw)
    _same_lists(got[0], want[0], "8192")
    assert torch.equal(_bits(got[1]), _bits(want[1])) and 3 < int(want[0]["counts"].min()) < 4000


@pytest.mark.parametrize("blk,heads", [(128, "kv"), (64, "q")])
def test_lists_are_what_the_mask_converts_to(blk, heads):
    from rectified_spaattn_amd import select_blocks
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, D = 2, 4, 2, 64
    q, k = _randn((B, H, 700, D), "bf16", 5), _randn((B, Hkv, 9000, D), "bf16", 6)
    kw = dict(block_size=blk, kv_len=[9000, 1500], causal=True, keep_first=1, keep_local=2, mask_heads=heads, top_p=0.8)
    mask = select_blocks(q, k, 40, **kw)
    lists, mass = select_blocks(q, k, 40, as_lists=True, return_mass=True, **kw)
    want = block_mask_to_lists(mask, B, Hkv if heads == "kv" else H)
    _same_lists(lists, want, (blk, heads))
    cols, cnt = lists["cols"].cpu().numpy(), lists["counts"].cpu().numpy()
    assert all((np.diff(cols[r, i, :cnt[r, i]]) > 0).all() for r in range(cols.shape[0]) for i in range(cols.shape[1]))
    assert int(cnt.max()) == 40 and int(cnt.min()) < 40 and float(mass.min()) >= 0.0 and float(mass.max()) <= 1.0


def test_two_calls_give_the_same_bytes():
    from rectified_spaattn_amd import select_blocks
    q, k = _randn((2, 8, 3000, 128), "bf16", 21), _randn((2, 2, 5000, 128), "bf16", 22)
    outs = [select_blocks(q, k, 30, kv_len=[5000, 4444], causal=True, keep_local=1, top_p=0.7, return_scores=True, return_mass=True)
            for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    assert bool(outs[0][0].any()) and not bool(outs[0][0].all())


@pytest.mark.parametrize("dtype,n", [(torch.int32, 3), (torch.int64, 1)])
def test_device_kv_len_gives_the_ints_result_and_is_not_read_on_the_host(monkeypatch, dtype, n):
    from rectified_spaattn_amd import pool_keys, select_blocks, select_blocks_pooled
    B, H, Hkv, D = 3, 4, 2, 128
    q, k = _randn((B, H, 640, D), "bf16", 9), _randn((B, Hkv, 900, D), "bf16", 10)
    lens = [900, 333, 517] if n == 3 else [517]
    kw = dict(causal=True, keep_first=1, keep_local=1, top_p=0.75, return_scores=True, return_mass=True)
    host = lens if n == 3 else lens[0]
    cache = pool_keys(k, kv_len=host)
    on_host = select_blocks(q, k, 6, kv_len=host, **kw), select_blocks_pooled(q, cache, 6, kv_len=host, **kw)
    kv = torch.tensor(lens, dtype=dtype, device=DEV)
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("kv_len was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        on_device = select_blocks(q, k, 6, kv_len=kv, **kw), select_blocks_pooled(q, cache, 6, kv_len=kv, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    for got, want in zip(on_device, on_host):
        for a, b in zip(got, want):
            assert torch.equal(_bits(a), _bits(b))
    assert bool(on_host[0][0].any()) and not bool(on_host[0][0].all())


def test_one_graph_for_the_decode_step_at_top_p():
    """pool_keys(start = prev) and select_blocks_pooled(top_p, lists, mass) captured on a side stream; then, in place, a new q, one
    more key per item in the cache, kv_len bumped.  The replay equals the eager calls."""
    from rectified_spaattn_amd import pool_keys, select_blocks_pooled
    B, H, Hkv, D, blk, Sk = 2, 8, 2, 128, 128, 5000
    NK = -(-Sk // blk)
    lens = [4096, 333]          # item 0's next key opens a new block
    q, k = _randn((B, H, 1, D), "bf16", 5), _randn((B, Hkv, Sk, D), "bf16", 6)
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    prev = kv_len.clone()
    cache = pool_keys(k, kv_len=kv_len, out=torch.full((B, Hkv, NK, D), float("nan"), device=DEV))
    kw = dict(kv_len=kv_len, causal=True, keep_first=1, keep_local=1, as_lists=True, top_p=0.6, return_mass=True)

    def step(cache):
        pool_keys(k, kv_len=kv_len, start=prev, out=cache)
        return select_blocks_pooled(q, cache, 24, **kw)

    def same(a, b):
        _same_lists(a[0], b[0], "graph")
        assert torch.equal(_bits(a[1]), _bits(b[1]))

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
    before = (got[0]["counts"].clone(), got[1].clone())
    prev.copy_(kv_len)
    q.copy_(_randn((B, H, 1, D), "bf16", 55))
    for b in range(B):
        k[b, :, lens[b]] = 3.0 * k[b, :, lens[b]]
    kv_len += 1
    stale = cache.clone()
    graph.replay()
    torch.cuda.synchronize()
    same(got, step(stale))
    assert not torch.equal(got[1], before[1]) and 2 <= int(got[0]["counts"].min()) and int(got[0]["counts"].max()) <= 24


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def test_top_p_lists_drive_the_paged_decode_against_fp64():
    from rectified_spaattn_amd import block_sparse_decode, pool_keys, select_blocks_pooled
    from rectified_spaattn_amd.block_sparse import lists_to_block_mask
    B, H, Hkv, Sq, D, blk, Sk, dt = 2, 8, 2, 1, 128, 128, 2500, "bf16"
    NK = -(-Sk // blk)
    lens = [Sk, 1333]
    g = torch.Generator().manual_seed(31)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, DT[dt])
    k, v = (torch.randn(B, Hkv, Sk, D, generator=g).to(DEV, DT[dt]) for _ in range(2))
    for b, n in enumerate(lens):
        k[b, :, n:] = float("nan")
        v[b, :, n:] = float("nan")
    kp, vp, table, _ = _pool(k, v, blk, lens, 3)
    cache = pool_keys(kp, kv_len=lens, block_table=table)
    lists, mass = select_blocks_pooled(q, cache, NK, kv_len=lens, causal=True, keep_first=1, keep_local=1, as_lists=True,
                                       top_p=0.7, score_scale=4.0 * pref.default_scale(H, Hkv, D), return_mass=True)
    out, lse = block_sparse_decode(q, kp, vp, lists, kv_len=lens, causal=True, block_table=table, return_lse=True)
    torch.cuda.synchronize()
    mask = lists_to_block_mask(lists["bitmask"], B, Hkv, 1, NK).view(torch.bool).cpu().numpy()
    cnt = mask.sum(-1)
    assert 2 <= cnt.min() and cnt.max() < NK and float(mass.min()) >= 0.7 - 0.01        # a real cut, not the cap
    qn, kn, vn = (t.float().cpu().numpy() for t in (q, k, v))
    seen = decode_ref.visible(mask, lens, Sq, Sk, blk, H, True)
    want, _ = decode_ref.attention(decode_ref.scores2(qn, kn, D ** -0.5), seen, vn)
    _, lse_hat = decode_ref.attention(decode_ref.scores2(qn, kn, D ** -0.5, dt), seen, vn)
    err = np.abs(out.float().cpu().numpy().astype(np.float64) - want)
    d_lse = float(np.abs(lse.cpu().numpy().astype(np.float64) - lse_hat).max())
    print(f"counts {cnt.reshape(-1).tolist()}: out max {err.max():.3e} mean {err.mean():.3e}, lse {d_lse:.3e}")
    assert seen.any(-1).all() and err.max() < TOL[DT[dt]][0] and err.mean() < TOL[DT[dt]][1] and d_lse <= LSE_TOL[dt]


def test_top_p_mask_drives_causal_attention_against_fp64():
    from rectified_spaattn_amd import block_sparse_attention, select_blocks
    B, H, Hkv, D, S = 2, 4, 2, 128, 9 * 128 + 40
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(B, h, S, D, generator=g).to(DEV, dt) for h in (H, Hkv, Hkv))
    q64, k64, v64 = q.double().cpu(), k.double().cpu(), v.double().cpu()
    lens = [S] * B
    mask = select_blocks(q, k, 10, causal=True, keep_first=1, keep_local=1, top_p=0.6, score_scale=0.5)
    m = mask.cpu().numpy()
    vis = ref.visible(S, S, lens, 128, True)
    frc = ref.forced(S, S, lens, 128, True, 1, 1)
    assert not (m & ~vis[:, None]).any() and not (frc[:, None] & ~m).any()
    counts = m.sum(-1)
    assert counts.max() > 2 and (counts[..., -1] < 10).any()
    out = block_sparse_attention(q, k, v, mask, causal=True)
    lo, hi = rule.window_ranges(S, lens, -1, 0)
    seen = rule.visible(_expand_heads(m, H), lo, hi, lens, S, S)
    right = torch.arange(H) // (H // Hkv)
    scores = torch.matmul(q64, k64[:, right].transpose(-1, -2)) * D ** -0.5
    want = _attend(scores, v64[:, right], seen)
    err = (out.double().cpu() - want).abs()
    mx, mean = TOL[dt]
    print(f"max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
    assert torch.isfinite(out.float()).all() and err.max() <= mx and err.mean() <= mean
    assert seen.any(-1).all()
