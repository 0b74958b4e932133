"""The e4m3 K/V cache on the device: append_kv_e4m3, block_sparse_decode and pool_keys over
float8_e4m3fn caches with one fp32 scale per K/V head.

    byte equality  with power-of-two scales every result equals the 2-byte call on the dequantised cache code * 2^e, byte for byte
                   (output, log-sum-exp, pooled keys, the lists of a whole step)
    any scales     against fp64 attention over the dequantised operands at the plain call's tolerance; the distance to attention
                   over the un-quantised K / V is the number format's: printed, not gated
    exact          visibility (zero scores, V of 0 / 1) and weights (integer scores) through the e4m3 form
    writer         bytes = (x.float() / s).clamp(-448, 448).to(float8_e4m3fn) on torch's CPU path, placed where the model of
                   tests/kv8_ref.py puts them, every other byte untouched
    one graph      append -> pool_keys(start = prev) -> select_blocks_pooled -> block_sparse_decode, replayed on changed contents

Shapes are the decode tests': capacity 700, B = 2; the cache beyond kv_len[b] and the spare pages hold the NaN code 0x7F."""
import numpy as np
import pytest
import torch

import decode_ref as ref
import kv8_ref as kv8
import select_ref
from test_gpu_decode import COMBOS, LENS, LSE_TOL, TOL, _hl, _id, _kv_arg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SK = ref.SK
E4M3 = torch.float8_e4m3fn
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = 0xA5


def _dev8(codes):
    """uint8 numpy codes -> the float8_e4m3fn device tensor that holds them."""
    return torch.from_numpy(np.ascontiguousarray(codes)).to(DEV).view(E4M3)


def _bytes(t):
    return t.view(torch.uint8) if t.dtype in (E4M3, torch.bool) else (t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b))


def _scales(pair):
    return tuple(torch.from_numpy(s).to(DEV) for s in pair)


def _quantised(kf, vf, scales, lens, dt):
    """(k8, v8, kd, vd): the e4m3 caches with the NaN code beyond kv_len[b], and the 2-byte caches code * scale (NaN there)."""
    ks, vs = scales
    kc, vc = kv8.quantize(kf, ks), kv8.quantize(vf, vs)
    for b, n in enumerate(lens):
        kc[b, :, n:] = kv8.NAN_CODE
        vc[b, :, n:] = kv8.NAN_CODE
    kd, vd = (torch.from_numpy(kv8.dequant(c, s)).to(DEV, TDT[dt]) for c, s in ((kc, ks), (vc, vs)))
    return kc, vc, kd, vd


def _pool8(kc, vc, blk, lens, seed, bad=-1):
    """test_gpu_decode._pool's layout over uint8 codes: B * NK + 3 pages placed by a random permutation, the spare ones and the
    ragged tails full of the NaN code, garbage table entries past ceil(kv_len[b] / block)."""
    B, Hkv, Sk, D = kc.shape
    NK = -(-Sk // blk)
    P = B * NK + 3
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed)).tolist()
    kp = np.full((P, Hkv, blk, D), kv8.NAN_CODE, np.uint8)
    vp = kp.copy()
    table = np.full((B, NK), P + 5 if bad == "P+5" else bad, np.int32)
    for b in range(B):
        for j in range(NK):
            if j * blk >= lens[b]:
                continue
            pg = perm[b * NK + j]
            rows = min(blk, Sk - j * blk)
            kp[pg, :, :rows] = kc[b, :, j * blk:j * blk + rows]
            vp[pg, :, :rows] = vc[b, :, j * blk:j * blk + rows]
            table[b, j] = pg
    return kp, vp, table, P


def _inputs(c):
    B, H, Hkv, Sq, D, blk = 2, c["H"], c["Hkv"], c["Sq"], c["D"], c["blk"]
    g = torch.Generator().manual_seed(c["seed"])
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, TDT[c["dt"]])
    kf, vf = (torch.randn(B, Hkv, SK, D, generator=g).numpy() for _ in range(2))
    mask = (torch.rand(B, _hl(c), 1, -(-SK // blk), generator=g) < 0.5).to(DEV)
    mask[:, ::2, 0, 0] = True
    lens = LENS[c["lens"]]
    kw = dict(kv_len=_kv_arg(c["lens"], lens), block_size=blk, causal=c["causal"], blocks_per_split=c["bps"], return_lse=True)
    return q, kf, vf, mask, lens, kw


# ---- 1. byte equality with the 2-byte call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_power_of_two_scales_give_the_bytes_of_the_two_byte_call(c):
    """Scales 2^e per head, e in -2 .. 2, different for K and V: the dequantised cache is exact in bf16 and fp16, and a power of
    two commutes with every fp32 rounding of the walk (N(0, 1) inputs: tests/test_kv8_cpu.py asserts the exponent range)."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    q, kf, vf, mask, lens, kw = _inputs(c)
    pair = kv8.pow2_scales(c["Hkv"], c["seed"])
    kc, vc, kd, vd = _quantised(kf, vf, pair, lens, c["dt"])
    ks, vs = _scales(pair)
    want = dec(q, kd, vd, mask, **kw)
    got = dec(q, _dev8(kc), _dev8(vc), mask, k_scale=ks, v_scale=vs, **kw)
    assert got[0].dtype == TDT[c["dt"]] and got[1].dtype == torch.float32
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert bool(torch.isfinite(got[0].float()).all())
    # paged = contiguous (garbage -1 / P + 5 in the table where no key is, 0x7F in every spare byte)
    kp, vp, table, _ = _pool8(kc, vc, c["blk"], lens, c["seed"], bad=-1 if c["seed"] % 2 else "P+5")
    kwp = dict(kw, kv_len=list(lens) if kw["kv_len"] is None else kw["kv_len"], block_table=torch.from_numpy(table).to(DEV))
    paged = dec(q, _dev8(kp), _dev8(vp), mask, k_scale=ks, v_scale=vs, **kwp)
    assert _same(paged[0], want[0]) and _same(paged[1], want[1])
    # the lists dict = the mask; two calls give the same bytes
    lists = block_mask_to_lists(mask, 2, _hl(c))
    for again in (dec(q, _dev8(kc), _dev8(vc), lists, k_scale=ks, v_scale=vs, **kw),
                  dec(q, _dev8(kc), _dev8(vc), mask, k_scale=ks, v_scale=vs, **kw)):
        assert _same(again[0], want[0]) and _same(again[1], want[1])


def test_scale_forms_and_strided_cache_views():
    """A Python float, a tensor of one value and a tensor of Hkv equal values are one call; [B, S, Hkv, D] views of the cache are
    read in place."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    c = COMBOS[18]      # (8 query heads over 2 K/V heads, kv_len [700, 333])
    assert c["Hkv"] == 2 and c["lens"] == "list"
    q, kf, vf, mask, lens, kw = _inputs(c)
    kc, vc, _, _ = _quantised(kf, vf, (np.float32(0.5), np.float32(2.0)), lens, c["dt"])
    k8, v8 = _dev8(kc), _dev8(vc)
    want = dec(q, k8, v8, mask, k_scale=torch.full((c["Hkv"],), 0.5, device=DEV), v_scale=torch.full((c["Hkv"],), 2.0, device=DEV), **kw)
    for ks, vs in ((0.5, 2.0), (torch.tensor([0.5], device=DEV), torch.tensor(2.0, device=DEV)), (0.5, torch.tensor([2.0], device=DEV))):
        got = dec(q, k8, v8, mask, k_scale=ks, v_scale=vs, **kw)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
    views = [t.view(torch.uint8).transpose(1, 2).contiguous().transpose(1, 2).view(E4M3) for t in (k8, v8)]
    assert not views[0].is_contiguous()
    got = dec(q, *views, mask, k_scale=0.5, v_scale=2.0, **kw)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and bool(got[0].any())


# ---- 2. arbitrary scales against fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", COMBOS, ids=_id)
def test_arbitrary_scales_against_fp64_over_the_dequantised_operands(c):
    """k_scale = 0.37, 1.9, ..., v_scale = 2.3, 0.11, ...: the plain call's tolerance over code * scale (the added roundings are
    two fp32 multiplies), the log-sum-exp within LSE_TOL of the reference on the operands the kernel multiplies."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    q, kf, vf, mask, lens, kw = _inputs(c)
    pair = kv8.odd_scales(c["Hkv"])
    kc, vc, _, _ = _quantised(kf, vf, pair, lens, c["dt"])
    ks, vs = _scales(pair)
    out, lse = dec(q, _dev8(kc), _dev8(vc), mask, k_scale=ks, v_scale=vs, **kw)
    torch.cuda.synchronize()
    qn = q.float().cpu().numpy()
    kd, vd = kv8.dequant(kc, pair[0]), kv8.dequant(vc, pair[1])
    seen = ref.visible(mask.cpu().numpy(), lens, c["Sq"], SK, c["blk"], c["H"], c["causal"])
    sm = c["D"] ** -0.5
    want, lse64 = ref.attention(ref.scores2(qn, kd, sm), seen, vd)
    _, lse_hat = ref.attention(ref.scores2(qn, kd, sm, c["dt"]), seen, vd)
    exact, _ = ref.attention(ref.scores2(qn, kf, sm), seen, vf)
    got, got_lse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    has = seen.any(-1)
    err = np.abs(got - want)
    d_hat = float(np.abs(got_lse[has] - lse_hat[has]).max()) if has.any() else 0.0
    fmt = np.abs(got - exact)
    print(f"{_id(c)}: out max {err.max():.3e} mean {err.mean():.3e}; lse vs quantised {d_hat:.3e} (bound {LSE_TOL[c['dt']]:.3e}); "
          f"vs attention over the un-quantised K / V (the format's, not gated): max {fmt.max():.3e} mean {fmt.mean():.3e}")
    assert np.isfinite(got).all()
    assert err.max() < TOL[c["dt"]][0] and err.mean() < TOL[c["dt"]][1]
    assert (got[~has] == 0).all() and np.isneginf(got_lse[~has]).all()
    assert np.isfinite(got_lse[has]).all() and d_hat <= LSE_TOL[c["dt"]]


# ---- 3. the exact witnesses ------------------------------------------------------------------------------------------------------------
def _run_case8(c, inp):
    """A witness case through the e4m3 form with power-of-two scales -> (out, lse, the dequantised inputs)."""
    from rectified_spaattn_amd import block_sparse_decode as dec
    pair = kv8.pow2_scales(c["Hkv"], c["seed"])
    kc, vc = kv8.quantize(inp["k"], pair[0]), kv8.quantize(inp["v"], pair[1])
    deq = dict(inp, k=kv8.dequant(kc, pair[0]).astype(np.float32), v=kv8.dequant(vc, pair[1]).astype(np.float32))
    for b, n in enumerate(c["lens"]):
        kc[b, :, n:] = kv8.NAN_CODE
        vc[b, :, n:] = kv8.NAN_CODE
    ks, vs = _scales(pair)
    q = torch.from_numpy(inp["q"]).to(DEV, TDT[c["dt"]])
    out, lse = dec(q, _dev8(kc), _dev8(vc), torch.from_numpy(inp["mask"]).to(DEV), kv_len=list(c["lens"]), sm_scale=inp["sm_scale"],
                   block_size=c["blk"], causal=c["causal"], blocks_per_split=c["C"], return_lse=True, k_scale=ks, v_scale=vs)
    return out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64), deq


@pytest.mark.parametrize("c", ref.VIS_CASES, ids=lambda c: c["id"])
def test_exact_visibility(c):
    """Zero scores (disjoint channel supports survive the quantisation) and a 0 / 1 V, whose codes are exact under a power-of-two
    scale: every output element is a count over the visible keys divided by their number."""
    inp = ref.vis_inputs(c)
    got, lse, deq = _run_case8(c, inp)
    assert np.array_equal(deq["v"], inp["v"]) and np.array_equal(deq["k"] != 0, inp["k"] != 0)
    want, lse_want, _ = ref.case_reference(c, deq)
    ok, worst = ref.within(got, want, c["dt"])
    print(f"{c['id']}: worst {worst:.3f} tolerances")
    assert ok, worst
    has = np.isfinite(lse_want)
    assert np.isneginf(lse[~has]).all() and np.isfinite(lse[has]).all()


@pytest.mark.parametrize("c", ref.WEIGHT_CASES, ids=lambda c: c["id"])
def test_exact_weights(c):
    """Integer scores (K = 8 n, n <= 10: exact codes under scales 2^-2 .. 2^2), so every weight is a power of two: visibility's
    bound on the output and 2^-21 relative on the log-sum-exp, as for the 2-byte call."""
    inp = ref.weight_inputs(c)
    total, spread = ref.weight_budget(c, inp)
    assert total < 2.0 ** 24 and spread <= ref.SPREAD
    got, lse, deq = _run_case8(c, inp)
    assert np.array_equal(deq["k"], inp["k"]) and np.array_equal(deq["v"], inp["v"])
    want, lse_want, _ = ref.case_reference(c, inp)
    ok, worst = ref.within(got, want, c["dt"])
    has = np.isfinite(lse_want)
    d = np.abs(lse[has] - lse_want[has]) / np.maximum(1.0, np.abs(lse_want[has]))
    print(f"{c['id']}: worst {worst:.3f} tolerances; lse {float(d.max()) * 2 ** 21 if has.any() else 0:.3f} x 2^-21")
    assert ok, worst
    assert np.isneginf(lse[~has]).all()
    assert (d <= 2.0 ** -21).all()


# ---- 4. the writer ---------------------------------------------------------------------------------------------------------------------
def _new_rows(B, Hkv, T, D, dt, scales, seed):
    """New rows of N(0, 1) with the special inputs sprinkled in: +-Inf, NaN (torch's cast to bf16 makes it a negative one, its
    cast to fp16 a positive one), values above 448 * scale, results that are e4m3 subnormals, ties and zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hkv, T, D, generator=g)
    flat = x.view(-1)
    spots = torch.randperm(flat.numel(), generator=g)[:64]
    smax = float(max(scales[0].max(), scales[1].max()))
    smin = float(min(scales[0].min(), scales[1].min()))
    special = [float("inf"), float("-inf"), float("nan"), 449.0 * smax, -470.0 * smax, 3000.0 * smax, 2.0 ** -9 * smin, 2.0 ** -10 * smin,
               1.5 * 2.0 ** -10 * smin, -(2.0 ** -8) * smin, 0.0, -0.0, 448.0 * smin, -448.0 * smin, 2.0 ** -7 * smax, 5e-4 * smin]
    flat[spots] = torch.tensor(special * 4)
    return x.to(TDT[dt])


def _writes(blk):
    """(start per item, n_new per item | None, T): inside a block, filling it, into the next, across two, n_new < T, a whole
    block, past the capacity, past it with a count."""
    return [([5, 70], None, 3), ([blk - 3, 2 * blk - 3], None, 3), ([blk - 2, 2 * blk - 2], None, 5),
            ([blk - 3, 2 * blk - 3], None, blk + 10), ([0, 130], [2, 0], 6), ([0, 0], None, blk), ([SK - 2, SK], None, 5),
            ([690, 3], [40, 1], 40)]


@pytest.mark.parametrize("dt,D,blk,paged", [("bf16", 128, 128, False), ("fp16", 64, 64, False), ("fp16", 128, 64, True),
                                            ("bf16", 64, 128, True)])
def test_writer_bytes_placement_and_untouched_sentinel(dt, D, blk, paged):
    from rectified_spaattn_amd import append_kv_e4m3
    B, Hkv = 2, 3
    NK = -(-SK // blk)
    pair = (np.array([0.37, 1.0, 4.0], np.float32), np.array([2.3, 0.11, 0.5], np.float32))
    ks, vs = _scales(pair)
    if paged:
        P = B * NK + 2
        table = np.random.default_rng(blk + D).permutation(P)[:B * NK].reshape(B, NK).astype(np.int32)
        table[0, 2], table[1, 1] = -1, P + 5            # two blocks without a page: their rows are dropped
        shape, tab = (P, Hkv, blk, D), torch.from_numpy(table).to(DEV)
    else:
        table, shape, tab = None, (B, Hkv, SK, D), None
    model_k, model_v = np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8)
    k8, v8 = _dev8(model_k), _dev8(model_v)
    dropped, codes_seen = 0, set()
    for i, (start, n_new, T) in enumerate(_writes(blk)):
        k_new, v_new = (_new_rows(B, Hkv, T, D, dt, pair, 10 * i + s) for s in (1, 2))
        append_kv_e4m3(k_new.to(DEV), v_new.to(DEV), k8, v8, start=start, n_new=n_new, k_scale=ks, v_scale=vs, block_size=blk,
                       block_table=tab)
        counts = [T, T] if n_new is None else n_new
        model_k, wk = kv8.append(model_k, kv8.quantize(k_new, pair[0]), start, counts, blk, table)
        model_v, _ = kv8.append(model_v, kv8.quantize(v_new, pair[1]), start, counts, blk, table)
        dropped += sum(counts) * Hkv * D - int(wk.sum())
        codes_seen.update(np.unique(model_k).tolist() + np.unique(model_v).tolist())
        assert np.array_equal(k8.view(torch.uint8).cpu().numpy(), model_k), (i, "k")
        assert np.array_equal(v8.view(torch.uint8).cpu().numpy(), model_v), (i, "v")
    assert dropped > 0                                   # (positions past the capacity -- and pageless ones -- wrote nothing)
    # the sentinel survives elsewhere; NaN, both saturated values and subnormal results were among the placed codes
    assert (model_k == SENTINEL).mean() > 0.3
    assert {0x7E, 0xFE} <= codes_seen and codes_seen & {kv8.NAN_CODE, 0xFF} and codes_seen & set(range(1, 8)) and codes_seen & set(range(0x81, 0x88))
    # the call again: the same bytes
    append_kv_e4m3(k_new.to(DEV), v_new.to(DEV), k8, v8, start=start, n_new=n_new, k_scale=ks, v_scale=vs, block_size=blk,
                   block_table=tab)
    assert np.array_equal(k8.view(torch.uint8).cpu().numpy(), model_k)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_writer_nan_codes_keep_the_sign_of_the_input(dt):
    """A NaN stays a NaN code, 0x7F or 0xFF by the sign bit of the input element, whatever its payload.  For bf16 that is torch's
    CPU expression for every NaN; torch's own fp16 -> fp32 cast keeps the sign of a NaN on its vector path and drops it on its
    scalar one, so for fp16 the expression is held to the positive ones -- what torch's casts to fp16 produce -- and the
    negative ones are pinned here."""
    from rectified_spaattn_amd import append_kv_e4m3
    pos = {"bf16": [0x7FC0, 0x7F81, 0x7FFF], "fp16": [0x7E00, 0x7C01, 0x7FFF]}[dt]
    bits = np.array(pos + [b | 0x8000 for b in pos] + [0x0000, 0x8000], np.uint16)
    x = torch.from_numpy(np.resize(bits, 2 * 64).view(np.int16).copy()).view(TDT[dt]).view(1, 1, 2, 64)
    want = np.resize(np.array([0x7F] * 3 + [0xFF] * 3 + [0x00, 0x80], np.uint8), 2 * 64).reshape(1, 1, 2, 64)
    by_torch = kv8.quantize(x, 0.37)
    agree = by_torch == want
    assert agree[..., :3].all() and agree.reshape(-1, 8)[:, 6:].all() and (agree.all() if dt == "bf16" else True)
    kc, vc = (_dev8(np.full((1, 1, 5, 64), SENTINEL, np.uint8)) for _ in range(2))
    append_kv_e4m3(x.to(DEV), x.to(DEV), kc, vc, start=1, k_scale=0.37, v_scale=torch.tensor([2.3], device=DEV))
    for c in (kc, vc):
        got = c.view(torch.uint8).cpu().numpy()
        assert np.array_equal(got[:, :, 1:3], want) and (got[:, :, [0, 3, 4]] == SENTINEL).all()


@pytest.mark.parametrize("dtype,n", [(torch.int32, 2), (torch.int64, 2), (torch.int64, 1)])
def test_writer_device_limits_are_not_read_on_the_host(monkeypatch, dtype, n):
    from rectified_spaattn_amd import append_kv_e4m3
    B, Hkv, T, D, blk = 2, 2, 9, 64, 64
    starts, counts = ([60, 697], [9, 4]) if n == 2 else ([60], [4])
    k_new, v_new = (torch.randn(B, Hkv, T, D, generator=torch.Generator().manual_seed(s)).to(DEV, torch.bfloat16) for s in (1, 2))
    caches = [_dev8(np.full((B, Hkv, SK, D), SENTINEL, np.uint8)) for _ in range(4)]
    one = lambda v: v if n == 2 else v[0]       # noqa: E731
    append_kv_e4m3(k_new, v_new, caches[0], caches[1], start=one(starts), n_new=one(counts), k_scale=0.5, v_scale=1.9, block_size=blk)
    st, nn = torch.tensor(starts, dtype=dtype, device=DEV), torch.tensor(counts, dtype=dtype, device=DEV)
    ks, vs = torch.tensor([0.5], device=DEV), torch.tensor([1.9, 1.9], device=DEV)
    torch.cuda.synchronize()

    def refuse(*a, **kws):
        raise AssertionError("a device limit was read on the host")
    for name in ("item", "tolist", "cpu"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        append_kv_e4m3(k_new, v_new, caches[2], caches[3], start=st, n_new=nn, k_scale=ks, v_scale=vs, block_size=blk)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        monkeypatch.undo()
    assert _same(caches[2], caches[0]) and _same(caches[3], caches[1])
    wrote = caches[0].view(torch.uint8) != SENTINEL
    assert bool(wrote.any()) and not bool(wrote[:, :, :60].any())
    # a device start beyond the capacity is clamped (nothing fits), a negative one is 0; a count beyond T is T
    wild = [_dev8(np.full((B, Hkv, SK, D), SENTINEL, np.uint8)) for _ in range(4)]
    append_kv_e4m3(k_new, v_new, wild[0], wild[1], start=torch.tensor([10 ** 6, -5], device=DEV), n_new=torch.tensor([10 ** 6], device=DEV),
                   k_scale=0.5, v_scale=1.9, block_size=blk)
    append_kv_e4m3(k_new, v_new, wild[2], wild[3], start=[SK, 0], k_scale=0.5, v_scale=1.9, block_size=blk)
    assert _same(wild[0], wild[2]) and _same(wild[1], wild[3]) and bool((wild[0].view(torch.uint8)[0] == SENTINEL).all())


def test_writer_reads_views_of_one_fused_projection_without_a_copy(monkeypatch):
    from rectified_spaattn_amd import _core, append_kv_e4m3
    B, H, Hkv, T, D, blk = 2, 8, 2, 5, 128, 128
    buf = torch.randn(B, T, (H + 2 * Hkv) * D, generator=torch.Generator().manual_seed(4)).to(DEV, torch.bfloat16)
    k_new = buf[..., H * D:(H + Hkv) * D].view(B, T, Hkv, D).permute(0, 2, 1, 3)
    v_new = buf[..., (H + Hkv) * D:].view(B, T, Hkv, D).permute(0, 2, 1, 3)
    assert not k_new.is_contiguous() and not v_new.is_contiguous()
    caches = [_dev8(np.full((B, Hkv, SK, D), SENTINEL, np.uint8)) for _ in range(4)]
    seen = []
    t4 = _core._t4
    monkeypatch.setattr(_core, "_t4", lambda t: (seen.append(t.data_ptr()), t4(t))[1])
    append_kv_e4m3(k_new, v_new, caches[0], caches[1], start=[126, 0], k_scale=0.37, v_scale=2.3)
    assert seen == [k_new.data_ptr(), v_new.data_ptr()]
    append_kv_e4m3(k_new.contiguous(), v_new.contiguous(), caches[2], caches[3], start=[126, 0], k_scale=0.37, v_scale=2.3)
    assert _same(caches[0], caches[2]) and _same(caches[1], caches[3])
    want = kv8.append(np.full((B, Hkv, SK, D), SENTINEL, np.uint8), kv8.quantize(v_new, 2.3), [126, 0], [T, T])[0]
    assert np.array_equal(caches[1].view(torch.uint8).cpu().numpy(), want)


# ---- 5. pool_keys from the e4m3 pool ----------------------------------------------------------------------------------------------------
POOL_CASES = [("bf16", 128, 128), ("fp16", 64, 64), ("bf16", 64, 128), ("fp16", 128, 64)]


@pytest.mark.parametrize("dt,D,blk", POOL_CASES, ids=[f"{a}-D{b}-b{c}" for a, b, c in POOL_CASES])
def test_pool_keys_equals_the_two_byte_pool_and_fp64(dt, D, blk):
    """Power-of-two scales: byte-equal to pool_keys on the dequantised 2-byte pool, contiguous and paged, NaN codes beyond the
    limits, an out-of-range entry of a written block gives zeros.
    Arbitrary scales against fp64: section 5.13 bounds the fp32 sum of b terms and its one division by 4 (b + 1) 2^-24 mean|k_d|;
    here the summed terms are float(code), exact, and the final multiply by k_scale adds one rounding, at most 2^-24 of the
    result's magnitude <= 2^-24 s mean|code_d|.  So |got - want| <= (4 (b + 1) + 1) 2^-24 s[hkv] mean|code_d| per channel."""
    from rectified_spaattn_amd import pool_keys
    B, Hkv = 2, 3
    NK = -(-SK // blk)
    lens = [SK, 333]
    kf = torch.randn(B, Hkv, SK, D, generator=torch.Generator().manual_seed(D + blk)).numpy()
    fill = lambda: torch.full((B, Hkv, NK, D), float("nan"), dtype=torch.float32, device=DEV)       # noqa: E731
    pair = kv8.pow2_scales(Hkv, D + blk)
    kc, _, kd, _ = _quantised(kf, kf, pair, lens, dt)
    ks = torch.from_numpy(pair[0]).to(DEV)
    want = pool_keys(kd, block_size=blk, kv_len=lens, out=fill())
    got = pool_keys(_dev8(kc), block_size=blk, kv_len=lens, out=fill(), k_scale=ks)
    assert _same(got, want) and bool(torch.isfinite(got[0]).all()) and bool(torch.isnan(got[1, :, -(-333 // blk):]).all())
    kp, _, table, P = _pool8(kc, kc, blk, lens, D, bad="P+5")
    tab = torch.from_numpy(table).to(DEV)
    assert _same(pool_keys(_dev8(kp), block_size=blk, kv_len=lens, block_table=tab, out=fill(), k_scale=ks), want)
    # device limits and an update through the table
    dev = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)       # noqa: E731
    upd = pool_keys(_dev8(kp), block_size=blk, kv_len=dev(lens), start=dev([blk + 1, 333]), block_table=tab, out=fill(), k_scale=ks)
    assert _same(upd[0, :, 1:], want[0, :, 1:]) and bool(torch.isnan(upd[0, :, 0]).all())
    last = 332 // blk
    assert _same(upd[1, :, last], want[1, :, last]) and bool(torch.isnan(upd[1, :, :last]).all())
    for entry in (P + 5, -1):
        t2 = tab.clone()
        t2[0, 1] = entry
        z = pool_keys(_dev8(kp), block_size=blk, kv_len=lens, block_table=t2, out=fill(), k_scale=ks)
        assert bool((z[0, :, 1] == 0).all())
        z[0, :, 1] = want[0, :, 1]
        assert _same(z, want)
    # arbitrary scales against fp64
    s = np.array([0.37, 1.9, 0.83], np.float32)
    kc = kv8.quantize(kf, s)
    for b, n in enumerate(lens):
        kc[b, :, n:] = kv8.NAN_CODE
    got = pool_keys(_dev8(kc), block_size=blk, kv_len=lens, k_scale=torch.from_numpy(s).to(DEV)).cpu().numpy().astype(np.float64)
    ref64 = kv8.pooled(kc, s, lens, blk)
    mean_abs = select_ref.pooled(np.abs(np.nan_to_num(kv8.code_values()[kc])), lens, blk) * s.astype(np.float64)[None, :, None, None]
    tol = (4 * (blk + 1) + 1) * 2.0 ** -24 * mean_abs
    live = np.zeros(got.shape, bool)
    for b, n in enumerate(lens):
        live[b, :, :-(-n // blk)] = True
    err = np.abs(np.where(live, got - ref64, 0.0))
    print(f"{dt} D{D} b{blk}: error / tol max {float((err[live] / tol[live]).max()):.3f}")
    assert np.isfinite(got[live]).all() and (err <= tol)[live].all()


@pytest.mark.parametrize("blk", [64, 128])
def test_pool_keys_incremental_equals_from_scratch(blk):
    from rectified_spaattn_amd import pool_keys
    B, Hkv, D = 2, 2, 64
    NK = -(-SK // blk)
    kf = torch.randn(B, Hkv, SK, D, generator=torch.Generator().manual_seed(blk)).numpy()
    s = torch.tensor([0.37, 1.9], device=DEV)
    full = kv8.quantize(kf, s.cpu().numpy())
    for old, new in (([blk - 1, blk], [blk, blk + 1]), ([2 * blk - 1, 5], [3 * blk + 1, 5]), ([SK - 1, 333], [SK, 334])):
        kc = full.copy()
        for b in range(B):
            kc[b, :, old[b]:] = kv8.NAN_CODE
        cache = pool_keys(_dev8(kc), block_size=blk, kv_len=old, out=torch.full((B, Hkv, NK, D), float("nan"), device=DEV), k_scale=s)
        for b in range(B):
            kc[b, :, old[b]:new[b]] = full[b, :, old[b]:new[b]]
        fresh = pool_keys(_dev8(kc), block_size=blk, kv_len=new, out=torch.full((B, Hkv, NK, D), float("nan"), device=DEV), k_scale=s)
        for wph in (None, 1, 3):
            upd = pool_keys(_dev8(kc), block_size=blk, kv_len=new, start=old, out=cache.clone(), k_scale=s, workgroups_per_head=wph)
            assert _same(upd, fresh), (old, new, wph)
        assert not _same(cache, fresh)


# ---- 6. one step, one graph --------------------------------------------------------------------------------------------------------------
def _same_lists(a, b):
    for name in ("bitmask", "counts"):
        assert torch.equal(a[name], b[name]), name
    live = torch.arange(a["cols"].shape[-1], device=DEV)[None, None, :] < b["counts"][..., None]
    assert torch.equal(torch.where(live, a["cols"], 0), torch.where(live, b["cols"], 0))


def test_one_graph_for_the_four_calls_of_a_decode_step():
    """append_kv_e4m3(start = prev) -> pool_keys(start = prev, out = pooled) -> select_blocks_pooled -> block_sparse_decode over a
    paged e4m3 cache, captured on a side stream.  Replayed after another token (item 0's opens a block), bumped device limits
    and a moved page it equals the eager calls, and -- power-of-two scales -- the all-2-byte step on the dequantised cache."""
    from rectified_spaattn_amd import append_kv_e4m3, block_sparse_decode, pool_keys, select_blocks_pooled
    B, H, Hkv, Sq, D, blk, dt = 2, 8, 2, 1, 128, 128, torch.bfloat16
    NK = -(-SK // blk)
    lens = [511, 332]           # the step's token lands at 511 / 332; the next one opens item 0's fifth block
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, dt)
    kf, vf = (torch.randn(B, Hkv, SK, D, generator=g).to(dt) for _ in range(2))
    pair = kv8.pow2_scales(Hkv, 3)
    ks, vs = _scales(pair)
    P = B * NK + 3
    perm = torch.randperm(P, generator=g)
    table = perm[:B * NK].reshape(B, NK).to(torch.int32).to(DEV)
    kp, vp = (_dev8(np.full((P, Hkv, blk, D), kv8.NAN_CODE, np.uint8)) for _ in range(2))
    kw8 = dict(k_scale=ks, v_scale=vs, block_table=table)
    append_kv_e4m3(kf.to(DEV), vf.to(DEV), kp, vp, start=0, n_new=lens, **kw8)      # the prefill is the same call
    kv_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    prev = kv_len.clone()
    pooled = pool_keys(kp, kv_len=kv_len, block_table=table, k_scale=ks, out=torch.full((B, Hkv, NK, D), float("nan"), device=DEV))
    tok_k, tok_v = (torch.empty(B, Hkv, 1, D, dtype=dt, device=DEV) for _ in range(2))
    sel_kw = dict(kv_len=kv_len, causal=True, keep_first=1, keep_local=1, as_lists=True)

    def feed(pos):              # the token of position pos[b], and the device limits after it
        for b in range(B):
            tok_k[b, :, 0], tok_v[b, :, 0] = kf[b, :, pos[b]].to(DEV), vf[b, :, pos[b]].to(DEV)
        prev.copy_(torch.tensor(pos, dtype=torch.int32))
        kv_len.copy_(prev + 1)

    def step(pooled, kp, vp):
        append_kv_e4m3(tok_k, tok_v, kp, vp, start=prev, **kw8)
        pool_keys(kp, kv_len=kv_len, start=prev, block_table=table, k_scale=ks, out=pooled)
        lists = select_blocks_pooled(q, pooled, 3, **sel_kw)
        return (lists,) + block_sparse_decode(q, kp, vp, lists, kv_len=kv_len, causal=True, return_lse=True, **kw8)

    def two_byte_step(kp, vp):
        kd, vd = ((p.cpu().float() * torch.from_numpy(s).view(1, -1, 1, 1)).to(dt).to(DEV) for p, s in ((kp, pair[0]), (vp, pair[1])))
        lists = select_blocks_pooled(q, pool_keys(kd, kv_len=kv_len, block_table=table), 3, **sel_kw)
        return (lists,) + block_sparse_decode(q, kd, vd, lists, kv_len=kv_len, causal=True, block_table=table, return_lse=True)

    def same(a, b):
        _same_lists(a[0], b[0])
        assert _same(a[1], b[1]) and _same(a[2], b[2])

    feed(lens)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(pooled.clone(), kp.clone(), vp.clone())        # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step(pooled, kp, vp)
    stale = (pooled.clone(), kp.clone(), vp.clone())
    graph.replay()
    torch.cuda.synchronize()
    same(got, step(*stale))
    assert _same(stale[1], kp) and _same(stale[2], vp) and _same(stale[0], pooled)
    same(got, two_byte_step(kp, vp))
    before = got[1].clone()
    # the next step: another token per item, the limits bumped on the device, a page moved
    feed([n + 1 for n in lens])
    spare = sorted(set(range(P)) - set(table.reshape(-1).tolist()))[0]
    moved = table[1, 2].item()
    kp.view(torch.uint8)[spare], vp.view(torch.uint8)[spare] = kp.view(torch.uint8)[moved].clone(), vp.view(torch.uint8)[moved].clone()
    kp.view(torch.uint8)[moved], vp.view(torch.uint8)[moved] = kv8.NAN_CODE, kv8.NAN_CODE
    table[1, 2] = spare
    stale = (pooled.clone(), kp.clone(), vp.clone())
    graph.replay()
    torch.cuda.synchronize()
    same(got, step(*stale))
    assert _same(stale[1], kp) and _same(stale[0], pooled)
    same(got, two_byte_step(kp, vp))
    opened = kp.view(torch.uint8)[table[0, 4].item(), :, 0]
    assert bool((opened != kv8.NAN_CODE).any()) and bool((kp.view(torch.uint8)[table[0, 4].item(), :, 1] == kv8.NAN_CODE).all())
    assert not torch.equal(got[1], before) and bool(torch.isfinite(got[1].float()).all())
    assert int(got[0]["counts"].min()) == 3
