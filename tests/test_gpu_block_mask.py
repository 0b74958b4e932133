"""Block-sparse attention over caller-supplied block masks on the MI355X: the mask <-> list conversion against the selection
pass's own lists, the reference's two building blocks against its golden vectors, and the plain kernel against fp64 attention."""
import zlib

import numpy as np
import pytest
import torch

from conftest import B2_CASES, OP_CASES, case_inputs, load_op_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = {torch.bfloat16: (2e-2, 2e-3), torch.float16: (2e-3, 2e-4)}
B64_CASES = ["b64_wan_pad_1450", "b64_hunyuan_1280", "b64_flux_1536", "b64_cogvideo_1058", "b64_wan_d64_1100",
             "b64_b2_hunyuan_1280", "b64_big_wan_16640"]
ALL_CASES = OP_CASES + B2_CASES + B64_CASES
VARIANT_MODULE = dict(hunyuan="rectified_hunyuan_attn", flux="rectified_flux_attn", cogvideo="rectified_cogvideo_attn",
                      wan="rectified_wan21_attn")


def _case(name, dt=torch.bfloat16):
    """(meta, gold, q, k, v on the device, LayoutSpec, neighbour matrix or None, block) of a golden operator case."""
    from rectified_spaattn_amd import _core, synth
    meta, gold = load_op_case(name)
    if name.startswith("b64_"):
        blk = 64
        q, k, v = synth.structured_qkv(meta["seed"], meta["B"], meta["H"], meta["S"], meta["D"], block=64)
        ctor = dict(hunyuan=lambda: _core.LayoutSpec.hunyuan(meta["S"], meta["num_true"], block=64),
                    flux=lambda: _core.LayoutSpec.flux(meta["S"], meta["text_length"], block=64),
                    cogvideo=lambda: _core.LayoutSpec.cogvideo(meta["S"], meta["text_length"], block=64),
                    wan=lambda: _core.LayoutSpec.wan(meta["S"], meta.get("ffb", 0), block=64))
        spec = ctor[meta["variant"]]()
        nbr = synth.banded_neighbors(spec.NBv, meta["nb_width"]) if meta["nb_width"] >= 0 else None
    else:
        blk = 128
        q, k, v, lay, nbr = case_inputs(meta)
        spec = _core.LayoutSpec(lay.S, lay.NB_total, lay.NBv, lay.n_txt, lay.kv_valid, lay.pool_valid, lay.text_end_block,
                                lay.ffb, lay.q_text_valid, lay.kv_text_valid)
    tq, tk, tv = (torch.from_numpy(x).to(DEV, dt) for x in (q, k, v))
    return meta, gold, tq, tk, tv, spec, (torch.from_numpy(nbr) if nbr is not None else None), blk


def _build(meta, q, k, spec, nbr, blk):
    """The variant's _build_block_index_with_importance_optimized, called as the reference's combine calls it (K rows the
    reference's caller zeroes in place are zeroed here first, on a copy)."""
    import importlib
    mod = importlib.import_module("rectified_spaattn." + VARIANT_MODULE[meta["variant"]])
    kz = k.clone()
    kz[:, :, spec.pool_valid:] = 0
    qv = q[:, :, :spec.NBv * blk] if meta["variant"] != "wan" else q
    kw = dict(first_frame_blocks=spec.first_frame_blocks) if meta["variant"] == "wan" else dict(attenable=spec.n_txt)
    return mod._build_block_index_with_importance_optimized(
        qv, kz, meta["top_k"], blk, blk, text_start_block=spec.NBv, text_end_block=torch.tensor([spec.text_end_block]),
        num_blocks=spec.NB_total, prob_threshold=meta["p"], block_neighbor_list=nbr, **kw), kz, mod


@pytest.mark.parametrize("name", ALL_CASES)
def test_round_trip_of_the_selection_lists(name):
    from rectified_spaattn_amd import _core, block_sparse
    meta, _, q, k, v, spec, nbr, blk = _case(name)
    _, parts = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], nbr, return_parts=True)
    B, H, NQ, NK = meta["B"], meta["H"], spec.NBv, spec.NB_total
    mask = block_sparse.lists_to_block_mask(parts["bitmask"], B, H, NQ, NK)
    lists = block_sparse.block_mask_to_lists(mask, B, H)
    torch.cuda.synchronize()
    assert torch.equal(mask.bool(), _core.unpack_bitmask(parts["bitmask"], NK).view(B, H, NQ, NK))
    assert torch.equal(lists["bitmask"], parts["bitmask"])
    assert torch.equal(lists["counts"], parts["counts"])
    written = torch.arange(NK, device=DEV) < parts["counts"][..., None]     # (entries past counts are never written)
    assert torch.equal(lists["cols"][written], parts["cols"][written])


@pytest.mark.parametrize("NK", [1, 31, 33, 64, 1023, 1024, 1090, 2049, 8192])
def test_conversion_of_random_masks_against_the_host(NK):
    """Rows of every length up to K5's limit (several 1 024-key passes of the conversion kernel, partial bitmask words),
    a broadcast head axis and a strided query axis: bitmask, cols and counts as K3 would write them, and back."""
    from rectified_spaattn_amd import block_sparse
    g = torch.Generator().manual_seed(NK)
    B, H, NQ = 2, 3, 5
    base = torch.rand((B, 1, NQ, NK + 5), generator=g) < 0.3
    base[0, 0, 0] = False
    base[1, 0, 1] = True
    m = base.to(DEV)[..., 2:2 + NK]                   # (query rows NK + 5 bytes apart, heads broadcast)
    lists = block_sparse.block_mask_to_lists(m, B, H)
    torch.cuda.synchronize()
    dense = base[..., 2:2 + NK].expand(B, H, NQ, NK).reshape(B * H, NQ, NK)
    NW = (NK + 31) // 32
    bits = torch.zeros(B * H, NQ, NW * 32, dtype=torch.int64)
    bits[..., :NK] = dense.long()
    words = (bits.view(B * H, NQ, NW, 32) << torch.arange(32)).sum(-1)
    assert torch.equal(lists["bitmask"].cpu().long() & 0xFFFFFFFF, words)
    assert torch.equal(lists["counts"].cpu(), dense.sum(-1).int())
    cols = lists["cols"].cpu()
    for r in range(B * H):
        for i in range(NQ):
            want = torch.nonzero(dense[r, i]).flatten().int()
            assert torch.equal(cols[r, i, :want.numel()], want), (r, i)
    back = block_sparse.lists_to_block_mask(lists["bitmask"], B, H, NQ, NK)
    assert torch.equal(back.cpu().bool().reshape(B * H, NQ, NK), dense)


@pytest.mark.parametrize("name", ALL_CASES)
def test_builder_against_the_reference(name):
    meta, gold, q, k, v, spec, nbr, blk = _case(name)
    (one_hot, probs, nogapr), _, _ = _build(meta, q, k, spec, nbr, blk)
    torch.cuda.synchronize()
    B, H, NQ, NB = meta["B"], meta["H"], spec.NBv, spec.NB_total
    assert one_hot.dtype == torch.bool and one_hot.shape == (B, H, NQ, NB)
    assert nogapr.dtype == torch.bool and nogapr.shape == (B, H, NQ, NQ)
    assert probs.dtype == torch.float32 and probs.shape == (B, H, NQ, spec.L)
    assert np.array_equal(one_hot.cpu().numpy(), gold["one_hot"].astype(bool)), f"{name}: one_hot differs from the reference"
    assert np.array_equal(nogapr.cpu().numpy(), gold["nogapr"].astype(bool)), f"{name}: nogapr differs from the reference"
    np.testing.assert_allclose(probs.cpu().numpy(), gold["probs"].reshape(probs.shape), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("name", ALL_CASES)
def test_composition_against_the_reference_output(name):
    """one_hot, probs, nogapr -> R and comp in fp32 as the variant's combine computes them (hunyuan :346-357, wan21 :328-338),
    then _triton_block_sparse_attention_onehot(...) * R + comp on the visual rows against the reference's output."""
    meta, gold, q, k, v, spec, nbr, blk = _case(name)
    (one_hot, probs, nogapr), kz, mod = _build(meta, q, k, spec, nbr, blk)
    B, H, S, D = q.shape
    NQ, NB = spec.NBv, spec.NB_total
    vz = v.clone()
    vz[:, :, spec.pool_valid:] = 0
    width = spec.text_end_block if meta["variant"] == "wan" else NQ + 1
    part = one_hot[..., :width].clone()
    part[..., :NQ] |= nogapr
    R = (probs * part).sum(-1)
    vpad = torch.zeros(B, H, NB * blk, D, dtype=torch.float32, device=DEV)
    vpad[:, :, :S] = vz.float()
    vpool = vpad.view(B, H, NB, blk, D).mean(-2)[:, :, :width]
    comp = torch.matmul(probs.masked_fill(part, 0.0), vpool)
    seqlens = torch.full((B,), spec.kv_valid, dtype=torch.int32)
    qv = q[:, :, :NQ * blk] if meta["variant"] != "wan" else q
    o = mod._triton_block_sparse_attention_onehot(qv, kz, vz, seqlens, one_hot, D ** -0.5, blk, blk)
    n = meta.get("out_rows", S)      # (long cases keep the first out_rows rows of O, stored as fp16)
    rows = min(NQ * blk, S, n)
    got = (o.float()[:, :, :rows] * R.repeat_interleave(blk, -1)[:, :, :rows, None]
           + comp.repeat_interleave(blk, -2)[:, :, :rows]).cpu().numpy()
    want = gold["out"].astype(np.float32).reshape(B, n, H, D).transpose(0, 2, 1, 3)[:, :, :rows]
    store = (2.0 ** -11) * np.abs(want) if gold["out"].dtype == np.float16 else 0.0   # half an fp16 ulp of the stored O
    err = np.abs(got - want)
    mx, mean = TOL[torch.bfloat16]
    assert np.all(err <= mx + store) and err.mean() <= mean + np.mean(store), \
        f"{name}: max {err.max():.3e} mean {err.mean():.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
def _reference(q, k, v, mask, lens, scale, blk):
    """fp64 masked attention on the host: row r sees key j iff mask[b, h, r // blk, j // blk] and j < lens[b]; 0 without keys."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    m = mask.to(torch.bool).cpu().expand(B, H, -1, -1)
    NK = m.shape[-1]
    vis = torch.zeros(B, H, Sq, Sk, dtype=torch.bool)
    cols = m.repeat_interleave(blk, -2)[:, :, :Sq].repeat_interleave(blk, -1)[..., :Sk]
    vis[..., :min(NK * blk, Sk)] = cols[..., :min(NK * blk, Sk)]
    keys = torch.arange(Sk)
    for b in range(B):
        vis[b] &= keys < lens[b]
    s = torch.matmul(q.double().cpu(), k.double().cpu().transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx).masked_fill(~vis, 0.0)
    den = e.sum(-1, keepdim=True)
    return torch.where(den > 0, torch.matmul(e, v.double().cpu()) / den.clamp_min(1e-300), torch.zeros(()))


def _rand_mask(g, shape, density):
    m = torch.rand(shape, generator=g) < density
    m[..., 0, :] = False        # an empty row
    if shape[-2] > 2:
        m[..., 1, :] = True     # a full row
    return m


PLAIN = [
    # (name, dtype, D, block, B, H, Sq, Sk, density, options)
    ("bf16_d128_b128", torch.bfloat16, 128, 128, 2, 3, 640, 640, 0.30, {}),
    ("fp16_d128_b128_sparse", torch.float16, 128, 128, 2, 3, 900, 1000, 0.05, {}),
    ("bf16_d64_b64_dense", torch.bfloat16, 64, 64, 2, 3, 700, 700, 0.60, {}),
    ("fp16_d64_b64_ragged", torch.float16, 64, 64, 2, 3, 300, 777, 0.30, dict(kv_len=[700, 513], sm_scale=0.05)),
    ("bf16_d128_b64_ragged", torch.bfloat16, 128, 64, 2, 3, 333, 1111, 0.25, dict(kv_len=torch.tensor([1111, 1000]))),
    ("bf16_d32_b128_padded", torch.bfloat16, 32, 128, 2, 3, 500, 600, 0.40, dict(sm_scale=0.3)),
    ("fp16_d32_b64_padded", torch.float16, 32, 64, 2, 3, 256, 300, 0.40, {}),
    ("bf16_heads_broadcast", torch.bfloat16, 128, 128, 2, 3, 512, 700, 0.30, dict(mask="heads")),
    ("fp16_batch_broadcast", torch.float16, 64, 128, 2, 3, 512, 700, 0.30, dict(mask="batch")),
    ("bf16_noncontig_mask", torch.bfloat16, 128, 64, 2, 3, 400, 500, 0.30, dict(mask="strided")),
    ("bf16_transposed_mask", torch.bfloat16, 64, 128, 2, 3, 400, 500, 0.30, dict(mask="transposed")),
    ("bf16_uint8_mask", torch.bfloat16, 128, 128, 2, 3, 384, 512, 0.30, dict(mask="uint8")),
    ("bf16_bshd_views", torch.bfloat16, 128, 128, 2, 3, 600, 650, 0.30, dict(bshd=True, kv_len=600)),
    ("fp16_bshd_views_b64", torch.float16, 64, 64, 2, 3, 250, 650, 0.30, dict(bshd=True)),
    ("bf16_short_nk", torch.bfloat16, 128, 128, 2, 3, 512, 1000, 0.50, dict(nk=4)),
    ("bf16_negative_scale", torch.bfloat16, 128, 128, 2, 3, 512, 600, 0.30, dict(sm_scale=-0.07)),
    ("fp16_zero_scale_b64", torch.float16, 64, 64, 2, 3, 300, 400, 0.30, dict(sm_scale=0.0)),
]


def _plain_inputs(dt, D, blk, B, H, Sq, Sk, density, opt, seed):
    g = torch.Generator().manual_seed(seed)
    if opt.get("bshd"):
        q = torch.randn(B, Sq, H, D, generator=g).to(DEV, dt).transpose(1, 2)
        k = torch.randn(B, Sk, H, D, generator=g).to(DEV, dt).transpose(1, 2)
        v = torch.randn(B, Sk, H, D, generator=g).to(DEV, dt).transpose(1, 2)
    else:
        q, k, v = (torch.randn(B, H, s, D, generator=g).to(DEV, dt) for s in (Sq, Sk, Sk))
    NQ, NK = -(-Sq // blk), opt.get("nk", -(-Sk // blk))
    kind = opt.get("mask")
    if kind == "heads":
        m = _rand_mask(g, (B, 1, NQ, NK), density)
    elif kind == "batch":
        m = _rand_mask(g, (1, H, NQ, NK), density)
    elif kind == "strided":     # (views made on the device: a copy there would be contiguous again)
        m = _rand_mask(g, (B, H, NQ, NK + 7), density).to(DEV)[..., 3:3 + NK]
    elif kind == "transposed":
        m = (torch.rand((B, H, NK, NQ), generator=g) < density).to(DEV).transpose(-1, -2)    # key axis not contiguous
    else:
        m = _rand_mask(g, (B, H, NQ, NK), density)
    if kind == "uint8":
        m = m.to(torch.uint8) * 3
    return q, k, v, m.to(DEV)


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_attention_against_fp64(case):
    from rectified_spaattn_amd import block_sparse_attention
    name, dt, D, blk, B, H, Sq, Sk, density, opt = case
    q, k, v, m = _plain_inputs(dt, D, blk, B, H, Sq, Sk, density, opt, zlib.crc32(name.encode()))
    kw = {n: opt[n] for n in ("kv_len", "sm_scale") if n in opt}
    out = block_sparse_attention(q, k, v, m, block_size=blk, **kw)
    assert out.shape == (B, H, Sq, D) and out.dtype == dt
    kv = opt.get("kv_len")
    lens = [Sk] * B if kv is None else ([int(kv)] * B if isinstance(kv, int) else [int(x) for x in kv])
    ref = _reference(q.float(), k.float(), v.float(), m, lens, opt.get("sm_scale", D ** -0.5), blk)
    err = (out.double().cpu() - ref).abs()
    mx, mean = TOL[dt]
    assert err.max() <= mx and err.mean() <= mean, f"{name}: max {err.max():.3e} mean {err.mean():.3e}"
    if not bool(m[..., 0, :].any()):
        assert float(out.float()[:, :, :blk].abs().max()) == 0.0, "an empty mask row must give 0"


@pytest.mark.parametrize("dt,D", [(torch.bfloat16, 128), (torch.float16, 128), (torch.bfloat16, 64), (torch.float16, 64)])
def test_64_token_blocks_agree_with_the_same_mask_in_128_token_blocks(dt, D):
    """A 128-token-block mask runs the 64-rows-per-wave kernel; the same mask with every entry repeated into 2 x 2 blocks of 64
    tokens has the same visibility and runs the 32-rows-per-wave kernel's pair walk.  Both against fp64 attention, and against
    each other within one output ulp at head dim 128 and two at head dim 64 (the two kernels add the row sums in a different
    order).  48 sparse workgroups: no tail split, so no block's summation order depends on the grid."""
    from rectified_spaattn_amd import block_sparse_attention
    B, H, Sq, Sk, kv_len = 2, 3, 900, 1000, [1000, 777]
    q, k, v, m = _plain_inputs(dt, D, 128, B, H, Sq, Sk, 0.3, {}, 64 + D)
    m64 = m.repeat_interleave(2, -2)[..., :-(-Sq // 64), :].repeat_interleave(2, -1)[..., :-(-Sk // 64)]
    ref = _reference(q.float(), k.float(), v.float(), m, kv_len, D ** -0.5, 128)
    outs = [block_sparse_attention(q, k, v, m, kv_len=kv_len, block_size=128),
            block_sparse_attention(q, k, v, m64, kv_len=kv_len, block_size=64)]
    mx, mean = TOL[dt]
    for blk, out in zip((128, 64), outs):
        err = (out.double().cpu() - ref).abs()
        assert err.max() <= mx and err.mean() <= mean, f"block {blk}: max {err.max():.3e} mean {err.mean():.3e}"
    ulp = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    dist = float((outs[0].double() - outs[1].double()).abs().max())
    bound = (1 if D == 128 else 2) * ulp * max(1.0, float(ref.abs().max()))
    assert dist <= bound, f"between the kernels: {dist:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("blk", [64, 128])
def test_rows_without_a_visible_key_are_exactly_zero(blk):
    from rectified_spaattn_amd import block_sparse_attention
    g = torch.Generator().manual_seed(7)
    B, H, S, D = 2, 2, 8 * blk, 128
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(DEV, torch.bfloat16) for _ in range(3))
    m = torch.zeros(B, H, 8, 8, dtype=torch.bool)
    m[:, :, 1, 0] = True          # row block 1 sees key block 0 only
    m[:, :, 2, 5:] = True         # row block 2 sees key blocks 5..7 only: beyond kv_len = 3 blocks for batch item 0
    m[:, :, 3, :] = True
    out = block_sparse_attention(q, k, v, m.to(DEV), kv_len=[3 * blk, S], block_size=blk).float().cpu()
    assert float(out[:, :, 0:blk].abs().max()) == 0.0                        # no kept block
    assert float(out[0, :, 2 * blk:3 * blk].abs().max()) == 0.0              # every kept key beyond kv_len
    assert float(out[1, :, 2 * blk:3 * blk].abs().max()) > 0.0
    assert float(out[:, :, 4 * blk:].abs().max()) == 0.0
    z = block_sparse_attention(q, k, v, m.to(DEV), kv_len=[0, S], block_size=blk).float().cpu()   # no key at all for item 0
    assert float(z[0].abs().max()) == 0.0 and torch.equal(z[1], out[1])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("blk,D", [(128, 128), (64, 64), (128, 64), (64, 128)])
def test_all_ones_mask_equals_flash_fullattn(dt, blk, D):
    from rectified_spaattn_amd import block_sparse_attention
    from rectified_spaattn_amd.attn import fullattn
    g = torch.Generator().manual_seed(blk + D)
    B, H, Sq, Sk = 2, 3, 1000, 1100
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, dt)
    k, v = (torch.randn(B, H, Sk, D, generator=g).to(DEV, dt) for _ in range(2))
    m = torch.ones(1, 1, -(-Sq // blk), -(-Sk // blk), dtype=torch.bool, device=DEV)
    out = block_sparse_attention(q, k, v, m, block_size=blk).float()
    ref = fullattn(q, k, v, mode="flash").float()
    err = (out - ref).abs()
    mx, mean = TOL[dt]
    assert float(err.max()) <= mx and float(err.mean()) <= mean


def test_two_identical_calls_give_the_same_bytes():
    from rectified_spaattn_amd import block_sparse_attention
    g = torch.Generator().manual_seed(11)
    B, H, S, D = 2, 3, 1500, 128
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(DEV, torch.bfloat16) for _ in range(3))
    m = (torch.rand(B, H, 12, 12, generator=g) < 0.3).to(DEV)
    a = block_sparse_attention(q, k, v, m, kv_len=[1400, 1500])
    b = block_sparse_attention(q, k, v, m, kv_len=[1400, 1500])
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_hunyuan_720p_launch_with_the_selections_own_mask():
    """One launch at the HunyuanVideo 720p geometry (900 x 902 blocks) on 3 heads, the mask = the selection's own at top_k 90."""
    import bench
    from rectified_spaattn_amd import block_sparse_attention
    from rectified_spaattn_amd.rectified_hunyuan_attn import _build_block_index_with_importance_optimized
    wl = bench.WORKLOADS["hunyuan_720p_128f"]
    spec = bench.make_spec(wl)
    q, k, v = bench.gen_inputs(wl, 3, 0, DEV, "iid")
    k = k.clone()
    v = v.clone()
    k[:, :, spec.pool_valid:] = 0
    v[:, :, spec.pool_valid:] = 0
    NQ, NB, b = spec.NBv, spec.NB_total, 128
    one_hot, _, _ = _build_block_index_with_importance_optimized(
        q[:, :, :NQ * b], k, 90, b, b, text_start_block=NQ, text_end_block=spec.text_end_block, num_blocks=NB,
        prob_threshold=0.0, attenable=spec.n_txt)
    assert one_hot.shape == (1, 3, NQ, NB)
    out = block_sparse_attention(q[:, :, :NQ * b], k, v, one_hot, kv_len=spec.kv_valid)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    mx, mean = TOL[torch.bfloat16]
    for h in range(3):
        for i in (0, 451, NQ - 1):
            rows = slice(i * b, (i + 1) * b)
            ref = _reference(q[:, h:h + 1, rows].float(), k[:, h:h + 1].float(), v[:, h:h + 1].float(),
                             one_hot[:, h:h + 1, i:i + 1], [spec.kv_valid], 128 ** -0.5, b)
            err = (out[:, h:h + 1, rows].double().cpu() - ref).abs()
            assert err.max() <= mx and err.mean() <= mean, (h, i, float(err.max()), float(err.mean()))
