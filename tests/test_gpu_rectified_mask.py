"""Rectified attention over a caller's block mask on the MI355X: the selection's own mask gives the rectified call byte for byte,
arbitrary masks against the fp64 oracle with R and w restated in the contract's order, edited selections against the reference's
torch composition, and the edges (empty rows, padded head dims, graph capture, the headline size)."""
import ctypes
import dataclasses
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
PART_NAMES = ("probs", "w", "R", "comp", "bitmask", "counts")


def _case(name, dt=torch.bfloat16):
    """(meta, q, k, v on the device, LayoutSpec, neighbour matrix or None, block) of a golden operator case."""
    from rectified_spaattn_amd import _core, synth
    meta, _ = load_op_case(name)
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
    return meta, tq, tk, tv, spec, (torch.from_numpy(nbr) if nbr is not None else None), blk


def _masked(q, k, v, spec, mask, **kw):
    """The masked call through _core (first_frame_blocks is a selection rule: the mask replaces it)."""
    from rectified_spaattn_amd import _core
    return _core.rectified_attention(q, k, v, dataclasses.replace(spec, first_frame_blocks=0), 0, 0.0, None,
                                     return_parts=True, block_mask=mask, **kw)


def _assert_same_call(a, b, NK, what):
    (oa, pa), (ob, pb) = a, b
    assert torch.equal(oa.view(torch.int16), ob.view(torch.int16)), f"{what}: O differs"
    for n in PART_NAMES:
        assert torch.equal(pa[n], pb[n]), f"{what}: {n} differs"
    written = torch.arange(NK, device=DEV) < pa["counts"][..., None]
    assert torch.equal(pa["cols"][written], pb["cols"][written]), f"{what}: cols differ"


# ---- 1. the selection's own mask: the rectified call, byte for byte -----------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ALL_CASES)
def test_own_mask_gives_the_rectified_call_byte_for_byte(name, dt):
    from rectified_spaattn_amd import _core, block_sparse
    meta, q, k, v, spec, nbr, blk = _case(name, dt)
    B, H = meta["B"], meta["H"]
    fp8s = [False, True, "pv"] if blk == 128 else [False]
    for fp8 in fp8s:
        ref = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], nbr, return_parts=True, qkv_fp8=fp8)
        mask = block_sparse.lists_to_block_mask(ref[1]["bitmask"], B, H, spec.NBv, spec.NB_total)
        got = _masked(q, k, v, spec, mask.view(torch.bool), qkv_fp8=fp8)
        torch.cuda.synchronize()
        _assert_same_call(ref, got, spec.NB_total, f"{name} qkv_fp8={fp8}")


@pytest.mark.parametrize("name", ["hunyuan_1280", "b64_flux_1536"])
def test_the_one_call_entry_gives_the_staged_call(name):
    """rsa_rectified_attention_masked(_ex) in one caller-provided workspace: the same bytes as the staged Python call."""
    from rectified_spaattn_amd import _core, _lib, block_sparse
    from rectified_spaattn_amd._lib import RsaOut4
    meta, q, k, v, spec, nbr, blk = _case(name)
    B, H, S, D = q.shape
    sel = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], nbr, return_parts=True)[1]
    mask = block_sparse.lists_to_block_mask(sel["bitmask"], B, H, spec.NBv, spec.NB_total)
    want, _ = _masked(q, k, v, spec, mask)
    L = _lib.lib()
    lay = spec.to_c_ex(B, H, D, q.dtype)
    sizes, total = (ctypes.c_size_t * _lib.NUM_BUFFERS)(), ctypes.c_size_t()
    _lib.check(L.rsa_buffer_bytes_ex(ctypes.byref(lay), ctypes.byref(sizes), ctypes.byref(total)), "rsa_buffer_bytes_ex")
    ws = torch.empty(total.value, dtype=torch.uint8, device=DEV)
    out = torch.empty((B, S, H, D), dtype=q.dtype, device=DEV)
    o4 = RsaOut4(out.data_ptr(), out.stride(0), out.stride(2), out.stride(1))
    _lib.check(L.rsa_rectified_attention_masked_ex(ctypes.byref(lay), _core._t4(q), _core._t4(k), _core._t4(v), mask.data_ptr(),
                                                   mask.stride(0), mask.stride(1), mask.stride(2), ws.data_ptr(), ws.numel(), o4,
                                                   _core._stream()), "rsa_rectified_attention_masked_ex")
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, S, H * D).view(torch.int16), want.view(torch.int16))


# ---- 2. arbitrary masks against the oracle (128-token blocks) ------------------------------------------------------------
def _c6_sum(x: np.ndarray) -> np.float32:
    """Contract C6 on the host: 256 strided fp32 partial sums (element j -> partial j % 256, sequential in j), pairwise tree."""
    n = -(-x.size // 256) * 256
    rows = np.zeros(n, np.float32)
    rows[:x.size] = x
    part = np.zeros(256, np.float32)
    for r in rows.reshape(-1, 256):
        part = part + r
    s = 1
    while s < 256:
        part[0::2 * s] = part[0::2 * s] + part[s::2 * s]
        s *= 2
    return part[0]


def _mask_for(kind, g, B, H, NQ, NK, nqv):
    """(device mask as the caller hands it over, its dense bool [B, H, NQ, NK] value on the host)."""
    def rnd(shape, density=0.3):
        m = torch.rand(shape, generator=g) < density
        m[..., 0, :] = False            # an empty row
        m[..., 1, :] = True             # a full row
        m[..., 2, :nqv] = False         # a row that keeps text blocks only (or nothing: wan)
        return m
    if kind == "random":
        m = rnd((B, H, NQ, NK))
        return m.to(DEV), m
    if kind == "no_text_column":
        m = rnd((B, H, NQ, NK))
        m[..., nqv:] = False
        return m.to(DEV), m
    if kind == "batch_broadcast":
        m = rnd((1, H, NQ, NK))
        return m.to(DEV), m.expand(B, H, NQ, NK)
    if kind == "head_broadcast":
        m = rnd((B, 1, NQ, NK))
        return m.to(DEV), m.expand(B, H, NQ, NK)
    if kind == "uint8_values":
        m = rnd((B, H, NQ, NK))
        vals = torch.randint(1, 256, (B, H, NQ, NK), generator=g, dtype=torch.int32).to(torch.uint8)
        return (m.to(torch.uint8) * vals).to(DEV), m
    if kind == "sliced":               # a view of a wider device tensor: query rows NK + 9 bytes apart
        m = rnd((B, H, NQ, NK + 9))
        return m.to(DEV)[..., 4:4 + NK], m[..., 4:4 + NK]
    if kind == "transposed":           # key axis not contiguous (copied on the host side)
        m = rnd((B, H, NQ, NK))
        return m.transpose(-1, -2).contiguous().to(DEV).transpose(-1, -2), m
    raise ValueError(kind)


ORACLE_CASES = [("hunyuan_1280", "random"), ("hunyuan_1280", "no_text_column"), ("b2_hunyuan_1280", "batch_broadcast"),
                ("b2_flux_1280", "head_broadcast"), ("b2_cogvideo_994", "random"), ("flux_1536", "uint8_values"),
                ("wan_pad_1450", "sliced"), ("wan_d64_1100", "transposed"), ("cogvideo_994", "no_text_column")]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,kind", ORACLE_CASES, ids=[f"{a}-{b}" for a, b in ORACLE_CASES])
def test_arbitrary_masks_against_the_oracle(name, kind, dt):
    from oracle import oracle as orc
    from rectified_spaattn_amd import _core, block_sparse
    meta, _ = load_op_case(name)
    qn, kn, vn, lay, nbr = case_inputs(meta)
    _, q, k, v, spec, tnbr, blk = _case(name, dt)
    B, H, S, D = q.shape
    NQ, NK, L = spec.NBv, spec.NB_total, spec.L
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{kind}".encode()))
    dmask, mask = _mask_for(kind, g, B, H, NQ, NK, NQ)
    out, parts = _masked(q, k, v, spec, dmask)
    rect = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], tnbr, return_parts=True)[1]
    lists = block_sparse.block_mask_to_lists(mask.to(DEV), B, H)
    torch.cuda.synchronize()
    assert torch.equal(parts["probs"], rect["probs"]), "probs differ from the rectified call's"
    for n in ("bitmask", "counts"):
        assert torch.equal(parts[n], lists[n]), n
    written = torch.arange(NK, device=DEV) < lists["counts"][..., None]
    assert torch.equal(parts["cols"][written], lists["cols"][written])
    assert bool(torch.isfinite(out.float()).all())
    # the reference, one head at a time, with the inputs rounded to dt as the device saw them
    rnd = orc.round_bf16 if dt == torch.bfloat16 else orc.round_fp16
    qn, kn, vn = rnd(qn), rnd(kn), rnd(vn)
    got = out.float().cpu().numpy().reshape(B, S, H, D)
    R_dev, w_dev = parts["R"].cpu().numpy(), parts["w"].cpu().numpy()
    mx, mean = TOL[dt]
    m_np = mask.numpy()
    err_all = []
    for b in range(B):
        for h in range(H):
            bh = b * H + h
            qq, kk, vv = qn[b, h], kn[b, h].copy(), vn[b, h].copy()
            kk[lay.pool_valid:] = 0
            vv[lay.pool_valid:] = 0
            sel = orc.select_head(qq, kk, vv, lay, meta["top_k"], meta["p"], nbr)
            kept = m_np[b, h].astype(np.uint8)
            M = kept[:, :L].astype(bool).copy()
            M[:, :NQ] |= sel["unrel"].astype(bool)
            for i in range(NQ):
                want_R = _c6_sum(np.where(M[i], sel["probs"][i], np.float32(0)))
                assert R_dev[bh, i].view(np.uint32) == want_R.view(np.uint32), (b, h, i, R_dev[bh, i], want_R)
            want_w = np.where(M, np.float32(0), sel["probs"])
            assert np.array_equal(w_dev[bh].view(np.uint32), want_w.view(np.uint32)), (b, h)
            sp = orc.sparse_attention_head(qq, kk, vv, lay, kept, list(range(NQ)))
            sp = np.nan_to_num(sp, nan=0.0)           # rows without a visible key: the sparse term is 0 (the reference: NaN)
            comp = want_w.astype(np.float64) @ sel["stats"].vbar[:L].astype(np.float64)
            o = sp * parts["R"][bh].cpu().numpy().astype(np.float64)[:, None, None] + comp[:, None, :]
            o = o.reshape(-1, D)[:min(S, NQ * blk)]
            ref = np.zeros((S, D))
            ref[:o.shape[0]] = o
            if lay.q_text_valid > 0:
                r0 = NQ * blk
                ref[r0:r0 + lay.q_text_valid] = orc.dense_attention(qq[r0:r0 + lay.q_text_valid], kk, vv, lay.kv_text_valid)
            err_all.append(np.abs(got[b, :, h] - ref))
    err = np.stack(err_all)
    assert err.max() <= mx and err.mean() <= mean, f"max {err.max():.3e} mean {err.mean():.3e}"


# ---- 3. edited selections against the reference's torch composition ------------------------------------------------------
VARIANT_MODULE = dict(hunyuan="rectified_hunyuan_attn", flux="rectified_flux_attn", cogvideo="rectified_cogvideo_attn",
                      wan="rectified_wan21_attn")
EDIT_CASES = ["hunyuan_1280", "flux_1536", "cogvideo_994", "wan_pad_1450", "b2_hunyuan_1280", "b64_hunyuan_1280",
              "b64_flux_1536", "b64_cogvideo_1058", "b64_wan_pad_1450", "b64_b2_hunyuan_1280"]


def _variant_call(mod, meta, spec, q, k, v, blk, mask):
    """The variant's public function with block_mask, given the geometry the way each variant takes it."""
    S = q.shape[2]
    kw = dict(block_size_M=blk, block_size_N=blk, block_mask=mask)
    if meta["variant"] == "hunyuan":
        cu = [0, meta["num_true"], S]
        kw.update(cu_seqlens_q=cu, cu_seqlens_kv=cu)
    elif meta["variant"] in ("flux", "cogvideo"):
        kw.update(text_length=meta["text_length"])
    return mod.rectified_block_sparse_attention(q, k, v, None, None, p_remain_rates=None, **kw)


@pytest.mark.parametrize("edit", ["no_neighbours", "band", "no_text_column"])
@pytest.mark.parametrize("name", EDIT_CASES)
def test_edited_selections_against_the_reference_composition(name, edit):
    import importlib
    from rectified_spaattn_amd import _core
    meta, q, k, v, spec, nbr, blk = _case(name)
    mod = importlib.import_module("rectified_spaattn_amd." + VARIANT_MODULE[meta["variant"]])
    B, H, S, D = q.shape
    NQ, NB = spec.NBv, spec.NB_total
    kz, vz = k.clone(), v.clone()
    kz[:, :, spec.pool_valid:] = 0
    vz[:, :, spec.pool_valid:] = 0
    qv = q[:, :, :NQ * blk] if meta["variant"] != "wan" else q
    kw = dict(first_frame_blocks=spec.first_frame_blocks) if meta["variant"] == "wan" else dict(attenable=spec.n_txt)
    one_hot, probs, nogapr = mod._build_block_index_with_importance_optimized(
        qv, kz, meta["top_k"], blk, blk, text_start_block=NQ, text_end_block=torch.tensor([spec.text_end_block]),
        num_blocks=NB, prob_threshold=meta["p"], block_neighbor_list=nbr, **kw)
    m = one_hot.clone()
    if nbr is not None:
        m[..., :NQ] &= ~nbr[:NQ, :NQ].to(DEV, torch.bool)
    if edit == "band":
        i = torch.arange(NQ, device=DEV)
        m[..., :NQ] |= (i[:, None] - i[None, :]).abs() <= 2
    elif edit == "no_text_column" and meta["variant"] != "wan":
        m[..., NQ] = False
    out = _variant_call(mod, meta, spec, q, k, v, blk, m)
    rect = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], nbr)
    # the composition of test_gpu_block_mask.py::test_composition_against_the_reference_output, on the edited mask
    width = spec.text_end_block if meta["variant"] == "wan" else NQ + 1
    part = m[..., :width].clone()
    part[..., :NQ] |= nogapr
    R = (probs * part).sum(-1)
    vpad = torch.zeros(B, H, NB * blk, D, dtype=torch.float32, device=DEV)
    vpad[:, :, :S] = vz.float()
    vpool = vpad.view(B, H, NB, blk, D).mean(-2)[:, :, :width]
    comp = torch.matmul(probs.masked_fill(part, 0.0), vpool)
    seqlens = torch.full((B,), spec.kv_valid, dtype=torch.int32)
    o = mod._triton_block_sparse_attention_onehot(qv, kz, vz, seqlens, m, D ** -0.5, blk, blk)
    rows = min(NQ * blk, S)
    want = o.float()[:, :, :rows] * R.repeat_interleave(blk, -1)[:, :, :rows, None] + comp.repeat_interleave(blk, -2)[:, :, :rows]
    got = out.view(B, S, H, D).transpose(1, 2).float()
    torch.cuda.synchronize()
    err = (got[:, :, :rows] - want).abs()
    mx, mean = TOL[torch.bfloat16]
    assert float(err.max()) <= mx and float(err.mean()) <= mean, f"max {float(err.max()):.3e} mean {float(err.mean()):.3e}"
    # text rows are dense over the valid keys: the rectified call's, whatever the mask
    assert torch.equal(out.view(B, S, H * D)[:, rows:].view(torch.int16), rect[:, rows:].view(torch.int16))


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blk", [128, 64])
def test_an_empty_visual_row_comes_out_as_comp(blk):
    from rectified_spaattn_amd import _core, synth
    B, H, S, D = 1, 2, 12 * 128 + 256, 128
    q, k, v = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(5, B, H, S, D))
    spec = _core.LayoutSpec.hunyuan(S, S - 40, block=blk)
    g = torch.Generator().manual_seed(blk)
    m = torch.rand(B, H, spec.NBv, spec.NB_total, generator=g) < 0.4
    m[:, :, 3] = False                                  # no kept block
    m[:, 1, 5] = False
    m[:, 1, 5, spec.NB_total - 1] = True                # only the last text block: every key of it at or past kv_valid
    out, parts = _masked(q, k, v, spec, m.to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    o = out.view(B, S, H, D)
    comp = parts["comp"].view(B, H, spec.NBv, D)
    for h, i in [(0, 3), (1, 3), (1, 5)]:
        rows = o[0, i * blk:(i + 1) * blk, h].float()
        want = comp[0, h, i].to(torch.bfloat16).float().expand_as(rows)
        assert torch.allclose(rows, want, rtol=2 ** -8, atol=1e-7), (h, i, float((rows - want).abs().max()))


@pytest.mark.parametrize("D,variant", [(16, "hunyuan"), (32, "wan"), (64, "cogvideo")])
def test_padded_and_small_head_dims_give_the_rectified_call(D, variant):
    from rectified_spaattn_amd import _core, block_sparse, synth
    B, H = 1, 2
    if variant == "hunyuan":
        S = 10 * 128 + 256
        spec = _core.LayoutSpec.hunyuan(S, S - 30)
    elif variant == "cogvideo":
        S = 9 * 128 + 226
        spec = _core.LayoutSpec.cogvideo(S, 226)
    else:
        S = 1100
        spec = _core.LayoutSpec.wan(S)
    q, k, v = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(D, B, H, S, D))
    nbr = torch.from_numpy(synth.banded_neighbors(spec.NBv, 1))
    ref = _core.rectified_attention(q, k, v, spec, 3, 0.3, nbr, return_parts=True)
    mask = block_sparse.lists_to_block_mask(ref[1]["bitmask"], B, H, spec.NBv, spec.NB_total)
    got = _masked(q, k, v, spec, mask)
    torch.cuda.synchronize()
    _assert_same_call(ref, got, spec.NB_total, f"D={D}")


def test_two_identical_calls_give_the_same_bytes():
    from rectified_spaattn_amd import _core, synth
    B, H, S, D = 2, 2, 1450, 128
    q, k, v = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(3, B, H, S, D))
    spec = _core.LayoutSpec.wan(S)
    g = torch.Generator().manual_seed(3)
    m = (torch.rand(B, H, spec.NBv, spec.NB_total, generator=g) < 0.3).to(DEV)
    a, pa = _masked(q, k, v, spec, m)
    b, pb = _masked(q, k, v, spec, m)
    torch.cuda.synchronize()
    _assert_same_call((a, pa), (b, pb), spec.NB_total, "second call")


def test_hip_graph_capture_and_replay_with_a_mask():
    """The masked call captured into a HIP graph: no allocation, no synchronisation; the replay on new inputs and a new mask (both
    written in place) gives the eager call's bytes."""
    from rectified_spaattn_amd import _core, synth
    qa, ka, va = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(31, 1, 2, 1024, 128))
    qb, kb, vb = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(32, 1, 2, 1024, 128))
    spec = _core.LayoutSpec.wan(1024)
    g = torch.Generator().manual_seed(4)
    ma, mb = ((torch.rand(1, 2, 8, 8, generator=g) < 0.4).to(DEV) for _ in range(2))
    q, k, v, m = qa.clone(), ka.clone(), va.clone(), ma.clone()
    call = _core.StagedCall(q, k, v, spec, 0, 0.0, None, block_mask=m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call.select(); call.attend()   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.select()
        call.attend()
    q.copy_(qb); k.copy_(kb); v.copy_(vb); m.copy_(mb)
    graph.replay()
    torch.cuda.synchronize()
    eager = _core.rectified_attention(qb, kb, vb, spec, 0, 0.0, None, block_mask=mb)
    assert torch.equal(call.out.view(1, 1024, 256).view(torch.int16), eager.view(torch.int16))


# ---- 5. the headline size --------------------------------------------------------------------------------------------------
def test_headline_size_own_mask_gives_the_rectified_call():
    """HunyuanVideo 720p, 24 heads (the bench's inputs, made on the device), top_k 90: one rectified launch, one masked launch
    on its own mask, byte for byte."""
    import bench
    from rectified_spaattn_amd import _core, block_sparse
    wl = bench.WORKLOADS["hunyuan_720p_128f"]
    spec = bench.make_spec(wl)
    q, k, v = bench.gen_inputs(wl, 24, 0, DEV, "iid")
    ref = _core.StagedCall(q, k, v, spec, 90, 0.0, None)
    ref.select()
    ref.attend()
    mask = block_sparse.lists_to_block_mask(ref.bufs["bitmask"], 1, 24, spec.NBv, spec.NB_total)
    got = _core.StagedCall(q, k, v, spec, 0, 0.0, None, block_mask=mask)
    got.select()
    got.attend()
    torch.cuda.synchronize()
    assert torch.equal(ref.out.view(torch.int16), got.out.view(torch.int16))
    for n in ("probs", "w", "R", "comp", "bitmask", "counts"):
        assert torch.equal(ref.bufs[n], got.bufs[n]), n
