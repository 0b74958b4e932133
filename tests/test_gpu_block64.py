"""64-token blocks (block_size_M = block_size_N = 64) on the MI355X, against the reference operator's own runs
(tests/golden/op_b64_*.npz, gapr_b64.npz: make_golden_block64.py) and, beyond the fixtures' sizes, against an fp64
restatement of K5 built from the call's own lists, R and comp."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import load_op_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B64_CASES = ["b64_wan_pad_1450", "b64_hunyuan_1280", "b64_flux_1536", "b64_cogvideo_1058", "b64_wan_d64_1100",
             "b64_b2_hunyuan_1280", "b64_big_wan_16640"]
TOL = {torch.bfloat16: (2e-2, 2e-3), torch.float16: (2e-3, 2e-4)}
DEV = torch.device("cuda:0")


def _inputs(meta, dt):
    from rectified_spaattn_amd import synth
    q, k, v = synth.structured_qkv(meta["seed"], meta["B"], meta["H"], meta["S"], meta["D"], block=64)
    return tuple(torch.from_numpy(x).to(DEV, dt) for x in (q, k, v))


def _spec(meta):
    from rectified_spaattn_amd import _core
    var, S = meta["variant"], meta["S"]
    if var == "hunyuan":
        return _core.LayoutSpec.hunyuan(S, meta["num_true"], block=64)
    if var == "flux":
        return _core.LayoutSpec.flux(S, meta["text_length"], block=64)
    if var == "cogvideo":
        return _core.LayoutSpec.cogvideo(S, meta["text_length"], block=64)
    return _core.LayoutSpec.wan(S, meta.get("ffb", 0), block=64)


def _public(meta, q, k, v, nbr, **kw):
    """The variant's public rectified_block_sparse_attention with 64-token blocks."""
    from rectified_spaattn_amd import (rectified_cogvideo_attn, rectified_flux_attn, rectified_hunyuan_attn,
                                       rectified_wan21_attn)
    var, S = meta["variant"], meta["S"]
    args = dict(top_k=meta["top_k"], block_size_M=64, block_size_N=64, block_neighbor_list=nbr,
                p_remain_rates=meta["p"], **kw)
    if var == "hunyuan":
        cu = [0, meta["num_true"], S]
        return rectified_hunyuan_attn.rectified_block_sparse_attention(q, k, v, None, cu_seqlens_q=cu, cu_seqlens_kv=cu, **args)
    if var == "flux":
        return rectified_flux_attn.rectified_block_sparse_attention(q, k, v, None, text_length=meta["text_length"], **args)
    if var == "cogvideo":
        return rectified_cogvideo_attn.rectified_block_sparse_attention(q, k, v, None, text_length=meta["text_length"],
                                                                        **args)
    return rectified_wan21_attn.rectified_block_sparse_attention(q, k, v, None, first_frame_blocks=meta.get("ffb", 0),
                                                                 **args)


def _nbr(meta):
    from rectified_spaattn_amd import synth
    return torch.from_numpy(synth.banded_neighbors(meta["NBv"], meta["nb_width"])) if meta["nb_width"] >= 0 else None


@pytest.mark.parametrize("name", B64_CASES)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_block64_against_reference(name, dt):
    from rectified_spaattn_amd import _core
    meta, gold = load_op_case(name)
    q, k, v = _inputs(meta, dt)
    spec = _spec(meta)
    nbr = _nbr(meta)
    out, parts = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], nbr, return_parts=True)
    pub = _public(meta, q, k, v, nbr)
    torch.cuda.synchronize()
    assert torch.equal(out, pub), f"{name}: the public entry point and the staged call differ"
    B, H, NBv, NB = meta["B"], meta["H"], spec.NBv, spec.NB_total
    kept = _core.unpack_bitmask(parts["bitmask"], NB).cpu().numpy().reshape(B, H, NBv, NB)
    assert np.array_equal(kept, gold["one_hot"].astype(bool)), f"{name}: block mask differs from the reference"
    assert np.array_equal(parts["unrel"].cpu().numpy().reshape(B, H, NBv, NBv), gold["nogapr"]), f"{name}: GAPR mask"
    np.testing.assert_allclose(parts["probs"].cpu().numpy().reshape(gold["probs"].shape), gold["probs"], rtol=2e-5, atol=1e-6)
    # kept lists = the mask's set bits, ascending
    cols, counts = parts["cols"].cpu().numpy(), parts["counts"].cpu().numpy()
    km = kept.reshape(B * H, NBv, NB)
    for bh in range(B * H):
        for i in range(NBv):
            assert np.array_equal(cols[bh, i, : counts[bh, i]], np.nonzero(km[bh, i])[0])
    n = meta.get("out_rows", meta["S"])    # (long cases keep the first out_rows rows of O)
    o = out.float().cpu().numpy().reshape(B, meta["S"], -1)[:, :n]
    ref = gold["out"].astype(np.float32).reshape(B, n, -1)
    rows = np.ones((B, n), bool)
    if B > 1:   # the reference's text-row flash call describes batch item 0 only (conftest.reference_rows)
        rows[1:, NBv * 64:] = False
    mx, mean = TOL[dt]
    # long cases store the reference O as fp16: its rounding (half an ulp, 2^-11 |O|) is added to the parity bound
    store = (2.0 ** -11) * np.abs(ref)[rows] if gold["out"].dtype == np.float16 else 0.0
    err = np.abs(o - ref)[rows]
    assert np.all(err <= mx + store) and err.mean() <= mean + np.mean(store), \
        f"{name} {dt}: max {err.max():.3e} mean {err.mean():.3e}"


def test_estimate_pr_gain_block64():
    from rectified_spaattn_amd import gapr_mask, synth
    z = np.load(os.path.join(GOLDEN, "gapr_b64.npz"))
    q, k, _ = synth.structured_qkv(int(z["seed"]), 1, 2, 1024, 128, block=64)
    Qb = torch.from_numpy(q).reshape(1, 2, 16, 64, 128).to(DEV, torch.bfloat16)
    Kb = torch.from_numpy(k).reshape(1, 2, 16, 64, 128).to(DEV, torch.bfloat16)
    g = gapr_mask.estimate_pr_gain(Qb, Kb, torch.from_numpy(z["q_pools"]).to(DEV), torch.from_numpy(z["k_pools"]).to(DEV),
                                   torch.from_numpy(z["scores"]).to(DEV))
    shape = tuple(z["shape"])
    want = np.unpackbits(z["mask"], axis=-1)[..., : shape[-1]].astype(bool)
    assert np.array_equal(g.cpu().numpy(), want)


def _dense_masked_restatement(q, k, v, parts, spec, bh):
    """fp64 K5 of one head from the call's own kept lists, R and comp: visual rows attend their kept 64-key blocks (keys
    < kv_valid), O = softmax(...) V * R + comp; text rows attend keys < kv_text_valid."""
    S, NBv, b = spec.S, spec.NBv, spec.block
    qh, kh, vh = (x[bh].double() for x in (q, k, v))
    D = qh.shape[-1]
    sc = (qh @ kh.T) * D ** -0.5
    keep = torch.zeros(S, S, dtype=torch.bool, device=q.device)
    cols, counts = parts["cols"][bh], parts["counts"][bh]
    col_ok = torch.arange(S, device=q.device)
    for i in range(NBv):
        blocks = cols[i, : int(counts[i])].long()
        km = torch.zeros(spec.NB_total, dtype=torch.bool, device=q.device)
        km[blocks] = True
        keep[i * b:(i + 1) * b] = km.repeat_interleave(b)[:S] & (col_ok < spec.kv_valid)
    keep[NBv * b:] = col_ok < spec.kv_text_valid
    p = torch.softmax(sc.masked_fill(~keep, float("-inf")), -1)
    o = p @ vh
    R, comp = parts["R"][bh].double(), parts["comp"][bh].double()
    nv = min(NBv * b, S)
    o[:nv] = o[:nv] * R.repeat_interleave(b)[:nv, None] + comp.repeat_interleave(b, 0)[:nv]
    o[NBv * b + spec.q_text_valid:] = 0
    return o


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_block64_k5_large_against_dense_restatement(dt):
    """About 33k tokens, 4 heads (Hunyuan layout: text rows included; 516 blocks per row): K5 against fp64."""
    from rectified_spaattn_amd import _core, synth
    B, H, S, D = 1, 4, 33024, 128
    num_true = S - 56
    q, k, v = (torch.from_numpy(x).to(DEV, dt) for x in synth.structured_qkv(31, B, H, S, D, block=64))
    spec = _core.LayoutSpec.hunyuan(S, num_true, block=64)
    nbr = torch.from_numpy(synth.banded_neighbors(spec.NBv, 2))
    out, parts = _core.rectified_attention(q, k, v, spec, 40, 0.3, nbr, return_parts=True, shape_xfuse=True)
    torch.cuda.synchronize()
    mx, mean = TOL[dt]
    for bh in range(B * H):
        ref = _dense_masked_restatement(q[0], k[0], v[0], parts, spec, bh)
        err = (out[0, :, bh].double() - ref).abs()
        assert float(err.max()) <= mx and float(err.mean()) <= mean, f"head {bh}: {float(err.max()):.3e} {float(err.mean()):.3e}"


def test_block64_shard_invariance():
    """set_shard_invariant(True): a 2-head slice of an 8-head call gives the same bytes at block 64."""
    from rectified_spaattn_amd import _core, _lib, synth
    B, H, S, D = 1, 8, 8448, 128
    q, k, v = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(5, B, H, S, D, block=64))
    spec = _core.LayoutSpec.hunyuan(S, S - 40, block=64)
    nbr = torch.from_numpy(synth.banded_neighbors(spec.NBv, 1))
    L = _lib.lib()
    prev = L.rsa_set_shard_invariant(1)
    try:
        full, pf = _core.rectified_attention(q, k, v, spec, 6, 0.3, nbr, return_parts=True, shape_xfuse=True)
        sl = slice(4, 6)
        part, pp = _core.rectified_attention(q[:, sl], k[:, sl], v[:, sl], spec, 6, 0.3, nbr, return_parts=True,
                                             shape_xfuse=True)
        torch.cuda.synchronize()
    finally:
        L.rsa_set_shard_invariant(prev)
    assert torch.equal(full[:, :, sl], part)
    for n in ("bitmask", "counts", "R", "comp"):
        assert torch.equal(pf[n][4:6], pp[n]), n
    cnt = pp["counts"]
    valid = torch.arange(spec.NB_total, device=DEV)[None, None, :] < cnt[..., None]   # (entries past counts are not written)
    assert torch.equal(pf["cols"][4:6][valid], pp["cols"][valid])


def test_block64_graph_replay_matches_eager():
    from rectified_spaattn_amd import _core, synth
    B, H, S, D = 1, 2, 4096, 128
    q, k, v = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(8, B, H, S, D, block=64))
    spec = _core.LayoutSpec.wan(S, 2, block=64)
    nbr = torch.from_numpy(synth.banded_neighbors(spec.NBv, 1))
    eager = _core.rectified_attention(q, k, v, spec, 5, 0.3, nbr)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _core.rectified_attention(q, k, v, spec, 5, 0.3, nbr)    # warm-up (device copy of the neighbours)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cap = _core.rectified_attention(q, k, v, spec, 5, 0.3, nbr)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager)


def test_block64_onecall_matches_staged():
    from rectified_spaattn_amd import _core
    meta, _ = load_op_case("b64_flux_1536")
    q, k, v = _inputs(meta, torch.bfloat16)
    spec = _spec(meta)
    a = _core.rectified_attention(q, k, v, spec, meta["top_k"], meta["p"], _nbr(meta))
    b, _ = _core.rectified_attention_onecall(q, k, v, spec, meta["top_k"], meta["p"], _nbr(meta))
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_block64_head_dim_32_padded():
    """Head dim 32 reaches the 64-token path zero-padded, like at block 128: same mask as the native-D contract."""
    from rectified_spaattn_amd import _core, synth
    q, k, v = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in synth.structured_qkv(3, 1, 2, 1280, 32, block=64))
    spec = _core.LayoutSpec.wan(1280, 1, block=64)
    out = _core.rectified_attention(q, k, v, spec, 3, 0.3, None)
    assert out.shape == (1, 1280, 64) and bool(torch.isfinite(out.float()).all())


def test_block64_fp8_fallback_and_refusals():
    from rectified_spaattn_amd import _operator, rectified_wan21_attn
    meta, _ = load_op_case("b64_wan_pad_1450")
    q, k, v = _inputs(meta, torch.bfloat16)
    nbr = _nbr(meta)
    plain = _public(meta, q, k, v, nbr)
    old = _operator.set_qkv_fp8(True)
    try:
        fallback = _public(meta, q, k, v, nbr)     # process default: the 2-byte kernel at block 64
    finally:
        _operator.set_qkv_fp8(old)
    torch.cuda.synchronize()
    assert torch.equal(plain, fallback)
    for mode in (True, "pv"):
        with pytest.raises(NotImplementedError):
            _public(meta, q, k, v, nbr, qkv_fp8=mode)
    with pytest.raises(NotImplementedError):
        rectified_wan21_attn.rectified_block_sparse_attention(q, k, v, None, 4, block_size_M=64, block_size_N=128,
                                                              block_neighbor_list=nbr)
    with pytest.raises(NotImplementedError):
        rectified_wan21_attn.rectified_block_sparse_attention(q, k, v, None, 4, block_size_M=32, block_size_N=32,
                                                              block_neighbor_list=nbr)


def test_block128_default_unchanged_by_explicit_block():
    """block 128 given explicitly = the default call, byte for byte."""
    from rectified_spaattn_amd import _core
    meta = ast.literal_eval(str(np.load(os.path.join(GOLDEN, "op_b64_hunyuan_1280.npz"))["meta"]))
    q, k, v = _inputs(meta, torch.bfloat16)
    a = _core.rectified_attention(q, k, v, _core.LayoutSpec.hunyuan(meta["S"], meta["num_true"]), 3, 0.3, None)
    b = _core.rectified_attention(q, k, v, _core.LayoutSpec.hunyuan(meta["S"], meta["num_true"], block=128), 3, 0.3, None)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
