"""block_sparse_attention_backward and block_sparse_attention_autograd on the device: the gradients
against fp64 with torch's own error in the input type as the bar, the exact gradient witness byte for byte, the visibility rule read
through dv, layouts and plumbing, and one captured graph of forward plus backward.  The references and case tables are
tests/bwd_ref.py's."""
import ctypes

import numpy as np
import pytest
import torch

import bwd_ref as ref
import weights
from rectified_spaattn_amd import (_core, _lib, block_sparse_attention, block_sparse_attention_autograd,
                                   block_sparse_attention_backward)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, TDT[dt])


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def nan_like(t):
    return torch.full_like(t, float("nan"))


def run(inp, dt, lens, blk, causal, out=None, **kw):
    """(out, dq, dk, dv) of the library on a case's inputs; out: the forward's unless given."""
    q, k, v, dout = (dev(inp[n], dt) for n in ("q", "k", "v", "dout"))
    mask = torch.from_numpy(inp["mask"]).to(DEV)
    opts = dict(kv_len=lens, sm_scale=inp["sm_scale"], block_size=blk, causal=causal)
    if out is None:
        out = block_sparse_attention(q, k, v, mask, **opts)
    res = block_sparse_attention_backward(dout, q, k, v, out, mask, **opts, **kw)
    torch.cuda.synchronize()
    return (out,) + tuple(res)


# ---- 1: against fp64, the bar measured against torch ---------------------------------------------------------------------------
def torch_yardstick(inp, seen, dt):
    """torch's own autograd in the input type on the device: softmax(((q sm_scale) k^T).masked_fill(~seen, -inf).float()).to(dtype)
    @ v with the K/V heads repeated.  A row that sees nothing would be NaN there and poison dk / dv: its scores are set to 0 and
    its weights to 0, which leaves every other row's expression as stated."""
    q, k, v, dout = (dev(inp[n], dt) for n in ("q", "k", "v", "dout"))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    g = q.shape[1] // k.shape[1]
    vis = torch.from_numpy(seen).to(DEV)
    some = vis.any(-1, keepdim=True)
    s = ((q * inp["sm_scale"]) @ k.repeat_interleave(g, 1).transpose(-1, -2)).masked_fill(~vis, float("-inf")).float()
    p = (torch.softmax(torch.where(some, s, torch.zeros_like(s)), -1) * some).to(q.dtype)
    (p @ v.repeat_interleave(g, 1)).backward(dout)
    return q.grad, k.grad, v.grad


def error_ratios(c):
    """[(causal, tensor name, max|got - ref| / max|torch - ref|, mean|got - ref| / mean|torch - ref|, a second call gives the same
    bytes, everything finite)] of one case: ref = the fp64 gradients on the rounded inputs.  `out`, an input of the backward like
    q, k, v and dout, is the fp64 forward rounded to the storage type: the bar measures the backward.  The forward's own result is
    not that everywhere: under causal, fp16, a row whose few visible keys score 24 or more (log2 domain) below a masked key of the
    same tile comes out of block_sparse_attention as 0 or coarse (its weights underflow fp16 against the tile's reference; item 1's
    row Sq - 140 at input scale 2), and delta = dout . out then carries that error into dq and dk of that row -- measured ratios of
    3.5 to 43.7 with the forward's out, 0.70 with this one.  The tests of the autograd function and of the
    captured graph run on the forward's out."""
    inp = ref.fp64_inputs(c)
    rows = []
    for causal in c["causals"]:
        seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], c["H"], causal)
        out64, *want = ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], seen, inp["sm_scale"])
        out = dev(out64.astype(np.float32), c["dt"])
        got = run(inp, c["dt"], c["lens"], c["blk"], causal, out=out)
        again = run(inp, c["dt"], c["lens"], c["blk"], causal, out=out)
        yard = torch_yardstick(inp, seen, c["dt"])
        for name, g, g2, y, w in zip(("dq", "dk", "dv"), got[1:], again[1:], yard, want):
            eg, ey = np.abs(f64(g) - w), np.abs(f64(y) - w)
            rows.append((causal, name, eg.max() / ey.max(), eg.mean() / ey.mean(),
                         torch.equal(g.view(torch.int16), g2.view(torch.int16)), bool(torch.isfinite(g).all())))
    return rows


@pytest.mark.parametrize("c", ref.FP64_CASES, ids=lambda c: c["id"])
def test_gradients_against_fp64_within_torchs_own_error(c):
    """Per tensor: max|got - ref| <= 2 max|torch - ref| (a one-element statistic: flash-attn's factor) and mean|got - ref| <=
    mean|torch - ref| (no margin: the mean is stable).

    Measured on an MI355X over the 324 (case, causal, tensor) rows: the ratios are printed; DESIGN.md section 5.21 holds the worst."""
    rows = error_ratios(c)
    for causal, name, rmax, rmean, same, finite in rows:
        print(f"bwd-ratio {c['id']} causal={int(causal)} {name} max {rmax:.3f} mean {rmean:.3f}")
    for causal, name, rmax, rmean, same, finite in rows:
        assert same, f"{name}: a second call gives other bytes"
        assert finite, name
        assert rmax <= 2.0, (name, causal, rmax)
        assert rmean <= 1.0, (name, causal, rmean)


# ---- 2: the exact gradient witness ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.EXACT_CASES, ids=lambda c: c["id"])
def test_exact_gradient_witness_byte_for_byte(c):
    inp = ref.exact_inputs(c)
    out, dq, dk, dv = ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], ref.exact_seen(), inp["sm_scale"])
    got = run(inp, c["dt"], inp["lens"], 128, False)
    assert not bool(got[0].any()), "the forward of the witness is exactly 0"
    for name, g, w in zip(("dq", "dk", "dv"), got[1:], (dq, dk, dv)):
        want = dev(w.astype(np.float32), c["dt"])
        assert bool(want.any()) == (name != ("dk" if c["kind"] == "dq" else "dq"))
        # the same bits (x + 0 gives a zero its plus sign on both sides: fp64 and fp32 sums may disagree about the sign of a zero)
        assert torch.equal((g.float() + 0).view(torch.int32), (want.float() + 0).view(torch.int32)), \
            (name, float((g.float() - want.float()).abs().max()))


# ---- 3: visibility through dv --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.VIS_CASES, ids=lambda c: c["id"])
def test_visibility_rule_through_dv(c):
    inp = ref.vis_inputs(c)
    seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], ref.VIS_H, c["causal"])
    _, dq, dk, dv = run(inp, "bf16", c["lens"], c["blk"], c["causal"])
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert not bool(torch.isnan(t).any()), f"{name} holds NaN"
    assert np.array_equal(f64(dv) != 0, ref.vis_pattern(c, inp))
    blind = torch.from_numpy(~seen.any(-1)).to(DEV)            # [B, H, Sq]
    assert not bool(dq[blind].any())
    if c["causal"]:
        assert bool(blind[1, :, :60].all()) and not bool(blind[1, :, 60:].any())
    for b, nb in enumerate(c["lens"]):
        assert not bool(dk[b, :, nb:].any()) and not bool(dv[b, :, nb:].any())
    # ... and with live scores beside the NaN keys: the same zero rows, nothing but numbers elsewhere
    g = np.random.default_rng(5)
    live = dict(inp, q=weights.round_dt(g.standard_normal(inp["q"].shape).astype(np.float32), "bf16"),
                dout=weights.round_dt(g.standard_normal(inp["q"].shape).astype(np.float32), "bf16"))
    _, dq, dk, dv = run(live, "bf16", c["lens"], c["blk"], c["causal"])
    for t in (dq, dk, dv):
        assert bool(torch.isfinite(t).all())
    # (a row that sees ONE key has P = 1 and dP = delta: its dq is an exact zero too; from two keys on it is not)
    several = torch.from_numpy(seen.sum(-1) >= 2).to(DEV)
    assert not bool(dq[blind].any()) and bool(dq[several].any(-1).all())
    for b, nb in enumerate(c["lens"]):
        assert not bool(dk[b, :, nb:].any()) and not bool(dv[b, :, nb:].any())
        unseen = torch.from_numpy(~seen[b].reshape(ref.VIS_HKV, -1, c["Sq"], ref.SK).any((1, 2))).to(DEV)      # [Hkv, Sk]
        assert not bool(dk[b][unseen].any()) and not bool(dv[b][unseen].any())


# ---- 4: layouts and plumbing ---------------------------------------------------------------------------------------------------
def _plumbing(S=200, H=4, Hkv=2, D=64, dt=torch.bfloat16, seed=3):
    g = torch.Generator(device="cpu").manual_seed(seed)
    fused = torch.randn(2, S, (H + 2 * Hkv) * D, generator=g).to(DEV, dt)
    dfused = torch.randn(2, S, H * D, generator=g).to(DEV, dt)
    mask = torch.from_numpy(ref.random_mask(seed, Hkv, -(-S // 128), -(-S // 128))).to(DEV)
    return fused, dfused, mask


def _views(fused, dfused, H, Hkv, D):
    B, S, _ = fused.shape
    q, k, v = fused.split([H * D, Hkv * D, Hkv * D], dim=-1)
    return (q.view(B, S, H, D).transpose(1, 2), k.view(B, S, Hkv, D).transpose(1, 2), v.view(B, S, Hkv, D).transpose(1, 2),
            dfused.view(B, S, H, D).transpose(1, 2))


def test_strided_views_of_a_fused_projection_give_the_contiguous_bytes():
    H, Hkv, D = 4, 2, 64
    fused, dfused, mask = _plumbing()
    q, k, v, dout = _views(fused, dfused, H, Hkv, D)
    assert not q.is_contiguous() and not k.is_contiguous() and q.data_ptr() == fused.data_ptr()
    opts = dict(kv_len=[200, 140], block_size=128, causal=True)
    qc, kc, vc, dc = (t.contiguous() for t in (q, k, v, dout))
    out = block_sparse_attention(qc, kc, vc, mask, **opts)
    want = block_sparse_attention_backward(dc, qc, kc, vc, out, mask, **opts)
    got = block_sparse_attention_backward(dout, q, k, v, out, mask, **opts)                        # fused views
    bshd = block_sparse_attention_backward(dout, q, k, v, out.transpose(1, 2).contiguous().transpose(1, 2), mask, **opts)
    for w, a, b in zip(want, got, bshd):
        assert w.is_contiguous() and torch.equal(w, a) and torch.equal(w, b)


def test_device_kv_len_gives_the_host_lists_bytes_and_is_not_read():
    fused, dfused, mask = _plumbing(seed=4)
    q, k, v, dout = (t.contiguous() for t in _views(fused, dfused, 4, 2, 64))
    for causal in (True, False):
        out = block_sparse_attention(q, k, v, mask, kv_len=[200, 140], causal=causal)
        want = block_sparse_attention_backward(dout, q, k, v, out, mask, kv_len=[200, 140], causal=causal)
        for lens in (torch.tensor([200, 140], device=DEV, dtype=torch.int32), torch.tensor([200, 140], device=DEV),
                     torch.tensor([900, 140], device=DEV)):       # (clamped into [0, Sk] on the device)
            got = block_sparse_attention_backward(dout, q, k, v, out, mask, kv_len=lens, causal=causal)
            assert all(torch.equal(w, g) for w, g in zip(want, got))
    one = block_sparse_attention_backward(dout, q, k, v, out, mask, kv_len=140)
    dev1 = block_sparse_attention_backward(dout, q, k, v, out, mask, kv_len=torch.tensor([140], device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(one, dev1))


@pytest.mark.parametrize("D", [32, 16])
def test_small_head_dims_equal_the_call_on_zero_padded_inputs(D):
    fused, dfused, mask = _plumbing(D=D, seed=6)
    q, k, v, dout = (t.contiguous() for t in _views(fused, dfused, 4, 2, D))
    opts = dict(kv_len=[200, 140], sm_scale=D ** -0.5, causal=True)
    out = block_sparse_attention(q, k, v, mask, **opts)
    got = block_sparse_attention_backward(dout, q, k, v, out, mask, **opts)
    pad = lambda t: torch.nn.functional.pad(t, (0, _core._PAD_HEAD_DIM[D] - D))       # noqa: E731
    want = block_sparse_attention_backward(pad(dout), pad(q), pad(k), pad(v), pad(out), mask, **opts)
    for g, w in zip(got, want):
        assert g.shape[-1] == D and torch.equal(g, w[..., :D]) and not bool(w[..., D:].any())


@pytest.mark.parametrize("blk,causal", [(128, True), (64, False)])
def test_autograd_function_is_the_forward_and_the_explicit_backward(blk, causal):
    fused, dfused, _ = _plumbing(seed=8)
    mask = torch.from_numpy(ref.random_mask(8, 2, -(-200 // blk), -(-200 // blk))).to(DEV)
    q, k, v, dout = (t.contiguous() for t in _views(fused, dfused, 4, 2, 64))
    opts = dict(kv_len=[200, 140], block_size=blk, causal=causal)
    plain = block_sparse_attention(q.clone().requires_grad_(), k, v, mask, **opts)
    assert plain.grad_fn is None                                # the plain call stays as it is: no graph
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    out = block_sparse_attention_autograd(ql, kl, vl, mask, **opts)
    assert out.requires_grad and torch.equal(out, plain)
    out.backward(dout)
    want = block_sparse_attention_backward(dout, q, k, v, plain, mask, **opts)
    for leaf, w in zip((ql, kl, vl), want):
        assert torch.equal(leaf.grad, w)
    with torch.no_grad():
        quiet = block_sparse_attention_autograd(ql, kl, vl, mask, **opts)
    assert not quiet.requires_grad and torch.equal(quiet, plain)
    # a loss whose gradient arrives as an expanded (stride 0) tensor
    ql.grad = None
    block_sparse_attention_autograd(ql, kl, vl, mask, **opts).sum().backward()
    assert torch.equal(ql.grad, block_sparse_attention_backward(torch.ones_like(plain), q, k, v, plain, mask, **opts)[0])


def test_refusals_on_the_device():
    fused, dfused, mask = _plumbing(seed=9)
    q, k, v, dout = (t.contiguous() for t in _views(fused, dfused, 4, 2, 64))
    out = block_sparse_attention(q, k, v, mask)
    with pytest.raises(NotImplementedError, match="window"):
        block_sparse_attention_backward(dout, q, k, v, out, mask, window=(8, 0))
    with pytest.raises(NotImplementedError, match="window"):
        block_sparse_attention_autograd(q, k, v, mask, window=(8, 0))
    with pytest.raises(ValueError, match="block_mask"):
        block_sparse_attention_backward(dout, q, k, v, out, mask[:, :, :1])
    with pytest.raises(ValueError, match="block_mask"):
        block_sparse_attention_backward(dout, q, k, v, out, mask.float())
    with pytest.raises(ValueError, match="one dtype"):
        block_sparse_attention_backward(dout, q, k.half(), v, out, mask)
    with pytest.raises(ValueError, match="do not divide"):
        block_sparse_attention_backward(dout[:, :3], q[:, :3], k, v, out[:, :3], mask)


def test_c_entry_statuses_without_a_launch():
    fused, dfused, mask = _plumbing(seed=10)
    q, k, v, dout = (t.contiguous() for t in _views(fused, dfused, 4, 2, 64))
    out = block_sparse_attention(q, k, v, mask)
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    rows = block_mask_to_lists(mask, 2, 2)
    cols = block_mask_to_lists(mask.transpose(-1, -2).contiguous(), 2, 2)
    L = _lib.lib()
    need = ctypes.c_size_t(0)
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 200, 64, 128, 2, 2, ctypes.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    res = [nan_like(q), nan_like(k), nan_like(v)]

    def call(block=128, ws_bytes=need.value):
        with torch.cuda.device(q.device):
            return L.rsa_block_sparse_bwd(2, 4, 2, 2, 200, 200, 64, _lib.RSA_BF16, block, 2, 2, 200, None, 0, 0.125, _core._t4(q),
                                          _core._t4(k), _core._t4(v), _core._t4(out), _core._t4(dout), rows["cols"].data_ptr(),
                                          rows["counts"].data_ptr(), cols["cols"].data_ptr(), cols["counts"].data_ptr(),
                                          ws.data_ptr(), ws_bytes, *(_lib.RsaOut4(t.data_ptr(), *t.stride()[:3]) for t in res),
                                          _core._stream())
    assert call(ws_bytes=need.value - 1) == -3 and call(block=96) == -2
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in res), "a refused call wrote something"
    assert call() == 0
    torch.cuda.synchronize()
    want = block_sparse_attention_backward(dout, q, k, v, out, mask, sm_scale=0.125)
    assert all(torch.equal(a, b) for a, b in zip(res, want)), "every element is written, as the Python call writes it"


# ---- 5: one captured graph -----------------------------------------------------------------------------------------------------
def test_forward_and_backward_in_one_captured_graph():
    fused, dfused, mask = _plumbing(seed=11)
    fused2, dfused2, _ = _plumbing(seed=12)
    q, k, v, dout = (t.contiguous() for t in _views(fused, dfused, 4, 2, 64))
    q2, k2, v2, dout2 = (t.contiguous() for t in _views(fused2, dfused2, 4, 2, 64))
    lens = torch.tensor([200, 140], device=DEV, dtype=torch.int32)

    def step():
        out = block_sparse_attention(q, k, v, mask, kv_len=lens, causal=True)
        return (out,) + tuple(block_sparse_attention_backward(dout, q, k, v, out, mask, kv_len=lens, causal=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = step()
    for n, (src, new_lens) in enumerate((((q, k, v, dout), [200, 140]), ((q2, k2, v2, dout2), [200, 140]),
                                         ((q2, k2, v2, dout2), [77, 200]))):
        if n:
            for dst, s in zip((q, k, v, dout), src):
                dst.copy_(s)
            lens.copy_(torch.tensor(new_lens, device=DEV, dtype=torch.int32))
        eager_src = [t.clone() for t in (q, k, v, dout)]
        graph.replay()
        torch.cuda.synchronize()
        qe, ke, ve, de = eager_src
        out = block_sparse_attention(qe, ke, ve, mask, kv_len=new_lens, causal=True)
        want = (out,) + tuple(block_sparse_attention_backward(de, qe, ke, ve, out, mask, kv_len=new_lens, causal=True))
        for g, w in zip(got, want):
            assert torch.equal(g, w), n
