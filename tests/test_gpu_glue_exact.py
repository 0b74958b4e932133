"""GPU witnesses of the producers either side of the path (csrc/rsa_glue.hip) at the widths production uses, against the per-element
references of tests/glue_ref.py: permute_tokens bit for bit, qk_norm_rope and norm_rope_across_heads inside the interval
reference on EVERY element (equal where the interval is a point), rel_l1's two sums equal to an integer count.  Each module run
prints, per kernel, the share of elements whose interval was wider than a point and how many of those took torch's value."""
import ctypes

import numpy as np
import pytest
import torch

import glue_ref as g

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (n, amb, same) in sorted(STATS.items()):
        print(f"\n{name}: {n} elements, {amb} ambiguous ({amb / max(n, 1):.5%}), {same} of those equal to torch's CPU value")


def _pattern(shape, seed):
    """a counter pattern as uint16, for the parts of a buffer a kernel must not read or must leave alone"""
    n = int(np.prod(shape))
    return ((np.arange(n, dtype=np.uint64) * np.uint64(25173) + np.uint64(seed)) & np.uint64(0xFFFF)).astype(np.uint16).reshape(shape)


def _dev(bits, dt):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(g._tdt(dt))


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _embed(x, layout, dt, seed):
    """x uint16 [B, S, W] -> a device view holding it: contiguous, a third of a fused [B, S, 3W] projection, a column slice
    of a wider row, or rows of a buffer with a larger batch stride"""
    B, S, W = x.shape
    if layout == "contig":
        return _dev(x, dt)
    if layout in ("q", "k", "v"):
        i = "qkv".index(layout)
        buf = _pattern((B, S, 3 * W), seed)
        buf[:, :, i * W:(i + 1) * W] = x
        return _dev(buf, dt)[:, :, i * W:(i + 1) * W]
    if layout == "cols":
        buf = _pattern((B, S, W + 24), seed)
        buf[:, :, 8:8 + W] = x
        return _dev(buf, dt)[:, :, 8:8 + W]
    buf = _pattern((B, S + 3, W), seed)
    buf[:, 1:S + 1] = x
    return _dev(buf, dt)[:, 1:S + 1]


def _judge(name, got_bits, dt, lo, hi, torch_ref, cid):
    got = g.widen(got_bits, dt)
    ok = g.inside(got, lo, hi)
    amb = lo != hi
    n, a, s = STATS.get(name, (0, 0, 0))
    STATS[name] = (n + got.size, a + int(amb.sum()), s + int((amb & (got == torch_ref)).sum()))
    bad = np.argwhere(~ok)
    assert ok.all(), (cid, len(bad), [(tuple(i), float(got[tuple(i)]), float(lo[tuple(i)]), float(hi[tuple(i)])) for i in bad[:6]])


def _f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("cid", [c["id"] for c in g.qk_cases()])
@torch.no_grad()
def test_qk_norm_rope_inside_the_interval(cid):
    from rectified_spaattn_amd import glue
    c = next(c for c in g.qk_cases() if c["id"] == cid)
    i = g.qk_inputs(cid)
    B, S, H, D, dt = c["B"], c["S"], c["H"], c["D"], c["dt"]
    x = _embed(i["x"].reshape(B, S, H * D), c["layout"], dt, c["seed"])
    norm = i["norm"]
    if norm is not None:
        norm = tuple(_f32(t) for t in norm[1:-1]) + (norm[-1],)       # (w, eps) or (w, b, eps)
    rope = None if i["rope"] is None else tuple(_f32(t) for t in i["rope"])
    if c["concat"]:
        before = _pattern((B, S + 5, H, D), c["seed"] + 1)
        buf = _dev(before, dt)
        glue.qk_norm_rope(x, H, norm, rope, c["s_rope"], out=buf[:, 3:3 + S])
        after = _bits(buf)
        assert np.array_equal(after[:, :3], before[:, :3]) and np.array_equal(after[:, 3 + S:], before[:, 3 + S:])
        got = after[:, 3:3 + S]
    else:
        got = _bits(glue.qk_norm_rope(x, H, norm, rope, c["s_rope"]).transpose(1, 2))
    lo, hi = g.qk_reference(cid)
    name = "qk_norm_rope/" + ("layernorm" if c["norm"].startswith("ln") else "rmsnorm")
    _judge(name, got, dt, lo, hi, g.torch_qk(cid), cid)


@pytest.mark.parametrize("cid", [c["id"] for c in g.across_cases()])
@torch.no_grad()
def test_norm_rope_across_heads_inside_the_interval(cid):
    from rectified_spaattn_amd import glue
    c = next(c for c in g.across_cases() if c["id"] == cid)
    i = g.across_inputs(cid)
    x = _embed(i["x"], c["layout"], c["dt"], c["seed"])
    norm = None if i["norm"] is None else (_f32(i["norm"][0]), i["norm"][1])
    rot = None
    if c["kind"] == 1:
        rot = torch.from_numpy(i["tables"])[None, None].to(DEV)
    elif c["kind"] == 2:
        rot = tuple(_f32(t)[None, :, None, :] for t in i["tables"])
    got = _bits(glue.norm_rope_across_heads(x, c["H"], norm, rot).transpose(1, 2))
    lo, hi = g.across_reference(cid)
    _judge("norm_rope_across_heads", got, c["dt"], lo, hi, g.torch_across(cid), cid)


@pytest.mark.parametrize("c", g.permute_cases(), ids=lambda c: c["id"])
def test_permute_tokens_bit_for_bit(c):
    from rectified_spaattn_amd import glue
    xb, order = g.permute_inputs(c)
    x = _embed(xb, c["layout"], c["dt"], c["seed"])
    idx = torch.from_numpy(order).to(DEV, torch.int64 if c["idx"] == "int64" else torch.int32)
    got = glue.permute_tokens(x, idx)
    assert got.shape == (c["B"], c["n"], c["C"]) and got.dtype == x.dtype
    assert np.array_equal(_bits(got), g.permute_reference(xb, order))


def test_permute_tokens_sees_an_order_changed_in_place():
    """the int32 copy of `order` is cached on the tensor, keyed by its in-place version counter"""
    from rectified_spaattn_amd import glue
    c = dict(B=2, S=7, C=520, n=5, seed=5100)
    xb, order = g.permute_inputs(c)
    x = _dev(xb, "bf16")
    idx = torch.from_numpy(order).to(DEV)
    assert np.array_equal(_bits(glue.permute_tokens(x, idx)), xb[:, order])
    assert np.array_equal(_bits(glue.permute_tokens(x, idx)), xb[:, order])            # served from the cache
    idx.copy_((idx + 3) % c["S"])
    order2 = (order + 3) % c["S"]
    assert np.array_equal(_bits(glue.permute_tokens(x, idx)), xb[:, order2])
    idx[1] = int(order2[0])
    order2[1] = order2[0]
    assert np.array_equal(_bits(glue.permute_tokens(x, idx)), xb[:, order2])


def _rel_l1_sums(a, b, n):
    """(sd, sb) of the first n elements as the device wrote them, through the entry the way teacache.rel_l1_distance
    calls it"""
    from rectified_spaattn_amd import _core, _lib
    out = torch.empty(2 + 2048, dtype=torch.float32, device=a.device)
    vp = ctypes.c_void_p
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().rsa_rel_l1(vp(a.data_ptr()), vp(b.data_ptr()), n, _core.dtype_code(a.dtype),
                                         vp(out.data_ptr()), vp(out[2:].data_ptr()), _core._stream()), "rsa_rel_l1")
    return tuple(out[:2].tolist())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", g.REL_L1_SIZES)
def test_rel_l1_sums_equal_the_integer_count(n, dt):
    from rectified_spaattn_amd.teacache import rel_l1_distance
    an, bn = g.rel_l1_inputs(n)
    sd, sb = g.rel_l1_counts(an, bn)
    # + 8 spare elements of another value: n = 0 still has storage to point the entry at, and a read past n would count
    wide_a, wide_b = (torch.full((n + 8,), v, dtype=dt, device=DEV) for v in (3.0, -5.0))
    a, b = wide_a[:n].copy_(torch.from_numpy(an)), wide_b[:n].copy_(torch.from_numpy(bn))
    assert _rel_l1_sums(wide_a, wide_b, n) == (float(sd), float(sb))
    if n == 0:
        assert np.isnan(rel_l1_distance(a, b))                     # the reference's expression on an empty tensor
    else:
        assert rel_l1_distance(a, b) == sd / sb
        assert rel_l1_distance(a, a) == 0.0
        z = torch.zeros_like(b)
        assert rel_l1_distance(a, z) == float("inf") and np.isnan(rel_l1_distance(z, z))


def test_refusals_come_before_any_launch():
    from rectified_spaattn_amd import _core, _lib, glue
    x = torch.zeros(1, 4, 3 * 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises((AssertionError, _lib.RsaError)):
        glue.norm_rope_across_heads(x, 3)                          # head dim 96 does not divide 512
    with pytest.raises((AssertionError, _lib.RsaError)):
        glue.qk_norm_rope(x, 3)                                    # the per-head kernel has D = 64 and 128 only
    with pytest.raises((AssertionError, _lib.RsaError)):
        glue.norm_rope_across_heads(torch.zeros(1, 4, 65 * 128, dtype=torch.bfloat16, device=DEV), 65)    # > 16 chunks per lane
    a = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(2 + 2048, dtype=torch.float32, device=DEV)
    vp, code = ctypes.c_void_p, _core.dtype_code(a.dtype)
    assert _lib.lib().rsa_rel_l1(vp(a.data_ptr()), vp(a.data_ptr()), -1, code, vp(out.data_ptr()), vp(out[2:].data_ptr()), None) != 0
    assert _lib.lib().rsa_rel_l1(vp(a.data_ptr() + 2), vp(a.data_ptr()), 8, code, vp(out.data_ptr()), vp(out[2:].data_ptr()), None) != 0
