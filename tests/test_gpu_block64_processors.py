"""Processors with block_size=64 (one per family): the sparse step hands block_size_M = block_size_N = 64 to the operator,
and what it gets back equals the operator called on the same q, k, v; the default (block_size=128) gives the same bytes
with and without the keyword."""
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
heads, hd = 2, 128
dim = heads * hd


def _spy(module):
    captured = {}
    orig = module.rectified_block_sparse_attention

    def spy(q, k, v, **kw):
        captured["qkv"] = tuple(x.clone() for x in (q, k, v))
        captured["kw"] = kw
        captured["out"] = orig(q, k, v, **kw)
        return captured["out"]

    module.rectified_block_sparse_attention = spy
    return captured, orig, lambda: setattr(module, "rectified_block_sparse_attention", orig)


def _family(name, block_size=None):
    """(module whose operator the processor calls, processor, call arguments) of one family at a small shape; the
    neighbour matrix is banded at the block size the processor runs with."""
    from rectified_spaattn_amd import rectified_cogvideo_attn as cog
    from rectified_spaattn_amd import rectified_flux_attn as fx
    from rectified_spaattn_amd import rectified_hunyuan_attn as hy
    from rectified_spaattn_amd import rectified_wan21_attn as w21
    from rectified_spaattn_amd import rectified_wan22_attn as w22
    from rectified_spaattn_amd import synth
    kw = {} if block_size is None else dict(block_size=block_size)
    b = block_size or 128
    if name == "hunyuan":
        a = helpers.attn_to(helpers.fake_attn(101, heads, hd, added=True), DEV, torch.bfloat16)
        hs = helpers.hidden(101, 20, 1, 1024, dim).to(DEV, torch.bfloat16)
        enc = helpers.hidden(101, 21, 1, 256, dim).to(DEV, torch.bfloat16)
        mask = torch.zeros(1, 1, 1, 1280, dtype=torch.bool, device=DEV)
        mask[..., :1224] = True
        rope = tuple(t.to(DEV) for t in helpers.rope_tables(1024, hd))
        nbr = torch.from_numpy(synth.banded_neighbors(1024 // b, 1))
        return hy, hy.RectifiedHunyuanVideoSpaAttnProcessor2_0("sparse", 2, nbr, 0.3, 3, **kw), (a, hs, enc, mask, rope)
    if name == "flux":
        a = helpers.attn_to(helpers.fake_attn(103, heads, hd, added=True), DEV, torch.bfloat16)
        hs = helpers.hidden(103, 20, 1, 1024, dim).to(DEV, torch.bfloat16)
        enc = helpers.hidden(103, 21, 1, 512, dim).to(DEV, torch.bfloat16)
        rope = tuple(t.to(DEV) for t in helpers.rope_tables(1536, hd))
        nbr = torch.from_numpy(synth.banded_neighbors(1024 // b, 1))
        return fx, fx.RectifiedFluxSpaAttnProcessor2_0("sparse", 2, nbr, 0.3, 0, 512, **kw), (a, hs, enc, None, rope)
    if name == "cogvideo":
        a = helpers.attn_to(helpers.fake_attn(106, 4, 64, added=False), DEV, torch.bfloat16)
        hs = helpers.hidden(106, 20, 1, 768, 256).to(DEV, torch.bfloat16)
        enc = helpers.hidden(106, 21, 1, 226, 256).to(DEV, torch.bfloat16)
        rope = tuple(t.to(DEV) for t in helpers.rope_tables(768, 64))
        nbr = torch.from_numpy(synth.banded_neighbors(768 // b, 1))
        p = cog.RectifiedCogVideoXVideoSpaAttnProcessor2_0("sparse", 2, nbr, 0.3, 0, **kw)
        p.current_step = 5
        return cog, p, (a, hs, enc, None, rope)
    a = helpers.attn_to(helpers.fake_attn(111, heads, hd, wan=True), DEV, torch.bfloat16)
    hs = helpers.hidden(111, 20, 1, 900, dim).to(DEV, torch.bfloat16)
    nbr = torch.from_numpy(synth.banded_neighbors((900 + b - 1) // b, 1))
    if name == "wan21":
        p = w21.RectifiedWanT2VSpaAttnProcessor2_0("sparse", 2, nbr, 0.3, 3, 1, **kw)
        p.current_step = 10
        return w21, p, (a, hs, None, None, helpers.wan_freqs(900, hd).to(DEV))
    p = w22.RectifiedWanTI2VSpaAttnProcessor2_0("sparse", 2, nbr, 0.3, 3, 1, **kw)   # (its operator: rectified_wan21_attn's)
    p.current_step = 10
    return w21, p, (a, hs, None, None, tuple(t.to(DEV) for t in helpers.wan22_rope(900, hd)))


FAMILIES = ["hunyuan", "flux", "cogvideo", "wan21", "wan22"]


@torch.no_grad()
@pytest.mark.parametrize("name", FAMILIES)
def test_processor_block64_equals_operator_call(name):
    module, p, args = _family(name, 64)
    assert p.block_size == 64
    captured, orig, restore = _spy(module)
    try:
        out = p(*args)
    finally:
        restore()
    assert "qkv" in captured, "the sparse branch did not run"
    kw = captured["kw"]
    assert kw["block_size_M"] == 64 and kw["block_size_N"] == 64
    again = orig(*captured["qkv"], **kw)
    torch.cuda.synchronize()
    assert torch.equal(captured["out"], again)
    assert all(bool(torch.isfinite(o.float()).all()) for o in (out if isinstance(out, tuple) else (out,)))


@torch.no_grad()
@pytest.mark.parametrize("name", FAMILIES)
def test_processor_block128_default_byte_identical(name):
    outs = []
    for bs in (None, 128):
        _, p, args = _family(name, bs)
        assert p.block_size == 128
        o = p(*args)
        outs.append(o if isinstance(o, tuple) else (o,))
    torch.cuda.synchronize()
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(x, y) for x, y in zip(*outs))


def test_processor_block_size_refused():
    from rectified_spaattn_amd import rectified_flux_attn as fx
    with pytest.raises(NotImplementedError):
        fx.RectifiedFluxSpaAttnProcessor2_0("sparse", 2, None, 0.3, 0, 512, block_size=32)
