"""Shard invariance across every decision that looks at the SIZE OF THE LAUNCH.  A rank that holds a slice of the heads (or of
the batch: the thresholds see B * H) computes, for its (b, h) pairs, the unsharded call's bitmask, lists, R, w, probs and comp
byte for byte -- always --, its O byte for byte wherever K5 planned the walk the same way, and everywhere under
set_shard_invariant(True).  tests/test_gpu_shard_invariance.py lists the three decisions; each case here puts the full call on
one side of a threshold and the slice on the other:

A  K4's form (rsa_stats.hip::compensation_b).  Until this file the form came from the grid (>= 512 workgroups: the bf16 hi / lo
   split kernel, below: the fp32 chain), so a full launch and a rank of it computed comp, and through the epilogue O, with
   different bits -- with shard invariance on as well.  The form is a function of the head's own NBv now.  The canary keeps
   the case honest: the two forms must differ on the very input the case compares.
B  The piece count of the dense text rows (rsa_plan_walk: 32 pieces at most on grids of fewer than 8 generations, else 16).
C  The tail split of the e4m3 and pv kernels, which plan with their own policy (rsa_attn_fp8_kernel.hip).
D  Case A through the one-call entry (rsa_rectified_attention), the path of a C host."""
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARTS = ("bitmask", "counts", "R", "w", "probs", "comp")


def _sliced(t, B, H, bs, hs):
    """Rows [bs, hs] of a [B * H, ...] statistics buffer, as the [b * h, ...] buffer of the sliced call."""
    return t.view(B, H, *t.shape[1:])[bs, hs].reshape(-1, *t.shape[1:])


def _assert_parts_equal(pb, fb, B, H, bs, hs, spec, what, extra=()):
    for name in PARTS + tuple(extra):
        assert torch.equal(pb[name], _sliced(fb[name], B, H, bs, hs)), f"{what}: {name} differs"
    valid = torch.arange(spec.NB_total, device=pb["cols"].device)[None, None, :] < pb["counts"][..., None]
    assert torch.equal(torch.where(valid, pb["cols"], -1), torch.where(valid, _sliced(fb["cols"], B, H, bs, hs), -1)), \
        f"{what}: cols below counts differ"


def _case_a(blk, D, nbv, B, H, seed):
    """Wan layout of nbv blocks, [B, H, S, D] inputs from the generator bench.gen_qkv wraps (one centroid per block of the layout)."""
    from rectified_spaattn_amd import _core, synth_device
    S = nbv * blk
    q, k, v = (x.view(B, H, S, D) for x in synth_device.structured_qkv_device(seed, B * H, 0, S, D, torch.device(DEV), block=blk))
    return q, k, v, _core.LayoutSpec.wan(S, 0, block=blk)


# (blk, D, NBv, B, H, batch slice, head slice): K4 workgroups = ceil(NBv / 32) * B * H, 512 in the full call
K4_CASES = [(128, 128, 8, 2, 256, slice(1, 2), slice(128, 192)),     # 1 per head: 512 against 64; a batch item AND a head range
            (64, 64, 40, 1, 256, slice(0, 1), slice(64, 128))]       # 2 per head, the second ragged: 512 against 128


@pytest.mark.parametrize("case", K4_CASES, ids=["b128_d128_nbv8_batch", "b64_d64_nbv40"])
def test_k4_form_does_not_depend_on_the_launch(case):
    """Full call: 512 K4 workgroups, the old threshold of the split form; slice: 64 / 128.  K5 plans nothing differently: the
    sparse units are B * H * NBp = 4096 against 512 (NBp = 8), and 256 x 24 = 6144 against 64 x 24 = 1536 (block 64: NBp =
    ceil(20 / 8) * 8 pairs of query blocks) -- multiples of a generation of 512, so no tail is split, and the layout has no text
    rows.  Every part and O byte for byte, with shard invariance off and on."""
    from rectified_spaattn_amd import _core, _lib, parallel
    blk, D, nbv, B, H, bs, hs = case
    q, k, v, spec = _case_a(blk, D, nbv, B, H, seed=41)
    NBp = (((nbv + 1) // 2 if blk == 64 else nbv) + 7) // 8 * 8
    nh = hs.stop - hs.start
    assert -(-nbv // 32) * B * H == 512 and (B * H * NBp) % 512 == 0 and (nh * NBp) % 512 == 0
    qs, ks, vs = q[bs, hs], k[bs, hs], v[bs, hs]
    # canary: on THIS input the two forms give different bytes, and comp is not zero
    L = _lib.lib()
    comps = {}
    try:
        for form in (2, 0):
            assert L.rsa_set_tuning(b"k4_split", form) == 0
            call = _core.StagedCall(qs, ks, vs, spec, 2, 0.05, None, reuse_buffers=False)
            call.select()
            torch.cuda.synchronize()
            comps[form] = call.bufs["comp"].clone()
    finally:
        L.rsa_set_tuning(b"k4_split", 1)
    assert float(comps[0].abs().max()) > 0.0
    assert not torch.equal(comps[2], comps[0]), "the split and the chain form agree on this input: the case proves nothing"
    for invariant in (False, True):
        prev = parallel.set_shard_invariant(invariant)
        try:
            full, fb = _core.rectified_attention(q, k, v, spec, 2, 0.05, None, return_parts=True, shape_xfuse=True)
            part, pb = _core.rectified_attention(qs, ks, vs, spec, 2, 0.05, None, return_parts=True, shape_xfuse=True)
            torch.cuda.synchronize()
        finally:
            parallel.set_shard_invariant(prev)
        what = f"shard invariance {'on' if invariant else 'off'}"
        _assert_parts_equal(pb, fb, B, H, bs, hs, spec, what)
        assert float(pb["comp"].abs().max()) > 0.0
        assert torch.equal(part, full[bs, :, hs]), f"{what}: O differs"


def test_one_call_entry_across_the_k4_threshold():
    """The first K4 case through rsa_rectified_attention (one workspace, the C host's path), shard invariance on: O of the
    slice [1:2, 128:192] byte for byte."""
    from rectified_spaattn_amd import _core, parallel
    blk, D, nbv, B, H, bs, hs = K4_CASES[0]
    q, k, v, spec = _case_a(blk, D, nbv, B, H, seed=41)
    S = nbv * blk
    prev = parallel.set_shard_invariant(True)
    try:
        full, _ = _core.rectified_attention_onecall(q, k, v, spec, 2, 0.05, None)
        part, _ = _core.rectified_attention_onecall(q[bs, hs], k[bs, hs], v[bs, hs], spec, 2, 0.05, None)
        torch.cuda.synchronize()
    finally:
        parallel.set_shard_invariant(prev)
    assert torch.equal(part.view(1, S, hs.stop - hs.start, D), full.view(B, S, H, D)[bs, :, hs])


def test_text_piece_cap_across_eight_generations():
    """HunyuanVideo layout, 272 visual blocks + 256 text tokens (200 valid), 16 heads: the text rows see 274 key blocks, 17
    sixteenths.  rsa_plan_walk by hand: the full launch has 16 x 272 = 4352 >= 4096 sparse units -> cap 16 -> 16 pieces of 18
    blocks; a 4-head slice has 1088 -> cap 32 -> 17 pieces of 17.  With shard invariance on both take 16: everything byte for byte.
    Off: the parts and every visual row byte for byte, the text rows within the bound of
    test_head_shard_where_one_side_splits_its_tail -- and at least one of them must differ, or the shape no longer crosses the
    threshold.
    The slice's 1088 units are two generations and 64 walks, which the DEFAULT plan would split beside its 136 text pieces
    (the full launch's 512 text pieces leave its own tail no room): that is the third decision, crossed elsewhere, and it would
    touch visual rows here.  k5_tail_split = 0 keeps it out while shard invariance is off, so the cap is the only variable."""
    from bench import gen_qkv
    from rectified_spaattn_amd import _core, _lib, parallel
    H, D, nbv = 16, 128, 272
    S = nbv * 128 + 256
    hs = slice(4, 8)
    dev = torch.device(DEV)
    spec = _core.LayoutSpec.hunyuan(S, S - 56)
    n_txt_items = (spec.kv_text_valid + 127) // 128
    assert spec.NBv == nbv and n_txt_items == 274 and n_txt_items // 16 == 17
    assert H * nbv >= 8 * 512 > (hs.stop - hs.start) * nbv
    q, k, v = gen_qkv(H, 0, S, S, D, dev, seed=29)
    L = _lib.lib()
    for invariant in (True, False):
        prev = parallel.set_shard_invariant(invariant)
        try:
            assert L.rsa_set_tuning(b"k5_tail_split", 1 if invariant else 0) == 0
            full, fb = _core.rectified_attention(q, k, v, spec, 12, 0.05, None, return_parts=True, shape_xfuse=True)
            part, pb = _core.rectified_attention(q[:, hs], k[:, hs], v[:, hs], spec, 12, 0.05, None, return_parts=True,
                                                 shape_xfuse=True)
            torch.cuda.synchronize()
        finally:
            L.rsa_set_tuning(b"k5_tail_split", 1)
            parallel.set_shard_invariant(prev)
        what = f"shard invariance {'on' if invariant else 'off'}"
        _assert_parts_equal(pb, fb, 1, H, slice(0, 1), hs, spec, what)
        want = full[:, :, hs]
        if invariant:
            assert torch.equal(part, want), f"{what}: O differs"
            continue
        r0 = nbv * 128
        assert torch.equal(part[:, :r0], want[:, :r0]), f"{what}: a visual row differs"
        diff = (part[:, r0:].float() - want[:, r0:].float()).abs()
        assert float(diff.max()) <= 2 * 2.0 ** -7 * max(1.0, float(want.float().abs().max()))
        assert float(diff.max()) > 0.0, "every text row byte-identical: do the two launches still take 17 and 16 pieces?"


@pytest.mark.parametrize("mode", [True, "pv"], ids=["e4m3", "pv"])
def test_fp8_kernels_where_one_side_splits_its_tail(mode):
    """The shape of test_head_shard_where_one_side_splits_its_tail (8 heads x 72 query blocks = 576 units: the full launch splits the
    64 walks of its second generation, a 4-head slice none) in the e4m3 and the pv kernel.  Shard invariance on: O, the parts, the
    e4m3 images and the block exponents byte for byte (the scales are per tensor, head and 128-row block).  Off: the parts and the
    images byte for byte, every block outside the split tail byte for byte, the split blocks within the tolerance
    test_gpu_tail_split.py::test_split_tail_in_the_e4m3_kernel applies between the split and the whole walk."""
    from bench import gen_qkv
    from rectified_spaattn_amd import _core, parallel
    H, D, nbv, world = 8, 128, 72, 2
    S = nbv * 128
    q, k, v = gen_qkv(H, 0, S, S, D, torch.device(DEV), seed=23)
    spec = _core.LayoutSpec.wan(S, 2)
    touched_full = helpers.tail_blocks(H, spec)
    assert int(touched_full.sum()) == 64 and int(helpers.tail_blocks(H // world, spec).sum()) == 0
    for invariant in (False, True):
        prev = parallel.set_shard_invariant(invariant)
        try:
            full, fb = _core.rectified_attention(q, k, v, spec, 12, 0.05, None, return_parts=True, shape_xfuse=True, qkv_fp8=mode)
            for rank in range(world):
                h0, hl = parallel.head_shard(H, world, rank)
                hs = slice(h0, h0 + hl)
                part, pb = _core.rectified_attention(q[:, hs], k[:, hs], v[:, hs], spec, 12, 0.05, None, return_parts=True,
                                                     shape_xfuse=True, qkv_fp8=mode)
                torch.cuda.synchronize()
                what = f"{mode}, shard invariance {'on' if invariant else 'off'}, rank {rank}"
                images = tuple(n for n in ("q8", "k8", "v8t") if fb[n].numel())
                assert "v8t" in images and (mode == "pv" or len(images) == 3)
                _assert_parts_equal(pb, fb, 1, H, slice(0, 1), hs, spec, what, extra=images + ("exps", "kmean"))
                want = full[:, :, hs]
                if invariant:
                    assert torch.equal(part, want), f"{what}: O differs"
                    continue
                diff = (part.float() - want.float()).abs()[0].reshape(nbv, 128, hl, D).amax(dim=(1, 3)).t().cpu()   # [hl, NBv]
                tf = touched_full[hs]
                assert (diff[~tf] == 0).all(), f"{what}: a block neither launch split differs"
                assert float(diff.max()) <= 2 * 2.0 ** -7 * max(1.0, float(want.float().abs().max()))
                if tf.any():
                    assert (diff[tf] > 0).any(), "the split blocks came out byte-identical: is the tail split still planned?"
        finally:
            parallel.set_shard_invariant(prev)
