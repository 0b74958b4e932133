"""merge_partials on the device (rsa_merge_partials): against the fp64 reference of tests/merge_ref.py inside
its bound, with dead partials that hold NaN and rows without a live entry; the exact statements (one live entry: its bytes; equal
weights: the correctly rounded mean; a sink equal to the one partial's lse: the partial halved); one kernel in two forms and over
every layout, byte for byte; the pipelines -- two key ranges of block_sparse_extend merged against the one call, exactly with
integer counts and per element on a cascade (a shared prefix beside each item's causal suffix); one captured graph of two extend
calls and the merge, replayed on changed contents."""
import numpy as np
import pytest
import torch

import merge_ref as ref
from rectified_spaattn_amd import block_sparse_extend as ext
from rectified_spaattn_amd import merge_partials as merge
from rectified_spaattn_amd.block_sparse import MERGE_MAX_GRID

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
SHAPES = {"padded": (2, 3, 5), "packed": (37, 3)}       # 30 and 111 rows: no multiple of any rows-per-workgroup count (8, 16, 32)


def _dev(c, kind):
    """A case of merge_ref.make_case on the device: (list of outs, list of lses, sink or None)."""
    outs = [torch.from_numpy(o).to(DEV, TDT[kind]) for o in c["outs"]]
    lses = [torch.from_numpy(x).to(DEV) for x in c["lses"]]
    return outs, lses, (None if c["sink"] is None else torch.from_numpy(c["sink"]).to(DEV))


def _same(a, b):
    """Two (out, lse) pairs, bit for bit."""
    return bool(torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


# ---- 1. against fp64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sink", [False, True], ids=["nosink", "sink"])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("form", ["padded", "packed"])
def test_against_fp64(form, D, kind, N, sink):
    c = ref.make_case(7 * N + D + sink, N, SHAPES[form] + (D,), kind, spread=3.0, mag=1.0, dead=0.2, sink=sink)
    outs, lses, sk = _dev(c, kind)
    out, lse = merge(outs, lses, sink=sk)
    assert out.shape == outs[0].shape and out.dtype == TDT[kind] and lse.shape == lses[0].shape and lse.dtype == torch.float32
    got_out, got_lse = _np(out), lse.cpu().numpy()
    assert not np.isnan(got_out).any() and not np.isnan(got_lse).any()
    ref_lse = ref.merge_ref(c["outs"], c["lses"], c["sink_rows"])[1]
    dead = ~np.isfinite(ref_lse)
    assert dead.any() and not dead.all() and np.isnan(c["outs"]).any()       # (the case has rows without a live entry, and NaN outs)
    assert (out.view(torch.int16).cpu().numpy()[dead] == 0).all() and (got_lse[dead] == -np.inf).all()       # 0 / -inf, bit for bit
    r_out, r_lse = ref.worst_ratios(got_out, got_lse, c["outs"], c["lses"], c["sink_rows"], kind)
    print(f"{form} D={D} {kind} N={N} sink={sink}: worst |got - fp64| / bound: out {r_out:.4f}, lse {r_lse:.4f}")
    assert r_out <= 1.0 and r_lse <= 1.0
    again = merge(outs, lses, sink=sk)
    assert _same((out, lse), again)                                         # two calls, the same bytes


# ---- 2. exact: one live entry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_one_live_entry_returns_its_bytes(D, kind):
    N, shape = 5, (2, 3, 5, D)
    c = ref.make_case(D + 1, N, shape, kind, spread=30.0, mag=7.0, dead=0.0, dead_rows=False)
    rows = int(np.prod(shape[:-1]))
    which = (np.arange(rows) * 3 % N).reshape(shape[:-1])                   # the live index varies from row to row
    off = np.arange(N).reshape(N, 1, 1, 1) != which[None]
    want_out = np.take_along_axis(c["outs"], which[None, ..., None], 0)[0].copy()
    want_lse = np.take_along_axis(c["lses"], which[None], 0)[0].copy()
    c["outs"][off] = np.nan
    c["lses"][off] = -np.inf
    outs, lses, _ = _dev(c, kind)
    want = (torch.from_numpy(want_out).to(DEV, TDT[kind]), torch.from_numpy(want_lse).to(DEV))
    plain = merge(outs, lses)
    assert _same(plain, want)
    assert _same(merge(outs, lses, sink=float("-inf")), plain)
    assert _same(merge(outs, lses, sink=torch.full((3,), -np.inf, device=DEV)), plain)
    assert _same(merge(torch.stack(outs), torch.stack(lses)), plain)


# ---- 3. exact: equal weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_equal_weights_give_the_correctly_rounded_mean(N, kind):
    """All lse of a row bytewise equal: every weight is exp2(0) = 1, acc is a sum of small integers over 8 (exact in fp32), l = N a
    power of two (the division exact): out is the mean rounded once.  lse = lse + ln 2 * log2 N: two roundings of positive terms."""
    D, shape = 128, (2, 3, 5)
    rng = np.random.default_rng(N)
    ints = rng.integers(-40, 41, size=(N,) + shape + (D,))
    outs = [torch.from_numpy(ints[i] / 8.0).to(DEV, TDT[kind]) for i in range(N)]
    row_lse = (0.5 + 3.5 * rng.random(shape)).astype(np.float32)
    lses = [torch.from_numpy(row_lse).to(DEV).clone() for _ in range(N)]
    out, lse = merge(outs, lses)
    want = ref.round_to(ints.sum(0) / 8.0 / N, kind)
    assert np.array_equal(ref.to_bits(_np(out), kind), ref.to_bits(want, kind))
    exact = row_lse.astype(np.float64) + np.log(N)
    err = np.abs(lse.cpu().numpy().astype(np.float64) - exact) / np.spacing(exact.astype(np.float32)).astype(np.float64)
    print(f"N={N} {kind}: lse error {err.max():.3f} fp32 ulps")
    assert err.max() <= 2.0


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_a_sink_equal_to_the_partials_lse_halves_it(kind):
    D, (B, H, S) = 64, (2, 3, 5)
    rng = np.random.default_rng(11)
    x = ref.round_to(rng.standard_normal((B, H, S, D)), kind)
    sink = (2.0 * rng.standard_normal(H)).astype(np.float32)
    lse_in = np.broadcast_to(sink[None, :, None], (B, H, S)).copy()
    out, lse = merge([torch.from_numpy(x).to(DEV, TDT[kind])], [torch.from_numpy(lse_in).to(DEV)], sink=torch.from_numpy(sink).to(DEV))
    assert np.array_equal(ref.to_bits(_np(out), kind), ref.to_bits(x / 2.0, kind))
    exact = lse_in.astype(np.float64) + np.log(2.0)
    assert (np.abs(lse.cpu().numpy() - exact) <= 2.0 ** -20 * np.maximum(1.0, np.abs(exact))).all()


# ---- 4. the forms agree ---------------------------------------------------------------------------------------------------------------
def _narrow(t):
    """A copy of t [..., D] whose row stride is D + 4 elements: 8-byte aligned rows, the 8-byte form."""
    buf = torch.empty(t.shape[:-1] + (t.shape[-1] + 4,), dtype=t.dtype, device=t.device)
    v = buf[..., :t.shape[-1]]
    v.copy_(t)
    assert v.stride(-2) % 8 == 4
    return v


def _shifted(t):
    """A copy of t that starts 4 elements into its allocation: an 8-byte aligned pointer that is not 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[4:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


@pytest.mark.parametrize("form", ["padded", "packed"])
@pytest.mark.parametrize("N,D,kind,sink", [(1, 128, "bf16", False), (2, 64, "fp16", True), (3, 128, "fp16", False), (8, 64, "bf16", True),
                                           (8, 128, "bf16", False)])
def test_both_forms_and_every_layout_give_the_same_bytes(form, N, D, kind, sink):
    shape = SHAPES[form] + (D,)
    c = ref.make_case(N + D, N, shape, kind, spread=5.0, sink=sink)
    outs, lses, sk = _dev(c, kind)
    want = merge(outs, lses, sink=sk)
    # the 8-byte form: a row stride, or a pointer, that is only 8-byte aligned -- in one partial, in all, in the result
    for i in {0, N - 1}:
        for make in (_narrow, _shifted):
            some = list(outs)
            some[i] = make(outs[i])
            assert _same(merge(some, lses, sink=sk), want)
    assert _same(merge([_narrow(o) for o in outs], lses, sink=sk), want)
    res = _narrow(torch.empty_like(outs[0]))
    got = merge(outs, lses, sink=sk, out=res)
    assert got[0] is res and _same(got, want)
    # stacked, a list, head-strided views of one wider buffer (all partials of a row side by side), lse tensors with odd strides
    assert _same(merge(torch.stack(outs), torch.stack(lses), sink=sk), want)
    H = shape[1]
    lead = shape[:1] + shape[2:-1] if form == "padded" else shape[:1]       # the axes in front of (partial, head, channel)
    wide = torch.empty(lead + (N, H, D), dtype=TDT[kind], device=DEV)
    views = []
    for i in range(N):
        v = wide[..., i, :, :]
        v = v.permute(0, 2, 1, 3) if form == "padded" else v                # [B, S, H, D] -> [B, H, S, D]
        v.copy_(outs[i])
        views.append(v)
    odd = torch.empty(shape[:-1] + (N, 3), device=DEV)
    lviews = []
    for i in range(N):
        lv = odd[..., i, 1]
        lv.copy_(lses[i])
        lviews.append(lv)
    assert (N == 1 or not views[0].is_contiguous()) and not lviews[0].is_contiguous()
    assert _same(merge(views, lviews, sink=sk), want)
    lse_res = torch.empty(shape[:-1] + (2,), device=DEV)[..., 1]
    got = merge(views, lviews, sink=sk, lse=lse_res)
    assert got[1] is lse_res and _same(got, want)
    assert torch.equal(merge(outs, lses, sink=sk, return_lse=False).view(torch.int16), want[0].view(torch.int16))
    # in place: out= is partial 0 (and lse= its lse), in either form; the other partials are left as they were
    for make in (lambda t: t.clone(), _narrow):
        mine, mine_l = [make(o) for o in outs], [x.clone() for x in lses]
        got = merge(mine, mine_l, sink=sk, out=mine[0], lse=mine_l[0])
        assert got[0] is mine[0] and got[1] is mine_l[0] and _same(got, want)
        for i in range(1, N):
            assert torch.equal(mine[i].view(torch.int16), outs[i].view(torch.int16))
    last = N - 1
    mine = [o.clone() for o in outs]
    assert _same(merge(mine, lses, sink=sk, out=mine[last]), want)


@pytest.mark.parametrize("narrow", [False, True], ids=["16-byte", "8-byte"])
def test_rows_beyond_one_pass_of_the_grid_equal_the_two_halves(narrow):
    """The launch holds at most MERGE_MAX_GRID workgroups of 16 rows (D = 128; 8 in the 8-byte form): 33 009 rows take a second
    pass of the grid-stride loop (a third and a fifth in the 8-byte form), and come out as the same rows merged in two calls, where
    every row falls to another workgroup and pass (16-byte form: one pass each)."""
    T, H, D, N = 11003, 3, 128, 2
    assert T * H > MERGE_MAX_GRID * 16 >= (T // 2 + 1) * H
    g = torch.Generator(device=DEV).manual_seed(3)
    outs = [torch.randn(T, H, D, device=DEV, generator=g).to(torch.bfloat16) for _ in range(N)]
    lses = [3.0 * torch.randn(T, H, device=DEV, generator=g) for _ in range(N)]
    lses[1][::5] = -np.inf
    outs[1][::5] = np.nan
    lses[0][10::35] = -np.inf
    if narrow:
        outs = [_narrow(o) for o in outs]
    out, lse = merge(outs, lses)
    cut = T // 2
    for lo, hi in ((0, cut), (cut, T)):
        part = merge([o[lo:hi] for o in outs], [x[lo:hi] for x in lses])
        assert _same(part, (out[lo:hi], lse[lo:hi]))
    assert not torch.isnan(out.float()).any() and bool((lse[10::35] == -np.inf).all()) and bool((out[10::35] == 0).all())
    assert bool(out[-1].float().abs().sum() > 0)


def test_offsets_beyond_2_to_the_31_elements():
    """A batch stride of 2^31 + 8 elements in a partial and in the result (views of two 4 GiB allocations that are never filled):
    the kernel's 64-bit offsets, against the same rows merged from compact copies."""
    H, S, D = 3, 5, 128
    big = 2 ** 31 + 8
    g = torch.Generator(device=DEV).manual_seed(9)
    outs = [torch.randn(2, H, S, D, device=DEV, generator=g).to(torch.bfloat16) for _ in range(2)]
    lses = [torch.randn(2, H, S, device=DEV, generator=g) for _ in range(2)]
    want = merge(outs, lses)
    store = torch.empty(big + H * S * D, dtype=torch.bfloat16, device=DEV)
    far = store.as_strided((2, H, S, D), (big, S * D, D, 1))
    far.copy_(outs[1])
    res = torch.empty(big + H * S * D, dtype=torch.bfloat16, device=DEV).as_strided((2, H, S, D), (big, S * D, D, 1))
    got = merge([outs[0], far], lses, out=res)
    assert _same(got, want)


# ---- 5. the pipeline, exact -----------------------------------------------------------------------------------------------------------
def test_two_key_ranges_merged_are_the_one_call_byte_for_byte():
    """Zero q, V of 0 / 1: every score is 0, a partial's out is a count over its 256 keys / 256 and its lse ln 256 -- the same bytes
    in both partials, so both weights are 1 and the merge is (count_A + count_B) / 256 / 2, rounded once like the one call's count
    over 512 keys / 512.  A swapped or dropped partial, a dropped weight or a wrong denominator moves the bytes."""
    B, H, Hkv, Sq, D, blk = 2, 4, 2, 37, 64, 128
    g = torch.Generator().manual_seed(21)
    q = torch.zeros(B, H, Sq, D, dtype=torch.bfloat16, device=DEV)
    k = torch.randn(B, Hkv, 512, D, generator=g).to(DEV, torch.bfloat16)
    v = (torch.rand(B, Hkv, 512, D, generator=g) < 0.5).to(DEV, torch.bfloat16)
    ones = lambda NK: torch.ones(B, Hkv, 1, NK, dtype=torch.bool, device=DEV)      # noqa: E731
    kw = dict(block_size=blk, causal=False, return_lse=True)
    a = ext(q, k[:, :, :256], v[:, :, :256], ones(2), blocks_per_split=1, **kw)
    b = ext(q, k[:, :, 256:], v[:, :, 256:], ones(2), blocks_per_split=2, **kw)
    whole = ext(q, k, v, ones(4), blocks_per_split=2, **kw)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and not torch.equal(a[0], b[0])
    out, lse = merge([a[0], b[0]], [a[1], b[1]])
    assert torch.equal(out.view(torch.int16), whole[0].view(torch.int16))
    counts = v.float().view(B, Hkv, 1, 512, D).sum(3).expand(B, Hkv, H // Hkv, D).reshape(B, H, 1, D) / 512.0
    assert torch.equal(out.float(), counts.to(torch.bfloat16).float().expand(B, H, Sq, D))       # (and it is the count itself)
    err = (lse.double() - whole[1].double()).abs() / torch.from_numpy(np.spacing(whole[1].cpu().numpy())).to(DEV).double()
    print(f"lse: {err.max().item():.3f} fp32 ulps from the one call's")
    assert err.max().item() <= 2.0
    # the merge of one is that one; the order of equal-weight partials does not matter to these bytes, a dropped partial does
    assert torch.equal(merge([b[0], a[0]], [b[1], a[1]])[0].view(torch.int16), out.view(torch.int16))
    assert not torch.equal(merge([a[0]], [a[1]])[0].view(torch.int16), out.view(torch.int16))


# ---- 6. the pipeline, cascade -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(200, 129), (200, 0)], ids=lambda x: f"suffix{x[0]}-{x[1]}")
def test_cascade_of_a_shared_prefix_and_causal_suffixes(lens):
    """B = 2 items share a 256-key prefix: attended once, q seen as one item of B * Sq rows, non-causal; each item's suffix (kv_len
    of a 256-key capacity, NaN beyond) causal; merged, against one causal call over the concatenated cache.  Per element at most 2
    units in the last place of bf16 at max(|out_A|, |out_B|, |out_whole|): half from each partial's rounding carried through a convex
    combination, half from the merge's rounding, half from the one call's, the rest for fp32 summation order.  An item without
    suffix keys takes the prefix partial's bytes (its whole-call rows follow another causal alignment and are not compared).
    q and K are normal; V is 1 + 0.5 * normal, because that error budget leaves out one term of extend's own numerics: P is rounded
    to the input type before P.V, against another row maximum in each of the three calls, an ABSOLUTE error near 2^-9 |v| sqrt(sum
    p^2) that no merge can undo.  It is far below an ulp where an output is of V's magnitude and many ulps where an output is a
    cancellation near zero: with zero-mean V this test measured 4.0 ulps on the device, and a numpy model of the three calls gives
    up to 22 ulps with P rounded to bf16 and 1.0 with P exact (the merge itself stays inside tests/merge_ref.py's bound of the fp64
    merge of the same partials: test_against_fp64).  With V away from zero the model gives 1.0 either way."""
    B, H, Hkv, Sq, D, blk, P, C = 2, 4, 2, 5, 128, 128, 256, 256
    g = torch.Generator().manual_seed(31 + lens[1])
    q_base = torch.randn(H, B, Sq, D, generator=g).to(DEV, torch.bfloat16)      # [H, B, Sq, D]: q of every item, and one item of B * Sq rows
    q, q_flat = q_base.permute(1, 0, 2, 3), q_base.view(1, H, B * Sq, D)
    kp, ks = (torch.randn(b, Hkv, n, D, generator=g).to(DEV, torch.bfloat16) for b, n in ((1, P), (B, C)))
    vp, vs = ((1.0 + 0.5 * torch.randn(b, Hkv, n, D, generator=g)).to(DEV, torch.bfloat16) for b, n in ((1, P), (B, C)))
    for b in range(B):
        ks[b, :, lens[b]:] = float("nan")
        vs[b, :, lens[b]:] = float("nan")
    kw_, vw = torch.cat([kp.expand(B, -1, -1, -1), ks], 2), torch.cat([vp.expand(B, -1, -1, -1), vs], 2)
    ones = lambda b, NK: torch.ones(b, Hkv, 1, NK, dtype=torch.bool, device=DEV)      # noqa: E731
    kw = dict(block_size=blk, return_lse=True)
    pre = ext(q_flat, kp, vp, ones(1, P // blk), causal=False, **kw)
    pre_out = pre[0][0].view(H, B, Sq, D).permute(1, 0, 2, 3)                     # back to [B, H, Sq, D]: views, no copy
    pre_lse = pre[1][0].view(H, B, Sq).permute(1, 0, 2)
    suf = ext(q, ks, vs, ones(B, C // blk), kv_len=list(lens), causal=True, **kw)
    whole = ext(q, kw_, vw, ones(B, (P + C) // blk), kv_len=[P + n for n in lens], causal=True, **kw)
    out, lse = merge([pre_out, suf[0]], [pre_lse, suf[1]])
    assert not torch.isnan(out.float()).any() and not torch.isnan(lse).any()
    items = [b for b in range(B) if lens[b] >= Sq]       # (from Sq suffix keys on, every row sees the whole prefix in both pictures)
    assert 0 in items
    for b in items:
        top = np.maximum(np.maximum(np.abs(_np(pre_out[b])), np.abs(_np(suf[0][b]))), np.abs(_np(whole[0][b])))
        err = np.abs(_np(out[b]) - _np(whole[0][b])) / ref.ulp(top, "bf16")
        wl = whole[1][b].cpu().numpy().astype(np.float64)
        lerr = np.abs(lse[b].cpu().numpy() - wl) / (2.0 ** -18 * np.maximum(1.0, np.abs(wl)))
        print(f"item {b}: out within {err.max():.3f} bf16 ulps of the one call, lse at {lerr.max():.4f} of its bound")
        assert err.max() <= 2.0 and lerr.max() <= 1.0
        assert bool((suf[1][b] > -np.inf).all()) and not torch.equal(out[b], pre_out[b])     # (the suffix did weigh in)
    for b in range(B):
        if lens[b] == 0:
            assert bool((suf[1][b] == -np.inf).all())
            assert _same((out[b], lse[b]), (pre_out[b].contiguous(), pre_lse[b].contiguous()))


# ---- 7. one graph ---------------------------------------------------------------------------------------------------------------------
def test_two_extend_calls_and_the_merge_in_one_graph_replayed_on_changed_contents():
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    B, H, Hkv, Sq, D, blk = 2, 4, 2, 5, 64, 128
    g = torch.Generator().manual_seed(41)
    q = torch.randn(B, H, Sq, D, generator=g).to(DEV, torch.bfloat16)
    k, v = (torch.randn(B, Hkv, 512, D, generator=g).to(DEV, torch.bfloat16) for _ in range(2))
    kv_len = torch.tensor([250, 131], dtype=torch.int32, device=DEV)             # of the second range; the first is full
    sink = torch.randn(H, generator=g).to(DEV)
    made = block_mask_to_lists(torch.ones(B, Hkv, 1, 2, dtype=torch.bool, device=DEV), B, Hkv)
    mask = dict(cols=made["cols"], counts=made["counts"])
    kw = dict(block_size=blk, return_lse=True, blocks_per_split=1)

    def step():
        a = ext(q, k[:, :, :256], v[:, :, :256], mask, causal=False, **kw)
        b = ext(q, k[:, :, 256:], v[:, :, 256:], mask, kv_len=kv_len, causal=True, **kw)
        return merge([a[0], b[0]], [a[1], b[1]], sink=sink)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                              # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out_g, lse_g = step()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(step(), (out_g, lse_g))
    before = out_g.clone()
    q.copy_(torch.randn(B, H, Sq, D, generator=g).to(DEV, torch.bfloat16))
    v[:, :, 100:300] = -v[:, :, 100:300]
    kv_len.copy_(torch.tensor([3, 256], dtype=torch.int32, device=DEV))          # (item 0: its first two rows now see no key of range two)
    sink.copy_(torch.tensor([-np.inf, 0.5, 3.0, -2.0], device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(step(), (out_g, lse_g))
    assert not torch.equal(out_g, before) and torch.isfinite(out_g.float()).all() and torch.isfinite(lse_g).all()
