"""Walk order of the 64-row K5 (rsa_walk_order.h, rsa_attn.hip::walk_order_unit_kernel and _sort_kernel; tuning keys k5_walk_order, k5_order_overlap).
With the order on, every XCD generation holds a run of consecutive walks of ONE head, the head's units sorted by the mean of
their kept key blocks (or left in index order where adjacent lists overlap by the threshold or more).  Which workgroup walks which
unit changes; what a walk computes does not: every result must be the same BYTES as with k5_walk_order = 0, the eighth map.
`out` is filled with a NaN pattern in front of every attend(), so a unit that no workgroup walks cannot pass on stale bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(H, nb, D, seed, dt, repeat=1, S=None):
    """Block centroids + noise (as tests/test_gpu_gsync.py); repeat = 8: the centroids repeat over 8 consecutive blocks, so the
    query blocks of a group keep nearly the same lists."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    S = nb * 128 if S is None else S
    cent = torch.randn(H, (nb + repeat - 1) // repeat, D, generator=g, device=DEV).repeat_interleave(repeat, 1)[:, :nb]

    def mk():
        return (cent.repeat_interleave(128, 1)[:, :S] + 0.7 * torch.randn(H, S, D, generator=g, device=DEV)).to(dt).view(1, H, S, D)
    return mk(), mk(), torch.randn(1, H, S, D, generator=g, device=DEV).to(dt)


class _Tuning:
    """rsa_set_tuning for the length of a with block; the product's defaults afterwards."""
    DEFAULTS = {b"k5_walk_order": 1, b"k5_order_overlap": 50, b"k5_tail_split": 1}

    def __init__(self):
        from rectified_spaattn_amd import _lib
        self.L = _lib.lib()

    def __enter__(self):
        return self

    def set(self, **kv):
        for key, val in kv.items():
            assert self.L.rsa_set_tuning(key.encode(), int(val)) == 0, key

    def __exit__(self, *exc):
        for key, val in self.DEFAULTS.items():
            self.L.rsa_set_tuning(key, val)


def _attend(call):
    """attend() into an `out` full of NaNs (0xFFFF is a NaN in bf16 and in fp16); the bytes of the result."""
    call.out.view(torch.int16).fill_(-1)
    call.attend()
    torch.cuda.synchronize()
    return call.out.view(torch.int16).cpu().numpy().copy()


def _table(call, H, D, tail_pieces=0):
    """The order table of the last attend(): u16 [BH, NBp] behind the text pieces' and the tail pieces' regions of tpart."""
    from rectified_spaattn_amd import _lib
    spec = call.spec
    NBp = (spec.NBv + 7) // 8 * 8
    pieces = H * (spec.NB_total - spec.NBv) * _lib.TEXT_SPLIT + tail_pieces
    flat = call.bufs["tpart"].view(-1)[pieces * 128 * (D + 2):].view(torch.int16)[:H * NBp]
    return flat.cpu().numpy().view(np.uint16).reshape(H, NBp).astype(np.int64)


def _sorted_table(call, H, n_whole=None, identity=False):
    """What the order kernels write: the units that are whole walks by (mean kept block in 1/64, unit) -- or in index order --, pads
    0xFFFF behind them; from work index n_whole on (a split tail) the units of the eighth map at their own ranks."""
    spec = call.spec
    NBp = (spec.NBv + 7) // 8 * 8
    cols = call.bufs["cols"].cpu().numpy().reshape(H, spec.NBv, -1).astype(np.int64)
    cnt = call.bufs["counts"].cpu().numpy().reshape(H, spec.NBv).astype(np.int64)
    want = np.full((H, NBp), 0xFFFF, dtype=np.int64)
    n_whole = H * NBp if n_whole is None else n_whole
    for h in range(H):
        r0 = min(max(n_whole - h * NBp, 0), NBp)
        keys = []
        for u in range(spec.NBv):
            if (u % (NBp // 8)) * 8 + u // (NBp // 8) >= r0:      # walked in pieces, by the eighth map
                continue
            n = int(cnt[h, u])
            keys.append((0 if identity else (((int(cols[h, u, :n].sum()) << 6) // n) if n else 0x7FFFE), u))
        want[h, :len(keys)] = [u for _, u in sorted(keys)]
        for r in range(r0, NBp):
            u = (r & 7) * (NBp // 8) + (r >> 3)
            want[h, r] = u if u < spec.NBv else 0xFFFF
    return want


def _adjacent_overlap(call, H):
    """mean over the units of |list_i & list_i+1| / |list_i|, per head"""
    from rectified_spaattn_amd import _core
    spec = call.spec
    res = []
    for h in range(H):
        bm = _core.unpack_bitmask(call.bufs["bitmask"][h], spec.NB_total)[:spec.NBv].bool()
        own = bm[:-1].sum(1).float()
        res.append(float(((bm[:-1] & bm[1:]).sum(1).float() / own)[own > 0].mean()))
    return res


def _identical_in_both_orders(call, seq=(0, 1, 0, 1), **extra):
    outs = []
    with _Tuning() as t:
        t.set(k5_tail_split=0, **extra)
        for order in seq:
            t.set(k5_walk_order=order)
            outs.append(_attend(call))
    assert np.isfinite(call.out.float().cpu().numpy()).all(), "a unit was never walked (or the result is not finite)"
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    return outs[0]


@pytest.mark.parametrize("D,dt", [(128, torch.bfloat16), (128, torch.float16), (64, torch.bfloat16), (64, torch.float16)])
def test_walk_order_does_not_change_a_byte(D, dt):
    """8 heads x 168 blocks, top_k 14: 1 344 workgroups, more than two generations of 8 x 64 -- the walks wait for their generation,
    and with the order on most runs of 64 lie inside one head, some straddle two."""
    from rectified_spaattn_amd import _core
    H, nb = 8, 168
    q, k, v = _inputs(H, nb, D, 11, dt)
    call = _core.StagedCall(q, k, v, _core.LayoutSpec.wan(nb * 128, 0), 14, 0.05, None)
    call.select()
    _identical_in_both_orders(call)
    assert np.array_equal(_table(call, H, D), _sorted_table(call, H)), "iid centroids: the heads are sorted by mean kept block"


def test_walk_order_with_padding_units_and_unequal_lists():
    """165 blocks (3 pad entries per head, which must stay idle workgroups), and p_remain 0.3 with a banded neighbour matrix: lists
    of unequal length."""
    from rectified_spaattn_amd import _core, synth
    H, nb = 8, 165
    q, k, v = _inputs(H, nb, 128, 12, torch.bfloat16)
    spec = _core.LayoutSpec.wan(nb * 128, 0)
    call = _core.StagedCall(q, k, v, spec, 14, 0.05, None)
    call.select()
    _identical_in_both_orders(call)
    tab = _table(call, H, 128)
    assert (tab[:, nb:] == 0xFFFF).all() and np.array_equal(np.sort(tab[:, :nb], axis=1), np.tile(np.arange(nb), (H, 1)))
    call = _core.StagedCall(q, k, v, spec, 14, 0.3, torch.from_numpy(synth.banded_neighbors(spec.NBv, 1)))
    call.select()
    cnt = call.bufs["counts"]
    assert int(cnt.min()) < int(cnt.max()), "the case has lists of one length only"
    _identical_in_both_orders(call)


def test_walk_order_on_a_layout_with_text_rows():
    """HunyuanVideo-type layout (190 visual blocks + a 256-token text tail, 200 valid), 6 heads: the split text-row pieces are the
    last workgroups of the grid, the sparse units start at work index 0 and are dealt in runs; the table sits behind the text pieces."""
    from rectified_spaattn_amd import _core
    H, nbv = 6, 190
    S = (nbv + 2) * 128
    q, k, v = _inputs(H, nbv + 2, 128, 31, torch.bfloat16)
    call = _core.StagedCall(q, k, v, _core.LayoutSpec.hunyuan(S, S - 56), 16, 0.05, None)
    call.select()
    _identical_in_both_orders(call)
    assert np.array_equal(_table(call, H, 128), _sorted_table(call, H))


def test_walk_order_on_less_than_one_generation():
    """One head of 60 blocks: 64 workgroups, no full generation -- position = work index, the unit comes from the table."""
    from rectified_spaattn_amd import _core
    q, k, v = _inputs(1, 60, 128, 14, torch.bfloat16)
    call = _core.StagedCall(q, k, v, _core.LayoutSpec.wan(60 * 128, 0), 8, 0.05, None)
    call.select()
    _identical_in_both_orders(call)


@pytest.mark.parametrize("repeat", [8, 1], ids=["lists-repeat", "lists-iid"])
def test_both_branches_of_the_order_kernel(repeat):
    """Centroids that repeat over 8 consecutive blocks: adjacent query blocks keep nearly the same lists, the head stays in index
    order (the identity branch); iid centroids: sorted.  The threshold keys 0 and 100 force each branch on both inputs; the bytes of
    O never change, and the table is exactly the branch's."""
    from rectified_spaattn_amd import _core
    H, nb = 8, 168
    q, k, v = _inputs(H, nb, 128, 15, torch.bfloat16, repeat=repeat)
    call = _core.StagedCall(q, k, v, _core.LayoutSpec.wan(nb * 128, 0), 14, 0.05, None)
    call.select()
    ovl = _adjacent_overlap(call, H)
    print(f"repeat {repeat}: adjacent overlap per head {[round(x, 3) for x in ovl]}")
    assert all(x > 0.6 for x in ovl) if repeat == 8 else all(x < 0.4 for x in ovl), "the input does not sit on the side of 50 % it is meant for"
    identity = np.full((H, nb), 0, dtype=np.int64) + np.arange(nb)
    ref = _identical_in_both_orders(call)
    assert np.array_equal(_table(call, H, 128), identity if repeat == 8 else _sorted_table(call, H))
    assert np.array_equal(_identical_in_both_orders(call, seq=(1, 0, 1), k5_order_overlap=0), ref)
    assert np.array_equal(_table(call, H, 128), identity)
    assert np.array_equal(_identical_in_both_orders(call, seq=(1, 0, 1), k5_order_overlap=100), ref)
    assert np.array_equal(_table(call, H, 128), _sorted_table(call, H))


def test_walk_order_beside_a_split_tail():
    """4 heads x 168 blocks, no text: 672 workgroups = one generation + 160 tail units x 3 pieces, WITH a table: the 512 whole walks
    are dealt in runs in sorted order, the pieces stay the eighth map's units.  The table (read back from behind the 480 tail
    pieces) is exactly that; every unit that is a whole walk in both orders is byte-identical to the run without a table -- so are
    the split ones, which are the same units cut the same way --; O agrees with the oracle within the operator tests' tolerance."""
    from oracle import oracle as orc
    from rectified_spaattn_amd import _core
    H, nb, top_k = 4, 168, 14
    S = nb * 128
    q, k, v = _inputs(H, nb, 128, 16, torch.bfloat16)
    call = _core.StagedCall(q, k, v, _core.LayoutSpec.wan(S, 0), top_k, 0.05, None)
    call.select()
    outs = {}
    with _Tuning() as t:
        t.set(k5_walk_order=1, k5_tail_split=0)
        whole = _attend(call)
        for order in (0, 1):
            t.set(k5_walk_order=order, k5_tail_split=1)
            call.bufs["tpart"].fill_(-7.0)              # (no table left over from the launch before)
            outs[order] = _attend(call)
            table = _table(call, H, 128, tail_pieces=160 * 3)
            if order == 0:
                flat = table.reshape(-1)                                              # (-7.0f is the two halves 0x0000, 0xC0E0)
                assert (flat[0::2] == 0).all() and (flat[1::2] == 0xC0E0).all(), "k5_walk_order = 0 wrote a table"
    got = call.out.float().cpu().numpy()            # [1, S, H, D]: order on, tail split on
    assert np.isfinite(got).all()
    want = _sorted_table(call, H, n_whole=512)
    assert np.array_equal(table, want), "the launch with a split tail has no table, or not the one of the whole walks"
    assert not np.array_equal(want[:3, :nb], np.tile(np.arange(nb), (3, 1))), "the case's table is the index order"
    split = np.zeros((H, nb), dtype=bool)
    for vv in range(512, H * nb):                   # NBp = 168: the units behind the last full generation, in both orders
        h, j = divmod(vv, nb)
        split[h, (j & 7) * (nb // 8) + (j >> 3)] = True
    assert split.sum() == 160
    differs = (outs[0] != outs[1]).reshape(nb, 128, H, 128).any(axis=(1, 3)).T      # [H, nb]
    assert not differs[~split].any(), "a unit that is a whole walk in both orders changed"
    assert not differs[split].any(), "a split unit changed: the same pieces of the same units must give the same bytes"
    cut = (outs[1] != whole).reshape(nb, 128, H, 128).any(axis=(1, 3)).T
    assert not cut[~split].any() and cut[split].any(), "the units walked in pieces are not the eighth map's"
    hd = 3                                          # the head the tail units belong to
    assert split[hd].any()
    qf, kf, vf = (x[0, hd].float().cpu().numpy() for x in (q, k, v))
    ref = orc.rectified_attention(qf[None, None], kf[None, None], vf[None, None], orc.layout_wan(S, 0), top_k, 0.05, None)
    err = np.abs(got[0, :, hd] - ref.reshape(S, 128))
    print(f"order on, tail split on: max|dO| {err.max():.3e} mean|dO| {err.mean():.3e}")
    assert err.max() <= 2e-2 and err.mean() <= 2e-3


def test_walk_order_inside_a_captured_graph():
    """The order kernel is one more node on the caller's stream: capture select + attend (order on), replay twice on new inputs,
    equal to the eager result."""
    from rectified_spaattn_amd import _core
    H, nb, top_k = 8, 168, 14
    q, k, v = _inputs(H, nb, 128, 21, torch.bfloat16)
    q2, k2, v2 = _inputs(H, nb, 128, 22, torch.bfloat16)
    spec = _core.LayoutSpec.wan(nb * 128, 0)
    call = _core.StagedCall(q, k, v, spec, top_k, 0.05, None)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call.select()                    # (torch's capture needs the allocator warm; K5 itself is NOT run before the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call.select()
        call.attend()
    eager = _core.StagedCall(q2, k2, v2, spec, top_k, 0.05, None)
    eager.select()
    want = _attend(eager)
    for _ in range(2):
        q.copy_(q2); k.copy_(k2); v.copy_(v2)
        call.out.view(torch.int16).fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(call.out.view(torch.int16).cpu().numpy(), want)
    assert np.array_equal(_table(call, H, 128), _sorted_table(eager, H))


def test_head_shard_with_the_order_on():
    """rsa_set_shard_invariant(1): a 2-head shard of an 8-head call (336 workgroups, less than a generation, against 1 344) is
    byte-identical to the unsharded call -- the order moves walks between workgroups, never a row's arithmetic."""
    from rectified_spaattn_amd import _core, parallel
    H, nb, top_k = 8, 168, 14
    q, k, v = _inputs(H, nb, 128, 23, torch.bfloat16)
    spec = _core.LayoutSpec.wan(nb * 128, 0)
    prev = parallel.set_shard_invariant(True)
    try:
        full = _core.StagedCall(q, k, v, spec, top_k, 0.05, None)
        full.select()
        want = _attend(full).reshape(nb * 128, H, 128)
        for h0 in (0, 6):
            part = _core.StagedCall(q[:, h0:h0 + 2].contiguous(), k[:, h0:h0 + 2].contiguous(), v[:, h0:h0 + 2].contiguous(), spec,
                                    top_k, 0.05, None)
            part.select()
            got = _attend(part).reshape(nb * 128, 2, 128)
            assert np.isfinite(part.out.float().cpu().numpy()).all()
            assert np.array_equal(got, want[:, h0:h0 + 2]), f"heads {h0}, {h0 + 1}: O differs"
            assert np.array_equal(_table(part, 2, 128), _sorted_table(part, 2)), "the shard's launch ran without its table"
        assert np.array_equal(_table(full, H, 128), _sorted_table(full, H)), "the unsharded launch ran without its table"
    finally:
        parallel.set_shard_invariant(prev)
