"""Per-row key ranges of block_sparse_attention (causal=, window=, row_range=) on the MI355X: the RANGED instantiations of the
64-rows-per-wave K5 through rsa_block_sparse_ranged_fwd.  Row r of batch item b and head h sees key j iff

    block_mask[b, h, r // 128, j // 128]  and  lo[b, r] <= j < hi[b, r]  and  j < kv_len[b]  and  j < NK * 128

(the counting form of the rule lives in tests/test_ranged_cpu.py, which checks its identities without a device)."""
import contextlib

import numpy as np
import pytest
import torch

import test_ranged_cpu as rule
import visibility as vis

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {torch.bfloat16: (2e-2, 2e-3), torch.float16: (2e-3, 2e-4)}       # max, mean: tests/test_gpu_block_mask.py
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
BLK = 128
FAR = 2_000_000_000


@contextlib.contextmanager
def _tuning(key: bytes, value: int, default: int = 1):
    from rectified_spaattn_amd import _lib
    L = _lib.lib()
    try:
        assert L.rsa_set_tuning(key, value) == 0
        yield
    finally:
        L.rsa_set_tuning(key, default)


def _i32(a):
    return torch.from_numpy(np.clip(np.asarray(a, np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)).to(DEV)


# ---- range kinds: name -> (keywords of the call, lo | None, hi) with lo / hi int64 numpy [B|1, Sq] ------------------------------
WINDOWS = {"causal": (-1, 0), "window_200_0": (200, 0), "window_100_50": (100, 50), "window_unb_64": (-1, 64), "window_0_0": (0, 0)}
KINDS = list(WINDOWS) + ["chunk_208", "random", "far_outside"]


def _ranges(kind, B, Sq, Sk, lens):
    r = np.arange(Sq, dtype=np.int64)
    if kind in WINDOWS:
        left, right = WINDOWS[kind]
        lo, hi = rule.window_ranges(Sq, lens, left, right)
        return (dict(causal=True) if kind == "causal" else dict(window=(left, right))), lo, hi
    if kind == "chunk_208":        # chunk-causal, the chunk no multiple of the block: up to the end of the row's own chunk
        lo, hi = None, ((r // 208 + 1) * 208)[None, :]
    elif kind == "random":         # no order along the rows, a tenth of them empty (hi <= lo), a different draw per batch item
        g = np.random.default_rng(Sq * 7 + Sk)
        lo = g.integers(-50, Sk, (B, Sq))
        hi = lo + g.integers(1, 300, (B, Sq))
        empty = g.random((B, Sq)) < 0.1
        hi[empty] = lo[empty] - g.integers(0, 40, (B, Sq))[empty]
    else:                          # far outside [0, Sk]: the device clamps; rows see everything / nothing / nothing / keys >= r - 3
        lo = np.select([r % 4 == 0, r % 4 == 1, r % 4 == 2], [-FAR, FAR - 5, -FAR], r - 3)[None, :]
        hi = np.select([r % 4 == 0, r % 4 == 1, r % 4 == 2], [FAR, FAR, -FAR + 7], FAR)[None, :]
    return dict(row_range=(None if lo is None else _i32(lo), _i32(hi))), lo, hi


# ---- masks: name -> bool numpy [B|1, H|1, NQ, NK] -------------------------------------------------------------------------------
MASKS = ["ones", "random", "lower", "outside", "broadcast"]


def _rand_mask(g, shape, density):       # (as tests/test_gpu_block_mask.py: one empty and one full row)
    m = torch.rand(shape, generator=g) < density
    m[..., 0, :] = False
    if shape[-2] > 2:
        m[..., 1, :] = True
    return m.numpy()


def _mask(name, B, H, NQ, NK, Sq, Sk, lo, hi, lens):
    g = torch.Generator().manual_seed(NQ * 31 + NK)
    if name == "ones":             # every block listed: the kernel's trim works at both ends
        return np.ones((B, H, NQ, NK), bool)
    if name == "random":
        return _rand_mask(g, (B, H, NQ, NK), 0.5)
    if name == "lower":
        return np.broadcast_to(np.tril(np.ones((NQ, NK), bool)), (B, H, NQ, NK)).copy()
    if name == "broadcast":
        return _rand_mask(g, (1, 1, NQ, NK), 0.5)
    # "outside": exactly the blocks in which no row of the query block sees a key -> every row is 0
    seen = rule.visible(np.ones((B, 1, NQ, NK), bool), lo, hi, lens, Sq, Sk)[:, 0]          # [B, Sq, Sk]
    pad = np.zeros((B, NQ * BLK, NK * BLK), bool)
    pad[:, :Sq, :min(Sk, NK * BLK)] = seen[:, :, :NK * BLK]
    any_seen = pad.reshape(B, NQ, BLK, NK, BLK).any(axis=(2, 4))
    return np.broadcast_to(~any_seen[:, None], (B, H, NQ, NK)).copy()


def _attend(scores, v64, vis_np):
    """fp64 attention on the host from the scaled scores [B, H, Sq, Sk]: 0 for a row without a visible key."""
    visible = torch.from_numpy(vis_np)
    s = scores.masked_fill(~visible, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    e = torch.exp(s - mx).masked_fill(~visible, 0.0)
    den = e.sum(-1, keepdim=True)
    return torch.where(den > 0, torch.matmul(e, v64) / den.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))


SHAPES = {  # name -> (Sq, Sk, kv_len as given to the call)
    "640x640": (640, 640, None),
    "500x650": (500, 650, None),                        # keys > rows: the diagonal sits 150 keys to the right
    "650x500": (650, 500, None),                        # rows > keys: the first 150 rows of a causal call see nothing
    "640x640_lens_list": (640, 640, [600, 333]),
    "640x640_lens_tensor": (640, 640, "tensor"),
}
FORMS = [("bf16", 128), ("fp16", 128), ("bf16", 64), ("fp16", 64)]
AGAINST_FP64 = [(dt, D, s) for dt, D in FORMS for s in SHAPES] + [("bf16", 32, "500x650")]       # (one zero-padded head dim)


@pytest.mark.parametrize("dt,D,shape", AGAINST_FP64, ids=[f"{a}-D{b}-{c}" for a, b, c in AGAINST_FP64])
def test_ranged_attention_against_fp64(dt, D, shape):
    """Every range kind over every mask: within the plain call's tolerance of fp64 attention over the rule's keys, and a row that
    sees no key exactly 0 (all of them, with the mask whose blocks lie outside the rows' ranges)."""
    from rectified_spaattn_amd import block_sparse_attention
    B, H = 2, 3
    Sq, Sk, kv = SHAPES[shape]
    lens = [Sk] * B if kv is None else [600, 333]
    kv_arg = torch.tensor(lens, dtype=torch.int32, device=DEV) if kv == "tensor" else kv
    g = torch.Generator().manual_seed(Sq * 1000 + Sk + D)
    q, k, v = (torch.randn(B, H, s, D, generator=g).to(DEV, DT[dt]) for s in (Sq, Sk, Sk))
    scale = D ** -0.5
    scores = torch.matmul(q.double().cpu(), k.double().cpu().transpose(-1, -2)) * scale     # once; shared, never modified
    v64 = v.double().cpu()
    NQ, NK = -(-Sq // BLK), -(-Sk // BLK)
    mx, mean = TOL[DT[dt]]
    for kind in KINDS:
        kw, lo, hi = _ranges(kind, B, Sq, Sk, lens)
        for mname in MASKS:
            m = _mask(mname, B, H, NQ, NK, Sq, Sk, lo, hi, lens)
            out = block_sparse_attention(q, k, v, torch.from_numpy(m).to(DEV), kv_len=kv_arg, **kw)
            assert out.shape == (B, H, Sq, D) and out.dtype == DT[dt]
            seen = np.broadcast_to(rule.visible(m, lo, hi, lens, Sq, Sk), (B, H, Sq, Sk)).copy()   # (a mask with one head)
            ref = _attend(scores, v64, seen)
            got = out.double().cpu()
            err = (got - ref).abs()
            what = f"{kind} / {mname}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}"
            assert torch.isfinite(got).all(), what
            assert err.max() <= mx and err.mean() <= mean, what
            blind = torch.from_numpy(~seen.any(-1))
            assert float(got[blind].abs().sum()) == 0.0, f"{kind} / {mname}: a row without a visible key is not exactly 0"
            if mname == "outside":
                assert bool(blind.all())
                assert m.any() or kind in ("random", "far_outside")     # (those leave no block unseen)
        if kind == "causal" and shape == "650x500":     # (the first 150 rows were among the rows checked to be exactly 0)
            every = rule.visible(np.ones((1, 1, NQ, NK), bool), lo, hi, lens, Sq, Sk)
            assert not every[:, :, :150].any() and every[:, :, 150:].any(-1).all()


# ---- exact visibility -----------------------------------------------------------------------------------------------------------
VIS_KINDS = ["causal", "window_100_50", "chunk_208"]
VIS_SHAPES = [(640, 640), (500, 650)]
PROBE_ROWS = (0, 63, 64, 127, 17, 45, 81, 109)      # first and last row of each wave, a row in each 32-row half


def _probe_keys(lo, hi, Sq, Sk, room):
    """Keys within two of hi and of lo of PROBE_ROWS in the last and in an inner query block, hi first, as many as fit."""
    keys = []
    NQ = -(-Sq // BLK)
    for limit in (hi, lo):
        if limit is None:
            continue
        for tile in (NQ - 1, NQ // 2, 0):
            for off in PROBE_ROWS:
                r = tile * BLK + off
                if r < Sq:
                    keys += [p for p in vis.around(int(limit[0, r])) if 0 <= p < Sk and p not in keys]
    return keys[:room]


@pytest.mark.parametrize("Sq,Sk", VIS_SHAPES, ids=[f"{a}x{b}" for a, b in VIS_SHAPES])
@pytest.mark.parametrize("kind", VIS_KINDS)
@pytest.mark.parametrize("dt,D", FORMS, ids=[f"{a}-D{b}" for a, b in FORMS])
def test_ranged_attention_sees_exactly_the_documented_keys(dt, D, kind, Sq, Sk):
    """Every score exactly zero, V of 0 / 1 (tests/visibility.py): the output row is the census of its visible keys over their
    number, within one output ulp, exactly 0 where the census is.  One key on the wrong side of lo or hi moves a probe channel
    between 0 and 1 / n."""
    from rectified_spaattn_amd import block_sparse_attention
    B, H = 2, 2
    lens = [Sk] * B
    kw, lo, hi = _ranges(kind, B, Sq, Sk, lens)
    NQ, NK = -(-Sq // BLK), -(-Sk // BLK)
    m = _rand_mask(torch.Generator().manual_seed(Sq + D), (B, H, NQ, NK), 0.6)
    m[:, :, 0] = True        # (the empty row of _rand_mask is covered against fp64; here every query block shows its limits)
    wv = vis.witness_v(Sk, D, _probe_keys(lo, hi, Sq, Sk, D // 2 - 8))
    qn, kn = vis.qk_inputs(B, H, Sq, Sk, D)
    q, k = torch.from_numpy(qn).to(DEV, DT[dt]), torch.from_numpy(kn).to(DEV, DT[dt])
    v = torch.from_numpy(wv).to(DEV, DT[dt]).expand(B, H, Sk, D).contiguous()
    out = block_sparse_attention(q, k, v, torch.from_numpy(m).to(DEV), **kw)
    seen = rule.visible(m, lo, hi, lens, Sq, Sk)                                   # [B, H, Sq, Sk]
    n = seen.sum(-1)
    census = (seen.astype(np.float32) @ wv).astype(np.float64)
    ref = np.where(n[..., None] > 0, census / np.maximum(n, 1)[..., None], 0.0)
    got = out.double().cpu().numpy()
    msg = vis.violations(got, ref, vis.ULP[dt])
    assert not msg, f"{kind} {Sq}x{Sk} {dt} D{D}: {msg}"


# ---- neutral ranges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D", FORMS, ids=[f"{a}-D{b}" for a, b in FORMS])
def test_neutral_ranges_give_the_plain_calls_bytes(dt, D):
    """row_range = (0, kv_len) for every row over a mask with NO kept block at or past ceil(kv_len / 128): nothing is trimmed,
    both calls walk the same lists with the same extremes, and the bytes agree.  (With kept blocks past the limit the ranged call
    drops them before the walk, which moves another block from the asm loop to the C++-driven steps: then only the tolerance
    holds, not the bytes.)"""
    from rectified_spaattn_amd import block_sparse_attention
    B, H, Sq, Sk, kv_len = 2, 3, 700, 900, 600
    g = torch.Generator().manual_seed(D + len(dt))
    q, k, v = (torch.randn(B, H, s, D, generator=g).to(DEV, DT[dt]) for s in (Sq, Sk, Sk))
    NK = -(-kv_len // BLK)
    m = torch.from_numpy(_rand_mask(g, (B, H, -(-Sq // BLK), NK), 0.5)).to(DEV)
    plain = block_sparse_attention(q, k, v, m, kv_len=kv_len)
    lo = torch.zeros(1, Sq, dtype=torch.int32, device=DEV)
    hi = torch.full((1, Sq), kv_len, dtype=torch.int32, device=DEV)
    for rr in ((lo, hi), (None, hi), (lo.expand(B, Sq).contiguous(), hi.expand(B, Sq).contiguous())):
        ranged = block_sparse_attention(q, k, v, m, kv_len=kv_len, row_range=rr)
        assert torch.equal(plain.view(torch.int16), ranged.view(torch.int16))
    assert float(plain.float().abs().max()) > 0


# ---- no host read, one launch -----------------------------------------------------------------------------------------------------
def test_device_kv_len_is_not_read_on_the_host_and_the_batch_is_one_launch(monkeypatch):
    from rectified_spaattn_amd import _lib, block_sparse_attention
    B, H, Sq, Sk, D = 3, 2, 640, 640, 128
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, H, s, D, generator=g).to(DEV, torch.bfloat16) for s in (Sq, Sk, Sk))
    m = torch.from_numpy(_rand_mask(g, (B, H, 5, 5), 0.6)).to(DEV)
    lens = [640, 333, 517]
    on_host = block_sparse_attention(q, k, v, m, kv_len=lens, causal=True)
    kv = torch.tensor(lens, dtype=torch.int32, device=DEV)
    calls = []
    check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda status, what: (calls.append(what), check(status, what))[1])
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        on_device = block_sparse_attention(q, k, v, m, kv_len=kv, causal=True)
        try:
            kv.tolist()
            raises = False
        except RuntimeError:
            raises = True
    finally:
        torch.cuda.set_sync_debug_mode(before)
    print(f"this build raises on a host read in sync debug mode: {raises}")
    assert calls.count("rsa_block_sparse_ranged_fwd") == 1 and "rsa_block_sparse_plain_fwd" not in calls, calls
    assert torch.equal(on_device.view(torch.int16), on_host.view(torch.int16))
    # ... and the host list was one launch too (the plain call runs one per distinct limit)
    calls.clear()
    block_sparse_attention(q, k, v, m, kv_len=lens, causal=True)
    assert calls.count("rsa_block_sparse_ranged_fwd") == 1 and "rsa_block_sparse_plain_fwd" not in calls, calls
    calls.clear()
    block_sparse_attention(q, k, v, m, kv_len=lens)
    assert calls.count("rsa_block_sparse_plain_fwd") == 3 and "rsa_block_sparse_ranged_fwd" not in calls, calls


# ---- the large launches -----------------------------------------------------------------------------------------------------------
def _device_reference(q, k, v, m, rows, scale, off=0):
    """fp32 causal attention on the device for the query rows `rows` (a slice) of one head: q [Sq, D], k / v [Sk, D], m bool
    [NQ, NK] on the device."""
    Sk = k.shape[0]
    r = torch.arange(rows.start, rows.stop, device=DEV)
    j = torch.arange(Sk, device=DEV)
    seen = m[r // BLK][:, j // BLK] & (j[None, :] <= r[:, None] + off)
    s = (q[rows].float() @ k.float().t()) * scale
    s = s.masked_fill(~seen, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(seen.any(-1, keepdim=True), p, torch.zeros_like(p))
    return p @ v.float()


def test_tail_split_with_trimmed_pieces():
    """8 x 72 = 576 workgroups: one full generation of 512 and 64 walks split 4 ways (tests/test_gpu_tail_split.py), causal over a
    30 % random mask: a piece whose part of the list lies wholly right of the diagonal is trimmed to nothing and must count for
    nothing in the merge.  Split against whole within two output ulps; two heads against fp32 attention."""
    from rectified_spaattn_amd import block_sparse_attention
    H, NB, D = 8, 72, 128
    S = NB * BLK
    g = torch.Generator(device=DEV).manual_seed(72)
    q, k, v = (torch.randn(1, H, S, D, generator=g, device=DEV).to(torch.bfloat16) for _ in range(3))
    m = torch.rand(1, H, NB, NB, generator=g, device=DEV) < 0.3
    # the pieces, from the lists on the host: workgroup w >= 512 walks part (w - 512) % 4 of query block (w - 512) // 4's list
    mh = m[0].cpu().numpy()
    NBp, first, P = 72, 512, 4
    assert H * NBp - first == 64
    trimmed = walked = 0
    for vv in range(first, H * NBp):
        h, jj = divmod(vv, NBp)
        qb = (jj & 7) * (NBp // 8) + (jj >> 3)
        cols = np.nonzero(mh[h, qb])[0]
        per = -(-len(cols) // P)
        for p in range(P):
            part = cols[p * per:(p + 1) * per]
            if len(part):
                walked += 1
                trimmed += int((part > qb).all())        # block j is seen by some row of block qb iff j <= qb
    assert trimmed > 0 and walked > trimmed, (trimmed, walked)
    outs = {}
    for split in (0, 1):
        with _tuning(b"k5_tail_split", split):
            outs[split] = block_sparse_attention(q, k, v, m, causal=True)
            torch.cuda.synchronize()
    whole, split = outs[0].float(), outs[1].float()
    assert torch.isfinite(split).all()
    diff = (split - whole).abs()
    assert float(diff.max()) <= 2 * 2.0 ** -7 * max(1.0, float(whole.abs().max()))
    assert float(diff.max()) > 0, "the case has no tail to split"
    mx, mean = TOL[torch.bfloat16]
    for h in (0, H - 1):
        ref = _device_reference(q[0, h], k[0, h], v[0, h], m[0, h], slice(0, S), D ** -0.5)
        err = (split[0, h] - ref).abs()
        assert float(err.max()) <= mx and float(err.mean()) <= mean, (h, float(err.max()), float(err.mean()))


def test_launch_of_3072_walks_with_aligned_starts():
    """24 heads x 128 query blocks, causal over a 25 % random mask: walks of 1 to ~32 kept blocks after the trim, six generations
    of workgroups, so the launch carries the start counters and every walk announces itself and passes the wait with its TRIMMED
    length.  Finite; the same bytes with the counters off; three query blocks of two heads against fp32 attention."""
    from rectified_spaattn_amd import block_sparse_attention
    H, S, D = 24, 16384, 128
    NB = S // BLK
    g = torch.Generator(device=DEV).manual_seed(3072)
    q, k, v = (torch.randn(1, H, S, D, generator=g, device=DEV).to(torch.bfloat16) for _ in range(3))
    m = torch.rand(1, H, NB, NB, generator=g, device=DEV) < 0.25
    outs = {}
    for gsync in (1, 0):
        with _tuning(b"k5_gsync", gsync):
            outs[gsync] = block_sparse_attention(q, k, v, m, causal=True)
            torch.cuda.synchronize()
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    mx, mean = TOL[torch.bfloat16]
    for h in (3, 23):
        for qb in (0, 61, NB - 1):
            rows = slice(qb * BLK, (qb + 1) * BLK)
            ref = _device_reference(q[0, h], k[0, h], v[0, h], m[0, h], rows, D ** -0.5)
            err = (outs[1][0, h, rows].float() - ref).abs()
            assert float(err.max()) <= mx and float(err.mean()) <= mean, (h, qb, float(err.max()), float(err.mean()))


def test_static_and_online_body_agree():
    """bf16, causal: the optimistic static softmax reference (entered only by waves whose rows all have a finite reference) and
    the online body alone, both within the tolerance of fp64."""
    from rectified_spaattn_amd import block_sparse_attention
    B, H, Sq, Sk, D = 1, 3, 1500, 1500, 128
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B, H, s, D, generator=g).to(DEV, torch.bfloat16) for s in (Sq, Sk, Sk))
    NQ = -(-Sq // BLK)
    m = _rand_mask(g, (B, H, NQ, NQ), 0.7)
    seen = rule.visible(m, *rule.window_ranges(Sq, [Sk], -1, 0), [Sk], Sq, Sk)
    scores = torch.matmul(q.double().cpu(), k.double().cpu().transpose(-1, -2)) * D ** -0.5
    ref = _attend(scores, v.double().cpu(), seen)
    mx, mean = TOL[torch.bfloat16]
    for static in (0, 1):
        with _tuning(b"k5_static", static):
            out = block_sparse_attention(q, k, v, torch.from_numpy(m).to(DEV), causal=True)
            torch.cuda.synchronize()
        err = (out.double().cpu() - ref).abs()
        assert err.max() <= mx and err.mean() <= mean, f"k5_static={static}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}"
