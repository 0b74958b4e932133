"""Grouped-query K/V heads of block_sparse_attention on the MI355X (rsa_block_sparse_gqa_fwd): k / v hold Hkv heads, query head h
reads K/V head h // (H // Hkv), the mask's head axis is H, Hkv or 1.  Two forms of the launch (tuning key
k5_gqa_pair): (a) every query head a walk of its own, (b) two query heads of one K/V head and one list row on one K/V ring.

    (a) = today's call on repeat_interleave'd K/V and an expanded mask, byte for byte
    (b) = (a), byte for byte (no walk here overflows the static softmax reference, and no grid here reaches the tail split)
    both within the plain call's tolerance of fp64 attention over the visibility rule of tests/test_ranged_cpu.py
"""
import contextlib
import itertools

import numpy as np
import pytest
import torch

import test_ranged_cpu as rule
import visibility as vis
from test_gpu_ranged import _attend, _rand_mask, _ranges

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = {torch.bfloat16: (2e-2, 2e-3), torch.float16: (2e-3, 2e-4)}       # max, mean: tests/test_gpu_block_mask.py
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
FORMS = [("bf16", 128), ("fp16", 128), ("bf16", 64), ("fp16", 64)]
B = 2
HEADS = [(8, 1), (8, 2), (8, 4), (6, 2)]                # (H, Hkv); the last has g = 3: no two neighbours share a K/V head
SHAPES = [(300, 520), (640, 640), (650, 500)]           # (Sq, Sk)
LENS = [500, 333]
KV_LENS = ["none", "list", "tensor"]
AXES = ["H", "Hkv", "1"]                                # the mask's head axis
RANGE_KINDS = ["causal", "window_100_50", "chunk_208", "random"]


@contextlib.contextmanager
def _pair(value: int):
    """Form (b) where the call is eligible (1) or form (a) throughout (0)."""
    from rectified_spaattn_amd import _lib
    L = _lib.lib()
    try:
        assert L.rsa_set_tuning(b"k5_gqa_pair", value) == 0
        yield
    finally:
        L.rsa_set_tuning(b"k5_gqa_pair", _lib.GQA_PAIR_DEFAULT)


def _kv(which, Sk):
    """-> (kv_len as given to the call, the B limits it stands for)"""
    if which == "none":
        return None, [Sk] * B
    return (LENS if which == "list" else torch.tensor(LENS, dtype=torch.int32, device=DEV)), LENS


def _inputs(H, Hkv, Sq, Sk, D, dt, seed=0):
    """q [B, H, Sq, D]; k, v [B, Hkv, Sk, D], drawn independently per K/V head."""
    g = torch.Generator().manual_seed(Sq * 1000 + Sk + D + 17 * H + Hkv + seed)
    return tuple(torch.randn(B, h, s, D, generator=g).to(DEV, DT[dt]) for h, s in ((H, Sq), (Hkv, Sk), (Hkv, Sk)))


def _mask_np(axis, H, Hkv, NQ, NK):
    heads = {"H": H, "Hkv": Hkv, "1": 1}[axis]
    return _rand_mask(torch.Generator().manual_seed(NQ * 31 + NK + heads), (B, heads, NQ, NK), 0.5)


def _expand_heads(m, H):
    """The mask per query head: list head h // (H // heads) for every query head h (torch.Tensor or numpy)."""
    g = H // m.shape[1]
    return m.repeat_interleave(g, dim=1) if isinstance(m, torch.Tensor) else np.repeat(m, g, axis=1)


def _bytes(t):
    return t.view(torch.int16)


def _visible(m, lo, hi, lens, Sq, Sk, blk):
    """bool [B, heads, Sq, Sk]: the rule of tests/test_ranged_cpu.py (128-token blocks; a plain call is the range [0, Sk) for
    every row), and the plain call's rule for 64-token blocks, which take no range."""
    if blk == rule.BLK:
        return rule.visible(m, lo, np.full((1, Sq), Sk) if hi is None else hi, lens, Sq, Sk)
    assert lo is None and hi is None
    NK = m.shape[-1]
    j, r = np.arange(Sk), np.arange(Sq)
    kept = m[:, :, r // blk][..., np.minimum(j // blk, NK - 1)] & (j < NK * blk)
    return kept & (j[None, None, None, :] < np.asarray(lens)[:, None, None, None])


def _combos(blk):
    """(H, Hkv, Sq, Sk, axis, kv_len, range kind | None): every head grouping x shape x mask axis x kv_len form of the plain call;
    at 128-token blocks every range kind over every grouping x shape x axis as well, the kv_len forms taking turns."""
    out = [(H, Hkv, Sq, Sk, ax, kv, None) for (H, Hkv), (Sq, Sk), ax, kv in itertools.product(HEADS, SHAPES, AXES, KV_LENS)]
    if blk == 128:
        turn = itertools.cycle(KV_LENS)
        out += [(H, Hkv, Sq, Sk, ax, next(turn), kind)
                for (H, Hkv), (Sq, Sk), ax, kind in itertools.product(HEADS, SHAPES, AXES, RANGE_KINDS)]
    return out


def _pairable(H, Hkv, axis, blk):
    from rectified_spaattn_amd.block_sparse import gqa_pairable
    return gqa_pairable(H, Hkv, {"H": H, "Hkv": Hkv, "1": 1}[axis], blk)


# ---- 1. form (a) is the MHA call on repeated K/V ---------------------------------------------------------------------------------
A_CASES = [(dt, D, blk) for dt, D in FORMS for blk in (128, 64)] + [("bf16", 32, 128)]


@pytest.mark.parametrize("dt,D,blk", A_CASES, ids=[f"{a}-D{b}-b{c}" for a, b, c in A_CASES])
def test_per_head_form_equals_mha_on_repeated_kv_byte_for_byte(dt, D, blk):
    from rectified_spaattn_amd import block_sparse_attention
    cache = {}
    n = 0
    with _pair(0):
        for H, Hkv, Sq, Sk, axis, kvw, kind in _combos(blk):
            if (H, Hkv, Sq, Sk) not in cache:
                q, k, v = _inputs(H, Hkv, Sq, Sk, D, dt)
                cache[H, Hkv, Sq, Sk] = (q, k, v, k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1))
            q, k, v, kx, vx = cache[H, Hkv, Sq, Sk]
            kv, lens = _kv(kvw, Sk)
            kw = dict(block_size=blk) if kind is None else _ranges(kind, B, Sq, Sk, lens)[0]
            m = torch.from_numpy(_mask_np(axis, H, Hkv, -(-Sq // blk), -(-Sk // blk))).to(DEV)
            got = block_sparse_attention(q, k, v, m, kv_len=kv, **kw)
            want = block_sparse_attention(q, kx, vx, _expand_heads(m, H), kv_len=kv, **kw)
            assert got.shape == (B, H, Sq, D) and got.dtype == DT[dt]
            assert torch.equal(_bytes(got), _bytes(want)), (H, Hkv, Sq, Sk, axis, kvw, kind)
            n += 1
    assert float(got.float().abs().max()) > 0 and n == len(_combos(blk))


# ---- 2. form (b) is form (a) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D", FORMS, ids=[f"{a}-D{b}" for a, b in FORMS])
def test_paired_form_equals_per_head_form_byte_for_byte(dt, D):
    """Every pairable combination, plain and ranged; the others (g = 3, a mask per query head, 64-token blocks) fall back to form
    (a) and give the same bytes under both settings."""
    from rectified_spaattn_amd import block_sparse_attention
    cache = {}
    paired = others = 0
    for blk in (128, 64):
        for H, Hkv, Sq, Sk, axis, kvw, kind in _combos(blk):
            if (H, Hkv, Sq, Sk) not in cache:
                cache[H, Hkv, Sq, Sk] = _inputs(H, Hkv, Sq, Sk, D, dt)
            q, k, v = cache[H, Hkv, Sq, Sk]
            kv, lens = _kv(kvw, Sk)
            kw = dict(block_size=blk) if kind is None else _ranges(kind, B, Sq, Sk, lens)[0]
            m = torch.from_numpy(_mask_np(axis, H, Hkv, -(-Sq // blk), -(-Sk // blk))).to(DEV)
            outs = []
            for form in (0, 1):
                with _pair(form):
                    outs.append(block_sparse_attention(q, k, v, m, kv_len=kv, **kw))
            assert torch.equal(_bytes(outs[0]), _bytes(outs[1])), (H, Hkv, Sq, Sk, axis, kvw, kind, blk)
            if _pairable(H, Hkv, axis, blk):
                paired += 1
            else:
                others += 1
    # H = 8 with the mask per K/V head or for all heads, 128-token blocks: 3 groupings x 3 shapes x 2 axes x (3 kv_len + 4 kinds)
    assert paired == 3 * 3 * 2 * 7 and others > 0


# ---- 3. both forms against fp64 --------------------------------------------------------------------------------------------------
FP64_CASES = [(dt, D, s) for dt, D in FORMS for s in range(len(SHAPES))] + [("bf16", 32, 0)]


@pytest.mark.parametrize("dt,D,shape", FP64_CASES, ids=[f"{a}-D{b}-{SHAPES[c][0]}x{SHAPES[c][1]}" for a, b, c in FP64_CASES])
def test_both_forms_against_fp64(dt, D, shape):
    """Per grouping: plain at both block sizes and two range kinds at 128, the mask axes and kv_len forms taking turns.  First, on
    the host: the reference built with the WRONG head map (h % Hkv) lies outside the tolerance, so these inputs tell the maps apart."""
    from rectified_spaattn_amd import block_sparse_attention
    Sq, Sk = SHAPES[shape]
    mx, mean = TOL[DT[dt]]
    scale = D ** -0.5
    axes, kvs = itertools.cycle(AXES), itertools.cycle(KV_LENS)
    for H, Hkv in HEADS:
        q, k, v = _inputs(H, Hkv, Sq, Sk, D, dt, seed=3)
        g = H // Hkv
        q64, k64, v64 = q.double().cpu(), k.double().cpu(), v.double().cpu()
        right = torch.arange(H) // g
        scores = torch.matmul(q64, k64[:, right].transpose(-1, -2)) * scale        # once per grouping; shared, never modified
        vx = v64[:, right]
        if Hkv in (2, 4):
            wrong = torch.arange(H) % Hkv
            everything = np.ones((B, H, Sq, Sk), bool)
            d = (_attend(torch.matmul(q64, k64[:, wrong].transpose(-1, -2)) * scale, v64[:, wrong], everything)
                 - _attend(scores, vx, everything)).abs()
            print(f"H {H} Hkv {Hkv}: wrong map against right map, max {float(d.max()):.3e} mean {float(d.mean()):.3e}")
            assert d.max() > mx and d.mean() > mean
        for blk, kind in ((128, None), (64, None), (128, "causal"), (128, "random")):
            axis, (kv, lens) = next(axes), _kv(next(kvs), Sk)
            kw, lo, hi = (dict(block_size=blk), None, None) if kind is None else _ranges(kind, B, Sq, Sk, lens)
            m = _mask_np(axis, H, Hkv, -(-Sq // blk), -(-Sk // blk))
            seen = _visible(_expand_heads(m, H), lo, hi, lens, Sq, Sk, blk)
            ref = _attend(scores, vx, seen)
            blind = torch.from_numpy(~seen.any(-1))
            assert bool(blind.any()) and not bool(blind.all())
            for form in (0, 1):
                with _pair(form):
                    out = block_sparse_attention(q, k, v, torch.from_numpy(m).to(DEV), kv_len=kv, **kw)
                got = out.double().cpu()
                err = (got - ref).abs()
                what = f"H {H} Hkv {Hkv} block {blk} {kind} axis {axis} form {'ab'[form]}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}"
                print(what)
                assert torch.isfinite(got).all(), what
                assert err.max() <= mx and err.mean() <= mean, what
                assert float(got[blind].abs().sum()) == 0.0, f"{what}: a row without a visible key is not exactly 0"


# ---- 4. exact visibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "causal"], ids=["plain", "causal"])
@pytest.mark.parametrize("H,Hkv", [(8, 2), (8, 1), (6, 2)], ids=["H8-Hkv2", "H8-Hkv1", "H6-Hkv2"])
@pytest.mark.parametrize("dt,D", FORMS, ids=[f"{a}-D{b}" for a, b in FORMS])
def test_grouped_attention_sees_exactly_the_documented_keys_of_its_kv_head(dt, D, H, Hkv, kind):
    """Every score exactly zero, V of 0 / 1 (tests/visibility.py): the output row is the census of its visible keys over their
    number.  K/V head c also sets channel D/2 - 1 - c for every key, and no other head does: that channel of query head h is 1 iff
    c == h // g (0 iff not), so the output names the K/V head it read as well as the keys."""
    from rectified_spaattn_amd import block_sparse_attention
    Sq, Sk = 640, 640
    lens = [Sk] * B
    NQ = NK = Sq // 128
    kw, lo, hi = (dict(), None, None) if kind is None else _ranges(kind, B, Sq, Sk, lens)
    m = _rand_mask(torch.Generator().manual_seed(Sq + D + Hkv), (B, Hkv, NQ, NK), 0.6)     # one mask row per K/V head
    m[:, :, 0] = True
    probes = [0, Sk - 1] + ([] if hi is None else [p for r in (0, 63, 64, 127, 300, 639) for p in vis.around(int(hi[0, r]))])
    base = vis.witness_v(Sk, D, [p for p in probes if 0 <= p < Sk][:D // 2 - 8])
    wv = np.repeat(base[None], Hkv, 0)                                                       # [Hkv, Sk, D]
    for c in range(Hkv):
        wv[:, :, D // 2 - 1 - c] = 0
        wv[c, :, D // 2 - 1 - c] = 1
    qn, kn = vis.qk_inputs(B, H, Sq, Sk, D)
    q = torch.from_numpy(qn).to(DEV, DT[dt])
    k = torch.from_numpy(kn[:, :Hkv]).to(DEV, DT[dt])
    v = torch.from_numpy(wv).to(DEV, DT[dt]).expand(B, Hkv, Sk, D).contiguous()
    g = H // Hkv
    seen = _visible(_expand_heads(m, H), lo, hi, lens, Sq, Sk, 128)                          # [B, H, Sq, Sk]
    n = seen.sum(-1)
    census = np.einsum("bhrk,hkd->bhrd", seen.astype(np.float32), wv[np.arange(H) // g]).astype(np.float64)
    ref = np.where(n[..., None] > 0, census / np.maximum(n, 1)[..., None], 0.0)
    for h in range(H):      # (the reference itself names the heads: 1 in the channel of h // g, 0 in the others', wherever a key is seen)
        for c in range(Hkv):
            assert np.array_equal(ref[:, h, :, D // 2 - 1 - c], (n[:, h] > 0) * float(c == h // g))
    for form in (0, 1):
        with _pair(form):
            out = block_sparse_attention(q, k, v, torch.from_numpy(m).to(DEV), **kw)
        msg = vis.violations(out.double().cpu().numpy(), ref, vis.ULP[dt])
        assert not msg, f"form {'ab'[form]} {dt} D{D} H{H} Hkv{Hkv} {kind}: {msg}"


# ---- 5. the fused-projection layout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("H,Hkv", [(8, 2), (8, 1), (6, 2)], ids=["H8-Hkv2", "H8-Hkv1", "H6-Hkv2"])
def test_views_of_one_fused_projection_run_without_a_copy(monkeypatch, H, Hkv, D):
    from rectified_spaattn_amd import _core, block_sparse_attention
    S = 640
    g = torch.Generator().manual_seed(H + Hkv + D)
    buf = torch.randn(B, S, (H + 2 * Hkv) * D, generator=g).to(DEV, torch.bfloat16)
    q = buf[..., :H * D].view(B, S, H, D).permute(0, 2, 1, 3)
    k = buf[..., H * D:(H + Hkv) * D].view(B, S, Hkv, D).permute(0, 2, 1, 3)
    v = buf[..., (H + Hkv) * D:].view(B, S, Hkv, D).permute(0, 2, 1, 3)
    m = torch.from_numpy(_mask_np("Hkv", H, Hkv, 5, 5)).to(DEV)
    seen = []
    as_bhsd = _core._as_bhsd
    monkeypatch.setattr(_core, "_as_bhsd", lambda t: (seen.append((t.data_ptr(), as_bhsd(t).data_ptr())), as_bhsd(t))[1])
    for kw in (dict(), dict(causal=True)):
        for form in (0, 1):
            seen.clear()
            with _pair(form):
                out = block_sparse_attention(q, k, v, m, **kw)
            assert [a for a, _ in seen] == [q.data_ptr(), k.data_ptr(), v.data_ptr()] and all(a == b for a, b in seen), seen
            with _pair(form):
                want = block_sparse_attention(q.contiguous(), k.contiguous(), v.contiguous(), m, **kw)
            assert torch.equal(_bytes(out), _bytes(want))
    assert float(out.float().abs().max()) > 0


# ---- 6. the redo in a pair -------------------------------------------------------------------------------------------------------
def test_one_head_of_a_pair_overflows_the_static_reference_and_both_are_redone():
    """Heads 0 and 1 share K/V head 0.  Every key from 256 on scores ~200 binary orders above the first keys for head 0 (the
    late_keys case of tests/test_gpu_static_reference.py: exp2(S - m) is infinite in the static body), and ordinary for head 1,
    whose queries have no component along the direction that makes them large.  The workgroup of a pair redoes both heads' walks
    through the online body; heads 2 and 3 (K/V head 1, ordinary keys) never leave the static body."""
    from rectified_spaattn_amd import block_sparse_attention
    H, Hkv, S, D = 4, 2, 1536, 128
    g = torch.Generator().manual_seed(9)
    u = torch.nn.functional.normalize(torch.randn(D, generator=g), dim=0)
    q = 0.3 * torch.randn(1, H, S, D, generator=g)
    k = 0.3 * torch.randn(1, Hkv, S, D, generator=g)
    v = torch.randn(1, Hkv, S, D, generator=g)
    q[:, 1] -= (q[:, 1] @ u)[..., None] * u           # head 1: nothing along u
    q[:, 0] = 0.05 * q[:, 0] + 8.0 * u                # head 0: 8 u and little else
    k[:, 0, 256:] += 200.0 * u
    q, k, v = (t.to(DEV, torch.bfloat16) for t in (q, k, v))
    scale = D ** -0.5
    s0 = (q[0, 0].double() @ k[0, 0].double().t() * scale * 1.4426950408889634).cpu()
    assert float(s0[:, 256:].min() - s0[:, :32].max()) > 150     # binary orders: far past the 127 the static reference can take
    right = torch.arange(H) // (H // Hkv)
    scores = torch.matmul(q.double().cpu(), k.double().cpu()[:, right].transpose(-1, -2)) * scale
    ref = _attend(scores, v.double().cpu()[:, right], np.ones((1, H, S, S), bool))
    m = torch.ones(1, Hkv, S // 128, S // 128, dtype=torch.bool, device=DEV)
    mx, mean = TOL[torch.bfloat16]
    for form in (1, 0):
        with _pair(form):
            out = block_sparse_attention(q, k, v, m)
        got = out.double().cpu()
        assert torch.isfinite(got).all(), f"form {'ab'[form]}"
        for h in range(H):
            err = (got[0, h] - ref[0, h]).abs()
            what = f"form {'ab'[form]} head {h}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}"
            print(what)
            assert err.max() <= mx and err.mean() <= mean, what


# ---- 7. Hkv == H -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(causal=True), dict(block_size=64)], ids=["plain", "causal", "block64"])
def test_as_many_kv_heads_as_query_heads_is_the_call_it_was(monkeypatch, kw):
    """The entry points of the MHA call, whatever the tuning key says, and the same bytes; the grouped entry asked for H K/V heads and
    H list heads launches the same kernels."""
    from rectified_spaattn_amd import _core, _lib, block_sparse_attention
    H, Sq, Sk, D = 4, 650, 500, 128
    blk = kw.get("block_size", 128)
    q, k, v = _inputs(H, H, Sq, Sk, D, "bf16")
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    m = torch.from_numpy(_mask_np("H", H, H, NQ, NK)).to(DEV)
    calls = []
    check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda status, what: (calls.append(what), check(status, what))[1])
    outs = []
    for form in (0, 1):
        with _pair(form):
            outs.append(block_sparse_attention(q, k, v, m, **kw))
    assert "rsa_block_sparse_gqa_fwd" not in calls
    assert calls.count("rsa_block_sparse_ranged_fwd" if "causal" in kw else "rsa_block_sparse_plain_fwd") == 2
    assert torch.equal(_bytes(outs[0]), _bytes(outs[1]))
    if "causal" in kw:
        return
    from rectified_spaattn_amd.block_sparse import block_mask_to_lists
    lists = block_mask_to_lists(m, B, H)
    out = torch.empty_like(outs[0])
    with _pair(1):
        check(_lib.lib().rsa_block_sparse_gqa_fwd(B, H, H, H, Sq, Sk, D, _core.dtype_code(q.dtype), blk, NQ, NK, Sk, D ** -0.5,
                                                  _core._t4(q), _core._t4(k), _core._t4(v), lists["cols"].data_ptr(),
                                                  lists["counts"].data_ptr(), None, None, 0, None, 0,
                                                  _lib.RsaOut4(out.data_ptr(), out.stride(0), out.stride(1), out.stride(2)),
                                                  _core._stream()), "rsa_block_sparse_gqa_fwd")
    assert torch.equal(_bytes(out), _bytes(outs[0]))
