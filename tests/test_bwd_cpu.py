"""block_sparse_attention_backward without a GPU: the numpy reference against torch's own fp64 autograd,
the exactness claims of the witnesses, what each deliberate mutation of the rule does to a witness, the Python refusals, and the C
entries' presence, refusals and workspace size (every call fails its host checks or has nothing to do: nothing is launched)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bwd_ref as ref
import weights
from rectified_spaattn_amd import _lib
from rectified_spaattn_amd import block_sparse as bs


def torch_grads(inp, seen):
    """torch's fp64 autograd of the dense-masked expression, K/V heads repeated; rows that see nothing are 0."""
    q, k, v, dout = (torch.from_numpy(np.nan_to_num(inp[n]).astype(np.float64)) for n in ("q", "k", "v", "dout"))
    q.requires_grad_(), k.requires_grad_(), v.requires_grad_()
    g = q.shape[1] // k.shape[1]
    vis = torch.from_numpy(seen)
    some = vis.any(-1, keepdim=True)
    s = (q * inp["sm_scale"]) @ k.repeat_interleave(g, 1).transpose(-1, -2)
    s = torch.where(some, s.masked_fill(~vis, -np.inf), torch.zeros_like(s))
    out = (torch.softmax(s, -1) * some) @ v.repeat_interleave(g, 1)
    out.backward(dout)
    return [x.detach().numpy() for x in (out, q.grad, k.grad, v.grad)]


@pytest.mark.parametrize("c", ref.FP64_CASES[::7], ids=lambda c: c["id"])
def test_reference_is_torchs_fp64_autograd(c):
    inp = ref.fp64_inputs(c)
    for causal in c["causals"]:
        seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], c["H"], causal)
        for got, want in zip(ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], seen, inp["sm_scale"]), torch_grads(inp, seen)):
            assert np.allclose(got, want, rtol=1e-10, atol=1e-12)


def test_case_tables_cover_what_they_claim():
    cs = ref.FP64_CASES
    assert len(cs) == 72 and len({c["id"] for c in cs}) == 72
    for key, vals in (("Hl", None), ("lens", 2), ("mask", 2), ("scale", 2), ("dt", 2), ("D", 2), ("blk", 2), ("Sq", 3)):
        for pair in ((4, 4), (8, 2), (6, 1)):
            sub = [c for c in cs if (c["H"], c["Hkv"]) == pair]
            seen = {str(c[key]) for c in sub}
            assert len(seen) == (vals or len({pair[0], pair[1], 1})), (key, pair, seen)
    assert all(-(-c["Sq"] // c["blk"]) >= 2 for c in cs) and all(c["causals"] == ((False, True) if c["blk"] == 128 else (False,))
                                                                 for c in cs)
    # a row group boundary inside a query block, a ragged last block, rows that see nothing under the causal limit
    assert any(c["lens"][1] < c["Sq"] and True in c["causals"] for c in cs)


@pytest.mark.parametrize("c", ref.EXACT_CASES, ids=lambda c: c["id"])
def test_exact_witness_is_exact(c):
    """Every intermediate is a value of the storage type and of fp32, so the contract's model IS the fp64 gradient, rounded."""
    inp = ref.exact_inputs(c)
    seen = ref.exact_seen()
    assert (seen.sum(-1) == 256).all()
    for n in ("q", "k", "v", "dout"):
        assert np.array_equal(inp[n], weights.round_dt(inp[n], c["dt"]))
    out, dq, dk, dv = ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], seen, inp["sm_scale"])
    assert not out.any()
    p = 2.0 ** -8
    dp = np.matmul(inp["dout"].astype(np.float64), np.repeat(inp["v"], 2, axis=1).astype(np.float64).transpose(0, 1, 3, 2))
    ds = p * dp * seen
    assert np.array_equal(ds, weights.round_dt(ds, c["dt"])) and np.array_equal(ds, ds.astype(np.float32))
    for x in (dq, dk, dv):          # the sums are exact in fp32: every term is a multiple of 2^-11 far below 2^13
        assert np.array_equal(x, x.astype(np.float32)) and np.array_equal(x * 2048, np.rint(x * 2048)) and np.abs(x).max() < 32
    got = ref.model(inp["q"], inp["k"], inp["v"], out, inp["dout"], seen, inp["sm_scale"], c["dt"])
    for g, want in zip(got, (dq, dk, dv)):
        assert np.array_equal(g, weights.round_dt(want, c["dt"]))
    zero, moving = (dk, (dq, dv)) if c["kind"] == "dq" else (dq, (dk, dv))
    assert not zero.any() and all(x.any() for x in moving)


def test_exact_mask_keeps_two_blocks_and_differs_between_heads():
    m = ref.exact_mask()
    assert (m.sum(-1) == 2).all()
    for b in range(ref.B):
        rows = {tuple(m[b, h, i]) for h in range(ref.EXACT_H) for i in range(2)}
        assert len(rows) >= 5
        for hk in range(ref.EXACT_HKV):     # the two query heads of a K/V head keep different pairs in every query block
            assert (m[b, 2 * hk] != m[b, 2 * hk + 1]).any(-1).all()


@pytest.mark.parametrize("c", ref.VIS_CASES, ids=lambda c: c["id"])
def test_visibility_witness_reads_the_rule_through_dv(c):
    inp = ref.vis_inputs(c)
    seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], ref.VIS_H, c["causal"])
    _, dq, dk, dv = ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], seen, inp["sm_scale"])
    want = ref.vis_pattern(c, inp)
    assert np.array_equal(dv != 0, want) and want.any() and not want.all()
    assert len(inp["owner"]) == ref.VIS_D                   # every channel is a probe
    rows = {r for _, r in inp["owner"]}
    assert {0, c["Sq"] - 1, 63, 64}.issubset(rows)
    if c["causal"]:
        assert {59, 60}.issubset(rows)                      # item 1: rows 0 .. 59 see nothing
        assert not seen[1, :, :60].any() and seen[1, :, 60].any()
        assert not dq[1, :, :60].any()
    for b, nb in enumerate(c["lens"]):
        assert not dk[b, :, nb:].any() and not dv[b, :, nb:].any()


# ---- mutations -------------------------------------------------------------------------------------------------------------------
def test_mutation_causal_off_by_one_changes_the_visibility_witness():
    c = next(c for c in ref.VIS_CASES if c["causal"])
    inp = ref.vis_inputs(c)
    for shift in (-1, 1):
        seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], ref.VIS_H, True, causal_shift=shift)
        assert not np.array_equal(ref.vis_pattern(c, inp, seen), ref.vis_pattern(c, inp))


@pytest.mark.parametrize("c", ref.VIS_CASES, ids=lambda c: c["id"])
def test_mutation_kv_len_ignored_changes_the_visibility_witness(c):
    inp = ref.vis_inputs(c)
    seen = ref.visible(inp["mask"], [ref.SK] * ref.B, c["Sq"], ref.SK, c["blk"], ref.VIS_H, False)
    if c["causal"]:     # (the limit ignored inside the causal offset too)
        seen = seen & ref.visible(inp["mask"], [ref.SK, ref.SK], c["Sq"], ref.SK, c["blk"], ref.VIS_H, True)
    assert not np.array_equal(ref.vis_pattern(c, inp, seen), ref.vis_pattern(c, inp))


def _model_of(c, inp, seen, **mut):
    out = ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], seen, inp["sm_scale"])[0]
    return ref.model(inp["q"], inp["k"], inp["v"], weights.round_dt(out, c["dt"]), inp["dout"], seen, inp["sm_scale"], c["dt"], **mut)


def test_mutation_group_not_summed_changes_the_witnesses():
    c = ref.VIS_CASES[0]
    inp = ref.vis_inputs(c)
    seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], ref.VIS_H, c["causal"])
    dv = _model_of(dict(c, dt="bf16"), inp, seen, sum_group=False)[2]
    assert not np.array_equal(dv != 0, ref.vis_pattern(c, inp))
    e = ref.EXACT_CASES[0]
    inp = ref.exact_inputs(e)
    good, bad = _model_of(e, inp, ref.exact_seen()), _model_of(e, inp, ref.exact_seen(), sum_group=False)
    assert np.array_equal(good[0], bad[0]) and not np.array_equal(good[2], bad[2])


def test_mutation_list_of_the_wrong_head_changes_the_exact_witness():
    for e in ref.EXACT_CASES[::3]:
        inp = ref.exact_inputs(e)
        wrong = ref.exact_seen(np.roll(ref.exact_mask(), 1, axis=1))
        good, bad = _model_of(e, inp, ref.exact_seen()), _model_of(e, inp, ref.exact_seen(), seen_kv=wrong)
        assert np.array_equal(good[0], bad[0]) and not np.array_equal(good[2], bad[2])
        if e["kind"] == "dk":
            assert not np.array_equal(good[1], bad[1])


def test_mutation_delta_dropped_breaks_the_fp64_bar():
    """The exact witness has delta = 0 by construction, so the witness for delta is a random case: without it dq and dk are off by
    far more than the contract's own rounding error."""
    c = ref.FP64_CASES[4]
    inp = ref.fp64_inputs(c)
    seen = ref.visible(inp["mask"], c["lens"], c["Sq"], ref.SK, c["blk"], c["H"], False)
    want = ref.grads(inp["q"], inp["k"], inp["v"], inp["dout"], seen, inp["sm_scale"])[1:]
    good, bad = _model_of(c, inp, seen), _model_of(c, inp, seen, use_delta=False)
    for i in (0, 1):
        assert np.abs(bad[i] - want[i]).max() > 10 * np.abs(good[i] - want[i]).max()
    assert np.array_equal(good[2], bad[2])
    for g, w in zip(good, want):        # ... and the contract itself sits where a 2-byte result can: a few output ulps
        assert np.abs(g - w).max() <= 0.02 * np.abs(w).max()


# ---- the Python refusals ---------------------------------------------------------------------------------------------------------
def _cpu_args(H=4, Hkv=2, Sq=200, Sk=400, D=64, dtype=torch.bfloat16, blk=128):
    q, k, v = torch.zeros(2, H, Sq, D, dtype=dtype), torch.zeros(2, Hkv, Sk, D, dtype=dtype), torch.zeros(2, Hkv, Sk, D, dtype=dtype)
    mask = torch.ones(2, Hkv, -(-Sq // blk), -(-Sk // blk), dtype=torch.bool)
    return [q.clone(), q, k, v, q.clone(), mask]


def test_python_refusals():
    a = _cpu_args()
    with pytest.raises(NotImplementedError, match="window"):
        bs.block_sparse_attention_backward(*a, window=(16, 0))
    with pytest.raises(NotImplementedError, match="row_range"):
        bs.block_sparse_attention_autograd(*a[1:4], a[5], row_range=(None, torch.zeros(1, 200, dtype=torch.int32)))
    with pytest.raises(NotImplementedError, match="causal"):
        bs.block_sparse_attention_backward(*_cpu_args(blk=64), block_size=64, causal=True)
    with pytest.raises(ValueError, match="do not divide"):
        bs.block_sparse_attention_backward(*_cpu_args(H=5, Hkv=2))
    with pytest.raises(ValueError, match="block_mask"):
        bs.block_sparse_attention_backward(*a[:5], a[5][:, :, :1])
    with pytest.raises(ValueError, match="block_mask"):
        bs.block_sparse_attention_backward(*a[:5], torch.ones(2, 3, 2, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="block_mask"):
        bs.block_sparse_attention_backward(*a[:5], a[5].float())
    with pytest.raises(ValueError, match="one dtype"):
        bs.block_sparse_attention_backward(*_cpu_args(dtype=torch.float32))
    with pytest.raises(ValueError, match="dout"):
        bs.block_sparse_attention_backward(a[0][:, :, :100], *a[1:])
    with pytest.raises(ValueError, match="out"):
        bs.block_sparse_attention_backward(*a[:4], a[4].half(), a[5])
    with pytest.raises(ValueError, match="kv_len"):
        bs.block_sparse_attention_backward(*a, kv_len=[400, 401])
    with pytest.raises(_lib.RsaError, match="device"):          # every check passed: only the device is missing
        bs.block_sparse_attention_backward(*a)


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="librsa_hip.so is not built")
T4, O4 = _lib.RsaTensor4, _lib.RsaOut4


def _bwd(L, shape=(2, 4, 2, 2, 200, 400, 64), dtype=0, block=128, NQ=None, NK=None, kv_valid=400, ptr=0x1000, stride=64,
         ws=0x2000, ws_bytes=1 << 20, lists=0x3000, out_stride=64):
    B, H, Hkv, Hl, Sq, Sk, D = shape
    NQ = -(-Sq // block) if NQ is None and block > 0 else NQ
    NK = -(-Sk // block) if NK is None and block > 0 else NK
    t = T4(ptr, stride * 1000, stride * 100, stride)
    o = O4(ptr, out_stride * 1000, out_stride * 100, out_stride)
    return L.rsa_block_sparse_bwd(*shape, dtype, block, NQ, NK, kv_valid, None, 0, 0.125, t, t, t, t, t, lists, lists, lists, lists,
                                  ws, ws_bytes, o, o, o, None)


@needs_lib
def test_c_entries_refuse_before_any_launch():
    L = _lib.lib()
    OK, BAD, UNSUP, WS = 0, -1, -2, -3
    assert L.rsa_status_string(WS).decode() and L.rsa_status_string(UNSUP).decode()
    need = ctypes.c_size_t(0)
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 400, 64, 128, 2, 4, ctypes.byref(need)) == OK
    assert need.value == 2 * 2 * 4 * 200 * 4
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 400, 64, 128, 2, 4, None) == BAD
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 400, 64, 96, 3, 5, ctypes.byref(need)) == UNSUP
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 400, 48, 128, 2, 4, ctypes.byref(need)) == UNSUP
    assert L.rsa_block_sparse_bwd_bytes(1, 1, 1, 1, 8193 * 64, 64, 64, 64, 8193, 1, ctypes.byref(need)) == UNSUP
    assert L.rsa_block_sparse_bwd_bytes(1, 1, 1, 1, 64, 8193 * 64, 64, 64, 1, 1, ctypes.byref(need)) == UNSUP
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 3, 1, 200, 400, 64, 128, 2, 4, ctypes.byref(need)) == BAD
    assert L.rsa_block_sparse_bwd_bytes(2, 8, 2, 4, 200, 400, 64, 128, 2, 4, ctypes.byref(need)) == BAD      # Hl not in {1, Hkv, H}
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 400, 64, 128, 3, 4, ctypes.byref(need)) == BAD
    assert L.rsa_block_sparse_bwd_bytes(2, 4, 2, 2, 200, 400, 64, 128, 2, 5, ctypes.byref(need)) == BAD
    assert _bwd(L, block=96, NQ=3, NK=5) == UNSUP
    assert _bwd(L, dtype=7) == UNSUP
    assert _bwd(L, shape=(2, 4, 2, 2, 200, 400, 32)) == UNSUP
    assert _bwd(L, ws_bytes=2 * 2 * 4 * 200 * 4 - 1) == WS
    assert _bwd(L, ptr=0) == BAD and _bwd(L, ptr=0x1008) == BAD and _bwd(L, stride=60) == BAD and _bwd(L, out_stride=62) == BAD
    assert _bwd(L, ws=0) == BAD and _bwd(L, ws=0x2004) == BAD and _bwd(L, lists=0) == BAD and _bwd(L, lists=0x3002) == BAD
    assert _bwd(L, kv_valid=401) == BAD and _bwd(L, kv_valid=-1) == BAD
    assert _bwd(L, out_stride=0) == BAD                         # a result row is written once
    # nothing to do: no launch (the pointers above are not memory)
    assert _bwd(L, shape=(0, 4, 2, 2, 200, 400, 64)) == OK
    assert _bwd(L, shape=(2, 0, 2, 2, 200, 400, 64)) == OK
    assert _bwd(L, shape=(2, 4, 2, 2, 0, 400, 64), NQ=0) == OK


def test_the_entries_are_in_the_prototype_table():
    assert "rsa_block_sparse_bwd" in _lib.PROTOTYPES and "rsa_block_sparse_bwd_bytes" in _lib.PROTOTYPES
    assert list(_lib.PROTOTYPES)[-3:] == ["rsa_block_sparse_extend_bytes", "rsa_block_sparse_extend", "rsa_block_sparse_extend_kv8"]
