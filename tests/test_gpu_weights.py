"""The softmax weights of the 2-byte, e4m3 and pv attention kernels, pinned exactly on the MI355X (tests/weights.py has the construction, the
weighted-count reference and the case tables; tests/test_weights_cpu.py shows that a weight on the wrong key of a sub-step, a row
with another row's scores, a rescale that skips O, l, a d-tile or a 32-row half, pieces merged without their weights or a query
head on the wrong K/V head would break the bound these tests hold the kernels to).  Every score is a small integer in binary
units, so every softmax weight, rescale factor and merge weight is a power of two and the sums are exact in fp32: the output must
equal sum 2^n v / sum 2^n over the visible keys within ONE output ulp -- visibility's bound, ULP and FLOOR imported from there --
and be exactly 0 where that is.  bf16 cases run with the static softmax reference on and off (tuning key k5_static).  The e4m3 and
pv forms (qkv_fp8=) run the rectified and the dense cases under the same bound: there every P is the e4m3 code of 1.5 times a power
of two, K minus its sampled mean and V times its block gain are exact in their images, and the "smooth K" of the product stays on.

Out of scope: Q's block exponent (one value by construction), the selection pass, and rsa_attn_masked.hip (its scale is applied in
fp32, so integer scores cannot be reached: tests/test_gpu_masked_witness.py witnesses it through integer biases instead)."""
import contextlib

import numpy as np
import pytest
import torch

import visibility as vis
import weights as w

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@contextlib.contextmanager
def _tuning(key: bytes, value: int, default: int = 1):
    from rectified_spaattn_amd import _lib
    L = _lib.lib()
    try:
        assert L.rsa_set_tuning(key, value) == 0
        yield
    finally:
        L.rsa_set_tuning(key, default)


def _statics(dt, fp8=False):
    """The settings of k5_static a case runs under: the static reference is a form of the 2-byte bf16 kernels."""
    return (1, 0) if dt == "bf16" and not fp8 else (1,)


def _inputs(m: w.Model):
    """q [B, H, Sq, D], k / v [B, Hkv, Sk, D] on the device in the case's type (exact: tests/test_weights_cpu.py)."""
    dt = DT[m.dt]
    q = torch.from_numpy(m.q()).to(DEV, dt)
    k = torch.from_numpy(m.k()).to(DEV, dt).expand(m.B, m.Hkv, m.Sk, m.D).contiguous()
    v = torch.from_numpy(m.v).to(DEV, dt).expand(m.B, m.Hkv, m.Sk, m.D).contiguous()
    return q, k, v


def _check(out_bhsd: torch.Tensor, want: np.ndarray, dt: str, what: str):
    got = out_bhsd.double().cpu().numpy().reshape(want.shape)
    ratio = np.abs(got - want) / vis.tolerance(want, vis.ULP[dt])
    print(f"{what}: max |got - ref| / bound = {float(ratio.max()):.3f}, max |got - ref| = {float(np.abs(got - want).max()):.3e}")
    msg = vis.violations(got, want, vis.ULP[dt])
    assert not msg, f"{what}: {msg}"


# ---- 0. the one assumption the bound does not derive -------------------------------------------------------------------------
def test_exp2_of_an_integer_is_the_exact_power_of_two_on_the_device():
    """torch.exp2 of the integers -40 .. 40 in fp32 on the device against ldexp.  Indicative, not proof: it may not be the
    kernels' instruction.  The largest deviation is printed; the weights tests' bound assumes it is 0."""
    n = torch.arange(-40, 41, dtype=torch.float32, device=DEV)
    got = torch.exp2(n).double().cpu().numpy()
    want = np.ldexp(1.0, np.arange(-40, 41))
    dev = float(np.abs(got / want - 1.0).max())
    print(f"largest relative deviation of exp2(integer) from the power of two: {dev:.3e}")
    assert dev == 0.0


# ---- 1. plain block_sparse_attention, the tail split among its cases ------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in w.PLAIN_CASES])
def test_plain_block_sparse_attention_weighs_every_key_exactly(cid):
    from rectified_spaattn_amd import block_sparse_attention
    c = w.CASES[cid]
    m = w.model(c)
    want = w.reference(m)
    print(f"{cid}: {w.exercised(m, sorted({0, m.H - 1}))} (first and last head)")
    q, k, v = _inputs(m)
    if c.get("bshd"):          # [B, S, H, D] storage, handed over as head-strided views
        q, k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v))
    mask = torch.from_numpy(m.mask).to(DEV)
    kv_len = list(c["kv_len"]) if len(c["kv_len"]) > 1 else int(c["kv_len"][0])
    kw = dict(sm_scale=c["sm_scale"]) if "sm_scale" in c else {}
    for static in _statics(m.dt):
        for split in c.get("tail_split", (1,)):
            with _tuning(b"k5_static", static), _tuning(b"k5_tail_split", split):
                out = block_sparse_attention(q, k, v, mask, kv_len=kv_len, block_size=c["blk"], **kw)
                torch.cuda.synchronize()
            _check(out, want, m.dt, f"{cid} k5_static={static} k5_tail_split={split}")


# ---- 2. dense attention --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in w.DENSE_CASES + w.DENSE_FP8_CASES])
def test_dense_attention_weighs_every_key_exactly(cid):
    """The 2-byte cases with the static reference and the 256-row form on and off; the e4m3 and pv cases (qkv_fp8=) as they are."""
    from rectified_spaattn_amd import _core
    c = w.CASES[cid]
    m = w.model(c)
    want = w.reference(m)
    print(f"{cid}: {w.exercised(m)}")
    q, k, v = _inputs(m)
    for static in _statics(m.dt, m.fp8):
        for rows256 in ((1, 0) if m.Sq > 256 and not m.fp8 else (1,)):
            with _tuning(b"k5_static", static), _tuning(b"k5_rows256", rows256):
                out = _core.dense_attention(q, k, v, q_split=c["q_split"], kv_split=c["kv_split"], causal=c["causal"], qkv_fp8=m.fp8)
                torch.cuda.synchronize()
            _check(out.permute(0, 2, 1, 3), want, m.dt, f"{cid} k5_static={static} k5_rows256={rows256}")


# ---- 3. the rectified call over a caller's mask -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in w.RECT_CASES + w.RECT_FP8_CASES])
def test_rectified_attention_over_a_mask_weighs_every_key_exactly(cid):
    """Visual rows: R * weighted census + comp with the call's own R and comp, as tests/test_gpu_visibility.py does (R pinned bit for
    bit by the selection tests, comp by tests/test_gpu_comp.py); text rows
    through the text split where the layout has one, visual walks through the tail split (on and off) in the 104-block layout.
    The sensitivity condition is checked again with the call's parts.  The e4m3 and pv cases go in as qkv_fp8=."""
    from rectified_spaattn_amd import _core
    c = w.CASES[cid]
    spec = vis.rect_spec(c)
    sp = vis.spec_numbers(spec)
    m0 = w.model(c)
    B, H, D, S = m0.B, m0.H, m0.D, sp.S
    q, k, v = _inputs(m0)
    mask = torch.from_numpy(m0.mask).to(DEV)
    m = None
    big = c["layout"] in ("hunyuan_tsplit", "hunyuan_tail")
    for static in _statics(m0.dt, m0.fp8):
        for split in c.get("tail_split", (1,)):
            with _tuning(b"k5_static", static), _tuning(b"k5_tail_split", split):
                out, parts = _core.rectified_attention(q, k, v, spec, 0, 0.0, None, return_parts=True, block_mask=mask,
                                                       qkv_fp8=m0.fp8)
                torch.cuda.synchronize()
            if m is None:       # (R and comp come from the selection statistics, which neither tuning key touches)
                dev_parts = (parts["R"].cpu().numpy().reshape(B * H, sp.NBv),
                             parts["comp"].cpu().numpy().reshape(B * H, sp.NBv, D))
                m = w.model(c, parts=dev_parts)
                want = w.reference(m)
                print(f"{cid}: {w.exercised(m, None, 7 if big else 1)}")
            _check(out.view(B, S, H, D).permute(0, 2, 1, 3), want, m.dt, f"{cid} k5_static={static} k5_tail_split={split}")
    missed, exempt = w.insensitive(m, sorted({0, H - 1}) if big else 1, (), 7 if big else 1)
    print(f"{cid}: exempt by rule: {exempt}")
    assert not missed, f"{cid}: with the call's own R and comp the bound would not notice: {missed[:12]}"


# ---- 4. per-row key ranges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in w.RANGED_CASES])
def test_ranged_attention_weighs_every_key_exactly(cid):
    from rectified_spaattn_amd import block_sparse_attention
    c = w.CASES[cid]
    m = w.model(c)
    want = w.reference(m)
    print(f"{cid}: {w.exercised(m)}")
    q, k, v = _inputs(m)
    kw, _, hi = w.ranged_limits(c)
    if "chunk" in kw:
        kw = dict(row_range=(None, torch.from_numpy(hi.astype(np.int32)).to(DEV)))
    for static in _statics(m.dt):
        with _tuning(b"k5_static", static):
            out = block_sparse_attention(q, k, v, torch.from_numpy(m.mask).to(DEV), **kw)
            torch.cuda.synchronize()
        _check(out, want, m.dt, f"{cid} k5_static={static}")


# ---- 5. grouped-query K/V heads -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in w.GQA_CASES])
def test_grouped_attention_weighs_every_key_of_its_kv_head_exactly(cid):
    from rectified_spaattn_amd import _lib, block_sparse_attention
    c = w.CASES[cid]
    m = w.model(c)
    want = w.reference(m)
    print(f"{cid}: {w.exercised(m)}")
    q, k, v = _inputs(m)
    if c.get("fused"):         # head-strided views of one fused projection [B, S, (H + 2 Hkv) D]
        B, H, Hkv, S, D = m.B, m.H, m.Hkv, m.Sq, m.D
        buf = torch.cat([t.permute(0, 2, 1, 3).reshape(B, S, -1) for t in (q, k, v)], dim=-1).contiguous()
        q = buf[..., :H * D].view(B, S, H, D).permute(0, 2, 1, 3)
        k = buf[..., H * D:(H + Hkv) * D].view(B, S, Hkv, D).permute(0, 2, 1, 3)
        v = buf[..., (H + Hkv) * D:].view(B, S, Hkv, D).permute(0, 2, 1, 3)
    mask = torch.from_numpy(m.mask).to(DEV)
    for static in _statics(m.dt):
        for pair in (1, 0):
            with _tuning(b"k5_static", static), _tuning(b"k5_gqa_pair", pair, _lib.GQA_PAIR_DEFAULT):
                out = block_sparse_attention(q, k, v, mask, kv_len=list(c["kv_len"]))
                torch.cuda.synchronize()
            _check(out, want, m.dt, f"{cid} k5_static={static} k5_gqa_pair={pair}")
