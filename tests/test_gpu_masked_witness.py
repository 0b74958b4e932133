"""The masked and dropout dense attention kernel (rsa_attn_masked.hip) held to exact witnesses on the MI355X.  tests/masked_witness.py
has the construction, the per-row references and the case tables; tests/test_masked_witness_cpu.py shows that one mask element on
the wrong side, a mask read from the neighbouring row / batch item / head / key / tile, two keys of a tile swapped, a lost rescale,
half a row sum or a dropout stream keyed by anything but (seed, b H + h, row, key) would break the bound these tests hold the
kernel to.  Every q . k is exactly 0; the weights come from the mask alone: 1 (class A), powers of two through float32 biases b with
fl(1.44269504f b) an integer (B), e^b of 2-byte biases (C, the one class that is not exact: 1.5 ulp), and the kept weights of the
numpy twin of drop_hash times the rounded keep_scale (D).  Classes A, B and D: |got - ref| <= ULP |ref| + FLOOR max|ref| with
visibility's ULP and FLOOR, exact zeros, and the rows without a key compared as NaN sets."""
import numpy as np
import pytest
import torch

import masked_witness as mw
import visibility as vis

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
WORST = {}                 # class -> the largest |got - ref| / bound seen


def _qkv(c, m):
    """q [B, H, Sq, D], k / v [B, H, Sk, D] on the device in the case's type; c["bshd"]: [B, S, H, D] storage, head-strided views."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    q, k = vis.qk_inputs(B, H, Sq, Sk, D)
    dt = DT[c["dt"]]
    q, k = torch.from_numpy(q).to(DEV, dt), torch.from_numpy(k).to(DEV, dt)
    v = torch.from_numpy(m.v).to(DEV, dt).expand(B, H, Sk, D).contiguous()
    if c.get("bshd"):
        q, k, v = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v))
        assert not q.is_contiguous()
    return q, k, v


def _mask(c, m):
    """The case's mask on the device in its kind (bool, the 2-byte type, float32) and memory form: contiguous; the transpose of a
    [.., Sk, Sq] tensor (key stride != 1); every second row and a column offset of a wider buffer full of other values; an expand
    over heads (stride 0 on an axis of size H)."""
    if m.logical is None:
        return None
    lg = m.logical
    tdt = {"bool": torch.bool, "add2": DT[c["dt"]], "add32": torch.float32}[c["mkind"]]
    mem = c["mem"]
    if mem == "transpose":
        t = torch.from_numpy(np.ascontiguousarray(np.swapaxes(lg, -1, -2))).to(DEV, tdt).transpose(-1, -2)
        assert t.stride(-1) != 1 or lg.shape[-2] == 1
    elif mem == "slice":
        rng = np.random.default_rng(3)
        Sq, Sk = lg.shape[-2:]
        buf = rng.choice(np.unique(lg), lg.shape[:-2] + (2 * Sq + 1, Sk + 7))
        buf[..., 1::2, 4:4 + Sk] = lg
        t = torch.from_numpy(buf).to(DEV, tdt)[..., 1::2, 4:4 + Sk]
        assert t.shape == lg.shape
    else:
        t = torch.from_numpy(lg).to(DEV, tdt)
        if mem == "expand":
            t = t.expand(c["B"], c["H"], c["Sq"], c["Sk"])
            assert t.stride(1) == 0
    assert np.array_equal(t.cpu().float().numpy(), np.broadcast_to(lg, t.shape).astype(np.float32), equal_nan=True)
    return t


def _run(c, m, q, k, v, mask):
    """-> the output as float64 [BH, Sq, D], through the entry point the case names."""
    from rectified_spaattn_amd import _core, attn
    nan = bool(c.get("empty_nan"))
    if c["entry"] == "masked":
        out = _core.dense_attention_masked(q, k, v, mask, empty_rows_nan=nan).permute(0, 2, 1, 3)
    elif c["entry"] == "dropout":
        out = _core.dense_attention_dropout(q, k, v, c["p"], m.seed, mask, causal=bool(c.get("causal")),
                                            empty_rows_nan=nan).permute(0, 2, 1, 3)
    else:
        if "torch_seed" in c:
            torch.manual_seed(c["torch_seed"])
        out = attn.fullattn(q, k, v, mode=c["mode"], attn_mask=mask, drop_rate=c.get("p", 0))
    torch.cuda.synchronize()
    assert out.dtype == DT[c["dt"]] and out.shape == (c["B"], c["H"], c["Sq"], c["D"])
    return out.double().cpu().numpy().reshape(m.BH, c["Sq"], c["D"])


def _ratio(got, want, bound):
    """max |got - ref| / bound (an all-zero reference has the bound 0: 0 when it is met, inf when not)."""
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def _check(got, want, c, what):
    nan_got, nan_want = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_got, nan_want), \
        f"{what}: NaN elements differ: {int(nan_got.sum())} got, {int(nan_want.sum())} expected, first at " \
        f"{tuple(np.argwhere(nan_got != nan_want)[0])}"
    got, want = np.where(nan_want, 0.0, got), np.where(nan_want, 0.0, want)
    ulp = vis.ULP[c["dt"]]
    cls = "C" if c["cls"] == "C" else {"DB": "D"}.get(c["cls"], c["cls"])
    if cls == "C":
        bound = mw.bound_c(want, ulp)
        ratio = _ratio(got, want, bound)
        msg = ""
        if not np.isfinite(got).all():
            msg = "non-finite elements"
        elif (got[want == 0] != 0).any():
            msg = f"{int((got[want == 0] != 0).sum())} elements must be exactly 0"
        elif ratio > 1:
            worst = np.unravel_index(np.argmax(np.abs(got - want) / bound), got.shape)
            msg = f"past the bound at {tuple(int(x) for x in worst)}: got {got[worst]!r}, ref {want[worst]!r}, {ratio:.2f} x the bound"
    else:
        ratio = _ratio(got, want, vis.tolerance(want, ulp))
        msg = vis.violations(got, want, ulp)
    WORST[cls] = max(WORST.get(cls, 0.0), ratio)
    print(f"{what}: max |got - ref| / bound = {ratio:.3f} (class {cls}), max |got - ref| = {float(np.abs(got - want).max()):.3e}")
    assert not msg, f"{what}: {msg}"


def _seed_fullattn_will_draw(torch_seed):
    """fullattn draws its dropout seed from torch's CPU generator: the same draw after the same torch.manual_seed."""
    torch.manual_seed(torch_seed)
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _case(cid):
    c = mw.CASES[cid]
    m = mw.model(c, seed=_seed_fullattn_will_draw(c["torch_seed"]) if "torch_seed" in c else None)
    q, k, v = _qkv(c, m)
    mask = _mask(c, m)
    got = _run(c, m, q, k, v, mask)
    _check(got, mw.reference(m), c, cid)
    return c, m, q, k, v, mask, got


# ---- A: which keys a row sees ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mw.by_class("A"))
def test_every_row_sums_the_keys_its_mask_admits(cid):
    _case(cid)


# ---- B: with what weight -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mw.by_class("B"))
def test_integer_biases_weigh_every_key_by_its_power_of_two(cid):
    _case(cid)


# ---- C: 2-byte additive masks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mw.by_class("C"))
def test_two_byte_additive_masks_stay_within_one_and_a_half_ulp(cid):
    """Measured on the MI355X: the largest |got - ref| / bound of the class is in DESIGN.md section 3."""
    _case(cid)


# ---- D: dropout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mw.by_class("D", "DB"))
def test_dropout_keeps_the_weights_the_pinned_stream_keeps(cid):
    from rectified_spaattn_amd import _core
    c, m, q, k, v, mask, got = _case(cid)
    if c["p"] == 1.0:
        assert not np.nan_to_num(got).any()
    if c.get("same_as_masked"):              # rate 0 through the dropout entry: the bytes of the dropout-free call
        base = _core.dense_attention_masked(q, k, v, mask, empty_rows_nan=bool(c.get("empty_nan")))
        out = _core.dense_attention_dropout(q, k, v, 0.0, m.seed, mask, empty_rows_nan=bool(c.get("empty_nan")))
        assert torch.equal(out.view(torch.int16), base.view(torch.int16))


def test_keep_decisions_do_not_depend_on_the_number_of_keys():
    """The decisions for the keys < Sk' = 256 are the same when K and V are cut to Sk': a call over 300 keys whose mask hides the
    keys from 256 on gives the bytes of the call over the first 256 keys (the tiles past them add exact zeros)."""
    from rectified_spaattn_amd import _core
    c = dict(B=2, H=3, Sq=130, Sk=300, D=128, dt="bf16")
    q, k = (torch.from_numpy(x).to(DEV, torch.bfloat16) for x in vis.qk_inputs(2, 3, 130, 300, 128))
    v = torch.from_numpy(vis.witness_v(300, 128, [0, 255, 256, 299])).to(DEV, torch.bfloat16).expand(2, 3, 300, 128).contiguous()
    mask = torch.rand(1, 1, 130, 300, generator=torch.Generator().manual_seed(1)) < 0.7
    mask[..., 256:] = False
    mask = mask.to(DEV)
    for p in (0.25, 0.5):
        whole = _core.dense_attention_dropout(q, k, v, p, 4242, mask, empty_rows_nan=False)
        cut = _core.dense_attention_dropout(q, k[:, :, :256], v[:, :, :256], p, 4242, mask[..., :256].contiguous(), empty_rows_nan=False)
        assert torch.equal(whole.view(torch.int16), cut.view(torch.int16)), (c, p)
        assert float(whole.float().abs().max()) > 0


def test_a_masked_and_an_unmasked_call_agree_on_the_keys_both_see():
    """Key j writes channel j alone (Sk = D = 128), so an output element is non-zero iff its weight was kept: the kept keys of the
    masked call are the kept keys of the unmasked call that the mask admits."""
    from rectified_spaattn_amd import _core
    B, H, Sq, Sk, D = 2, 3, 130, 128, 128
    q, k = (torch.from_numpy(x).to(DEV, torch.float16) for x in vis.qk_inputs(B, H, Sq, Sk, D))
    v = torch.eye(Sk, D, dtype=torch.float16, device=DEV).expand(B, H, Sk, D).contiguous()
    mask = (torch.rand(B, H, Sq, Sk, generator=torch.Generator().manual_seed(2)) < 0.6).to(DEV)
    plain = _core.dense_attention_dropout(q, k, v, 0.5, 99, None, empty_rows_nan=False).permute(0, 2, 1, 3)
    masked = _core.dense_attention_dropout(q, k, v, 0.5, 99, mask, empty_rows_nan=False).permute(0, 2, 1, 3)
    kept = plain != 0
    share = float(kept.float().mean())
    assert 0.45 < share < 0.55, share
    assert torch.equal(masked != 0, kept & mask)


def test_zz_the_largest_deviation_of_each_class():
    """Prints the maxima the tests above collected (DESIGN.md section 3 records them)."""
    for cls in sorted(WORST):
        print(f"class {cls}: largest |got - ref| / bound = {WORST[cls]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
