"""Which keys each row sees, pinned exactly on the MI355X for every K5 form (tests/visibility.py has the design, the counting
references and the case tables; tests/test_visibility_cpu.py shows that one key on the wrong side of any limit, or one 64-key
tile dropped or counted twice, would break the bound these tests hold the kernels to): every score is exactly zero, V of
0 / 1 says which keys were summed, and the output must equal the census within ONE output ulp -- and be exactly 0 where the
census is."""
import contextlib

import numpy as np
import pytest
import torch

import visibility as vis

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


def _inputs(B, H, Sq, Sk, v, dt):
    D = v.shape[1]
    q, k = vis.qk_inputs(B, H, Sq, Sk, D)
    tv = torch.from_numpy(v).to(DEV, dt).expand(B, H, Sk, D).contiguous()
    return torch.from_numpy(q).to(DEV, dt), torch.from_numpy(k).to(DEV, dt), tv


def _check(out_bhsd: torch.Tensor, ref: vis.Ref, ulp: float, what: str):
    """out [B, H, Sq, D] against the reference's rows: the bound of the module docstring, zeros exact."""
    got = out_bhsd.double().cpu().numpy().reshape(-1, *out_bhsd.shape[2:])
    want = np.broadcast_to(ref.rows(), got.shape)
    ratio = np.abs(got - want) / vis.tolerance(want, ulp)
    print(f"{what}: max |got - ref| / bound = {float(ratio.max()):.3f}, max |got - ref| = {float(np.abs(got - want).max()):.3e}")
    msg = vis.violations(got, want, ulp)
    assert not msg, f"{what}: {msg}"


# ---- 1. plain block_sparse_attention -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in vis.PLAIN_CASES])
def test_plain_block_sparse_attention_sees_exactly_the_documented_keys(cid):
    """kv_len at, one short of and one past the tile and block edges (two values per call: one launch per batch item), a
    ragged last query block and an odd number of 64-token query blocks, fewer mask columns than key blocks, mask rows that
    keep everything / only the boundary block / the blocks from or up to it / only a block past kv_len (exactly 0), and the
    tail split with uneven pieces and kv_len inside the last key block, switched on and off."""
    from rectified_spaattn_amd import block_sparse_attention
    c = vis.CASES[cid]
    ref, mask = vis.plain_ref(c)
    q, k, v = _inputs(c["B"], c["H"], c["Sq"], c["Sk"], ref.v, DT[c["dt"]])
    kv_len = list(c["kv_len"]) if len(c["kv_len"]) > 1 else int(c["kv_len"][0])
    for split in c.get("tail_split", (1,)):
        with _tuning(b"k5_tail_split", split):
            out = block_sparse_attention(q, k, v, torch.from_numpy(mask).to(DEV), kv_len=kv_len, block_size=c["blk"])
            torch.cuda.synchronize()
        _check(out, ref, vis.ULP[c["dt"]], f"{cid} k5_tail_split={split}")


# ---- 2. dense attention --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk", vis.DENSE_SHAPES, ids=[f"{a}x{b}" for a, b in vis.DENSE_SHAPES])
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("dt,fp8", vis.DENSE_FORMS, ids=["bf16", "fp16", "e4m3", "pv"])
def test_dense_attention_sees_exactly_the_documented_keys(dt, fp8, D, Sq, Sk):
    """One or two segments with the split at a multiple of 128 and one to either side of it, the ends (q_split = 0: every row
    in the second segment; kv_split = Sk: the second segment's rows see nothing and are exactly 0), causal and not; 2-byte calls
    of more than 256 rows in the 256-row and the 128-row form, byte for byte the same."""
    from rectified_spaattn_amd import _core
    cases = [c for c in vis.DENSE_CASES if (c["D"], c["Sq"], c["Sk"]) == (D, Sq, Sk)]
    assert len(cases) >= 8
    for c in cases:
        ref = vis.dense_ref(c)
        q, k, v = _inputs(c["B"], c["H"], Sq, Sk, ref.v, DT[dt])
        kw = dict(q_split=c["q_split"], kv_split=c["kv_split"], causal=c["causal"], qkv_fp8=fp8)
        outs = []
        for rows256 in ((1, 0) if not fp8 and Sq > 256 else (1,)):
            with _tuning(b"k5_rows256", rows256):
                out = _core.dense_attention(q, k, v, **kw)
                torch.cuda.synchronize()
            _check(out.permute(0, 2, 1, 3), ref, vis.ULP[dt], f"{c['id']} {dt} qkv_fp8={fp8} k5_rows256={rows256}")
            outs.append(out)
        if len(outs) == 2:
            assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{c['id']}: 256-row and 128-row forms differ"


# ---- 3. the rectified call over a caller's mask ------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in vis.RECT_CASES])
def test_rectified_attention_over_a_mask_sees_exactly_the_documented_keys(cid):
    """Every limit of the four layouts inside a block (kv_valid, kv_text_valid, q_text_valid, the keys between kv_valid and
    pool_valid of the Flux layout, a ragged last block), 128- and 64-token blocks (an odd number of 64-token text blocks among
    them), the 2-byte, e4m3 and pv kernels; text rows whose walk is split (the tile census of those rows shows that the pieces
    tile [0, kv_text_valid) exactly) and the tail split with text pieces behind it.  Visual rows: R * census + comp with the
    call's own R and comp (R is pinned bit for bit against the oracle by the selection tests; comp, which has no bit-exact oracle, by
    the exact and per-element witnesses of tests/test_gpu_comp.py); the sensitivity condition is checked again with them."""
    from rectified_spaattn_amd import _core
    c = vis.CASES[cid]
    spec = vis.rect_spec(c)
    sp = vis.spec_numbers(spec)
    B, H, D, S = c["B"], c["H"], c["D"], sp.S
    model, mask = vis.rect_ref(c, sp)
    q, k, v = _inputs(B, H, S, S, model.v, DT[c["dt"]])
    ulp = vis.ULP[c["dt"]]
    for split in c.get("tail_split", (1,)):
        with _tuning(b"k5_tail_split", split):
            out, parts = _core.rectified_attention(q, k, v, spec, 0, 0.0, None, return_parts=True,
                                                   block_mask=torch.from_numpy(mask).to(DEV), qkv_fp8=c["fp8"])
            torch.cuda.synchronize()
        dev_parts = (parts["R"].cpu().numpy().reshape(B * H, sp.NBv), parts["comp"].cpu().numpy().reshape(B * H, sp.NBv, D))
        ref = vis.reference(c, parts=dev_parts)
        _check(out.view(B, S, H, D).permute(0, 2, 1, 3), ref, ulp, f"{cid} k5_tail_split={split}")
    missed = vis.insensitive(c, ulp, parts=dev_parts)
    assert not missed, f"{cid}: with the call's own R and comp the bound would not notice: {missed}"
