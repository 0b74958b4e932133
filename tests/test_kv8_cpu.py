"""The e4m3 K/V cache without a device: the model of tests/kv8_ref.py against naive loops and against
both e4m3 references (torch's cast, oracle.quantize_e4m3), dequantised attention, the exponent range of the byte-equality
cases, and every refusal of the Python layer and of the three C entries (whose checks run before the first HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import decode_ref as ref
import kv8_ref as kv8
from oracle import oracle as orc

E4M3 = torch.float8_e4m3fn
NAMES = ("rsa_kv8_append", "rsa_block_sparse_decode_kv8", "rsa_pool_keys_kv8")


# ---- the byte contract ---------------------------------------------------------------------------------------------------------------
EDGES = [448.0, -448.0, 449.0, 465.0, -465.0, 1e9, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, -(2.0 ** -10), 0.0, 1.0, 0.3]
EDGE_CODES = [0x7E, 0xFE, 0x7E, 0x7E, 0xFE, 0x7E, 0x01, 0x00, 0x01, 0x80, 0x00, 0x38, 0x2A]


def test_edge_values_against_both_e4m3_references():
    x = np.array(EDGES, np.float32).reshape(1, 1, -1, 1)
    got = kv8.quantize(x, 1.0).reshape(-1)
    assert got.tolist() == EDGE_CODES
    assert np.array_equal(got, orc.quantize_e4m3(x.reshape(-1)).reshape(-1).astype(np.uint8))
    # without the clamp torch gives NaN above 464: the contract is the clamped form
    assert torch.tensor([465.0]).to(E4M3).view(torch.uint8).item() == 0x7F
    # NaN stays a NaN code, +-Inf saturate
    special = kv8.quantize(np.array([np.nan, np.inf, -np.inf], np.float32).reshape(1, 1, 3, 1), 1.0).reshape(-1)
    assert special.tolist() == [0x7F, 0x7E, 0xFE]
    # the scale divides: one fp32 division per element, per head
    x2 = np.array([[[[3.0]], [[3.0]]]], np.float32)
    assert kv8.quantize(x2, [0.37, 2.0]).reshape(-1).tolist() == kv8.quantize(x2 / np.array([0.37, 2.0], np.float32).reshape(1, 2, 1, 1),
                                                                             1.0).reshape(-1).tolist()


def test_random_values_agree_with_the_oracle_cast_and_every_finite_code_is_a_bf16_and_an_fp16():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(20000) * np.exp2(rng.integers(-12, 10, 20000))).astype(np.float32)
    got = kv8.quantize(x.reshape(1, 1, -1, 1), 1.0).reshape(-1)
    assert np.array_equal(got, orc.quantize_e4m3(x).astype(np.uint8))
    vals = kv8.code_values()
    finite = np.isfinite(vals)
    assert finite.sum() == 254 and np.flatnonzero(~finite).tolist() == [0x7F, 0xFF]
    for dt in (torch.bfloat16, torch.float16):
        back = torch.from_numpy(vals[finite]).to(dt).double().numpy()
        assert np.array_equal(back, vals[finite])
        for e in range(-2, 3):      # ... and so is code * 2^e, the dequantised cache of the byte-equality tests
            assert np.array_equal(torch.from_numpy(vals[finite] * 2.0 ** e).to(dt).double().numpy(), vals[finite] * 2.0 ** e)


# ---- the writer's placement ------------------------------------------------------------------------------------------------------------
def _naive_append(cache, new, starts, counts, blk, table):
    out = cache.copy()
    B, Hkv, T, D = new.shape
    for b in range(B):
        for h in range(Hkv):
            for t in range(T):
                if t >= counts[b]:
                    continue
                pos = starts[b] + t
                if table is None:
                    if pos < cache.shape[2]:
                        out[b, h, pos] = new[b, h, t]
                elif pos < table.shape[1] * blk and 0 <= table[b, pos // blk] < cache.shape[0]:
                    out[table[b, pos // blk], h, pos % blk] = new[b, h, t]
    return out


@pytest.mark.parametrize("paged", [False, True])
def test_placement_model_against_a_naive_loop(paged):
    rng = np.random.default_rng(3)
    B, Hkv, T, D, blk, Sk = 2, 2, 70, 8, 64, 200
    new = rng.integers(0, 255, (B, Hkv, T, D)).astype(np.uint8)
    table = None
    if paged:
        cache = np.full((9, Hkv, blk, D), 0xAA, np.uint8)
        table = np.array([[0, 3, 5, 7], [1, -1, 9, 2]], np.int32)           # item 1: one negative entry, one at P
    else:
        cache = np.full((B, Hkv, Sk, D), 0xAA, np.uint8)
    for starts, counts in (([0, 0], [T, T]), ([60, 63], [T, 3]), ([190, 130], [T, T]), ([Sk, 256], [T, 0]), ([64, 120], [64, 9])):
        got, wrote = kv8.append(cache, new, starts, counts, blk, table)
        assert np.array_equal(got, _naive_append(cache, new, starts, counts, blk, table)), (starts, counts)
        assert (got[~wrote] == 0xAA).all()          # the untouched bytes
        placed = sum(1 for b in range(B) for t in range(counts[b])
                     if (starts[b] + t < (Sk if not paged else 4 * blk))
                     and (not paged or 0 <= table[b, (starts[b] + t) // blk] < 9))
        assert wrote.sum() == placed * Hkv * D
    # clamps: a start beyond the capacity writes nothing, a count beyond T is T
    got, wrote = kv8.append(cache, new, [10 ** 6, -5], [T, 10 ** 6], blk, table)
    assert not wrote[0 if not paged else [0, 3, 5, 7]].any() and wrote.any()


# ---- dequantised attention and the exponent range ---------------------------------------------------------------------------------------
def test_dequantised_attention_with_log_sum_exp_and_where_the_scales_act():
    """fp64 attention over code * scale: the K scale acts on the scores (and so on the log-sum-exp), the V scale on the output
    alone; with power-of-two scales the kernel's placement (scale the finished score, scale the merged row) is the same fp64
    number as attention over the dequantised cache."""
    B, H, Hkv, Sq, D, blk = 2, 4, 2, 3, 64, 64
    rng = np.random.default_rng(5)
    q = rng.standard_normal((B, H, Sq, D)).astype(np.float32)
    k, v = (rng.standard_normal((B, Hkv, ref.SK, D)).astype(np.float32) for _ in range(2))
    mask = rng.random((B, Hkv, 1, -(-ref.SK // blk))) < 0.5
    mask[..., 0] = True
    lens = [ref.SK, 333]
    seen = ref.visible(mask, lens, Sq, ref.SK, blk, H, True)
    for ks, vs in (kv8.pow2_scales(Hkv, 1), kv8.odd_scales(Hkv)):
        kc, vc = kv8.quantize(k, ks), kv8.quantize(v, vs)
        kd, vd = kv8.dequant(kc, ks), kv8.dequant(vc, vs)
        out, lse = ref.attention(ref.scores2(q, kd, D ** -0.5), seen, vd)
        # the kernel's placement: scores over the bare codes times k_scale, the merged row over the bare codes times v_scale
        s2 = ref.scores2(q, kv8.dequant(kc, 1.0), D ** -0.5) * np.repeat(ks.astype(np.float64), H // Hkv)[None, :, None, None]
        out2, lse2 = ref.attention(s2, seen, kv8.dequant(vc, 1.0))
        out2 = out2 * np.repeat(vs.astype(np.float64), H // Hkv)[None, :, None, None]
        assert np.allclose(out, out2, rtol=1e-12, atol=1e-13) and np.allclose(lse, lse2, rtol=1e-12, atol=1e-12)
        # the format's distance from attention over the un-quantised K / V: e4m3 has three mantissa bits
        exact, _ = ref.attention(ref.scores2(q, k, D ** -0.5), seen, v)
        assert 1e-4 < np.abs(out - exact).max() < 0.2
        # v_scale does not reach the log-sum-exp
        _, lse3 = ref.attention(ref.scores2(q, kd, D ** -0.5), seen, vd * 3.0)
        assert np.array_equal(lse, lse3)


def test_exponent_range_of_the_byte_equality_inputs():
    """N(0, 1) inputs under scales 2^-2 .. 2^2: every magnitude the walk forms lies between 2^-40 and 2^20, far inside fp32 (and
    the operands inside fp16), so a power-of-two scale commutes with every rounding."""
    for seed, (H, Hkv) in enumerate(ref.GROUPS):
        for D in (64, 128):
            g = torch.Generator().manual_seed(1000 * seed)
            q = torch.randn(2, H, 8, D, generator=g).numpy()
            k, v = (torch.randn(2, Hkv, ref.SK, D, generator=g).numpy() for _ in range(2))
            ks, vs = kv8.pow2_scales(Hkv, seed)
            kd, vd = kv8.dequant(kv8.quantize(k, ks), ks), kv8.dequant(kv8.quantize(v, vs), vs)
            lo, hi = kv8.exponent_range(q, kd, vd, D ** -0.5)
            assert -40 <= lo and hi <= 20, (lo, hi)
            assert np.abs(kd).max() < 2.0 ** 8 and np.abs(vd).max() < 2.0 ** 8


def test_pow2_scales_differ_between_k_and_v_and_cover_the_range():
    seen = set()
    for seed in range(40):
        ks, vs = kv8.pow2_scales(8, seed)
        assert (ks != vs).all()
        seen.update(np.log2(ks).astype(int).tolist() + np.log2(vs).astype(int).tolist())
    assert seen == {-2, -1, 0, 1, 2}


# ---- the pooled value -------------------------------------------------------------------------------------------------------------------
def test_pooled_value_model():
    rng = np.random.default_rng(9)
    B, Hkv, Sk, D, blk = 2, 2, 300, 8, 64
    codes = rng.integers(0, 0x7E, (B, Hkv, Sk, D)).astype(np.uint8) | (rng.integers(0, 2, (B, Hkv, Sk, D)).astype(np.uint8) << 7)
    lens = [300, 77]
    codes[1, :, 77:] = kv8.NAN_CODE
    scale = np.array([0.37, 4.0], np.float32)
    got = kv8.pooled(codes, scale, lens, blk)
    vals = kv8.code_values()
    for b in range(B):
        for j in range(-(-Sk // blk)):
            rows = [r for r in range(j * blk, min((j + 1) * blk, Sk)) if r < lens[b]]
            for h in range(Hkv):
                want = sum(vals[codes[b, h, r]] for r in rows) / len(rows) * float(scale[h]) if rows else 0.0
                assert np.allclose(got[b, h, j], want, rtol=1e-13, atol=0), (b, h, j)
    assert np.isfinite(got).all()


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) -----------------------------------------------
def _q(B=2, H=8, Sq=1, D=64, dt=torch.bfloat16):
    return torch.zeros(B, H, Sq, D, dtype=dt)


def _c8(B=2, Hkv=2, Sk=700, D=64):
    return torch.zeros(B, Hkv, Sk, D, dtype=torch.uint8).view(E4M3)


def _mask(B=2, Hl=2, NK=6):
    return torch.ones(B, Hl, 1, NK, dtype=torch.bool)


def test_the_writer_is_exported_from_the_package():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import append_kv_e4m3, block_sparse
    assert callable(append_kv_e4m3) and callable(block_sparse.append_kv_e4m3)
    assert "append_kv_e4m3" in dir(rectified_spaattn_amd)


def test_decode_refusals():
    from rectified_spaattn_amd import block_sparse_decode as dec
    q, k, v, m = _q(), _c8(), _c8(), _mask()
    ok = dict(k_scale=1.0, v_scale=0.5)
    # scales missing, or given with a 2-byte cache
    for kw in (dict(), dict(k_scale=1.0), dict(v_scale=1.0)):
        with pytest.raises(ValueError, match="required"):
            dec(q, k, v, m, **kw)
    k2 = torch.zeros(2, 2, 700, 64, dtype=torch.bfloat16)
    for kw in (dict(k_scale=1.0), dict(v_scale=torch.ones(2)), ok):
        with pytest.raises(ValueError, match="float8_e4m3fn cache"):
            dec(q, k2, k2, m, **kw)
    # a k / v dtype mix, an e4m3 q
    with pytest.raises(ValueError, match="both float8_e4m3fn"):
        dec(q, k, k2, m, **ok)
    with pytest.raises(ValueError, match="both float8_e4m3fn"):
        dec(q, k2, v, m, **ok)
    with pytest.raises(ValueError, match="bfloat16 / float16 q"):
        dec(_c8(Hkv=8, Sk=1), k, v, m, **ok)
    with pytest.raises(ValueError, match="dtype"):
        dec(q, k.view(torch.float8_e5m2), v.view(torch.float8_e5m2), m, **ok)
    # a scale of the wrong length, dtype, device, value
    for bad in (torch.ones(3), torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.bfloat16), torch.ones(2, device="meta"),
                0.0, -1.0, float("inf"), float("nan"), True, "1", [1.0, 1.0]):
        with pytest.raises(ValueError, match="k_scale"):
            dec(q, k, v, m, k_scale=bad, v_scale=1.0)
        with pytest.raises(ValueError, match="v_scale"):
            dec(q, k, v, m, k_scale=1.0, v_scale=bad)
    # head dims 16 / 32, a head dim outside the list
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            dec(_q(D=D), _c8(D=D), _c8(D=D), m, **ok)
    with pytest.raises(ValueError, match="head dim"):
        dec(_q(D=48), _c8(D=48), _c8(D=48), m, **ok)
    # misaligned views are refused, never copied: K is loaded 8 bytes a lane, V 16
    flat = torch.zeros(2 * 2 * 700 * 64 + 64, dtype=torch.uint8).view(E4M3)
    off8 = flat[8:8 + 2 * 2 * 700 * 64].view(2, 2, 700, 64)
    off4 = flat[4:4 + 2 * 2 * 700 * 64].view(2, 2, 700, 64)
    assert off8.data_ptr() % 16 == 8 and off4.data_ptr() % 8 == 4
    with pytest.raises(ValueError, match="k: .*8 bytes"):
        dec(q, off4, v, m, **ok)
    with pytest.raises(ValueError, match="v: .*16 bytes"):
        dec(q, k, off8, m, **ok)
    wide = torch.zeros(2, 2, 700, 72, dtype=torch.uint8).view(E4M3)[..., :64]       # rows 72 bytes apart: fine for K, not for V
    with pytest.raises(ValueError, match="v: .*16 bytes"):
        dec(q, wide, wide, m, **ok)
    with pytest.raises(ValueError, match="not copied"):
        dec(q, k.transpose(2, 3).contiguous().transpose(2, 3), v, m, **ok)
    # the existing refusals hold through the new form
    with pytest.raises(NotImplementedError, match="block_size"):
        dec(q, k, v, m, block_size=96, **ok)
    with pytest.raises(ValueError, match="same K/V heads"):
        dec(q, k, v[:, :1], m, **ok)
    with pytest.raises(ValueError, match="one query block"):
        dec(_q(Sq=129), k, v, m, **ok)
    with pytest.raises(ValueError, match="kv_len"):
        dec(q, k, v, m, kv_len=701, **ok)
    with pytest.raises(ValueError, match="key blocks"):
        dec(q, k, v, _mask(NK=7), **ok)
    with pytest.raises(NotImplementedError, match="block_sparse_attention"):
        dec(_q(Sq=17), k, v, m, **ok)
    pool = torch.zeros(9, 2, 128, 64, dtype=torch.uint8).view(E4M3)
    with pytest.raises(ValueError, match="block_table"):
        dec(q, pool, pool, m, block_table=torch.zeros(2, 6, dtype=torch.int64), **ok)
    with pytest.raises(ValueError, match="page pools"):
        dec(q, pool[:, :, :64], pool[:, :, :64], m, block_table=torch.zeros(2, 6, dtype=torch.int32), **ok)


def test_pool_keys_refusals():
    from rectified_spaattn_amd import pool_keys
    k = _c8()
    with pytest.raises(ValueError, match="required"):
        pool_keys(k)
    with pytest.raises(ValueError, match="float8_e4m3fn cache"):
        pool_keys(torch.zeros(2, 2, 700, 64, dtype=torch.bfloat16), k_scale=1.0)
    for bad in (torch.ones(3), torch.ones(2, dtype=torch.float16), torch.ones(2, device="meta"), 0.0, -2.0):
        with pytest.raises(ValueError, match="k_scale"):
            pool_keys(k, k_scale=bad)
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            pool_keys(_c8(D=D), k_scale=1.0)
    flat = torch.zeros(2 * 2 * 700 * 64 + 64, dtype=torch.uint8).view(E4M3)
    with pytest.raises(ValueError, match="8 bytes"):
        pool_keys(flat[4:4 + 2 * 2 * 700 * 64].view(2, 2, 700, 64), k_scale=1.0)
    with pytest.raises(ValueError, match="out: required"):
        pool_keys(k, k_scale=1.0, start=5)
    with pytest.raises(ValueError, match="kv_len"):
        pool_keys(k, k_scale=1.0, kv_len=701)
    with pytest.raises(ValueError, match="out"):
        pool_keys(k, k_scale=1.0, out=torch.zeros(2, 2, 5, 64))
    with pytest.raises(ValueError, match="block_table"):
        pool_keys(torch.zeros(9, 2, 128, 64, dtype=torch.uint8).view(E4M3), k_scale=1.0, block_table=torch.zeros(12, dtype=torch.int32))


def test_writer_refusals():
    from rectified_spaattn_amd import append_kv_e4m3 as app
    new = torch.zeros(2, 2, 5, 64, dtype=torch.bfloat16)
    kc, vc = _c8(), _c8()
    ok = dict(start=0, k_scale=1.0, v_scale=1.0)
    with pytest.raises(TypeError):
        app(new, new, kc, vc, start=0)              # the scales are required keywords
    with pytest.raises(ValueError, match="required"):
        app(new, new, kc, vc, start=0, k_scale=None, v_scale=1.0)
    with pytest.raises(NotImplementedError, match="block_size"):
        app(new, new, kc, vc, block_size=96, **ok)
    with pytest.raises(ValueError, match="dtype"):
        app(new.float(), new.float(), kc, vc, **ok)
    with pytest.raises(ValueError, match="dtype"):
        app(new, new.half(), kc, vc, **ok)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        app(new, new, torch.zeros(2, 2, 700, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 700, 64, dtype=torch.bfloat16), **ok)
    with pytest.raises(ValueError, match="both float8_e4m3fn"):
        app(new, new, kc, torch.zeros(2, 2, 700, 64, dtype=torch.bfloat16), **ok)
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            app(new[..., :D].contiguous(), new[..., :D].contiguous(), _c8(D=D), _c8(D=D), **ok)
    with pytest.raises(ValueError, match="match"):
        app(new, new, _c8(Hkv=3), _c8(Hkv=3), **ok)
    with pytest.raises(ValueError, match="match"):
        app(new, new, _c8(B=3), _c8(B=3), **ok)
    with pytest.raises(ValueError, match="match"):
        app(new, new, _c8(D=128), _c8(D=128), **ok)
    with pytest.raises(ValueError, match="match"):
        app(new, new[:, :, :4], kc, vc, **ok)
    for start in (701, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="start"):
            app(new, new, kc, vc, start=start, k_scale=1.0, v_scale=1.0)
    for n in (6, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="n_new"):
            app(new, new, kc, vc, n_new=n, **ok)
    for bad in (torch.ones(3), torch.ones(2, dtype=torch.float64), torch.ones(2, device="meta"), 0.0, float("nan")):
        with pytest.raises(ValueError, match="v_scale"):
            app(new, new, kc, vc, start=0, k_scale=1.0, v_scale=bad)
    # the inputs are never copied: views that would need one are refused; so are caches off the store alignment
    with pytest.raises(ValueError, match="not copied"):
        app(new.transpose(2, 3).contiguous().transpose(2, 3), new, kc, vc, **ok)
    flat = torch.zeros(2 * 2 * 700 * 64 + 64, dtype=torch.uint8).view(E4M3)
    with pytest.raises(ValueError, match="k_cache: .*8 bytes"):
        app(new, new, flat[4:4 + 2 * 2 * 700 * 64].view(2, 2, 700, 64), vc, **ok)
    # the paged form
    pool = torch.zeros(9, 2, 128, 64, dtype=torch.uint8).view(E4M3)
    for table in (torch.zeros(2, 6, dtype=torch.int64), torch.zeros(3, 6, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)):
        with pytest.raises(ValueError, match="block_table"):
            app(new, new, pool, pool, block_table=table, **ok)
    with pytest.raises(ValueError, match="page pools"):
        app(new, new, pool[:, :, :64], pool[:, :, :64], block_table=torch.zeros(2, 6, dtype=torch.int32), **ok)
    with pytest.raises(ValueError, match="start"):
        app(new, new, pool, pool, block_table=torch.zeros(2, 6, dtype=torch.int32), start=769, k_scale=1.0, v_scale=1.0)


@pytest.mark.parametrize("what", ["decode", "decode-paged-tensor-scales", "pool", "append", "append-paged"])
def test_a_well_formed_call_on_cpu_tensors_reaches_the_device_check(what):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, append_kv_e4m3, block_sparse_decode, pool_keys
    pool, table = torch.zeros(15, 2, 128, 64, dtype=torch.uint8).view(E4M3), torch.zeros(2, 6, dtype=torch.int32)
    new = torch.zeros(2, 2, 5, 64, dtype=torch.float16)
    with pytest.raises(_lib.RsaError):
        if what == "decode":
            block_sparse_decode(_q(), _c8(), _c8(), _mask(), k_scale=0.5, v_scale=2, causal=True, return_lse=True)
        elif what == "decode-paged-tensor-scales":
            block_sparse_decode(_q(dt=torch.float16), pool, pool, _mask(), k_scale=torch.ones(2), v_scale=torch.ones(1),
                                block_table=table, kv_len=[700, 333])
        elif what == "pool":
            pool_keys(_c8(), k_scale=torch.ones(2), kv_len=[700, 333])
        elif what == "append":
            append_kv_e4m3(new, new, _c8(), _c8(), start=[3, 695], n_new=[5, 2], k_scale=1.0, v_scale=torch.ones(2))
        else:
            append_kv_e4m3(new, new, pool, pool, start=0, k_scale=1.0, v_scale=1.0, block_table=table)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_declared_listed_and_exported_and_the_version_stays():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTED, name
    order = [n for n in re.findall(r"\bint\s+(rsa_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)) if n in _lib.PROTOTYPES]
    assert [n for n in _lib.PROTOTYPES if n in NAMES] == [n for n in order if n in NAMES]       # the header's order
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    mk = open(os.path.join(root, "rectified_spaattn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^rsa_kv8\.o:.*\n\t.*-ffp-contract=off", mk, re.M) and re.search(r"^\.\./librsa_hip\.so:.*\brsa_kv8\.o\b", mk, re.M)
    _, L = _lib_or_skip()
    assert all(hasattr(L, name) for name in NAMES)
    assert L.rsa_version() == 601


def test_decode_kv8_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    tq = _lib.RsaTensor4(4096, 8 * 128, 128, 128)
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)        # an e4m3 cache: strides in bytes
    o = _lib.RsaOut4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks
    big = 1 << 30

    def call(B=1, H=8, Hkv=2, Hl=2, Sq=1, Sk=700, D=128, dt=0, blk=128, NK=6, kv=None, kvv=700, causal=0, scale=0.1, q=tq, k=t, v=t,
             table=None, tsb=6, pages=0, cols=p, counts=p, bps=0, ws=p, wsb=big, out=o, lse=None, ks=p, vs=p):
        return L.rsa_block_sparse_decode_kv8(B, H, Hkv, Hl, Sq, Sk, D, dt, blk, NK, kv, kvv, causal, scale, q, k, v, table, tsb,
                                             pages, cols, counts, bps, ws, wsb, out, lse, ks, vs, None)

    for base in (dict(), dict(Hl=8), dict(causal=1, Sq=3), dict(lse=p), dict(kv=p), dict(table=p, pages=20), dict(bps=2), dict(dt=1)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(wsb=0) == WS                        # (everything else passes: the workspace is checked last)
        # NULL or misaligned scale pointers
        assert c(ks=None) == BAD and c(vs=None) == BAD
        assert c(ks=ctypes.c_void_p(4098)) == BAD and c(vs=ctypes.c_void_p(4097)) == BAD
        # K: 8 bytes, V: 16
        assert c(k=_lib.RsaTensor4(4104, 2 * 128 * 700, 128 * 700, 128), wsb=0) == WS
        assert c(k=_lib.RsaTensor4(4100, 2 * 128 * 700, 128 * 700, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 136), wsb=0) == WS
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(v=_lib.RsaTensor4(4104, 2 * 128 * 700, 128 * 700, 128)) == BAD
        assert c(v=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 136)) == BAD
        assert c(v=_lib.RsaTensor4(4096, 2 * 128 * 700 + 8, 128 * 700, 128)) == BAD
        assert c(v=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 144), wsb=0) == WS
        assert c(k=_lib.RsaTensor4(None, 2 * 128 * 700, 128 * 700, 128)) == BAD
        assert c(v=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        # the existing bad-argument cases through the new entry
        assert c(blk=96) == UNS and c(blk=32) == UNS
        assert c(D=96) == UNS and c(D=32) == UNS and c(D=16) == UNS
        assert c(dt=7) == UNS
        assert c(B=0) == BAD and c(Sq=0) == BAD and c(Sk=0) == BAD and c(NK=0) == BAD
        assert c(NK=7) == BAD and c(blk=64, NK=12) == BAD
        assert c(Sq=129, H=2, Hkv=2, Hl=2) == BAD
        assert c(bps=-1) == BAD
        assert c(ws=None) == BAD and c(ws=ctypes.c_void_p(4104)) == BAD
        assert c(cols=None) == BAD and c(counts=None) == BAD
        assert c(cols=ctypes.c_void_p(4098)) == BAD and c(lse=ctypes.c_void_p(4098)) == BAD and c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(table=p, pages=0) == BAD and c(table=p, pages=20, tsb=-6) == BAD
        assert c(q=_lib.RsaTensor4(4100, 8 * 128, 128, 128)) == BAD
        assert c(out=_lib.RsaOut4(None, 8 * 128, 128, 128)) == BAD and c(out=_lib.RsaOut4(4096, 8 * 128, 130, 128)) == BAD
        if "kv" not in base:
            assert c(kvv=-1) == BAD and c(kvv=701) == BAD
    assert call(Hkv=3, Hl=3) == BAD and call(Hl=4) == BAD
    assert call(Sq=17) == UNS and call(Sq=16, wsb=0) == WS
    # the workspace is rsa_block_sparse_decode_bytes'
    n = ctypes.c_size_t(0)
    assert L.rsa_block_sparse_decode_bytes(1, 8, 2, 2, 1, 128, 6, 0, ctypes.byref(n)) == 0
    assert call(wsb=n.value - 1) == WS and call(wsb=n.value, blk=96) == UNS


def test_pool_keys_kv8_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS = -1, -2
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    p = ctypes.c_void_p(4096)

    def call(B=2, Hkv=2, Sk=700, D=128, blk=128, NK=6, k=t, table=None, tsb=6, pages=0, kv=None, kvv=700, st=None, stv=0, wph=0,
             out=p, ks=p):
        return L.rsa_pool_keys_kv8(B, Hkv, Sk, D, blk, NK, k, table, tsb, pages, kv, kvv, st, stv, wph, out, ks, None)

    for base in (dict(), dict(kv=p), dict(st=p), dict(table=p, pages=20, Sk=768), dict(wph=3), dict(D=64)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(ks=None) == BAD and c(ks=ctypes.c_void_p(4098)) == BAD
        assert c(D=16) == UNS and c(D=32) == UNS and c(D=96) == UNS
        assert c(blk=96) == UNS
        assert c(Sk=8193 * 128, NK=8193) == UNS
        assert c(B=0) == BAD and c(Hkv=0) == BAD and c(Sk=0) == BAD and c(NK=0) == BAD
        assert c(NK=7) == BAD and c(blk=64, NK=6) == BAD
        assert c(wph=-1) == BAD
        assert c(out=None) == BAD and c(out=ctypes.c_void_p(4104)) == BAD
        assert c(kv=ctypes.c_void_p(4098)) == BAD and c(st=ctypes.c_void_p(4097)) == BAD
        assert c(table=p, pages=0) == BAD and c(table=p, pages=20, tsb=-6) == BAD
        assert c(k=_lib.RsaTensor4(None, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4100, 2 * 128 * 700, 128 * 700, 128)) == BAD        # 8-byte loads
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        if "kv" not in base:
            assert c(kvv=-1) == BAD and c(kvv=base.get("Sk", 700) + 1) == BAD
        if "st" not in base:
            assert c(stv=-1) == BAD and c(stv=base.get("Sk", 700) + 1) == BAD


def test_writer_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS = -1, -2
    src = _lib.RsaTensor4(4096, 2 * 128 * 5, 128 * 5, 128)
    dst = _lib.RsaOut4(4096, 2 * 128 * 700, 128 * 700, 128)
    p = ctypes.c_void_p(4096)

    def call(B=2, Hkv=2, T=5, Sk=700, D=128, dt=0, blk=128, kn=src, vn=src, kc=dst, vc=dst, table=None, tsb=6, pages=0, st=None,
             stv=0, nn=None, nv=5, ks=p, vs=p):
        return L.rsa_kv8_append(B, Hkv, T, Sk, D, dt, blk, kn, vn, kc, vc, table, tsb, pages, st, stv, nn, nv, ks, vs, None)

    for base in (dict(), dict(st=p), dict(nn=p), dict(st=p, nn=p), dict(table=p, pages=20, Sk=768), dict(dt=1), dict(D=64), dict(blk=64)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(ks=None) == BAD and c(vs=None) == BAD
        assert c(ks=ctypes.c_void_p(4098)) == BAD and c(vs=ctypes.c_void_p(4097)) == BAD
        assert c(D=16) == UNS and c(D=32) == UNS and c(D=96) == UNS
        assert c(blk=96) == UNS and c(dt=7) == UNS
        assert c(B=0) == BAD and c(Hkv=0) == BAD and c(T=0) == BAD and c(Sk=0) == BAD and c(T=-3) == BAD
        assert c(st=ctypes.c_void_p(4098)) == BAD and c(nn=ctypes.c_void_p(4097)) == BAD
        assert c(table=ctypes.c_void_p(4098), pages=20, Sk=768) == BAD
        assert c(table=p, pages=0, Sk=768) == BAD and c(table=p, pages=20, tsb=-6, Sk=768) == BAD
        assert c(table=p, pages=20, Sk=700) == BAD                      # a paged capacity is whole blocks
        assert c(kn=_lib.RsaTensor4(None, 2 * 128 * 5, 128 * 5, 128)) == BAD
        assert c(vn=_lib.RsaTensor4(4100, 2 * 128 * 5, 128 * 5, 128)) == BAD
        assert c(kn=_lib.RsaTensor4(4096, 2 * 128 * 5, 128 * 5, 132)) == BAD
        assert c(vn=_lib.RsaTensor4(4096, 2 * 128 * 5, 128 * 5, -128)) == BAD
        assert c(kc=_lib.RsaOut4(None, 2 * 128 * 700, 128 * 700, 128)) == BAD
        assert c(vc=_lib.RsaOut4(4100, 2 * 128 * 700, 128 * 700, 128)) == BAD      # 8-byte stores
        assert c(kc=_lib.RsaOut4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(vc=_lib.RsaOut4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        if "st" not in base:
            assert c(stv=-1) == BAD and c(stv=base.get("Sk", 700) + 1) == BAD
        if "nn" not in base:
            assert c(nv=-1) == BAD and c(nv=6) == BAD
