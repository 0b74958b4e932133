"""The MXFP4 K/V cache without a device: tests/kv4_ref.py itself -- the contract the writer is held to --
the Python refusals of the calls that take such a cache, and the three C entries in the header and the prototype table."""
import os
import re

import numpy as np
import pytest
import torch

import kv4_ref as kv4
from rectified_spaattn_amd import _lib, block_sparse as bs

NAMES = ("rsa_kv4_append", "rsa_block_sparse_decode_kv4", "rsa_pool_keys_kv4")
TIES = [(0.25, 0), (0.75, 2), (1.25, 2), (1.75, 4), (2.5, 4), (3.5, 6), (5.0, 6)]       # value -> code, under e = 0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_every_value_of_the_format_is_exact_in_both_two_byte_types(dt):
    e = np.arange(kv4.E_MIN, kv4.E_MAX + 1)
    vals = torch.from_numpy((kv4.E2M1[None, :] * np.exp2(e)[:, None]).astype(np.float32))
    assert torch.equal(vals.to(dt).float(), vals) and float(vals.max()) == 49152.0
    nz = vals[vals > 0]
    assert float(nz.min()) == 2.0 ** -14 >= torch.finfo(dt).tiny         # a normal number of both types


def _row(first, rest=0.0):
    x = np.full((1, 32), rest, np.float32)
    x[0, :len(first)] = first
    return x


def test_named_edges_ties_saturation_inf_nan_and_minus_zero():
    # a group maximum of 4 gives e = 0: the ties go to the even code, both signs
    for sign in (1.0, -1.0):
        codes, scales = kv4.quantize(_row([4.0] + [sign * v for v, _ in TIES]))
        nib = np.stack([codes & 0xF, codes >> 4], -1).reshape(-1)
        assert scales[0, 0] == 127 and nib[0] == 6
        assert nib[1:8].tolist() == [c | (8 if sign < 0 else 0) for _, c in TIES]
    # saturation (7.9 under e = 0), +-Inf at e = 13, NaN -> 0x0 and out of the maximum, -0 and a small negative -> 0x8
    codes, scales = kv4.quantize(_row([7.9, -7.5, float("nan"), -0.0, -1e-3, 0.0]))
    assert scales[0, 0] == 127 and (codes[0, :3].tolist() == [0xF7, 0x80, 0x08])
    codes, scales = kv4.quantize(_row([float("inf"), float("-inf"), 49152.0, 1e4, float("nan")]))
    assert scales[0, 0] == 127 + 13
    assert codes[0, 0] == 0xF7 and codes[0, 1] == 0x27 and codes[0, 2] == 0x00         # 49152 = 6 * 2^13, 1e4 / 2^13 = 1.22 -> 1
    codes, scales = kv4.quantize(_row([float("nan")] * 32))
    assert scales[0, 0] == 127 + kv4.E_MIN and not codes.any()


@pytest.mark.parametrize("a,byte", [(0.0, 114), (1e-40, 114), (2.0 ** -12, 114), (2.0 ** -11, 114), (2.0 ** -10, 115), (2.0 ** 14, 139),
                                    (2.0 ** 15, 140), (3e38, 140), (1.0, 125), (7.9, 127)])
def test_group_maximum_at_both_clamp_ends(a, byte):
    codes, scales = kv4.quantize(_row([a]))
    assert scales[0, 0] == byte and kv4.E_MIN <= int(scales[0, 0]) - 127 <= kv4.E_MAX
    if a >= 2.0 ** -11 and a < 2.0 ** 15:
        assert 4.0 <= a * 2.0 ** (127 - byte) < 8.0 and (codes[0, 0] & 0xF) in (6, 7)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_round_trip_is_within_half_a_grid_step_where_nothing_saturates(dt):
    x = (torch.randn(64, 128, generator=torch.Generator().manual_seed(0)) * 3.0).to(dt)
    codes, scales = kv4.quantize(x)
    back, xs = kv4.dequant(codes, scales), x.double().numpy()
    unit = np.repeat(np.exp2(scales.astype(np.float64) - 127), 32, -1)
    y = np.abs(xs) / unit
    half = np.where(y < 2, 0.25, np.where(y < 4, 0.5, 1.0)) * unit
    free = y <= 6
    assert free.mean() > 0.9 and (np.abs(back - xs)[free] <= half[free]).all()
    assert (np.abs(back)[~free] == 6 * unit[~free]).all() and codes.shape == (64, 64) and scales.shape == (64, 4)


def _cache(D=128, Sk=256, code_dt=torch.uint8):
    z = lambda last: torch.zeros(1, 2, Sk, last, dtype=torch.uint8)      # noqa: E731
    return z(D // 2).view(code_dt), z(D // 32), z(D // 2).view(code_dt), z(D // 32)


REFUSALS = {
    "one scale without the other": (ValueError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_decode(q, kc, vc, m, k_block_scale=ks)),
    "wrong scale shape": (ValueError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_decode(q, kc, vc, m, k_block_scale=ks[..., :2], v_block_scale=vs)),
    "wrong scale dtype": (ValueError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_decode(q, kc, vc, m, k_block_scale=ks.float(), v_block_scale=vs)),
    "scales beside a 2-byte cache": (ValueError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_decode(q, q.expand(1, 2, 256, 128), q.expand(1, 2, 256, 128), m, k_block_scale=ks, v_block_scale=vs)),
    "scales beside an e4m3 cache": (ValueError, lambda q, kc, ks, vc, vs, m: bs.pool_keys(torch.zeros(1, 2, 256, 128).to(torch.float8_e4m3fn), k_block_scale=ks)),
    "head dim 32": (NotImplementedError, lambda q, kc, ks, vc, vs, m: bs.pool_keys(kc[..., :16], k_block_scale=ks[..., :1])),
    "a per-head scale beside the block scales": (NotImplementedError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_decode(q, kc, vc, m, k_scale=1.0, v_scale=1.0, k_block_scale=ks, v_block_scale=vs)),
    "a misaligned K view": (ValueError, lambda q, kc, ks, vc, vs, m: bs.pool_keys(torch.zeros(1, 2, 256, 66, dtype=torch.uint8)[..., 1:65], k_block_scale=ks)),
    "block_sparse_extend": (NotImplementedError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_extend(q, kc, vc, m, k_block_scale=ks, v_block_scale=vs)),
    "pool_key_bounds": (NotImplementedError, lambda q, kc, ks, vc, vs, m: bs.pool_key_bounds(kc, k_block_scale=ks)),
    "the packed writer": (NotImplementedError, lambda q, kc, ks, vc, vs, m: bs.append_kv_mxfp4(q, q, kc, ks, vc, vs, start=0, cu_seqlens=torch.zeros(2, dtype=torch.int32))),
    "block_sparse_attention": (NotImplementedError, lambda q, kc, ks, vc, vs, m: bs.block_sparse_attention(q, kc.view(torch.float4_e2m1fn_x2), vc.view(torch.float4_e2m1fn_x2), m)),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_python_refusals(name):
    exc, call = REFUSALS[name]
    q, mask = torch.zeros(1, 2, 1, 128, dtype=torch.bfloat16), torch.ones(1, 2, 1, 2, dtype=torch.bool)
    with pytest.raises(exc):
        call(q, *_cache(), mask)


def test_the_three_entries_in_the_header_the_table_and_the_export_list():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rsa.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    order = [n for n in re.findall(r"\bint\s+(rsa_\w+)\s*\(", hdr) if n in NAMES]
    assert order == list(NAMES) == [n for n in _lib.PROTOTYPES if n in NAMES] and all(n in _lib.EXPORTED for n in NAMES)
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    dec, dec4 = _lib.PROTOTYPES["rsa_block_sparse_decode"][1], _lib.PROTOTYPES["rsa_block_sparse_decode_kv4"][1]
    assert dec4 == dec[:-1] + [_lib.RsaTensor4, _lib.RsaTensor4] + dec[-1:]      # the two scale views in front of the stream
    import rectified_spaattn_amd
    assert callable(rectified_spaattn_amd.append_kv_mxfp4) and callable(bs.append_kv_mxfp4)
