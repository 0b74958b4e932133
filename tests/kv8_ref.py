"""The model of the e4m3 K/V cache: a plain helper module, no device.

    quantize       the writer's byte contract per element, on torch's CPU path:
                   (x.float() / scale[hkv]).clamp(-448, 448).to(torch.float8_e4m3fn), as uint8 codes
    dequant        float(code) * scale[hkv], fp64 (a NaN code reads as NaN)
    append         where the writer puts the rows of a call, which it drops, and that no other byte moves
    pooled         the value of a key block in pool_keys: the mean of float(code) over the keys below the limit, times the scale
    pow2_scales    per-head powers of two 2^e, e in -2 .. 2, different for K and V: code * 2^e is then exact in bf16 and in fp16
    exponent_range the binary exponents a byte-equality case touches: a power of two commutes with every fp32 rounding of the
                   walk only while nothing under- or overflows
"""
from __future__ import annotations

import numpy as np
import torch

import select_ref

E4M3 = torch.float8_e4m3fn
NAN_CODE = 0x7F
E4M3_MAX = 448.0


def scale_vector(scale, Hkv: int) -> np.ndarray:
    s = np.asarray(scale, np.float32).reshape(-1)
    return np.broadcast_to(s, (Hkv,)).copy() if s.size == 1 else s


def quantize(x, scale) -> np.ndarray:
    """x [B, Hkv, S, D] (numpy fp32, or a torch tensor of any float dtype) -> uint8 codes, one fp32 division per element."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, np.float32))
    s = torch.from_numpy(scale_vector(scale, t.shape[1])).view(1, -1, 1, 1)
    return (t.float().cpu() / s).clamp(-E4M3_MAX, E4M3_MAX).to(E4M3).view(torch.uint8).numpy()


def code_values() -> np.ndarray:
    """fp64 [256]: the value of every code (NaN for 0x7F and 0xFF)."""
    return torch.arange(256, dtype=torch.uint8).view(E4M3).double().numpy()


def dequant(codes, scale) -> np.ndarray:
    codes = np.asarray(codes, np.uint8)
    return code_values()[codes] * scale_vector(scale, codes.shape[1]).astype(np.float64)[None, :, None, None]


def pow2_scales(Hkv: int, seed: int):
    """(k_scale, v_scale), fp32 [Hkv] each: 2^e with e drawn from -2 .. 2 per head, and v's exponent never k's."""
    rng = np.random.default_rng(seed)
    ek = rng.integers(-2, 3, Hkv)
    ev = (ek + 2 + rng.integers(1, 5, Hkv)) % 5 - 2
    assert (ek != ev).all()
    return np.exp2(ek).astype(np.float32), np.exp2(ev).astype(np.float32)


def odd_scales(Hkv: int):
    """The issue's arbitrary scales, cycled over the heads."""
    ks, vs = [0.37, 1.9, 0.83, 2.6], [2.3, 0.11, 1.45, 0.52]
    return (np.array([ks[h % 4] for h in range(Hkv)], np.float32), np.array([vs[h % 4] for h in range(Hkv)], np.float32))


# ---- the writer's placement --------------------------------------------------------------------------------------------------------
def append(k_cache, new_codes, starts, counts, blk=None, table=None):
    """The cache after one call.  Contiguous: k_cache uint8 [B, Hkv, Sk, D].  Paged: k_cache is the pool [P, Hkv, blk, D] and
    table int [B, NKt].  new_codes uint8 [B, Hkv, T, D]; starts / counts: B ints (start clamped into [0, capacity], count into
    [0, T]).  Returns (new cache, bool mask of the bytes the call wrote)."""
    out = k_cache.copy()
    wrote = np.zeros(k_cache.shape, bool)
    B, _, T, _ = new_codes.shape
    cap = k_cache.shape[2] if table is None else table.shape[1] * blk
    for b in range(B):
        st, n = min(max(int(starts[b]), 0), cap), min(max(int(counts[b]), 0), T)
        for t in range(n):
            pos = st + t
            if pos >= cap:
                continue
            if table is None:
                item, row = b, pos
            else:
                item, row = int(table[b, pos // blk]), pos % blk
                if not 0 <= item < k_cache.shape[0]:
                    continue
            out[item, :, row] = new_codes[b, :, t]
            wrote[item, :, row] = True
    return out, wrote


# ---- pool_keys ------------------------------------------------------------------------------------------------------------------------
def pooled(codes, scale, lens, blk: int) -> np.ndarray:
    """fp64 [B, Hkv, NK, D]: select_ref.pooled over float(code) (codes at or beyond the limit are never read), times the scale."""
    vals = np.nan_to_num(code_values()[np.asarray(codes, np.uint8)], nan=0.0)
    return select_ref.pooled(vals, lens, blk) * scale_vector(scale, codes.shape[1]).astype(np.float64)[None, :, None, None]


# ---- the exponent range of a byte-equality case ---------------------------------------------------------------------------------------
def exponent_range(q, kd, vd, sm_scale: float):
    """(lowest, highest) binary exponent over the non-zero magnitudes a decode call forms from q and the DEQUANTISED cache kd /
    vd (fp64, NaN = never read): the operands, every q_d k_d product and every |v|, and the largest score and row of V sums.
    The lowest stays far above fp32's 2^-126 and the highest far below 2^127 (and fp16's 2^15 for the operands)."""
    q, kd, vd = (np.nan_to_num(np.abs(np.asarray(t, np.float64))) for t in (q, kd, vd))
    qs = q * float(sm_scale) * 1.4426950408889634
    lo, hi = [], []
    for t in (qs, kd, vd):
        nz = t[t > 0]
        lo.append(nz.min())
        hi.append(nz.max())
    lo.append(lo[0] * lo[1])                              # the smallest product inside a score
    hi.append(hi[0] * hi[1] * q.shape[-1])                # no score is larger
    hi.append(hi[2] * kd.shape[2])                        # no un-normalised O is larger (weights <= 1)
    return int(np.floor(np.log2(min(lo)))), int(np.ceil(np.log2(max(hi))))
