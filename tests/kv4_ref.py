"""The model of the MXFP4 K/V cache: a plain helper module, no device.  This file is the contract.

    quantize   the writer, per row and 32-channel group, in numpy:
                 a      = max |x_d| by fmax, so a NaN element does not take part
                 e      = clamp(exponent_field(a as fp32) - 127 - 2, -13, 13); a = 0 or a subnormal a gives -13
                 scale  = e + 127, one byte
                 code_d = x_d * 2^-e (exact) rounded to nearest even onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6, with the
                          sign bit of x_d (-0 and a negative that rounds to zero are 0x8); a NaN element is 0x0
               element 2 i in the low nibble of byte i
    dequant    e2m1(code_d) * 2^(scale[d // 32] - 127), fp64
    paged      a contiguous cache as page pools behind a block table, 0xFF in every byte no visible key owns
"""
from __future__ import annotations

import numpy as np
import torch

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
GROUP = 32
E_MIN, E_MAX = -13, 13
FILL = 0xFF


def quantize(x):
    """x [..., D] (a torch tensor of any float dtype, or numpy) -> (codes uint8 [..., D / 2], scales uint8 [..., D / 32])."""
    x = x.float().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float32)
    g = np.ascontiguousarray(x.reshape(x.shape[:-1] + (-1, GROUP)))
    a = np.ascontiguousarray(np.fmax.reduce(np.abs(g), axis=-1, initial=np.float32(0)), np.float32)
    e = np.clip(((a.view(np.uint32) >> 23) & 0xFF).astype(np.int64) - 127 - 2, E_MIN, E_MAX)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.abs(g).astype(np.float64) * np.exp2(-e.astype(np.float64))[..., None]
        # the midpoints of the grid: a tie goes to the neighbour whose code is even (NaN compares false everywhere: code 0)
        mag = ((y > 0.25).astype(np.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5.0)).astype(np.uint8)
    nib = (mag | ((np.signbit(g) & ~np.isnan(g)).astype(np.uint8) << 3)).reshape(x.shape)
    return nib[..., 0::2] | (nib[..., 1::2] << 4), (e + 127).astype(np.uint8)


def dequant(codes, scales) -> np.ndarray:
    """fp64 [..., D]; a scale byte of 0xFF reads as 2^128 here, which no test multiplies."""
    codes, scales = np.asarray(codes, np.uint8), np.asarray(scales, np.uint8)
    nib = np.stack([codes & 0xF, codes >> 4], -1).reshape(codes.shape[:-1] + (-1,))
    val = np.where(nib & 8, -1.0, 1.0) * E2M1[nib & 7]
    return val * np.repeat(np.exp2(scales.astype(np.float64) - 127), GROUP, -1)


def paged(arrays, blk: int, lens, seed: int, bad: int, fill: int = FILL, perm=None):
    """arrays: contiguous [B, Hkv, Sk, X] uint8 caches that share B and Sk -> (their page pools [P, Hkv, blk, X], table int32
    [B, NK], P): B * NK + 3 pages placed by one random permutation (perm, else numpy's for the seed), `fill` in spare pages and
    ragged tails, `bad` in the table where no key is.  The e4m3 tests' pools come from here too (test_gpu_kv8._pool8)."""
    B, _, Sk, _ = arrays[0].shape
    NK = -(-Sk // blk)
    P = B * NK + 3
    perm = np.random.default_rng(seed).permutation(P) if perm is None else perm
    pools = [np.full((P, a.shape[1], blk, a.shape[3]), fill, np.uint8) for a in arrays]
    table = np.full((B, NK), bad, np.int32)
    for b in range(B):
        for j in range(-(-lens[b] // blk)):
            rows = min(blk, Sk - j * blk)
            table[b, j] = perm[b * NK + j]
            for pool, a in zip(pools, arrays):
                pool[table[b, j], :, :rows] = a[b, :, j * blk:j * blk + rows]
    return pools, table, P
