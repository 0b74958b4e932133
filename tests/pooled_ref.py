"""The numpy model of the pooled-key cache (pool_keys): select_ref.pooled per block, plus the range of
blocks a call writes.  tests/test_pooled_keys_cpu.py holds it against a naive per-block loop.

    k [B, Hkv, Sk, D] float64; lens / starts: B ints in [0, Sk]; blk: 64 or 128; the cache fp64 [B, Hkv, ceil(Sk / blk), D]
"""
import numpy as np

import select_ref


def written(start: int, length: int, blk: int):
    """The blocks one batch item's call writes: start // blk <= j < ceil(length / blk); none when start > length."""
    if start > length:
        return range(0)
    return range(start // blk, -(-length // blk))


def update(cache, k, lens, starts, blk):
    """The cache after pool_keys(k, kv_len=lens, start=starts, out=cache): the written blocks hold select_ref.pooled's value at
    lens, every other element is the old one.  Returns (new cache, bool [B, NK] of the written blocks)."""
    B = k.shape[0]
    fresh = select_ref.pooled(k, lens, blk)
    out = cache.copy()
    wrote = np.zeros((B, fresh.shape[2]), bool)
    for b in range(B):
        for j in written(starts[b], lens[b], blk):
            out[b, :, j] = fresh[b, :, j]
            wrote[b, j] = True
    return out, wrote


def make(k, lens, blk, fill=np.nan):
    """pool_keys(k, kv_len=lens) into a cache that held `fill`."""
    B, Hkv, Sk, D = k.shape
    return update(np.full((B, Hkv, -(-Sk // blk), D), fill), k, lens, [0] * B, blk)


def block_naive(k, b, j, length, blk):
    """Block j of batch item b, key by key: [Hkv, D], or None when the block holds no key below `length`."""
    rows = [r for r in range(j * blk, (j + 1) * blk) if r < length and r < k.shape[2]]
    if not rows:
        return None
    acc = np.zeros((k.shape[1], k.shape[3]))
    for r in rows:
        acc += k[b, :, r]
    return acc / len(rows)
