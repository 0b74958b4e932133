"""The reference of the bounds cache and of select_blocks_bound in numpy fp64: per key block and channel
the minimum and the maximum of the keys below the limit, the score t = sum_d max(qs_d mn_d, qs_d mx_d) of the pooled query qs
against them, and behind the score select_ref's visible / forced / kept sets and select_p_ref's budget, unchanged.
tests/test_select_bound_cpu.py holds the vectorised forms against naive loops.

    q [B, H, Sq, D], k [B, Hkv, Sk, D] float64; lens / starts: B ints in [0, Sk]; blk: 64 or 128
    the cache fp64 [B, Hkv, ceil(Sk / blk), 2, D]: [..., 0, :] the minima, [..., 1, :] the maxima, 0 where a block has no key
"""
import numpy as np

import pooled_ref
import select_p_ref
import select_ref


def bounds(k, lens, blk):
    """[B, Hkv, Sk, D] -> [B, Hkv, NK, 2, D]: min and max over each block's keys < lens[b] (0 where it has none)."""
    B, Hkv, Sk, D = k.shape
    NK = -(-Sk // blk)
    out = np.zeros((B, Hkv, NK, 2, D))
    for b in range(B):
        for j in range(NK):
            lo, hi = j * blk, min((j + 1) * blk, Sk, lens[b])
            if hi > lo:
                out[b, :, j, 0] = k[b, :, lo:hi].min(axis=1)
                out[b, :, j, 1] = k[b, :, lo:hi].max(axis=1)
    return out + 0.0        # (+ 0.0: -0 is 0)


def update(cache, k, lens, starts, blk):
    """The cache after pool_key_bounds(k, kv_len=lens, start=starts, out=cache): the blocks of pooled_ref.written hold bounds'
    value at lens, every other element is the old one.  Returns (new cache, bool [B, NK] of the written blocks)."""
    B = k.shape[0]
    fresh = bounds(k, lens, blk)
    out = cache.copy()
    wrote = np.zeros((B, fresh.shape[2]), bool)
    for b in range(B):
        for j in pooled_ref.written(starts[b], lens[b], blk):
            out[b, :, j] = fresh[b, :, j]
            wrote[b, j] = True
    return out, wrote


def pooled_query(q, blk, mask_heads, Hkv, q_rows=None):
    """qs [B, Hl, NQ, D]: the sum over the list head's query heads of each head's mean over the block's rows < q_rows[b]."""
    B, H, Sq, D = q.shape
    qbar = select_ref.pooled(q, [Sq] * B if q_rows is None else list(q_rows), blk)
    if mask_heads == "q":
        return qbar
    return qbar.reshape(B, Hkv, H // Hkv, *qbar.shape[2:]).sum(axis=2)


def scores(q, bnd, blk, mask_heads="kv", q_rows=None):
    """t [B, Hl, NQ, NK] (every block, visible or not) = sum over d of max(qs_d mn_d, qs_d mx_d)."""
    Hkv = bnd.shape[1]
    qs = pooled_query(q, blk, mask_heads, Hkv, q_rows)
    per = np.repeat(bnd, qs.shape[1] // Hkv, axis=1)                    # the K/V head of each list head
    lo = qs[:, :, :, None, :] * per[:, :, None, :, 0, :]
    hi = qs[:, :, :, None, :] * per[:, :, None, :, 1, :]
    return np.maximum(lo, hi).sum(-1) + 0.0


def magnitude(q, bnd, blk, mask_heads="kv", q_rows=None):
    """M [B, Hl, NQ, NK] = sum over d of |qs_d| max(|mn_d|, |mx_d|): the scale of the fp32 rounding error of t, and the bound on
    every partial sum of it."""
    Hkv = bnd.shape[1]
    qs = np.abs(pooled_query(q, blk, mask_heads, Hkv, q_rows))
    per = np.abs(np.repeat(bnd, qs.shape[1] // Hkv, axis=1)).max(axis=3)
    return (qs[:, :, :, None, :] * per[:, :, None, :, :]).sum(-1)


def select(q, k, top_k, *, blk=128, lens=None, causal=False, keep_first=0, keep_local=0, mask_heads="kv", top_p=None,
           score_scale=None, naive=False):
    """-> dict(mask bool [B, Hl, NQ, NK], t fp64 with -inf at invisible blocks, vis, frc bool [B, NQ, NK]; with top_p also u and
    mass): select_ref.select / select_p_ref.select with the bound scores in place of the mean ones."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    lens = [Sk] * B if lens is None else list(lens)
    t = scores(q, bounds(k, lens, blk), blk, mask_heads)
    vis = select_ref.visible(Sq, Sk, lens, blk, causal)
    frc = select_ref.forced(Sq, Sk, lens, blk, causal, keep_first, keep_local)
    out = dict(t=np.where(vis[:, None], t, -np.inf), vis=vis, frc=frc)
    if top_p is None:
        out["mask"] = (select_ref.kept_naive if naive else select_ref.kept_vectorised)(t, vis, frc, top_k)
        return out
    Hl = Hkv if mask_heads == "kv" else H
    c = select_p_ref.c_of(select_p_ref.default_scale(H, Hl, D) if score_scale is None else score_scale)
    u = select_p_ref.weights(t, vis, frc, c)
    kept = select_p_ref.kept_naive if naive else select_p_ref.kept_vectorised
    out["mask"] = kept(t, vis, frc, min(top_k, t.shape[-1]), u, select_p_ref.p16_of(top_p))
    out.update(u=u, mass=select_p_ref.mass_of(out["mask"], u))
    return out


# ---- the needle: one aligned key among keys that point the other way ----------------------------------------------------------------
def needle_inputs(B, H, Hkv, D, blk, NK, needle, seed):
    """q [B, H, 1, D] with entries +-2 (every query head of a K/V head the same row), k [B, Hkv, NK * blk, D], all integers:
    block needle[b] holds one key equal to +q and blk - 1 keys equal to -q / 2 -- its mean score is (4 - 2 (blk - 1)) D g / blk
    < 0, its bound 4 D g; every other block is constant, q / 2 or 0 (block 0: q / 2) -- mean score = bound = 2 D g or 0."""
    rng = np.random.default_rng(seed)
    row = rng.choice([-2.0, 2.0], (B, Hkv, D))
    q = np.repeat(row, H // Hkv, axis=1)[:, :, None, :]
    on = rng.integers(0, 2, (B, Hkv, NK)).astype(np.float64)
    on[:, :, 0] = 1.0
    k = np.repeat(on[..., None] * (row / 2)[:, :, None, :], blk, axis=2)
    for b in range(B):
        j = needle[b]
        k[b, :, j * blk:(j + 1) * blk] = -row[b, :, None, :] / 2
        k[b, :, j * blk + (7 * b + 3) % blk] = row[b]
    return q, k
