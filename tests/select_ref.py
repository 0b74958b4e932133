"""The reference of select_blocks in numpy fp64: a direct transcription of the semantics -- pooling, the
score t, the visible and the forced blocks, the kept blocks with the tie rule -- in a vectorised form and as a deliberately naive
loop over the rows, which tests/test_select_blocks_cpu.py holds against one another.

    q [B, H, Sq, D], k [B, Hkv, Sk, D] float64 arrays; lens: B key limits; blk: 64 or 128; g = H // Hkv
    list heads Hl = Hkv (mask_heads "kv") or H ("q"); list head hl holds the query heads hl * (H // Hl) ... ascending
"""
import numpy as np


def pooled(x, limits, blk):
    """[B, heads, S, D] -> [B, heads, ceil(S / blk), D]: per block the mean of its rows < limits[b] (0 where it has none)."""
    B, Hh, S, D = x.shape
    N = -(-S // blk)
    out = np.zeros((B, Hh, N, D))
    for b in range(B):
        for n in range(N):
            lo, hi = n * blk, min((n + 1) * blk, S, limits[b])
            if hi > lo:
                out[b, :, n] = x[b, :, lo:hi].sum(axis=1) / (hi - lo)
    return out


def scores(q, k, lens, blk, mask_heads="kv"):
    """t [B, Hl, NQ, NK] (every block, visible or not): the group's summed pooled query against the K/V head's pooled keys."""
    B, H, Sq, _ = q.shape
    Hkv = k.shape[1]
    g = H // Hkv
    qbar, kbar = pooled(q, [Sq] * B, blk), pooled(k, lens, blk)
    per_head = np.einsum("bhid,bhjd->bhij", qbar, np.repeat(kbar, g, axis=1))
    if mask_heads == "q":
        return per_head + 0.0
    return per_head.reshape(B, Hkv, g, *per_head.shape[2:]).sum(axis=2) + 0.0      # (+ 0.0: -0 is 0)


def visible(Sq, Sk, lens, blk, causal):
    """bool [B, NQ, NK]."""
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    j = np.arange(NK)[None, None, :]
    r1 = np.minimum((np.arange(NQ) + 1) * blk, Sq)[None, :, None] - 1
    ln = np.asarray(lens, np.int64)[:, None, None]
    vis = np.broadcast_to(j * blk < ln, (len(lens), NQ, NK)).copy()
    if causal:
        vis &= j * blk <= r1 + (ln - Sq)
    return vis


def forced(Sq, Sk, lens, blk, causal, keep_first, keep_local):
    """bool [B, NQ, NK]: within the visible blocks."""
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    j = np.arange(NK)[None, None, :]
    r0 = (np.arange(NQ) * blk)[None, :, None]
    r1 = np.minimum((np.arange(NQ) + 1) * blk, Sq)[None, :, None] - 1
    ln = np.asarray(lens, np.int64)[:, None, None]
    off = ln - Sq
    f = np.broadcast_to(j < keep_first, (len(lens), NQ, NK)).copy()
    if keep_local >= 1:
        jd_lo = np.maximum(r0 + off, 0) // blk
        jd_hi = np.minimum(np.maximum(r1 + off, 0), ln - 1) // blk
        hi = jd_hi if causal else jd_hi + (keep_local - 1)
        f |= (j >= jd_lo - (keep_local - 1)) & (j <= hi)
    return f & visible(Sq, Sk, lens, blk, causal)


def kept_vectorised(t, vis, frc, top_k):
    """t [B, Hl, NQ, NK], vis / frc [B, NQ, NK] -> kept bool [B, Hl, NQ, NK]."""
    vis, frc = (np.broadcast_to(a[:, None], t.shape) for a in (vis, frc))
    cand = vis & ~frc
    need = np.maximum(top_k - frc.sum(-1), 0)
    j = np.broadcast_to(np.arange(t.shape[-1]), t.shape)
    order = np.lexsort((j, -np.where(cand, t, 0.0), ~cand), axis=-1)      # candidates first, t descending, then j ascending
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, j, axis=-1)
    return frc | (cand & (rank < need[..., None]))


def kept_naive(t, vis, frc, top_k):
    """The same, row by row."""
    B, Hl, NQ, NK = t.shape
    out = np.zeros(t.shape, bool)
    for b in range(B):
        for h in range(Hl):
            for i in range(NQ):
                kept = [jj for jj in range(NK) if frc[b, i, jj]]
                cand = [jj for jj in range(NK) if vis[b, i, jj] and not frc[b, i, jj]]
                cand.sort(key=lambda jj: (-t[b, h, i, jj], jj))
                kept += cand[:max(top_k - len(kept), 0)]
                out[b, h, i, kept] = True
    return out


def select(q, k, top_k, *, blk=128, lens=None, causal=False, keep_first=0, keep_local=0, mask_heads="kv", naive=False):
    """-> dict(mask bool [B, Hl, NQ, NK], t fp64 [B, Hl, NQ, NK] with -inf at invisible blocks, vis, frc bool [B, NQ, NK])."""
    B, _, Sq, _ = q.shape
    Sk = k.shape[2]
    lens = [Sk] * B if lens is None else list(lens)
    t = scores(q, k, lens, blk, mask_heads)
    vis = visible(Sq, Sk, lens, blk, causal)
    frc = forced(Sq, Sk, lens, blk, causal, keep_first, keep_local)
    mask = (kept_naive if naive else kept_vectorised)(t, vis, frc, top_k)
    return dict(mask=mask, t=np.where(vis[:, None], t, -np.inf), vis=vis, frc=frc)


def magnitude(q, k, lens, blk, mask_heads="kv"):
    """M [B, Hl, NQ, NK] = sum over the group's heads and the channels of mean|q_d| * mean|k_d|: the scale of the fp32 rounding
    error of t."""
    return scores(np.abs(q), np.abs(k), lens, blk, mask_heads)
