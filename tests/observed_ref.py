"""The reference of select_blocks_observed's score in numpy fp64, vectorised and as four loops.
q [B, H, W, D], k [B, Hkv, Sk, D]; row r of item b sees key j iff j < lens[b] and, with causal, j <= r + lens[b] - W; p = the softmax
of sm_scale <q, k> over the keys a row sees; P [B, Hl, NK] = its sum over the list head's heads, the live rows and a block's keys."""
import numpy as np


def row_visible(W, Sk, n, causal):
    """bool [W, Sk]."""
    j, r = np.arange(Sk)[None, :], np.arange(W)[:, None]
    return (j < n) & ((j <= r + n - W) if causal else (r >= 0))


def mass(q, k, lens, blk, causal=False, sm_scale=None, mask_heads="kv"):
    B, H, W, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g, NK = H // Hkv, -(-Sk // blk)
    scale = D ** -0.5 if sm_scale is None else sm_scale
    P = np.zeros((B, H, NK))
    for b in range(B):
        vis = row_visible(W, Sk, lens[b], causal)
        kz = np.where((np.arange(Sk) < lens[b])[None, :, None], k[b], 0.0)      # (keys beyond the limit may hold NaN)
        x = np.where(vis[None], scale * np.einsum("hrd,hjd->hrj", q[b], np.repeat(kz, g, axis=0)), -np.inf)
        e = np.exp(x - np.where(vis.any(-1), x.max(-1), 0.0)[..., None])
        p = e / np.where(vis.any(-1), e.sum(-1), 1.0)[..., None]
        P[b] = np.pad(p.sum(1), ((0, 0), (0, NK * blk - Sk))).reshape(H, NK, blk).sum(-1)
    return P if mask_heads == "q" else P.reshape(B, Hkv, g, NK).sum(2)


def naive_mass(q, k, lens, blk, causal=False, sm_scale=None, mask_heads="kv"):
    B, H, W, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g, NK = H // Hkv, -(-Sk // blk)
    scale = D ** -0.5 if sm_scale is None else sm_scale
    Hl = H if mask_heads == "q" else Hkv
    P = np.zeros((B, Hl, NK))
    for b in range(B):
        for h in range(H):
            for r in range(W):
                seen = [j for j in range(Sk) if j < lens[b] and (not causal or j <= r + lens[b] - W)]
                x = [scale * float(np.dot(q[b, h, r], k[b, h // g, j])) for j in seen]
                den = sum(np.exp(y - max(x)) for y in x)
                for j, xj in zip(seen, x):
                    P[b, h * Hl // H, j // blk] += np.exp(xj - max(x)) / den
    return P


def scores(P, Sk, lens, blk):
    """t fp64 [B, Hl, 1, NK]: ln(max(P, 2^-126)), -inf at invisible blocks (block j is visible iff j blk < lens[b])."""
    vis = np.arange(P.shape[-1])[None, :] * blk < np.asarray(lens)[:, None]
    return np.where(vis[:, None], np.log(np.maximum(P, 2.0 ** -126)), -np.inf)[:, :, None]
