"""The reference of select_blocks_antidiag in numpy fp64: the strided anti-diagonal logits as a reshape, a
flip and an einsum, the masked softmax over the visible key groups, the block masses and t = ln(max(P, 2^-126)); the decision is
select_ref's / select_p_ref's on this t.  naive_mass is steps 1-4 as four loops, which tests/test_select_antidiag_cpu.py holds
against the vectorised form.  The input maker, planted: whole key blocks aligned with a row block, or (one_key) one needle a block.

    q [B, H, Sq, D], k [B, Hkv, Sk, D] float64; lens: B key limits; s: the stride; blk: 64 or 128
"""
import numpy as np

import select_p_ref as pref
import select_ref as ref

TINY = 2.0 ** -126


def _groups(x, n, s):
    """[B, heads, S, D] -> [B, heads, ceil(S / s), s, D]: rows >= n are zeros (whatever they held)."""
    B, Hh, S, D = x.shape
    N = -(-S // s)
    out = np.zeros((B, Hh, N * s, D))
    out[:, :, :min(n, S)] = x[:, :, :min(n, S)]
    return out.reshape(B, Hh, N, s, D)


def group_visible(Sq, Sk, ln, s, causal):
    """bool [NU, NW]: key group w is visible to the live row group u."""
    u, w = np.arange(-(-Sq // s))[:, None], np.arange(-(-Sk // s))[None, :]
    vis = np.broadcast_to(w * s < ln, (u.shape[0], w.shape[1])).copy()
    if causal:
        vis &= w * s <= u * s + s - 1 + (ln - Sq)
    return vis


def mass(q, k, lens, s, blk, causal, sm_scale=None, mask_heads="kv"):
    """P [B, Hl, NQ, NK]: steps 1-4 of the contract."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g, G = H // Hkv, blk // s
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    scale = (D ** -0.5 if sm_scale is None else sm_scale) / s
    P = np.zeros((B, H, NQ, NK))
    for b in range(B):
        kz = np.where(np.arange(Sk)[None, :, None] < lens[b], k[b:b + 1], 0.0)      # (NaN beyond the limit never reaches a product)
        qg, kg = _groups(q[b:b + 1], Sq, s)[0], np.repeat(_groups(kz, lens[b], s)[0], g, axis=0)
        x = np.einsum("hutd,hwtd->huw", qg[:, :, ::-1], kg) * scale
        vis = group_visible(Sq, Sk, lens[b], s, causal)
        x = np.where(vis[None], x, -np.inf)
        mx = np.where(vis.any(-1), x.max(-1, initial=-np.inf), 0.0)[..., None]
        e = np.exp(x - mx)
        tot = e.sum(-1, keepdims=True)
        p = np.divide(e, tot, out=np.zeros_like(e), where=tot > 0)
        pad = np.zeros((H, NQ * G, NK * G))
        pad[:, :p.shape[1], :p.shape[2]] = p
        P[b] = pad.reshape(H, NQ, G, NK, G).sum(axis=(2, 4))
    return P if mask_heads == "q" else P.reshape(B, Hkv, g, NQ, NK).sum(axis=2)


def naive_mass(q, k, lens, s, blk, causal, sm_scale=None, mask_heads="kv"):
    """The same by loops over (head, row group, key group, t)."""
    B, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = H // Hkv
    scale = (D ** -0.5 if sm_scale is None else sm_scale) / s
    P = np.zeros((B, H if mask_heads == "q" else Hkv, -(-Sq // blk), -(-Sk // blk)))
    for b in range(B):
        off = lens[b] - Sq
        for h in range(H):
            for u in range(-(-Sq // s)):
                ws = [w for w in range(-(-Sk // s)) if w * s < lens[b] and (not causal or w * s <= u * s + s - 1 + off)]
                x = []
                for w in ws:
                    a = 0.0
                    for t in range(s):
                        r, c = u * s + s - 1 - t, w * s + t
                        if r < Sq and c < lens[b]:
                            a += float(q[b, h, r] @ k[b, h // g, c])
                    x.append(a * scale)
                if ws:
                    e = np.exp(np.array(x) - max(x))
                    for w, pw in zip(ws, e / e.sum()):
                        P[b, h if mask_heads == "q" else h // g, u * s // blk, w * s // blk] += pw
    return P


def select(q, k, top_k, s, *, blk=128, lens=None, causal=False, keep_first=0, keep_local=0, mask_heads="kv", sm_scale=None,
           top_p=None, score_scale=1.0, t=None):
    """-> dict(mask, t fp64 with -inf at invisible blocks, vis, frc[, u, mass]).  t: scores to decide on instead (the kernel's own)."""
    B, _, Sq, _ = q.shape
    Sk = k.shape[2]
    lens = [Sk] * B if lens is None else list(lens)
    if t is None:
        t = np.log(np.maximum(mass(q, k, lens, s, blk, causal, sm_scale, mask_heads), TINY))
    vis, frc = ref.visible(Sq, Sk, lens, blk, causal), ref.forced(Sq, Sk, lens, blk, causal, keep_first, keep_local)
    out = dict(t=np.where(vis[:, None], t, -np.inf), vis=vis, frc=frc)
    top_k = min(top_k, t.shape[-1])
    if top_p is None:
        return dict(out, mask=ref.kept_vectorised(np.where(vis[:, None], t, 0.0), vis, frc, top_k))
    u = pref.weights(t, vis, frc, pref.c_of(score_scale))
    mask = pref.kept_vectorised(np.where(vis[:, None], t, 0.0), vis, frc, top_k, u, pref.p16_of(top_p))
    return dict(out, mask=mask, u=u, mass=pref.mass_of(mask, u))


def cut_gap(t, vis, frc, top_k):
    """The smallest gap, over the rows with a cut, between the last kept and the first dropped unforced score."""
    cand = np.broadcast_to((vis & ~frc)[:, None], t.shape)
    need = np.maximum(top_k - frc.sum(-1), 0)[:, None, :, None]
    srt = -np.sort(-np.where(cand, t, -np.inf), axis=-1)
    n = np.broadcast_to(need, t.shape[:3] + (1,))
    has = (n[..., 0] > 0) & (n[..., 0] < cand.sum(-1))
    last = np.take_along_axis(srt, np.maximum(n - 1, 0), -1)[..., 0]
    first = np.take_along_axis(srt, np.minimum(n, t.shape[-1] - 1), -1)[..., 0]
    return np.where(has, last - first, np.inf).min()


def planted(seed, B, H, Hkv, Sq, Sk, D, blk, per_row, causal, one_key=False, amp=8.0):
    """q, k (values on a 1/8 grid: exact in bf16 and fp16) and the planted blocks, bool [B, Hkv, NQ, NK].  Every query row of block
    i of the heads of K/V head hk is d(b, hk, i) plus noise, |d| = amp; up to per_row key blocks that the row block sees and no
    other row block took hold keys d -- all their keys, or with one_key a single key 8 d at a random phase -- among noise."""
    rng = np.random.default_rng(seed)
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    grid = lambda x: np.round(x * 8) / 8
    q, k = grid(rng.standard_normal((B, H, Sq, D)) * 0.25), grid(rng.standard_normal((B, Hkv, Sk, D)) * 0.25)
    where = np.zeros((B, Hkv, NQ, NK), bool)
    vis = ref.visible(Sq, Sk, [Sk] * B, blk, causal)
    g = H // Hkv
    for b in range(B):
        for hk in range(Hkv):
            for i in range(NQ):
                d = grid(np.sign(rng.standard_normal(D)) * amp / np.sqrt(D))
                q[b, hk * g:(hk + 1) * g, i * blk:min((i + 1) * blk, Sq)] += d
                whole = (np.arange(NK) + 1) * blk <= (i * blk + Sk - Sq + 1 if causal else Sk)      # every row sees every key of it
                free = np.flatnonzero(vis[b, i] & whole & ~where[b, hk].any(0))
                for j in rng.choice(free, size=min(per_row, len(free)), replace=False):
                    where[b, hk, i, j] = True
                    lo, n = j * blk, min(blk, Sk - j * blk)
                    keys = [lo + rng.integers(n)] if one_key else range(lo, lo + n)
                    k[b, hk, keys] = d * (8.0 if one_key else 1.0)
    return q, k, where
