"""The reference of the top-p selection in numpy: select_ref's pooling, scores, visible and forced sets,
and on top of them the integer weights, the target, the kept prefix with the cap, and the kept mass -- vectorised, and as a naive
sort-and-accumulate loop over the rows, which tests/test_select_p_cpu.py holds against one another.

    u_j     = floor(exp2((t_j - t_max) * c) * 2^18 + 0.5) in fp32 steps, c = float32(score_scale * log2(e))
    target  = (total * P16 + 65535) >> 16, P16 = round(top_p * 65536), total = the sum of u over the visible blocks
    kept    = forced + the first min(n_p, n_k) unforced visible blocks by (t descending, j ascending)

MUTANTS are flags of both forms: the ways a correct-looking kernel goes wrong exactly where the exact-class cases look.
"""
import math

import numpy as np

import select_ref as ref

ONE = 1 << 18
LOG2_E = 1.4426950408889634
MUTANTS = ("target off by one unit", "> for >= at an exact landing", "ties to the higher j", "forced mass left out",
           "t_max over the unforced blocks", "cap ignored")


def default_scale(H, Hl, D):
    return 1.0 / ((H // Hl) * math.sqrt(D))


def c_of(score_scale):
    return np.float32(score_scale * LOG2_E)


def p16_of(top_p):
    return int(round(top_p * 65536.0))


def weights(t, vis, frc, c, mut=""):
    """t [B, Hl, NQ, NK] (fp32 values; anything at invisible blocks), vis / frc [B, NQ, NK] -> u int64 [B, Hl, NQ, NK], 0 at
    invisible blocks.  exp2 is taken in fp64 and rounded to fp32 (exact at integers); every other step is fp32."""
    vis, frc = (np.broadcast_to(a[:, None], t.shape) for a in (vis, frc))
    t32 = np.where(vis, t, 0.0).astype(np.float32)
    over = vis & ~frc if mut == "t_max over the unforced blocks" else vis
    tmax = np.where(over, t32, -np.inf).max(-1, keepdims=True).astype(np.float32)
    tmax = np.where(np.isfinite(tmax), tmax, np.float32(0))       # (a row that sees nothing: no weight is used)
    a = (t32 - tmax) * np.float32(c)
    assert a.dtype == np.float32
    e = np.exp2(a.astype(np.float64)).astype(np.float32)
    x = e * np.float32(ONE) + np.float32(0.5)
    assert x.dtype == np.float32
    u = np.where(x >= 1, np.minimum(np.floor(x), ONE), 0).astype(np.int64)
    return np.where(vis, u, 0)


def _target(total, p16, mut):
    return ((total * p16 + 65535) >> 16) + (1 if mut == "target off by one unit" else 0)


def kept_vectorised(t, vis, frc, top_k, u, p16, mut=""):
    """-> kept bool [B, Hl, NQ, NK]."""
    vis, frc = (np.broadcast_to(a[:, None], t.shape) for a in (vis, frc))
    cand = vis & ~frc
    total = u.sum(-1)
    fmass = np.zeros_like(total) if mut == "forced mass left out" else np.where(frc, u, 0).sum(-1)
    target = _target(total, p16, mut)
    j = np.broadcast_to(np.arange(t.shape[-1]), t.shape)
    tie = -j if mut == "ties to the higher j" else j
    order = np.lexsort((tie, -np.where(cand, t, 0.0), ~cand), axis=-1)     # candidates first, t descending, then j ascending
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, j, axis=-1)
    cum = fmass[..., None] + np.cumsum(np.take_along_axis(np.where(cand, u, 0), order, axis=-1), axis=-1)
    before = np.concatenate([fmass[..., None], cum[..., :-1]], axis=-1)     # the sum in front of each position of the order
    short = before <= target[..., None] if mut.startswith(">") else before < target[..., None]
    n_p = short.sum(-1)                                                      # positions still needed: a prefix of the order
    n_k = np.maximum(top_k - frc.sum(-1), 0)
    n = n_p if mut == "cap ignored" else np.minimum(n_p, n_k)
    return frc | (cand & (rank < n[..., None]))


def kept_naive(t, vis, frc, top_k, u, p16, mut=""):
    """The same, row by row: sort, accumulate, stop."""
    B, Hl, NQ, NK = t.shape
    out = np.zeros(t.shape, bool)
    for b in range(B):
        for h in range(Hl):
            for i in range(NQ):
                forced = [jj for jj in range(NK) if frc[b, i, jj]]
                cand = [jj for jj in range(NK) if vis[b, i, jj] and not frc[b, i, jj]]
                cand.sort(key=lambda jj: (-t[b, h, i, jj], -jj if mut == "ties to the higher j" else jj))
                total = sum(int(u[b, h, i, jj]) for jj in range(NK) if vis[b, i, jj])
                target = _target(total, p16, mut)
                acc = 0 if mut == "forced mass left out" else sum(int(u[b, h, i, jj]) for jj in forced)
                cap = max(top_k - len(forced), 0)
                kept = list(forced)
                for n, jj in enumerate(cand):
                    if (acc > target if mut.startswith(">") else acc >= target) or (n >= cap and mut != "cap ignored"):
                        break
                    kept.append(jj)
                    acc += int(u[b, h, i, jj])
                out[b, h, i, kept] = True
    return out


def mass_of(kept, u):
    """fp32 [B, Hl, NQ]: float32(sum of the kept u) / float32(total), 0 where total is 0."""
    total = u.sum(-1)
    got = np.where(kept, u, 0).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = got.astype(np.float32) / total.astype(np.float32)
    return np.where(total > 0, m, np.float32(0)).astype(np.float32)


def select(q, k, top_k, top_p, *, score_scale=None, blk=128, lens=None, causal=False, keep_first=0, keep_local=0, mask_heads="kv",
           naive=False, mut="", t=None):
    """-> dict(mask, t (fp64, -inf at invisible blocks), vis, frc, u, mass).  t: the scores of ref.scores for these inputs, if the
    caller has them already."""
    B, H, Sq, D = q.shape
    Sk, Hkv = k.shape[2], k.shape[1]
    lens = [Sk] * B if lens is None else list(lens)
    t = ref.scores(q, k, lens, blk, mask_heads) if t is None else t
    vis = ref.visible(Sq, Sk, lens, blk, causal)
    frc = ref.forced(Sq, Sk, lens, blk, causal, keep_first, keep_local)
    Hl = Hkv if mask_heads == "kv" else H
    c = c_of(default_scale(H, Hl, D) if score_scale is None else score_scale)
    u = weights(t, vis, frc, c, mut)
    mask = (kept_naive if naive else kept_vectorised)(t, vis, frc, min(top_k, t.shape[-1]), u, p16_of(top_p), mut)
    return dict(mask=mask, t=np.where(vis[:, None], t, -np.inf), vis=vis, frc=frc, u=u, mass=mass_of(mask, u))


# ---- the exact class: inputs whose pooled scores are small integers ------------------------------------------------------------------
def _mix(*xs):
    h = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for x in xs:
            h = (h ^ np.asarray(x).astype(np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            h = h ^ (h >> np.uint64(31))
        h = h * np.uint64(0x94D049BB133111EB)
        return h ^ (h >> np.uint64(29))


PROFILES = ("landing", "plateau", "zero tail")


def levels(profile, NK, seed):
    """NK integers in [-20, 0], placed in a hashed order of j.
    landing    1, 1, 1/2 x 4, then weights that round to 0: at top_p = 0.5 the sum lands on the target after two blocks
    plateau    1, 1/2, 1/4, then 6 .. 40 blocks at 1/8, then 2^-8 .. 2^-12: a cut at 0.9 falls inside the plateau
    zero tail  2^0 .. 2^-19 (u = 2^18 .. 1, the last from 0.5 + 0.5), then 2^-19 and 2^-20 (u = 0) in turn"""
    n = np.arange(NK)
    if profile == "landing":
        lv = np.where(n < 2, 0, np.where(n < 6, -1, -20))
    elif profile == "plateau":
        m = 6 + int(_mix(NK, seed, 1) % np.uint64(35))
        lv = np.where(n < 3, -n, np.where(n < 3 + m, -3, -8 - n % 5))
    else:
        lv = np.where(n < 20, -n, -19 - n % 2)
    out = np.empty(NK, np.int64)
    out[np.argsort(_mix(n, NK, seed, 2), kind="stable")] = lv
    return out


def exact_inputs(B, H, Hkv, Sq, Sk, D, blk, mask_heads, seed, shift=0):
    """q, k float64 (values exact in bf16 and fp16) with t[b, hl, i, j] = (1 + i % 2) * level[b, hk, j]: every q row is
    (1 + i % 2) / g_l along channel 0, g_l = H // Hl the query heads a list head sums; key block j of (b, hk) is constant, its
    level along channel 0.  Profile (b * Hkv + hk + shift) % 3."""
    NK = -(-Sk // blk)
    Hl = Hkv if mask_heads == "kv" else H
    q = np.zeros((B, H, Sq, D))
    q[..., 0] = ((1 + (np.arange(Sq) // blk) % 2) / (H // Hl))[None, None, :]
    k = np.zeros((B, Hkv, Sk, D))
    for b in range(B):
        for hk in range(Hkv):
            lv = levels(PROFILES[(b * Hkv + hk + shift) % 3], NK, seed + 7 * (b * Hkv + hk))
            k[b, hk, :, 0] = np.repeat(lv, blk)[:Sk]
    return q, k


# (top_p, top_k, keep_first, keep_local): exact landings at 0.5, plateaus across the cut at 0.9, a cap that binds (8, 3) and one that
# does not, forced blocks that alone pass a small target, the zero tail at top_p = 1, and top_p = 0
EXACT_PARAMS = [(0.5, "NK", 0, 0), (0.9, "NK", 0, 0), (0.9, 8, 1, 1), (1.0, "NK+5", 0, 1), (0.0, 5, 1, 2), (0.02, 6, 2, 1),
                (0.5, 3, 0, 0), (1.0, 12, 0, 0)]
SCALE_EXACT = math.log(2.0)         # c_of(SCALE_EXACT) == 1: every weight is a power of two or 0
_FORMS = [(Hkv, heads, causal) for Hkv in (4, 2, 1) for heads in ("kv", "q") for causal in (False, True)]


def exact_cases():
    """Twelve shapes with B = 2 (a key limit per item) and H = 4: NK in 3, 70, 300; Sq = 1, 3, one block, 2.5 blocks; both block
    sizes, D = 16, 64, 128, both dtypes; the twelve (Hkv, mask_heads, causal) forms, one each."""
    out = []
    for m in range(12):
        blk = (64, 128)[m % 2]
        Hkv, heads, causal = _FORMS[(5 * m + 2) % 12]
        NK = (3, 70, 300)[m % 3]
        Sk = (NK - 1) * blk + blk // 2 + 3
        out.append(dict(dt=("bf16", "fp16")[(m // 3) % 2], D=(16, 64, 128)[(m // 2) % 3], blk=blk, NK=NK,
                        Sq=(1, 3, blk, 2 * blk + blk // 2)[m % 4], Sk=Sk, lens=[Sk, max(Sk - 2 * blk - 17, 5)], B=2, H=4, Hkv=Hkv,
                        heads=heads, causal=causal, seed=100 + m))
    return out


def exact_top_k(tk, NK):
    return {"NK": NK, "NK+5": NK + 5}.get(tk, tk)


# ---- where the two budgets coincide: top_p = 1 over rows without a zero weight ---------------------------------------------------------
def plateau_inputs(B, H, Hkv, Sq, Sk, D, blk, mask_heads, seed):
    """exact_inputs with the plateau profile for every (b, hk) and without the doubled odd query blocks: t[b, hl, i, j] =
    level[b, hk, j] in [-12, 0], so at c == 1 every visible block weighs at least 2^6 and top_p = 1 keeps what top-k keeps."""
    NK = -(-Sk // blk)
    Hl = Hkv if mask_heads == "kv" else H
    q = np.zeros((B, H, Sq, D))
    q[..., 0] = 1.0 / (H // Hl)
    k = np.zeros((B, Hkv, Sk, D))
    for b in range(B):
        for hk in range(Hkv):
            k[b, hk, :, 0] = np.repeat(levels("plateau", NK, seed + 7 * (b * Hkv + hk)), blk)[:Sk]
    return q, k


PLATEAU_BUDGETS = [(1, 0, 0), (5, 0, 0), (8, 1, 1), (12, 2, 2), ("NK+5", 0, 1), (0, 1, 0)]      # (top_k, keep_first, keep_local)


def plateau_cases():
    """The grid of 72 shapes (B = 2, H = 4, D = 16), each for the six PLATEAU_BUDGETS."""
    out = []
    for blk in (64, 128):
        for NK in (3, 70, 300):
            Sk = (NK - 1) * blk + blk // 2 + 3
            for Hkv, heads in ((4, "kv"), (2, "q"), (1, "kv")):
                for causal in (False, True):
                    for Sq in (1, blk):
                        out.append(dict(B=2, H=4, D=16, blk=blk, NK=NK, Sk=Sk, lens=[Sk, max(Sk - 2 * blk - 17, 5)], Hkv=Hkv,
                                        heads=heads, causal=causal, Sq=Sq, seed=300 + NK))
    return out
