"""numpy reference of block_sparse_decode: a plain helper module, no device.

    visible        row r of (b, h) sees key j iff mask[b, hl(h), 0, j // block] and j < kv_len[b] and j < NK * block and, with
                   causal, j <= r + kv_len[b] - Sq (bottom-right aligned)
    scores2        the scores in the log2 domain, fp64: exact (q . k sm_scale log2 e) or on the operands the kernel multiplies,
                   q_hat = round_dt(fp32(q) * qk_scale(sm_scale))
    attention      softmax over the visible keys in fp64 and the natural log-sum-exp; a row without a visible key: 0, -inf
    split_parts    (m, l, O) of every split of the kept list, merge() their combination in ascending split order -- the model of
                   the kernel's split and merge, with the mutations the CPU test applies to it
    paged          make_pool scatters a contiguous cache into pages, gather reads it back through the table
    witness cases  the inputs of the exact tests of tests/test_gpu_decode.py, built here so that the CPU test can walk them"""
from __future__ import annotations

import numpy as np

import visibility as vis
import weights

LN2 = float(np.log(2.0))
LOG2E = float(np.log2(np.e))


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def visible(mask, lens, Sq: int, Sk: int, blk: int, H: int, causal: bool, kv_shift: int = 0, top_left: bool = False):
    """bool [B, H, Sq, Sk].  mask bool [B|1, Hl, 1, NK]; lens B ints.  Mutations: kv_shift moves the key limit, top_left aligns
    the causal diagonal at the first key instead of the last."""
    B = len(lens)
    mask = np.asarray(mask, bool)
    Hl, NK = mask.shape[1], mask.shape[3]
    m = np.broadcast_to(mask, (B, Hl, 1, NK))[:, :, 0]
    hl = np.arange(H) // (H // Hl)
    j = np.arange(Sk)
    r = np.arange(Sq)
    out = np.zeros((B, H, Sq, Sk), bool)
    inside = j < NK * blk
    for b in range(B):
        kept = np.zeros((H, Sk), bool)
        kept[:, inside] = m[b][hl][:, j[inside] // blk]
        lim = j < lens[b] + kv_shift
        row = np.broadcast_to(lim, (Sq, Sk))
        if causal:
            off = 0 if top_left else lens[b] - Sq
            row = row & (j[None, :] <= r[:, None] + off)
        out[b] = kept[:, None, :] & row[None]
    return out


def visible_naive(mask, lens, Sq, Sk, blk, H, causal):
    """The same rule as a loop over every (b, h, r, j)."""
    B = len(lens)
    mask = np.asarray(mask, bool)
    Hl, NK = mask.shape[1], mask.shape[3]
    out = np.zeros((B, H, Sq, Sk), bool)
    for b in range(B):
        mb = mask[b if mask.shape[0] > 1 else 0]
        for h in range(H):
            for r in range(Sq):
                for j in range(Sk):
                    ok = j // blk < NK and mb[h // (H // Hl), 0, min(j // blk, NK - 1)] and j < lens[b]
                    if causal:
                        ok = ok and j <= r + lens[b] - Sq
                    out[b, h, r, j] = ok
    return out


# ---- scores, attention -----------------------------------------------------------------------------------------------------------
def scores2(q, k, sm_scale: float, dt=None):
    """fp64 [B, H, Sq, Sk], log2 domain.  dt None: the exact scores; "bf16" / "fp16": on the operands the kernel multiplies."""
    q = np.asarray(q, np.float32)
    k = np.nan_to_num(np.asarray(k, np.float64), nan=0.0, posinf=0.0, neginf=0.0)     # (unwritten keys: never visible)
    H, Hkv = q.shape[1], k.shape[1]
    if dt is None:
        qs = q.astype(np.float64) * (float(sm_scale) * LOG2E)
    else:
        qs = weights.round_dt(q * weights.qk_scale(sm_scale), dt).astype(np.float64)
    kk = k[:, np.arange(H) // (H // Hkv)]
    return np.einsum("bhrd,bhjd->bhrj", qs, kk)


def parts(s2, seen, v):
    """(m [B,H,Sq], l [B,H,Sq], O [B,H,Sq,D]) over the keys `seen` (bool [B,H,Sq,Sk]): m = max score (-inf: none), l = sum
    2^(s - m), O = sum 2^(s - m) v, fp64."""
    H, Hkv = s2.shape[1], v.shape[1]
    vv = np.nan_to_num(np.asarray(v, np.float64), nan=0.0, posinf=0.0, neginf=0.0)[:, np.arange(H) // (H // Hkv)]
    s = np.where(seen, s2, -np.inf)
    m = s.max(-1)
    mref = np.where(np.isfinite(m), m, 0.0)
    p = np.where(seen, np.exp2(s - mref[..., None]), 0.0)
    return m, p.sum(-1), np.einsum("bhrj,bhjd->bhrd", p, vv)


def finish(m, l, o):
    """(out, natural log-sum-exp); a row without a visible key: 0 and -inf."""
    has = l > 0
    out = np.where(has[..., None], o / np.where(has, l, 1.0)[..., None], 0.0)
    with np.errstate(divide="ignore"):
        lse = np.where(has, (np.where(has, m, 0.0) + np.log2(np.where(has, l, 1.0))) * LN2, -np.inf)
    return out, lse


def attention(s2, seen, v):
    return finish(*parts(s2, seen, v))


# ---- splits and their merge ------------------------------------------------------------------------------------------------------
def split_keys(mask, B: int, H: int, Sk: int, blk: int, C: int):
    """bool [S, B, H, Sk]: the keys of split s = entries [s C, (s + 1) C) of the ascending kept list of (b, list head of h);
    S = ceil(NK / C) (splits past the list's end are empty)."""
    mask = np.asarray(mask, bool)
    Hl, NK = mask.shape[1], mask.shape[3]
    S = -(-NK // C)
    out = np.zeros((S, B, H, Sk), bool)
    for b in range(B):
        for h in range(H):
            cols = np.flatnonzero(mask[b if mask.shape[0] > 1 else 0, h // (H // Hl), 0])
            for e, jb in enumerate(cols):
                out[e // C, b, h, jb * blk:min((jb + 1) * blk, Sk)] = True
    return out


def split_parts(s2, seen, v, mask, blk: int, C: int):
    B, H, _, Sk = s2.shape
    return [parts(s2, seen & sk[:, :, None, :], v) for sk in split_keys(mask, B, H, Sk, blk, C)]


def merge(pieces, drop=None, bump=None):
    """The merge kernel: m* = max m_s, O = sum 2^(m_s - m*) O_s, l = sum 2^(m_s - m*) l_s in ascending s.  Mutations: drop = a
    split whose partial is left out; bump = a split whose factor is one step (a factor of two) too large."""
    ms = np.stack([p[0] for p in pieces])
    mstar = ms.max(0)
    mref = np.where(np.isfinite(mstar), mstar, 0.0)
    l = np.zeros_like(mstar)
    o = np.zeros_like(pieces[0][2])
    for s, (m, ls, os_) in enumerate(pieces):
        if s == drop:
            continue
        f = np.where(ls > 0, np.exp2(np.where(np.isfinite(m), m, 0.0) - mref), 0.0) * (2.0 if s == bump else 1.0)
        l = l + f * ls
        o = o + f[..., None] * os_
    return mstar, l, o


# ---- paged cache -----------------------------------------------------------------------------------------------------------------
def make_pool(cache, blk: int, P: int, perm, fill=np.nan):
    """cache [B, Hkv, Sk, D] -> (pool [P, Hkv, blk, D], table int32 [B, NK]): block j of batch item b goes to page
    perm[b * NK + j]; a ragged last block and the spare pages are filled with `fill`."""
    B, Hkv, Sk, D = cache.shape
    NK = -(-Sk // blk)
    pool = np.full((P, Hkv, blk, D), fill, cache.dtype)
    table = np.zeros((B, NK), np.int32)
    for b in range(B):
        for j in range(NK):
            pg = int(perm[b * NK + j])
            rows = cache[b, :, j * blk:(j + 1) * blk]
            pool[pg, :, :rows.shape[1]] = rows
            table[b, j] = pg
    return pool, table


def gather(pool, table):
    """The cache the table describes: [B, Hkv, NKt * blk, D]; entries outside [0, P) read as NaN pages."""
    P, Hkv, blk, D = pool.shape
    B, NKt = table.shape
    out = np.full((B, Hkv, NKt * blk, D), np.nan, pool.dtype)
    for b in range(B):
        for j in range(NKt):
            if 0 <= table[b, j] < P:
                out[b, :, j * blk:(j + 1) * blk] = pool[table[b, j]]
    return out


# ---- witness cases ---------------------------------------------------------------------------------------------------------------
SK = 700
GROUPS = ((8, 1), (8, 2), (8, 8), (6, 2))


def witness_mask(B, Hl, NK, lens, blk):
    """bool [B, Hl, 1, NK]: everything kept but one block per list head that lies between two kept ones and below the limit."""
    m = np.ones((B, Hl, 1, NK), bool)
    for b in range(B):
        last = max((lens[b] - 1) // blk, 0)
        for hl in range(Hl):
            if last >= 2:
                m[b, hl, 0, 1 + hl % (last - 1)] = False
    return m


def _cases(kind):
    out = []
    for gi, (H, Hkv) in enumerate(GROUPS):
        for i in range(4):
            dt = ("bf16", "fp16")[(i + gi) % 2]
            D = (64, 128)[(i // 2 + gi) % 2]
            blk = (128, 64)[i % 2]
            Sq = (3, 1, 8, 3)[(i + gi) % 4]
            axis = ("H", "Hkv", "1")[(i + gi) % 3]
            NK = -(-SK // blk)
            out.append(dict(kind=kind, id=f"{kind}-H{H}kv{Hkv}-{dt}-D{D}-b{blk}-Sq{Sq}-m{axis}", H=H, Hkv=Hkv, dt=dt, D=D, blk=blk,
                            Sq=Sq, Hl={"H": H, "Hkv": Hkv, "1": 1}[axis], lens=[SK, 333] if i % 2 == 0 else [129, 2],
                            causal=bool((i + gi) % 4 != 1), C=(2, 1, 3, NK)[(i + gi) % 4], seed=100 * gi + i))
    return out


VIS_CASES = _cases("vis")
WEIGHT_CASES = _cases("wts")


def split_starts(mask, blk, C):
    """The first key of every split of every list row."""
    out = set()
    for mb in np.asarray(mask, bool).reshape(-1, mask.shape[-1]):
        out.update(int(jb) * blk for jb in np.flatnonzero(mb)[::C])
    return sorted(out)


def vis_inputs(c):
    """Zero scores, V of 0 / 1 with probe channels around the key limits (which the causal limits of the last rows sit on), the
    edges of each dropped block and as many first keys of splits as still fit D / 2 channels."""
    B, H, Hkv, D, blk, Sq = 2, c["H"], c["Hkv"], c["D"], c["blk"], c["Sq"]
    NK = -(-SK // blk)
    mask = witness_mask(B, c["Hl"], NK, c["lens"], blk)
    q, k = vis.zero_score_qk(c["seed"], B, H, Sq, SK, D)
    probes = []
    for n in c["lens"]:
        probes += vis.around(n)
        if c["causal"]:
            probes += [n - Sq, n - Sq - 1]
    for jb in sorted({int(x) for x in np.argwhere(~mask)[:, 3]})[:2]:
        probes += vis.around(jb * blk) + vis.around((jb + 1) * blk)
    probes = sorted({p for p in probes if 0 <= p < SK})
    for s0 in split_starts(mask, blk, c["C"]):
        extra = [p for p in (s0 - 1, s0) if 0 <= p < SK and p not in probes]
        if len(probes) + len(extra) <= D // 2:
            probes = sorted(probes + extra)
    v = np.broadcast_to(vis.witness_v(SK, D, probes), (B, Hkv, SK, D)).copy()
    return dict(q=q, k=k[:, :Hkv].copy(), v=v, mask=mask, sm_scale=D ** -0.5)


SPREAD = 10


def weight_inputs(c):
    """Integer scores: Q rows one-hot with weights.find_a's amplitude (round(a qk_scale) = 2^-3), K = 8 n.  Class 0 (row 0 of a
    head) has its maximum in the last visible block, class 1 in the first, class 2 steps up by 8 at the first key of the second
    split; the base is 0 .. 2, so a row's spread is at most 10.  V is visibility's 0 / 1 census."""
    B, H, Hkv, D, blk, Sq = 2, c["H"], c["Hkv"], c["D"], c["blk"], c["Sq"]
    NK = -(-SK // blk)
    sm = D ** -0.5
    a = float(weights.find_a(c["dt"], sm)[0][0])
    mask = witness_mask(B, c["Hl"], NK, c["lens"], blk)
    rng = np.random.default_rng(c["seed"])
    n = rng.integers(0, 3, (B, Hkv, SK, 4)).astype(np.int64)
    starts = split_starts(mask, blk, c["C"])
    for b, len_b in enumerate(c["lens"]):
        n[b, :, max(len_b - 2, 0), 0] += 6          # the maximum in the last visible block
        n[b, :, min(3, len_b - 1), 1] += 6          # ... in the first
        edge = [s for s in starts if 0 < s < len_b]
        if edge:
            n[b, :, edge[0]:edge[0] + 2, 2] = 10    # a +8 step at a split edge (over the base's maximum, 2)
    q = np.zeros((B, H, Sq, D), np.float32)
    for h in range(H):
        for r in range(Sq):
            q[:, h, r, (r + h) % 4] = a
    k = np.zeros((B, Hkv, SK, D), np.float32)
    k[..., :4] = 8.0 * n
    v = np.broadcast_to(vis.witness_v(SK, D, []), (B, Hkv, SK, D)).copy()
    return dict(q=q, k=k, v=v, mask=mask, sm_scale=sm, n=n)


def weight_budget(c, inp):
    """max over the rows of sum 2^(n - n_min) over the visible keys, and the largest spread: the sums stay exact in fp32 while
    the first is below 2^24."""
    s2 = scores2(inp["q"], inp["k"], inp["sm_scale"], c["dt"])
    seen = visible(inp["mask"], c["lens"], c["Sq"], SK, c["blk"], c["H"], c["causal"])
    assert np.array_equal(s2, np.rint(s2)), "the scores are integers in the kernel's units"
    lo = np.where(seen, s2, np.inf).min(-1)
    hi = np.where(seen, s2, -np.inf).max(-1)
    has = seen.any(-1)
    tot = np.where(seen, np.exp2(s2 - np.where(has, lo, 0.0)[..., None]), 0.0).sum(-1)
    return float(tot.max()), float(np.where(has, hi - lo, 0.0).max())


def case_inputs(c):
    return vis_inputs(c) if c["kind"] == "vis" else weight_inputs(c)


def case_reference(c, inp, **mut):
    """(out, lse, pieces) of a witness case on the operands the kernel multiplies; mut: visible()'s mutations."""
    s2 = scores2(inp["q"], inp["k"], inp["sm_scale"], c["dt"])
    seen = visible(inp["mask"], c["lens"], c["Sq"], SK, c["blk"], c["H"], c["causal"], **mut)
    out, lse = attention(s2, seen, inp["v"])
    return out, lse, split_parts(s2, seen, inp["v"], inp["mask"], c["blk"], c["C"])


def within(got, ref, dt):
    """visibility's bound: |got - ref| <= ULP |ref| + FLOOR max|ref|, and exactly 0 where the reference is."""
    tol = vis.tolerance(ref, vis.ULP[dt])
    err = np.abs(np.asarray(got, np.float64) - ref)
    return bool((err <= tol).all() and (np.asarray(got)[ref == 0] == 0).all()), float((err / tol).max())
