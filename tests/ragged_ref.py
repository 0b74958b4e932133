"""numpy reference of the ragged calls: block_sparse_extend(q_len=) and select_blocks(_pooled)(q_len=).  A
plain helper module, no device.  The contract is "item b of the padded batch is the existing call on its first n_b rows", so the
references are the existing ones (extend_ref, select_ref, select_p_ref) applied per item to the truncated operands and embedded
into the padded shape; beside them stands a direct form of each rule with the mutations the CPU test applies.

    visible            extend_ref.visible of (q[b, :, :n_b], mask[b, :, :ceil(n_b / block)], kv_len[b]) per item; rows >= n_b see nothing
    visible_direct     the same rule written out with n_b in it, and its mutants
    visible_naive      ... as a loop over every (b, h, r, j)
    select             select_ref.select / select_p_ref.select per item on the truncated q; query blocks without a row are empty
    select_direct      the selection rule with n_b in it (pooling divisor, r1, off_b), and its mutants"""
from __future__ import annotations

import numpy as np

import decode_ref as dref
import extend_ref as eref
import select_p_ref as pref
import select_ref as sref

B, SQ, SK = 4, 300, dref.SK
QLENS = ((300, 129, 1, 0), (64, 65, 128, 128))
RAW_QLEN = (128, 129, SQ + 7, -3)        # a device tensor's values before the clamp: (128, 129, 300, 0)


def clamp(q_len, Sq: int):
    return [min(max(int(n), 0), Sq) for n in q_len]


def live_blocks(n: int, blk: int) -> int:
    return -(-n // blk)


# ---- the extend rule -------------------------------------------------------------------------------------------------------------
def visible(mask, lens, q_lens, Sq: int, Sk: int, blk: int, H: int, causal: bool):
    """bool [B, H, Sq, Sk]: per item the existing rule on the truncated call, embedded; rows >= n_b see nothing."""
    mask = np.asarray(mask, bool)
    nb = len(lens)
    m = np.broadcast_to(mask, (nb,) + mask.shape[1:])
    out = np.zeros((nb, H, Sq, Sk), bool)
    for b, n in enumerate(clamp(q_lens, Sq)):
        if n:
            out[b, :, :n] = eref.visible(m[b:b + 1, :, :live_blocks(n, blk)], [lens[b]], n, Sk, blk, H, causal)[0]
    return out


MUTANTS = ("causal offset from Sq", "n of the next item", "row limit + 1", "row limit - 1", "mask row beyond the live blocks")


def visible_direct(mask, lens, q_lens, Sq: int, Sk: int, blk: int, H: int, causal: bool, mut: str = ""):
    """The rule with n_b written in: row r < n_b sees key j iff mask[b, hl(h), r // block, j // block], j < kv_len[b],
    j < NK * block and, with causal, j <= r + kv_len[b] - n_b.  mut: one of MUTANTS."""
    assert mut in ("",) + MUTANTS
    mask = np.asarray(mask, bool)
    nb = len(lens)
    Hl, NQ, NK = mask.shape[1:]
    m = np.broadcast_to(mask, (nb, Hl, NQ, NK))
    hl = np.arange(H) // (H // Hl)
    j, r = np.arange(Sk), np.arange(Sq)
    inside = j < NK * blk
    ns = clamp(q_lens, Sq)
    out = np.zeros((nb, H, Sq, Sk), bool)
    for b in range(nb):
        n = ns[(b + 1) % nb] if mut == "n of the next item" else ns[b]
        live = n + {"row limit + 1": 1, "row limit - 1": -1}.get(mut, 0)
        qb = r // blk
        if mut == "mask row beyond the live blocks":     # the rows of the last live block read the list row behind it
            qb = np.where(qb == live_blocks(n, blk) - 1, np.minimum(qb + 1, NQ - 1), qb)
        kept = np.zeros((H, Sq, Sk), bool)
        kept[:, :, inside] = m[b][hl][:, qb][:, :, j[inside] // blk]
        row = np.broadcast_to(j < lens[b], (Sq, Sk))
        if causal:
            last = r + lens[b] - (Sq if mut == "causal offset from Sq" else n)
            row = row & (j[None, :] <= last[:, None])
        out[b] = kept & row[None] & (r < min(max(live, 0), Sq))[None, :, None]
    return out


def visible_naive(mask, lens, q_lens, Sq, Sk, blk, H, causal):
    mask = np.asarray(mask, bool)
    Hl, NQ, NK = mask.shape[1:]
    ns = clamp(q_lens, Sq)
    out = np.zeros((len(lens), H, Sq, Sk), bool)
    for b in range(len(lens)):
        mb = mask[b if mask.shape[0] > 1 else 0]
        for h in range(H):
            for r in range(ns[b]):
                row = mb[h // (H // Hl), r // blk]
                for j in range(min(lens[b], NK * blk, Sk)):
                    if causal and j > r + lens[b] - ns[b]:
                        break
                    out[b, h, r, j] = row[j // blk]
    return out


def attention(q, k, v, seen, sm_scale, dt=None):
    """(out, lse) fp64 over `seen`; q's rows may hold NaN where no key is seen (they are zeroed here: never multiplied there)."""
    qz = np.where(seen.any(-1)[..., None], np.asarray(q, np.float32), np.float32(0))
    return eref.attention(eref.scores2(qz, k, sm_scale, dt), seen, v)


# ---- the selection ---------------------------------------------------------------------------------------------------------------
def select(q, k, top_k, q_lens, *, top_p=None, blk=128, lens=None, causal=False, keep_first=0, keep_local=0, mask_heads="kv"):
    """dict(mask bool [B, Hl, NQ, NK], t fp64 (-inf at invisible blocks and at blocks without a row), mass fp32 [B, Hl, NQ] | None):
    the existing references on q[b:b+1, :, :n_b], embedded; a query block without a row keeps nothing."""
    nb, H, Sq, _ = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    Hl = Hkv if mask_heads == "kv" else H
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    lens = [Sk] * nb if lens is None else list(lens)
    mask = np.zeros((nb, Hl, NQ, NK), bool)
    t = np.full((nb, Hl, NQ, NK), -np.inf)
    mass = None if top_p is None else np.zeros((nb, Hl, NQ), np.float32)
    kw = dict(blk=blk, causal=causal, keep_first=keep_first, keep_local=keep_local, mask_heads=mask_heads)
    for b, n in enumerate(clamp(q_lens, Sq)):
        if not n:
            continue
        qb, kb, nq = q[b:b + 1, :, :n], k[b:b + 1], live_blocks(n, blk)
        if top_p is None:
            r = sref.select(qb, kb, top_k, lens=[lens[b]], **kw)
        else:
            r = pref.select(qb, kb, top_k, top_p, lens=[lens[b]], **kw)
            mass[b, :, :nq] = r["mass"][0]
        mask[b, :, :nq], t[b, :, :nq] = r["mask"][0], r["t"][0]
    return dict(mask=mask, t=t, mass=mass)


SELECT_MUTANTS = ("mean over the full block", "r1 from Sq", "off from Sq")


def select_direct(q, k, top_k, q_lens, *, top_p=None, blk=128, lens=None, causal=False, keep_first=0, keep_local=0,
                  mask_heads="kv", mut=""):
    """The selection contract with n_b written in -- qbar the mean over the rows < n_b, r1 = min((i + 1) block, n_b) - 1,
    off_b = len_b - n_b, nothing visible in a block without a row (r1 < r0) -- and its mutants.  In the last live block
    r1 + off_b = len_b - 1 whatever n_b is, and the visible and forced sets are capped there by kv_len anyway: what "r1 from Sq"
    changes is which query blocks count as having rows (the padding blocks then keep lists)."""
    assert mut in ("",) + SELECT_MUTANTS
    nb, H, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    g = H // Hkv
    Hl = Hkv if mask_heads == "kv" else H
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    lens = [Sk] * nb if lens is None else list(lens)
    ns = clamp(q_lens, Sq)
    qz = np.array(q, np.float64)
    for b, n in enumerate(ns):
        qz[b, :, n:] = 0.0          # (rows at or beyond n_b are never read)
    qbar = sref.pooled(qz, ns, blk)
    if mut == "mean over the full block":
        for b, n in enumerate(ns):
            for i in range(NQ):
                rows, full = min((i + 1) * blk, n) - i * blk, min((i + 1) * blk, Sq) - i * blk
                if rows > 0:
                    qbar[b, :, i] *= rows / full
    kbar = sref.pooled(np.nan_to_num(np.asarray(k, np.float64)), lens, blk)
    t = np.einsum("bhid,bhjd->bhij", qbar, np.repeat(kbar, g, axis=1))
    t = (t if mask_heads == "q" else t.reshape(nb, Hkv, g, NQ, NK).sum(2)) + 0.0
    i, j = np.arange(NQ)[None, :, None], np.arange(NK)[None, None, :]
    n_, ln = np.asarray(ns, np.int64)[:, None, None], np.asarray(lens, np.int64)[:, None, None]
    r0 = i * blk
    r1 = np.minimum((i + 1) * blk, Sq if mut == "r1 from Sq" else n_) - 1
    off = ln - (Sq if mut == "off from Sq" else n_)
    vis = np.broadcast_to((j * blk < ln) & (r1 >= r0), (nb, NQ, NK)).copy()       # (r1 < r0: a query block without a row)
    if causal:
        vis &= j * blk <= r1 + off
    frc = np.broadcast_to(j < keep_first, (nb, NQ, NK)).copy()
    if keep_local >= 1:
        jd_lo = np.maximum(r0 + off, 0) // blk
        jd_hi = np.minimum(np.maximum(r1 + off, 0), ln - 1) // blk
        frc |= (j >= jd_lo - (keep_local - 1)) & (j <= (jd_hi if causal else jd_hi + (keep_local - 1)))
    frc &= vis
    mass = None
    if top_p is None:
        mask = sref.kept_vectorised(t, vis, frc, top_k)
    else:
        u = pref.weights(t, vis, frc, pref.c_of(pref.default_scale(H, Hl, D)))
        mask = pref.kept_vectorised(t, vis, frc, min(top_k, NK), u, pref.p16_of(top_p))
        mass = pref.mass_of(mask, u)
    return dict(mask=mask, t=np.where(vis[:, None], t, -np.inf), mass=mass, vis=vis, frc=frc)


# ---- the cases of tests/test_gpu_ragged.py ------------------------------------------------------------------------------------------
def gpu_combos():
    """Parameters take turns over the product, as tests/test_gpu_extend.py's: every value of every axis meets every head grouping.
    qset 0 / 1: QLENS on the host; 2: RAW_QLEN as a device tensor (a negative value and one above Sq, both clamped)."""
    out = []
    for gi, (H, Hkv) in enumerate(eref.GROUPS):
        for i in range(12):
            blk = (128, 64)[(i // 4) % 2]
            out.append(dict(H=H, Hkv=Hkv, D=64 if H == 72 else (64, 128)[i % 2], dt=("bf16", "fp16")[(i // 2) % 2], blk=blk,
                            axis=("H", "Hkv", "1")[(i + i // 3) % 3], causal=bool((i // 3) % 2), qset=(i + gi) % 3,
                            q_dev=bool((i + gi) % 3 == 2 or (i // 2 + gi) % 2), kv_dev=bool((i + gi // 2) % 2),
                            bps=(None, 1, 2, -(-SK // blk))[(i + gi) % 4], seed=2000 * gi + i))
    return out


def combo_qlens(c):
    """The combo's q_len as the caller gives it (before the clamp)."""
    return RAW_QLEN if c["qset"] == 2 else QLENS[c["qset"]]


def combo_lens(c, q_lens):
    """kv_len per item: the length after the append.  One item is shorter than its chunk (kv_len[b] < q_len[b]: rows above the
    diagonal's start see nothing), one fills the capacity, the others sit either side of a block boundary."""
    base = (SK, 40, 333, 129) if c["seed"] % 2 else (385, 50, SK, 256)
    return [int(x) for x in base]


# ---- witness cases: zero scores, V of 0 / 1 (visibility.witness_v) on a ragged batch ---------------------------------------------------
def _witness_cases():
    out = []
    for i, (H, Hkv, axis, D, blk, dt, qset, C) in enumerate((
            (8, 2, "Hkv", 64, 128, "bf16", 0, 2), (2, 2, "H", 64, 64, "fp16", 1, 1), (72, 1, "1", 64, 128, "fp16", 2, 6),
            (8, 8, "H", 128, 64, "bf16", 0, 3))):
        c = dict(H=H, Hkv=Hkv, Hl={"H": H, "Hkv": Hkv, "1": 1}[axis], D=D, blk=blk, dt=dt, qset=qset, C=C, causal=True, seed=300 + i)
        c["q_lens"] = clamp(combo_qlens(c), SQ)
        c["lens"] = combo_lens(c, c["q_lens"])
        c["id"] = f"vis-H{H}kv{Hkv}-{dt}-D{D}-b{blk}-q{qset}-m{axis}"
        out.append(c)
    return out


def witness_probes(c):
    """The probe keys, by priority, cut to D / 2 channels: either side of each item's own causal diagonal at its first and at its
    last live row (keys r + kv_len[b] - n_b and the next), then either side of kv_len[b]."""
    wanted = []
    for n, ln in zip(c["q_lens"], c["lens"]):
        if n:
            for r in (0, n - 1):
                wanted += [r + ln - n, r + ln - n + 1]
    for ln in c["lens"]:
        wanted += [ln - 1, ln]
    probes = []
    for p in wanted:
        if 0 <= p < SK and p not in probes and len(probes) < c["D"] // 2:
            probes.append(p)
    return sorted(probes)


def witness_inputs(c):
    import visibility as vis
    NQ, NK = -(-SQ // c["blk"]), -(-SK // c["blk"])
    mask = eref.witness_mask(B, c["Hl"], NQ, NK, c["lens"], c["blk"])
    q, k = vis.zero_score_qk(c["seed"], B, c["H"], SQ, SK, c["D"])
    v = np.broadcast_to(vis.witness_v(SK, c["D"], witness_probes(c)), (B, c["Hkv"], SK, c["D"])).copy()
    return dict(q=q, k=k[:, :c["Hkv"]].copy(), v=v, mask=mask, sm_scale=c["D"] ** -0.5)


def witness_reference(c, inp, mut=None):
    """(out, lse) fp64: every output element is a count over the visible keys divided by their number.  mut None: the embedded
    rule; "" or one of MUTANTS: the direct form."""
    args = (inp["mask"], c["lens"], c["q_lens"], SQ, SK, c["blk"], c["H"], c["causal"])
    seen = visible(*args) if mut is None else visible_direct(*args, mut=mut)
    return attention(inp["q"], inp["k"], inp["v"], seen, inp["sm_scale"], c["dt"])


WITNESS_CASES = _witness_cases()
