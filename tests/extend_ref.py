"""numpy reference of block_sparse_extend: a plain helper module, no device.  decode_ref's pieces
(parts, finish, merge, split_keys, the paged helpers) are reused by import; what is new here is the rule at NQ query blocks, the
row groups, and witness cases that span more than one query block and more than one row group.

    visible        row r of (b, h) sees key j iff mask[b, hl(h), r // block, j // block] and j < kv_len[b] and j < NK * block and,
                   with causal, j <= r + kv_len[b] - Sq (bottom-right aligned, r counted in the whole call); with the mutations
                   the CPU test applies
    row_groups     how the kernel cuts the gu x rows rectangle of a unit's query block into groups of at most 64 rows
    scores2        decode_ref.scores2 as one batched matrix product (the extend shapes are a hundred times decode's)
    split_parts    (m, l, O) of every split of every query block's kept list; decode_ref.merge combines them
    witness cases  the inputs of the exact tests of tests/test_gpu_extend.py"""
from __future__ import annotations

import numpy as np

import decode_ref as dref
import visibility as vis
import weights

SK = dref.SK
ROWS = 64           # rows of a row group, at most


# ---- row groups ------------------------------------------------------------------------------------------------------------------
def row_groups(gu: int, Sq: int, blk: int):
    """(gh, qg): a group is gh heads of the unit x qg consecutive query rows of one query block.  gh = the unit's gu heads in
    ceil(gu / 64) even chunks; qg = as many rows as still fit 64, at most a query block's."""
    hc = -(-gu // ROWS)
    gh = -(-gu // hc)
    return gh, min(ROWS // gh, Sq, blk)


def group_rows(gu: int, Sq: int, blk: int):
    """(first, count) int [Sq]: the first query row and the row count of the group that holds query row r (the same for every
    head: groups are heads x contiguous rows)."""
    _, qg = row_groups(gu, Sq, blk)
    r = np.arange(Sq)
    first = r // blk * blk + r % blk // qg * qg
    end = np.minimum(np.minimum(first + qg, (r // blk + 1) * blk), Sq)
    return first, end - first


def group_count(B: int, H: int, Hkv: int, Hl: int, Sq: int, blk: int) -> int:
    """Workgroups per split of a call."""
    U = max(Hl, Hkv)
    gu = H // U
    gh, qg = row_groups(gu, Sq, blk)
    NQ = -(-Sq // blk)
    qc = sum(-(-(min((i + 1) * blk, Sq) - i * blk) // qg) for i in range(NQ))
    return B * U * -(-gu // gh) * qc


def rows16(gu: int, Sq: int, blk: int) -> int:
    gh, qg = row_groups(gu, Sq, blk)
    return 16 if gh * qg <= 16 else (32 if gh * qg <= 32 else 64)


def default_split(groups: int, NK: int) -> int:
    """blocks_per_split=None, as documented: min(8, NK) below 256 row groups, one split from there on."""
    return min(8, NK) if groups < 256 else NK


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def visible(mask, lens, Sq: int, Sk: int, blk: int, H: int, causal: bool, kv_shift: int = 0, causal_shift: int = 0,
            mask_row=None, sq_as=None, row_as=None, group_limit=None, gu: int = 1):
    """bool [B, H, Sq, Sk].  mask bool [B|1, Hl, NQ, NK]; lens B ints.  Mutations (gu: the heads of a unit, for the groups):
        kv_shift, causal_shift   the key limit / the causal limit off by that many keys
        mask_row="next"          the mask row taken as (r + 1) // block
        mask_row=("run", G)      groups pretended to be runs of G rows counted from row 0 (they straddle query blocks when G does
                                 not divide the block), the mask row taken from the run's first row
        sq_as="block" | "group"  the causal offset computed with the row count of the row's block / group in place of Sq
        row_as="block" | "group" the row's index in its block / group in place of its index in the whole call
        group_limit="first"      the causal limit of the group's first row applied to all of the group's rows"""
    B = len(lens)
    mask = np.asarray(mask, bool)
    Hl, NQ, NK = mask.shape[1:]
    assert NQ == -(-Sq // blk)
    m = np.broadcast_to(mask, (B, Hl, NQ, NK))
    hl = np.arange(H) // (H // Hl)
    j = np.arange(Sk)
    r = np.arange(Sq)
    inside = j < NK * blk
    qb = r // blk
    if mask_row == "next":
        qb = np.minimum((r + 1) // blk, NQ - 1)
    elif mask_row is not None:
        qb = r // mask_row[1] * mask_row[1] // blk
    gfirst, gcount = group_rows(gu, Sq, blk)
    bfirst = r // blk * blk
    bcount = np.minimum(bfirst + blk, Sq) - bfirst
    out = np.zeros((B, H, Sq, Sk), bool)
    for b in range(B):
        kept = np.zeros((H, Sq, Sk), bool)
        kept[:, :, inside] = m[b][hl][:, qb][:, :, j[inside] // blk]
        row = np.broadcast_to(j < lens[b] + kv_shift, (Sq, Sk))
        if causal:
            rows = {None: Sq, "block": bcount, "group": gcount}[sq_as]
            idx = {None: r, "block": r - bfirst, "group": r - gfirst}[row_as]
            last = idx + lens[b] - rows + causal_shift         # the last key the row sees
            if group_limit == "first":
                last = last[gfirst]
            row = row & (j[None, :] <= last[:, None])
        out[b] = kept & row[None]
    return out


def visible_naive(mask, lens, Sq, Sk, blk, H, causal):
    """The same rule as a loop over every (b, h, r, j)."""
    B = len(lens)
    mask = np.asarray(mask, bool)
    Hl, NQ, NK = mask.shape[1:]
    out = np.zeros((B, H, Sq, Sk), bool)
    for b in range(B):
        mb = mask[b if mask.shape[0] > 1 else 0]
        for h in range(H):
            for r in range(Sq):
                for j in range(Sk):
                    ok = j // blk < NK and mb[h // (H // Hl), r // blk, min(j // blk, NK - 1)] and j < lens[b]
                    if causal:
                        ok = ok and j <= r + lens[b] - Sq
                    out[b, h, r, j] = ok
    return out


# ---- scores, attention -----------------------------------------------------------------------------------------------------------
def scores2(q, k, sm_scale: float, dt=None):
    """decode_ref.scores2 (fp64 [B, H, Sq, Sk], log2 domain) as one batched matrix product."""
    q = np.asarray(q, np.float32)
    k = np.nan_to_num(np.asarray(k, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    H, Hkv = q.shape[1], k.shape[1]
    if dt is None:
        qs = q.astype(np.float64) * (float(sm_scale) * dref.LOG2E)
    else:
        qs = weights.round_dt(q * weights.qk_scale(sm_scale), dt).astype(np.float64)
    g = H // Hkv
    B, _, Sq, D = q.shape
    s = np.matmul(qs.reshape(B, Hkv, g * Sq, D), k.transpose(0, 1, 3, 2))
    return s.reshape(B, H, Sq, k.shape[2])


def parts(s2, seen, v):
    """decode_ref.parts with the products as batched matrix products."""
    B, H, Sq, Sk = s2.shape
    Hkv = v.shape[1]
    vv = np.nan_to_num(np.asarray(v, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    s = np.where(seen, s2, -np.inf)
    m = s.max(-1)
    mref = np.where(np.isfinite(m), m, 0.0)
    p = np.where(seen, np.exp2(s - mref[..., None]), 0.0)
    o = np.matmul(p.reshape(B, Hkv, (H // Hkv) * Sq, Sk), vv).reshape(B, H, Sq, v.shape[3])
    return m, p.sum(-1), o


def attention(s2, seen, v):
    return dref.finish(*parts(s2, seen, v))


# ---- splits ----------------------------------------------------------------------------------------------------------------------
def split_parts(s2, seen, v, mask, blk: int, C: int):
    """[(m, l, O)] per split s = entries [s C, (s + 1) C) of the ascending kept list of (b, list head, QUERY BLOCK): what the
    workgroups (row group, s) of a query block's groups write.  S = ceil(NK / C) for every query block."""
    B, H, Sq, Sk = s2.shape
    mask = np.asarray(mask, bool)
    NQ = mask.shape[2]
    per_block = []
    for i in range(NQ):
        rows = slice(i * blk, min((i + 1) * blk, Sq))
        keys = dref.split_keys(mask[:, :, i:i + 1], B, H, Sk, blk, C)
        per_block.append([parts(s2[:, :, rows], seen[:, :, rows] & sk[:, :, None, :], v) for sk in keys])
    return [tuple(np.concatenate([pb[s][x] for pb in per_block], axis=2) for x in range(3)) for s in range(len(per_block[0]))]


# ---- witness cases ---------------------------------------------------------------------------------------------------------------
GROUPS = dref.GROUPS + ((72, 1),)


def witness_mask(B, Hl, NQ, NK, lens, blk):
    """bool [B, Hl, NQ, NK]: everything kept but one block per (list head, query block) that lies between two kept ones and below
    the limit; neighbouring query blocks drop different ones."""
    m = np.ones((B, Hl, NQ, NK), bool)
    for b in range(B):
        last = max((lens[b] - 1) // blk, 0)
        for hl in range(Hl):
            for i in range(NQ):
                if last >= 2:
                    m[b, hl, i, 1 + (hl + i) % (last - 1)] = False
    return m


def _cases(kind):
    """Two query blocks at least, more than one row group in a query block, a unit of 72 heads; D = 64 wherever H = 72."""
    out = []
    for gi, (H, Hkv) in enumerate(GROUPS):
        for i in range(2 if kind == "wts" else 3):
            dt = ("bf16", "fp16")[(i + gi) % 2]
            D = 64 if H == 72 else (64, 128)[(i + gi) % 2]
            blk = (128, 64)[i % 2]
            Sq = {128: (129, 200, 300), 64: (65, 150, 129)}[blk][(i + gi) % 3]
            axis = ("Hkv", "1", "H")[(i + gi) % 3]
            NK = -(-SK // blk)
            out.append(dict(kind=kind, id=f"{kind}-H{H}kv{Hkv}-{dt}-D{D}-b{blk}-Sq{Sq}-m{axis}", H=H, Hkv=Hkv, dt=dt, D=D, blk=blk,
                            Sq=Sq, Hl={"H": H, "Hkv": Hkv, "1": 1}[axis], lens=[SK, 333] if i % 2 == 0 else [400, 140],
                            causal=bool((i + gi) % 4 != 3), C=(2, 1, 3, NK)[(i + gi) % 4], seed=100 * gi + i))
    return out


VIS_CASES = _cases("vis")
WEIGHT_CASES = _cases("wts")


def case_groups(c):
    """(gu, first, count) of a case: the heads of a unit, the first row and the row count of each query row's group."""
    gu = c["H"] // max(c["Hl"], c["Hkv"])
    return (gu,) + group_rows(gu, c["Sq"], c["blk"])


def vis_probes(c, mask):
    """The probe keys of a visibility case, by priority, cut to D / 2 channels: the two keys either side of kv_len and of the
    causal limits of the first and last row of every query block and of every row pair a group boundary runs through (rows 63 / 64
    of a unit's block where a group is 64 rows); the edges of a dropped block; the first keys of splits."""
    Sq, blk, half = c["Sq"], c["blk"], c["D"] // 2
    _, first, _ = case_groups(c)
    starts = [r for r in range(1, Sq) if first[r] == r]        # the first row of every group but the first
    rows = sorted({0, Sq - 1} | set(starts) | {r - 1 for r in starts})
    wanted = []
    for n in c["lens"]:
        wanted += [n - 1, n]
    if c["causal"]:
        for n in c["lens"]:
            for r in rows:
                wanted += [r + n - Sq, r + n - Sq + 1]
    for n in c["lens"]:
        wanted += [n - 2, n + 1]
    for jb in sorted({int(x) for x in np.argwhere(~mask)[:, 3]})[:2]:
        wanted += [jb * blk - 1, jb * blk, (jb + 1) * blk - 1, (jb + 1) * blk]
    for i in range(mask.shape[2]):
        for s0 in dref.split_starts(mask[:, :, i], blk, c["C"]):
            wanted += [s0 - 1, s0]
    probes = []
    for p in wanted:
        if 0 <= p < SK and p not in probes and len(probes) < half:
            probes.append(p)
    return sorted(probes)


def vis_inputs(c):
    """Zero scores, V of 0 / 1 (visibility.witness_v: probe channels, a key census, a tile census)."""
    B, H, Hkv, D, blk, Sq = 2, c["H"], c["Hkv"], c["D"], c["blk"], c["Sq"]
    NK = -(-SK // blk)
    mask = witness_mask(B, c["Hl"], -(-Sq // blk), NK, c["lens"], blk)
    q, k = vis.zero_score_qk(c["seed"], B, H, Sq, SK, D)
    v = np.broadcast_to(vis.witness_v(SK, D, vis_probes(c, mask)), (B, Hkv, SK, D)).copy()
    return dict(q=q, k=k[:, :Hkv].copy(), v=v, mask=mask, sm_scale=D ** -0.5)


def weight_inputs(c):
    """decode_ref.weight_inputs at NQ query blocks: integer scores n (Q rows one-hot with weights.find_a's amplitude, K = 8 n).
    Class 0 has its maximum in the last visible block of the cache, class 1 in the first, class 2 steps up by 8 at the first key
    of a query block's second split; the base is 0 .. 2, so a row's spread is at most 10."""
    B, H, Hkv, D, blk, Sq = 2, c["H"], c["Hkv"], c["D"], c["blk"], c["Sq"]
    NK = -(-SK // blk)
    sm = D ** -0.5
    a = float(weights.find_a(c["dt"], sm)[0][0])
    mask = witness_mask(B, c["Hl"], -(-Sq // blk), NK, c["lens"], blk)
    rng = np.random.default_rng(c["seed"])
    n = rng.integers(0, 3, (B, Hkv, SK, 4)).astype(np.int64)
    for b, len_b in enumerate(c["lens"]):
        n[b, :, max(len_b - 2, 0), 0] += 6
        n[b, :, min(3, len_b - 1), 1] += 6
        for i in range(mask.shape[2]):
            edge = [s for s in dref.split_starts(mask[:, :, i], blk, c["C"]) if 0 < s < len_b]
            if edge:
                n[b, :, edge[0]:edge[0] + 2, 2] = 10
    q = np.zeros((B, H, Sq, D), np.float32)
    for h in range(H):
        for r in range(Sq):
            q[:, h, r, (r + h) % 4] = a
    k = np.zeros((B, Hkv, SK, D), np.float32)
    k[..., :4] = 8.0 * n
    v = np.broadcast_to(vis.witness_v(SK, D, []), (B, Hkv, SK, D)).copy()
    return dict(q=q, k=k, v=v, mask=mask, sm_scale=sm, n=n)


def weight_budget(c, inp):
    """decode_ref.weight_budget under this module's rule."""
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


def case_reference(c, inp, want_pieces: bool = False, **mut):
    """(out, lse, pieces | None) of a witness case on the operands the kernel multiplies; mut: visible()'s mutations."""
    s2 = scores2(inp["q"], inp["k"], inp["sm_scale"], c["dt"])
    seen = visible(inp["mask"], c["lens"], c["Sq"], SK, c["blk"], c["H"], c["causal"], gu=case_groups(c)[0], **mut)
    out, lse = attention(s2, seen, inp["v"])
    return out, lse, split_parts(s2, seen, inp["v"], inp["mask"], c["blk"], c["C"]) if want_pieces else None


within = dref.within
