"""Exact visibility tests of the attention kernels: inputs for which the answer is known by counting.

Every score is exactly zero (Q lives on channels [0, D/2), K on [D/2, D)), so every visible key of a row has the same
probability and the output row is (sum of V over the visible keys) / (number of visible keys), once rounded.  V holds only
0 and 1 and says which keys were summed:

    channels [0, P)          one PROBE channel for each key within two of a boundary under test
    channels [P, D/2)        key census: the other keys, key j in channel P + j mod (D/2 - P)
    channels [D/2, D)        tile census: key j in channel D/2 + (j // 64) mod (D/2)

One key wrongly visible or hidden at a boundary moves its probe channel between 0 and 1/n; a 64-key tile dropped or counted
twice moves its tile channel by a large fraction.  The references below only count, from the visibility rule each entry point
documents (README, INTEGRATION.md, the docstrings of block_sparse_attention, _core.dense_attention and LayoutSpec):

    plain   block_sparse_attention: row r sees key j iff block_mask[b, h, r // block, j // block] and j < kv_len[b]
            (keys past NK * block are never visited); a row without a visible key is 0
    dense   _core.dense_attention: rows < q_split see keys [0, kv_split), the others [kv_split, Sk); causal: inside a
            segment key j is visible to row i iff j <= i + (keys - rows); a row without a visible key is 0
    rect    _core.rectified_attention(block_mask=): visual row r sees key j iff block_mask[b, h, r // block, j // block]
            and j < kv_valid, its output is R * census + comp; text rows [NBv * block, NBv * block + q_text_valid) see
            the keys < kv_text_valid; later rows are 0

Tolerance (derived): sums of equal constants with at most 4 significant bits over fewer than 2^20 keys are exact in fp32;
what is left is one normalisation in fp32 and one conversion to the output type, so |got - ref| <= ulp * |ref| +
1e-6 * max|ref| with ulp = 2^-7 (bf16) / 2^-10 (fp16), and an element whose reference is 0 must be exactly 0.

A plain helper module: the case tables live here so that the CPU test can walk them without a device."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import numpy as np

ULP = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}
FLOOR = 1e-6          # x max|ref|: the absolute part of the bound
SENSITIVITY = 8.0     # a mutation must move an element by this many tolerances
TILE = 64             # keys per tile of the census (the kernels' K/V tile)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def zero_score_qk(seed: int, B: int, H: int, Sq: int, Sk: int, D: int) -> Tuple[np.ndarray, np.ndarray]:
    """q [B, H, Sq, D], k [B, H, Sk, D] fp32 with disjoint channel supports: every q . k is exactly 0.  The non-zero entries
    are random multiples of 1/8 in [-3, 3] without 0 (exact in bf16, fp16 and fp32)."""
    rng = np.random.default_rng(seed)

    def vals(shape):
        return (rng.integers(1, 25, shape) * rng.choice([-1, 1], shape)).astype(np.float32) / np.float32(8)
    q = np.zeros((B, H, Sq, D), np.float32)
    k = np.zeros((B, H, Sk, D), np.float32)
    q[..., :D // 2] = vals((B, H, Sq, D // 2))
    k[..., D // 2:] = vals((B, H, Sk, D // 2))
    return q, k


def around(key: int) -> List[int]:
    """The keys within two of a limit: the two just inside and the two just outside."""
    return [key - 2, key - 1, key, key + 1]


def witness_v(Sk: int, D: int, probes) -> np.ndarray:
    """[Sk, D] fp32 of 0 / 1 (module docstring): probes, key census, tile census.  Every key sets exactly two channels."""
    half = D // 2
    probes = sorted({int(p) for p in probes if 0 <= p < Sk})
    assert len(probes) <= half, f"{len(probes)} probe keys do not fit {half} channels"
    v = np.zeros((Sk, D), np.float32)
    j = np.arange(Sk)
    for c, p in enumerate(probes):
        v[p, c] = 1
    rest = half - len(probes)
    if rest:
        others = j[~np.isin(j, probes)]
        v[others, len(probes) + others % rest] = 1
    v[j, half + (j // TILE) % half] = 1
    return v


# ---- the counting reference ----------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Ref:
    """Which keys each GROUP of rows sees (rows of a group share their keys), and what turns the census into the output."""
    vis: np.ndarray                      # bool [BH | 1, G, Sk]
    r2g: np.ndarray                      # int [Sq]: the group of a row, -1 = a row that is written as 0
    v: np.ndarray                        # [Sk, D]
    R: Optional[np.ndarray] = None       # [BH, G] (rect: R of the visual groups, 1 for the text group)
    comp: Optional[np.ndarray] = None    # [BH, G, D] (rect: comp of the visual groups, 0 for the text group)

    def counts(self):
        """(sum of V over the visible keys [BH, G, D], number of visible keys [BH, G]): integers below 2^24, exact in fp32."""
        return (self.vis.astype(np.float32) @ self.v).astype(np.float64), self.vis.sum(-1).astype(np.int64)

    def finish(self, s, n):
        c = np.where(n[..., None] > 0, s / np.maximum(n, 1)[..., None], 0.0)
        if self.R is not None:
            c = self.R.astype(np.float64)[..., None] * c + self.comp.astype(np.float64)
        return c

    def groups(self) -> np.ndarray:
        return self.finish(*self.counts())

    def rows(self) -> np.ndarray:
        """float64 [BH | 1, Sq, D]."""
        g = self.groups()
        out = np.zeros((g.shape[0], self.r2g.shape[0], g.shape[2]))
        has = self.r2g >= 0
        out[:, has] = g[:, self.r2g[has]]
        return out


def tolerance(ref: np.ndarray, ulp: float) -> np.ndarray:
    return ulp * np.abs(ref) + FLOOR * float(np.abs(ref).max())


# ---- plain block_sparse_attention ------------------------------------------------------------------------------------------
MASK_KINDS = ("all", "boundary", "from_boundary", "past", "to_boundary")


def plain_mask(B, H, NQ, NK, blk, kv_len) -> np.ndarray:
    """bool [B, H, NQ, NK]: query block i of head h takes kind (i + 2 h) mod 5 -- all kept; only the block that holds key
    kv_len - 1; the blocks at or after it; only a block wholly past kv_len (none kept when there is none: 0 either way); the
    blocks up to it.  Neighbouring query blocks (the two of a 64-token pair) never share a kind."""
    m = np.zeros((B, H, NQ, NK), bool)
    for b in range(B):
        bb = min((kv_len[b] - 1) // blk, NK - 1)
        for h in range(H):
            for i in range(NQ):
                kind = MASK_KINDS[(i + 2 * h) % 5]
                if kind == "all":
                    m[b, h, i] = True
                elif kind == "boundary":
                    m[b, h, i, bb] = True
                elif kind == "from_boundary":
                    m[b, h, i, bb:] = True
                elif kind == "past":
                    if -(-kv_len[b] // blk) < NK:
                        m[b, h, i, -(-kv_len[b] // blk)] = True
                else:
                    m[b, h, i, :bb + 1] = True
    return m


def tail_mask(H, NQ, NK, seed) -> np.ndarray:
    """bool [1, H, NQ, NK]: 9 to 11 kept blocks per row (uneven pieces of a split walk), the last key block in every second."""
    rng = np.random.default_rng(seed)
    m = np.zeros((1, H, NQ, NK), bool)
    for h in range(H):
        for i in range(NQ):
            n = 9 + (h + i) % 3
            if i % 2 == 0:
                m[0, h, i, NK - 1] = True
                n -= 1
            m[0, h, i, rng.choice(NK - 1, n, replace=False)] = True
    return m


def _plain_cases() -> List[dict]:
    cases = []
    for dt in ("bf16", "fp16"):
        for D, blk in ((128, 128), (64, 128), (128, 64), (64, 64), (32, 128)):
            Sk = 5 * blk + 17
            pairs = [(1, Sk), (63, Sk - 1), (64, 2 * blk + 37), (65, blk + 1), (blk - 1, blk)]
            if D == 32:                                   # one padded case
                pairs = [(65, Sk - 1)]
            for kv in pairs:
                cases.append(dict(id=f"plain-{dt}-D{D}-b{blk}-kv{kv[0]}_{kv[1]}", family="plain", dt=dt, D=D, blk=blk, B=2, H=2,
                                  Sq=300, Sk=Sk, kv_len=kv, NK=-(-Sk // blk), mask="kinds"))
        # fewer mask columns than key blocks: keys past NK * block are never visited
        for D, blk in ((128, 128), (64, 64)):
            Sk = 5 * blk + 17
            cases.append(dict(id=f"plain-{dt}-D{D}-b{blk}-NK3", family="plain", dt=dt, D=D, blk=blk, B=2, H=2, Sq=300, Sk=Sk,
                              kv_len=(Sk, 2 * blk + 37), NK=3, mask="kinds"))
        # the tail split (head dim 128, 128-token blocks only): 9 x 64 = 576 workgroups, the last 64 walks split 4 ways
        cases.append(dict(id=f"plain-{dt}-tail", family="plain", dt=dt, D=128, blk=128, B=1, H=9, Sq=64 * 128, Sk=64 * 128,
                          kv_len=(64 * 128 - 70,), NK=64, mask="tail", tail_split=(1, 0)))
    return cases


def plain_ref(c: dict, H: Optional[int] = None, kv_len=None, col_limit=None, key_lo=0) -> Ref:
    B, blk, Sq, Sk, NK = c["B"], c["blk"], c["Sq"], c["Sk"], c["NK"]
    H = c["H"] if H is None else H
    NQ = -(-Sq // blk)
    nominal = list(c["kv_len"])
    mask = plain_mask(B, H, NQ, NK, blk, nominal) if c["mask"] == "kinds" else tail_mask(H, NQ, NK, 7)
    kv_len = nominal if kv_len is None else kv_len
    col_limit = NK * blk if col_limit is None else col_limit
    j = np.arange(Sk)
    kept = mask[..., np.minimum(j // blk, NK - 1)]                          # [B, H, NQ, Sk]
    lim = np.asarray(kv_len)[:, None, None, None]
    vis = kept & (j < lim) & (j < col_limit) & (j >= key_lo)
    probes = [0, Sk - 1] + [p for n in nominal for p in around(n)] + (around(NK * blk) if NK * blk < Sk else [])
    return Ref(vis.reshape(B * H, NQ, Sk), np.arange(Sq) // blk, witness_v(Sk, c["D"], probes)), mask


def plain_mutants(c: dict, H: int):
    Sk, NK, blk = c["Sk"], c["NK"], c["blk"]
    kv = list(c["kv_len"])
    for b, n in enumerate(kv):
        for d in (-1, 1):
            if n + d <= Sk and n <= NK * blk:      # (past NK * block the mask's width is the limit, not kv_len)
                yield f"kv_len[{b}]{d:+d}", dict(kv_len=kv[:b] + [n + d] + kv[b + 1:])
    if NK * blk < Sk:
        for d in (-1, 1):
            yield f"NK*block{d:+d}", dict(col_limit=NK * blk + d)
    yield "key 0 hidden", dict(key_lo=1)


# ---- dense attention -------------------------------------------------------------------------------------------------------
DENSE_SHAPES = [(300, 520), (520, 300), (257, 257), (1, 129), (700, 1100)]
DENSE_FORMS = [("bf16", False), ("fp16", False), ("bf16", True), ("bf16", "pv")]       # (dtype of q / k / v and O, qkv_fp8)


def dense_splits(Sq: int, Sk: int) -> List[Tuple[Optional[int], Optional[int]]]:
    """No split; q_split / kv_split at a multiple of 128 and one to either side; the ends q_split = 0 and kv_split = Sk."""
    qa = 128 * max(1, Sq // 256) if Sq > 128 else Sq
    ka = 128 * max(1, Sk // 256)
    out = [(None, None)]
    for qs, ks in ((qa, ka), (qa - 1, ka - 1), (qa + 1, ka + 1), (0, ka), (qa, Sk)):
        pair = (min(max(qs, 0), Sq), min(max(ks, 0), Sk))
        if pair not in out:
            out.append(pair)
    return out


def _dense_cases() -> List[dict]:
    cases = []
    for D in (128, 64):
        for Sq, Sk in DENSE_SHAPES:
            for qs, ks in dense_splits(Sq, Sk):
                for causal in (False, True):
                    name = "whole" if qs is None else f"q{qs}_kv{ks}"
                    cases.append(dict(id=f"dense-D{D}-{Sq}x{Sk}-{name}{'-causal' if causal else ''}", family="dense", D=D, B=2, H=2,
                                      Sq=Sq, Sk=Sk, q_split=qs, kv_split=ks, causal=causal))
    return cases


def dense_ref(c: dict, hi1=None, lo2=None, shift=0, qs=None, key_lo=0, key_hi=None) -> Ref:
    Sq, Sk = c["Sq"], c["Sk"]
    q_split = Sq if c["q_split"] is None else c["q_split"]
    kv_split = Sk if c["kv_split"] is None else c["kv_split"]
    hi1 = kv_split if hi1 is None else hi1
    lo2 = kv_split if lo2 is None else lo2
    qs = q_split if qs is None else qs
    key_hi = Sk if key_hi is None else key_hi
    i, j = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
    seg2 = i >= qs
    vis = (j >= np.where(seg2, lo2, 0)) & (j < np.where(seg2, Sk, hi1)) & (j >= key_lo) & (j < key_hi)
    if c["causal"]:
        keys = np.where(seg2, Sk - kv_split, kv_split)
        rows = np.where(seg2, Sq - qs, qs)
        vis &= (j - np.where(seg2, kv_split, 0)) <= (i - np.where(seg2, qs, 0)) + (keys - rows) + shift
    probes = [0, 1, Sk - 2, Sk - 1] + (around(kv_split) if 0 < kv_split < Sk else [])
    return Ref(vis[None], np.arange(Sq), witness_v(Sk, c["D"], probes))


def dense_mutants(c: dict):
    Sq, Sk = c["Sq"], c["Sk"]
    q_split = Sq if c["q_split"] is None else c["q_split"]
    kv_split = Sk if c["kv_split"] is None else c["kv_split"]
    if q_split > 0:                                # segment 1 has rows
        for d in (-1, 1):
            if 0 <= kv_split + d <= Sk:
                yield f"end of segment 1 {d:+d}", dict(hi1=kv_split + d)
    if q_split < Sq:                               # segment 2 has rows
        for d in (-1, 1):
            if 0 <= kv_split + d <= Sk:
                yield f"start of segment 2 {d:+d}", dict(lo2=kv_split + d)
        if kv_split < Sk:
            yield "last key hidden", dict(key_hi=Sk - 1)
    if 0 < q_split < Sq and 0 < kv_split < Sk:
        for d in (-1, 1):
            yield f"q_split{d:+d}", dict(qs=q_split + d)
    if q_split > 0 and kv_split > 0:
        yield "key 0 hidden", dict(key_lo=1)
    if c["causal"] and dense_ref(c).vis.any():
        for d in (-1, 1):
            yield f"diagonal{d:+d}", dict(shift=d)


# ---- rectified attention over a caller's mask ----------------------------------------------------------------------------------
RECT_LAYOUTS = {  # name -> (LayoutSpec constructor, arguments besides block=)
    "hunyuan": ("hunyuan", (8 * 128, 6 * 128 + 77)),
    "flux": ("flux", (7 * 128, 256, 7 * 128 - 45)),                 # keys in [kv_valid, pool_valid) are invisible
    "cogvideo": ("cogvideo", (128 * 4 + 226, 226)),
    "wan": ("wan", (6 * 128 - 37,)),
    "cogvideo_odd": ("cogvideo", (8 * 64 + 170, 170)),              # block 64: three text blocks (odd: half a 128-row text unit)
    "hunyuan_tsplit": ("hunyuan", (34 * 128, 32 * 128 + 100)),      # 33 text key blocks: the text rows' walk is split
    "hunyuan_tail": ("hunyuan", (104 * 128, 104 * 128 - 56)),       # 6 heads x 104 padded blocks: a tail of 112 walks split 4 ways
}
RECT_FORMS = [("bf16", False, 128), ("fp16", False, 128), ("bf16", False, 64), ("fp16", False, 64), ("bf16", True, 128),
              ("bf16", "pv", 128)]


def _rect_cases() -> List[dict]:
    def case(layout, dt, fp8, blk, D, B=2, H=2, **kw):
        form = {False: dt, True: "e4m3", "pv": "pv"}[fp8]
        return dict(id=f"rect-{layout}-{form}-b{blk}-D{D}", family="rect", layout=layout, dt=dt, fp8=fp8, blk=blk, D=D, B=B, H=H, **kw)
    cases = []
    for D in (128, 64):
        for dt, fp8, blk in RECT_FORMS:
            for layout in ("hunyuan", "flux", "cogvideo", "wan"):
                cases.append(case(layout, dt, fp8, blk, D))
            if blk == 64:
                cases.append(case("cogvideo_odd", dt, fp8, blk, D))
    for dt, fp8 in (("bf16", False), ("bf16", True), ("bf16", "pv")):
        cases.append(case("hunyuan_tsplit", dt, fp8, 128, 128, B=1))
    cases.append(case("hunyuan_tsplit", "bf16", False, 128, 64, B=1))
    for dt, fp8 in (("bf16", False), ("bf16", True)):
        cases.append(case("hunyuan_tail", dt, fp8, 128, 128, B=1, H=6, tail_split=(1, 0)))
    return cases


@dataclasses.dataclass
class Spec:
    """The numbers of _core.LayoutSpec the visibility rule needs (restated so that this module needs no device library)."""
    S: int
    NB_total: int
    NBv: int
    n_txt: int
    kv_valid: int
    pool_valid: int
    q_text_valid: int
    kv_text_valid: int
    block: int


def rect_spec(c: dict):
    """The case's _core.LayoutSpec."""
    from rectified_spaattn_amd import _core
    ctor, args = RECT_LAYOUTS[c["layout"]]
    return getattr(_core.LayoutSpec, ctor)(*args, block=c["blk"])


def rect_mask(B, H, sp: Spec, seed) -> np.ndarray:
    """bool [B, H, NBv, NB_total]: rows 0..3 of every head are all kept / the block that holds key kv_valid - 1 / the blocks
    from it on (both beside block 0: a row that keeps nothing among the first L blocks has R = 0 and shows nothing of its
    walk) / only a block wholly past kv_valid (no block where there is none: the row is comp alone); the others keep 3 to 5
    random blocks, every second one the boundary block too."""
    rng = np.random.default_rng(seed)
    NQ, NK, blk = sp.NBv, sp.NB_total, sp.block
    bb = (sp.kv_valid - 1) // blk
    past = -(-sp.kv_valid // blk)
    m = np.zeros((B, H, NQ, NK), bool)
    for b in range(B):
        for h in range(H):
            for i in range(NQ):
                kind = (i + h) % NQ if NQ < 8 else i
                if kind == 0:
                    m[b, h, i] = True
                elif kind == 1:
                    m[b, h, i, [0, bb]] = True
                elif kind == 2:
                    m[b, h, i, 0] = True
                    m[b, h, i, bb:] = True
                elif kind == 3:
                    if past < NK:
                        m[b, h, i, past] = True
                else:
                    m[b, h, i, rng.choice(NK, min(NK, 3 + i % 3), replace=False)] = True
                    if i % 2:
                        m[b, h, i, bb] = True
    return m


def rect_ref(c: dict, sp: Spec, H: Optional[int] = None, R=None, comp=None, kv_valid=None, kv_text_valid=None,
             q_text_valid=None, key_lo=0):
    """R [BH, NBv] / comp [BH, NBv, D]: the call's own (return_parts), or None for the model of rect_model_parts."""
    B, blk, S, D = c["B"], sp.block, sp.S, c["D"]
    H = c["H"] if H is None else H
    NQ = sp.NBv
    mask = rect_mask(B, H, sp, 11)
    kv_valid = sp.kv_valid if kv_valid is None else kv_valid
    kv_text_valid = sp.kv_text_valid if kv_text_valid is None else kv_text_valid
    q_text_valid = sp.q_text_valid if q_text_valid is None else q_text_valid
    j = np.arange(S)
    vis = np.zeros((B * H, NQ + 1, S), bool)
    vis[:, :NQ] = (mask[..., j // blk] & (j < kv_valid) & (j >= key_lo)).reshape(B * H, NQ, S)
    vis[:, NQ] = (j < kv_text_valid) & (j >= key_lo)
    r = np.arange(S)
    r2g = np.where(r < NQ * blk, r // blk, np.where(r < NQ * blk + q_text_valid, NQ, -1))
    probes = [0, S - 1] + around(sp.kv_valid) + around(sp.kv_text_valid)
    v = witness_v(S, D, probes)
    if R is None:
        R, comp = rect_model_parts(sp, mask, v)
    Rg = np.ones((B * H, NQ + 1))
    Rg[:, :NQ] = np.asarray(R, np.float64).reshape(B * H, NQ)
    cg = np.zeros((B * H, NQ + 1, D))
    cg[:, :NQ] = np.asarray(comp, np.float64).reshape(B * H, NQ, D)
    return Ref(vis, r2g, v, Rg, cg), mask


def rect_model_parts(sp: Spec, mask: np.ndarray, v: np.ndarray):
    """R and comp for the CPU checks, where no device call supplies them: the rectification's formula (DESIGN.md section 5.8:
    R = sum of probs over M, w = probs off M, comp = w . vbar) with uniform probabilities -- every pooled score of these inputs
    is 0 -- and no GAPR bit, which leaves the most weight in comp.  The GPU test repeats the sensitivity check with the
    call's own R and comp."""
    B, H, NQ, _ = mask.shape
    L = sp.NBv + (1 if sp.n_txt > 0 else 0)
    M = mask[..., :L]
    R = M.sum(-1) / L
    vp = np.zeros((sp.NB_total * sp.block, v.shape[1]))
    n = min(sp.S, sp.pool_valid)
    vp[:n] = v[:n]
    vbar = vp.reshape(sp.NB_total, sp.block, -1).mean(1)
    comp = ((~M) / L) @ vbar[:L]
    return R.reshape(B * H, NQ), comp.reshape(B * H, NQ, -1)


def rect_mutants(sp: Spec):
    for d in (-1, 1):
        if sp.kv_valid + d <= sp.S:
            yield f"kv_valid{d:+d}", dict(kv_valid=sp.kv_valid + d)
    if sp.q_text_valid > 0:
        for d in (-1, 1):
            if sp.kv_text_valid + d <= sp.S:
                yield f"kv_text_valid{d:+d}", dict(kv_text_valid=sp.kv_text_valid + d)
            if sp.NBv * sp.block + sp.q_text_valid + d <= sp.S:
                yield f"q_text_valid{d:+d}", dict(q_text_valid=sp.q_text_valid + d)
    yield "key 0 hidden", dict(key_lo=1)


# ---- the tables --------------------------------------------------------------------------------------------------------------
PLAIN_CASES = _plain_cases()
DENSE_CASES = _dense_cases()
RECT_CASES = _rect_cases()
CASES: Dict[str, dict] = {c["id"]: c for c in PLAIN_CASES + DENSE_CASES + RECT_CASES}
assert len(CASES) == len(PLAIN_CASES) + len(DENSE_CASES) + len(RECT_CASES)


def case_ulp(c: dict) -> float:
    """One ulp of the case's output type (the dense table is shared by its forms: bf16 is the coarser of them)."""
    return ULP[c.get("dt", "bf16")]


def spec_numbers(spec) -> Spec:
    return Spec(spec.S, spec.NB_total, spec.NBv, spec.n_txt, spec.kv_valid, spec.pool_valid, spec.q_text_valid,
                spec.kv_text_valid, spec.block)


def reference(c: dict, H: Optional[int] = None, parts=None, **mutation) -> Ref:
    """The case's counting reference (for H heads instead of the case's own; with one limit moved: the mutants below)."""
    if c["family"] == "plain":
        return plain_ref(c, H, **mutation)[0]
    if c["family"] == "dense":
        return dense_ref(c, **mutation)
    R, comp = parts if parts is not None else (None, None)
    return rect_ref(c, spec_numbers(rect_spec(c)), H, R, comp, **mutation)[0]


def mutants(c: dict, H: Optional[int] = None):
    if c["family"] == "plain":
        return plain_mutants(c, c["H"] if H is None else H)
    if c["family"] == "dense":
        return dense_mutants(c)
    return rect_mutants(spec_numbers(rect_spec(c)))


# ---- the sensitivity condition -------------------------------------------------------------------------------------------------
def insensitive(c: dict, ulp: float, H: Optional[int] = None, parts=None) -> List[str]:
    """The mutations of the case's reference that the bound would NOT notice (empty = the condition holds): every limit of the
    case moved by one key (or row) to either side, and every 64-key tile of every group's walk dropped or counted twice, must
    move at least one output element by SENSITIVITY tolerances.  Left out, because no output can show them: counting a tile
    twice in a walk that has no other tile (sum / count is unchanged exactly), the walk of a rectified row with R = 0, and
    a limit behind which another one hides every key anyway."""
    base = reference(c, H, parts)
    rows0 = base.rows()
    tol = tolerance(rows0, ulp)
    missed = []
    for name, mutation in mutants(c, H):
        mut = reference(c, H, parts, **mutation)
        if np.array_equal(mut.r2g, base.r2g) and np.array_equal(mut.vis, base.vis):
            continue        # no row's keys change: another limit binds first (the causal diagonal in front of a segment's end)
        rows1 = mut.rows()
        if not (np.abs(rows1 - rows0) >= SENSITIVITY * tol).any():
            missed.append(name)
    s, n = base.counts()
    g0 = base.finish(s, n)
    tolg = ulp * np.abs(g0) + FLOOR * float(np.abs(rows0).max())
    live = np.isin(np.arange(base.vis.shape[1]), base.r2g)                 # groups that have rows
    for t in range(-(-base.vis.shape[2] // TILE)):
        sl = slice(t * TILE, (t + 1) * TILE)
        part = base.vis[..., sl]
        nt = part.sum(-1)
        if not nt.any():
            continue
        st = (part.astype(np.float32) @ base.v[sl]).astype(np.float64)
        for sign, what in ((-1, "dropped"), (1, "doubled")):
            g1 = base.finish(s + sign * st, n + sign * nt)
            moved = (np.abs(g1 - g0) >= SENSITIVITY * tolg).any(-1)
            need = (nt > 0) & live[None, :]
            if sign > 0:
                need &= nt < n
            if base.R is not None:
                need &= base.R != 0                                        # (R = 0: the row is comp, whatever its walk)
            bad = need & ~moved
            if bad.any():
                bh, g = np.argwhere(bad)[0]
                missed.append(f"tile {t} {what} (e.g. head {bh}, group {g}: {int(bad.sum())} walks)")
    return missed


# ---- the check itself ------------------------------------------------------------------------------------------------------------
def violations(got: np.ndarray, ref: np.ndarray, ulp: float) -> str:
    """'' when got (float64, the output widened exactly) meets the bound against ref, else what is wrong and where."""
    ref = np.broadcast_to(ref, got.shape)
    err = np.abs(got - ref)
    tol = tolerance(ref, ulp)
    msgs = []
    if not np.isfinite(got).all():
        msgs.append(f"{int((~np.isfinite(got)).sum())} non-finite elements")
    zero = ref == 0
    if (got[zero] != 0).any():
        idx = np.argwhere(zero & (got != 0))
        msgs.append(f"{len(idx)} elements must be exactly 0, first at {tuple(idx[0])}: {got[tuple(idx[0])]!r}")
    over = err > tol
    if over.any():
        idx = np.argwhere(over)
        worst = np.unravel_index(np.argmax(err / tol), err.shape)
        msgs.append(f"{len(idx)} elements past the bound, worst at {tuple(int(x) for x in worst)} (last axis = the channel that "
                    f"names the keys): got {got[worst]!r}, ref {ref[worst]!r}, {err[worst] / tol[worst]:.1f} x the bound; "
                    f"channels of that row past the bound: {np.nonzero(over[worst[:-1]])[0].tolist()[:16]}")
    return "; ".join(msgs)


@functools.lru_cache(maxsize=None)
def qk_inputs(B, H, Sq, Sk, D):
    return zero_score_qk(Sq * 131 + Sk * 7 + D + H, B, H, Sq, Sk, D)
