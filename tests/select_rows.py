"""Designed rows for the selection pass (K3: select_mask_kernel<KPL, PASS> and select_mask_long_kernel in rsa_stats.hip).

Every other test that holds K3 to the oracle feeds it random or structured activations: no two probabilities of a row are equal
there, no cumulative sum lands on p_remain, nothing underflows.  The rows here are written straight into K3's input (the unscaled
score buffer and the GAPR bytes), so any fp32 pattern can be reached, and each row is built around a case in which the contract
rules C7 (probability descending, lower column first) and C8 (c <= thr, n = max(count + 1, top_k)) decide the answer:

    A  a plateau with an EXACT cut.  A1: the whole row equal.  A2: 2^k equal scores at the maximum, every other score so low
       that its exponential is exactly 0: Z = 2^k, p = 2^-k, every partial sum exact, so at p_remain = 0.25 the sum EQUALS the
       threshold at element 2^(k-2): count = 2^(k-2), n = count + 1, kept = the lowest columns of the plateau.
    B  a plateau across the top_k cut: h < top_k distinct scores (the first one heavier than p_remain: count = 0), then m equal
       ones with h + m > top_k.  The plateau's columns are a hashed subset that holds column 0, column NBv - 1 and columns that
       are far apart in the kernel's load order (lane + 64 m) but close in its sort order (lane * KPL + s).
    C  a plateau across the p_remain cut: the sequential sum first exceeds p_remain inside the plateau, the level of the row's
       tail solved (by bisection through the model below) so that the crossing element is the first, or the last, element a lane of
       cumsum_count owns -- for KPL keys per lane (the full sort) and for 4 (the sorted head of the prefix path).
    D  (L > 256) plateaus against the prefix path's window need <= #{p >= t} <= 256: the count of the values above the second
       plateau is exactly 128, 127, 256 or 257; a distinct head of 100 and then a plateau of 300 (no t exists).
    E  (L > 256) probabilities ONE ULP apart on either side of a cut (top_k's, p_remain's): the score bit pattern is searched on
       the CPU until the neighbour's probability is the adjacent float; the larger one in the higher column, and in the lower.
    F  peaked rows: a few scores at the maximum, the rest between 60 and 100 below it (scaled): the tail goes from normal
       through subnormal (exp never returns a subnormal; x / Z with Z > 1 and IPAR's (x * blk) / denom do) to exactly 0, a plateau
       of zeros.  top_k ends among the normal values, among the subnormal ones, among the zeros (kept by column ascending).
    G  threshold extremes, as launch parameters (param_sets()): p_remain below the first probability, 0, 1.0 and above it -- with a
       small top_k, so that the never-passing sum's count gives n = L + 1 and the clamp decides, and with top_k in {L, L + 5} --, top_k
       0 and 1, and for the long rows top_k in {128, 129, 256, 257} and a cut deep in the row (p_remain = 0.9).
    H  unions on tied rows: banded neighbours, a first-frame square (the layouts without text) and hashed GAPR bytes on the
       plateaus, so that M = kept | unrel, R and w depend on WHICH members of a plateau were kept.

Row r of a head is of class classes(sh)[r % P], variant (r // P) % (number of variants); the second head holds the first head's rows
permuted.  The builder records per row what it aimed at (Row.info); tests/test_select_rows_cpu.py checks every such claim on the
oracle's output, so nothing rests on the construction.

model_row() is an independent restatement of C5..C8 in numpy float32 (exp element by element through oracle.orc_exp, the 256
strided sums written out, np.lexsort, a sequential sum), and MUTANTS are flags of it: the ways a correct-looking kernel goes wrong
exactly where these rows look."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional

import numpy as np

from oracle import oracle as orc

F32 = np.float32
TOP_K, P_REMAIN = 8, 0.25           # the parameters the rows are designed for
TINY = np.finfo(np.float32).tiny    # the smallest normal float32


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Shape:
    """One launch geometry.  Text layouts are HunyuanVideo-style (a 256-token text tail, n_txt of it valid); the others are Wan-style
    with a first-frame square of ffb blocks.  band: the half-width of the banded neighbour matrix."""
    NBv: int
    n_txt: int = 0
    block: int = 128
    D: int = 64
    ffb: int = 0
    band: int = 0

    @property
    def name(self) -> str:
        return f"{self.NBv}" + (f"+{self.n_txt}txt" if self.n_txt else "") + (f"/b{self.block}" if self.block != 128 else "")

    @property
    def L(self) -> int:
        return self.NBv + (1 if self.n_txt else 0)

    @property
    def NB_total(self) -> int:
        return self.NBv + (256 // self.block if self.n_txt else 0)

    @property
    def S(self) -> int:
        return self.NB_total * self.block

    @property
    def num_true(self) -> int:
        return self.NBv * self.block + self.n_txt

    @property
    def KPL(self) -> int:
        n2 = 64
        while n2 < self.L:
            n2 <<= 1
        return n2 // 64

    @property
    def long(self) -> bool:
        return self.L > 256

    @property
    def scale(self) -> np.float32:
        return orc.softmax_scale(self.D)

    def layout(self) -> orc.Layout:
        if self.n_txt:
            return orc.Layout(self.S, self.NB_total, self.NBv, self.n_txt, self.num_true, self.num_true, self.NBv + 1, 0,
                              self.n_txt, self.num_true, "hunyuan")
        return orc.Layout(self.S, self.NBv, self.NBv, 0, self.S, self.S, self.NBv, self.ffb, 0, self.S, "wan")

    def neighbor(self, on: bool = True) -> Optional[np.ndarray]:
        return _band(self.NBv, self.band) if on else None


@functools.lru_cache(maxsize=None)
def _band(n: int, width: int) -> np.ndarray:
    i = np.arange(n)
    m = (np.abs(i[:, None] - i[None, :]) <= width).astype(np.uint8)
    m.setflags(write=False)
    return m


# the smallest geometries that reach each instantiation of K3 (KPL 1 .. 64, the two-pass launch from L = 257, the _ex entry)
# Every shape has a neighbour band (the GPU test also launches each without a neighbour list) and, where the layout has one, a
# first-frame square.  64 without text is the issue's whole-row case at L = 64.
SHAPES = [Shape(63, 3, band=1), Shape(64, ffb=4, band=1), Shape(64, 3, band=2), Shape(128, ffb=5, band=1), Shape(129, D=128, ffb=4, band=1),
          Shape(256, ffb=5, band=2), Shape(257, ffb=4, band=1), Shape(300, 5, block=64, D=128, band=2), Shape(520, ffb=3, band=1),
          Shape(1030, D=128, ffb=3, band=1), Shape(2100, ffb=6, band=1)]


def param_sets(sh: Shape) -> Dict[str, tuple]:
    """name -> (top_k, p_remain): the designed pair, the exact half (class A at p_remain = 0.5), class G's extremes -- p_remain >= 1
    with a SMALL top_k, so that n = L + 1 comes from the count of a sum that never passes and the clamp is what keeps it at L, and
    with top_k >= L --, and for the long rows the window's edges and a deep cut."""
    ps = {"designed": (TOP_K, P_REMAIN), "exact half": (TOP_K, 0.5), "p below the first probability, top_k 0": (0, 1e-9),
          "p 0, top_k 1": (1, 0.0), "p 1, top_k 8": (TOP_K, 1.0), "p above 1, top_k 8": (TOP_K, 1.5), "p above 1, top_k 0": (0, 1.5),
          "p 1, top_k L": (sh.L, 1.0), "p above 1, top_k L + 5": (sh.L + 5, 1.5)}
    if sh.long:
        ps.update({f"top_k {k}": (k, P_REMAIN) for k in (128, 129, 256, 257)})
        ps["deep cut"] = (TOP_K, 0.9)
    return ps


# ---- hashing ---------------------------------------------------------------------------------------------------------------
def _mix(*xs) -> np.ndarray:
    h = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for x in xs:
            h = (h ^ np.asarray(x).astype(np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            h = h ^ (h >> np.uint64(31))
        h = h * np.uint64(0x94D049BB133111EB)
        return h ^ (h >> np.uint64(29))


def _h(*xs) -> int:
    return int(_mix(*xs))


def _perm(n: int, *seed) -> np.ndarray:
    return np.argsort(_mix(np.arange(n), *seed), kind="stable")


# ---- the independent model -----------------------------------------------------------------------------------------------
_EXP: Dict[int, np.float32] = {}


def exp_each(d: np.ndarray) -> np.ndarray:
    """orc_exp element by element (one call per distinct bit pattern)."""
    d = np.ascontiguousarray(d, np.float32)
    u, inv = np.unique(d.view(np.uint32), return_inverse=True)
    vals = np.empty(len(u), np.float32)
    for i, b in enumerate(u.tolist()):
        v = _EXP.get(b)
        if v is None:
            v = _EXP[b] = F32(orc.orc_exp(float(np.array(b, np.uint32).view(np.float32))))
        vals[i] = v
    return vals[inv]


def strided_sum(v: np.ndarray) -> np.float32:
    """C6: 256 strided partial sums (element j into partial j % 256, j ascending), then the pairwise tree."""
    v = np.asarray(v, np.float32)
    part = np.zeros(256, np.float32)
    for j0 in range(0, len(v), 256):
        c = v[j0:j0 + 256]
        part[:len(c)] = part[:len(c)] + c
    s = 1
    while s < 256:
        part[0::2 * s] = part[0::2 * s] + part[s::2 * s]
        s *= 2
    return part[0]


def seq_sum_loop(sp: np.ndarray) -> np.ndarray:
    """C8's sum as a plain loop (what model_row's np.cumsum in float32 is checked against)."""
    out = np.empty(len(sp), np.float32)
    acc = F32(0)
    for k in range(len(sp)):
        acc = F32(acc + sp[k])
        out[k] = acc
    return out


def model_probs(s_vis, s_txt, scale, blk) -> np.ndarray:
    nbv = len(s_vis)
    x = np.concatenate([s_vis, s_txt]).astype(np.float32) * F32(scale)
    e = exp_each(x - x.max())
    x = e / strided_sum(e)
    if len(s_txt) == 0:
        return x
    ns, ts = strided_sum(x[:nbv]), strided_sum(x[nbv:])
    denom = F32(F32(ns * F32(blk)) + ts)
    return np.concatenate([(x[:nbv] * F32(blk)) / denom, np.array([ts / denom], np.float32)]).astype(np.float32)


MUTANTS = {
    "tie order reversed (higher column first)": "BCA",
    "ties broken by the load order lane + 64 m": "BCA",
    "probabilities one ulp apart treated as ties": "E",
    "c < thr for c <= thr": "A",
    "n = count for count + 1": "CA",
    "top_k applied before the + 1": "BF",
    "n not clamped to L": "G",
    "subnormals flushed before the sort": "F",
    "subnormals flushed in w": "F",
    "subnormals flushed in the sums of R": "F",
    "zeros excluded from the sort": "F",
    "sum restarted at each 256-key head": "AD",
    "first-frame square applied before the cut": "H",
    "neighbour union applied before the cut": "H",
    "R summed over kept without unrel": "H",
}


def model_row(probs: np.ndarray, unrel: np.ndarray, nbr_row, sh: Shape, qblk: int, top_k: int, p: float, mut: str = "", memo=None):
    """kept [NB_total] u8, n_needed, R, w, oob (mutant "n not clamped": a key past the row's end would be decoded) from the row's
    probabilities: C7, C8, the unions, R and w, with at most one MUTANTS flag.  memo: a dict that keeps the unmutated row's sorted
    order and running sums between calls (they depend on the probabilities alone, not on top_k or p)."""
    assert mut == "" or mut in MUTANTS
    L, nbv = sh.L, sh.NBv
    idx = np.arange(L)
    ps = probs
    if mut == "subnormals flushed before the sort":
        ps = np.where(probs < TINY, F32(0), probs)
    tie = idx
    if mut.startswith("tie order reversed"):
        tie = -idx
    elif mut.startswith("ties broken by the load order"):
        tie = (idx % 64) * sh.KPL + idx // 64
    if mut == "" and memo is not None and "order" in memo:
        order, c = memo["order"], memo["c"]
    else:
        order = np.lexsort((tie, -ps))
        if mut.startswith("probabilities one ulp apart"):      # a near-tie goes to the lower column, as a tie would
            bits = ps.view(np.uint32).astype(np.int64)
            k = np.nonzero((bits[order[:-1]] - bits[order[1:]] == 1) & (order[:-1] > order[1:]))[0]
            k = k[np.concatenate([[True], np.diff(k) > 1])[:len(k)]]     # (of a run of such pairs, the first)
            order[k], order[k + 1] = order[k + 1], order[k]
        if mut == "zeros excluded from the sort":
            order = order[ps[order] > 0]
        sp = ps[order]
        if mut.startswith("sum restarted"):
            c = np.concatenate([np.cumsum(sp[a:a + 256], dtype=np.float32) for a in range(0, len(sp), 256)])
        else:
            c = np.cumsum(sp, dtype=np.float32)          # sequential in float32 (checked against seq_sum_loop by the CPU test)
        if mut == "" and memo is not None:
            memo["order"], memo["c"] = order, c
    thr = F32(p)
    count = int((c < thr).sum()) if mut.startswith("c < thr") else int((c <= thr).sum())
    if mut.startswith("n = count"):
        n = max(count, top_k)
    elif mut.startswith("top_k applied before"):
        n = max(count, top_k) + 1
    else:
        n = max(count + 1, top_k)
    n_needed, oob = n, False
    if n > len(order):
        oob = mut.startswith("n not clamped") and n > L
        n = len(order)
    kept = np.zeros(sh.NB_total, np.uint8)
    kept[order[:n]] = 1
    if nbr_row is not None and mut != "neighbour union applied before the cut":
        kept[:nbv] |= (nbr_row != 0)
    if sh.n_txt:
        kept[nbv:nbv + 1] = 1                         # text blocks [NBv, text_end_block)
    if sh.ffb and qblk < sh.ffb and mut != "first-frame square applied before the cut":
        kept[:sh.ffb] = 1
    M = kept[:L].astype(bool)
    MR = M.copy()
    M[:nbv] |= (unrel != 0)
    if mut != "R summed over kept without unrel":
        MR = M
    pr = np.where(probs < TINY, F32(0), probs) if mut == "subnormals flushed in the sums of R" else probs
    R = strided_sum(np.where(MR, pr, F32(0)))
    w = np.where(M, F32(0), np.where(probs < TINY, F32(0), probs) if mut == "subnormals flushed in w" else probs).astype(np.float32)
    return kept, n_needed, R, w, oob


# ---- the rows ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Row:
    cls: str
    variant: int
    s_vis: np.ndarray            # [NBv] fp32 unscaled scores
    s_txt: np.ndarray            # [n_txt]
    info: dict                   # what the builder aimed at (checked by the CPU test on the oracle's output)


def _scores(sh: Shape, x: np.ndarray, off: float = 0.0) -> np.ndarray:
    """Unscaled scores whose scaled values are x (+ a common offset, which the softmax removes)."""
    return ((np.asarray(x, np.float64) + off) / float(sh.scale)).astype(np.float32)


def _txt(sh: Shape, level: float, off: float) -> np.ndarray:
    return _scores(sh, level - 0.1 * np.arange(sh.n_txt), off)


def _place(sh: Shape, levels: List[np.ndarray], first_cols: List[int], *seed):
    """x [NBv]: the groups of `levels`, in turn, take the columns first_cols (group 1, the plateau) and then a hashed order."""
    order = [int(c) for c in _perm(sh.NBv, *seed)]
    forced = [c for c in dict.fromkeys(first_cols) if 0 <= c < sh.NBv][:len(levels[1])]
    fs = set(forced)
    rest = [c for c in order if c not in fs]
    x = np.zeros(sh.NBv)
    cols_of = []
    for g, lv in enumerate(levels):
        nr = len(lv) - len(forced) if g == 1 else len(lv)
        take, rest = (forced if g == 1 else []) + rest[:nr], rest[nr:]
        x[take] = lv
        cols_of.append(np.array(sorted(take), dtype=np.int64))
    assert not rest
    return x, cols_of


def _plateau_cols(sh: Shape, v: int) -> List[int]:
    c = _h(sh.NBv, v, 11) % 48
    return [0, sh.NBv - 1, 63, 64, c + 1, c + 64, c + 65, c + 128]


def _offset(sh: Shape, v: int, tag: int) -> float:
    return (0.0, 0.5, 2.0, -1.0)[_h(sh.NBv, v, tag) % 4]


def row_B(sh: Shape, v: int) -> Row:
    h = 5
    m = 6 + _h(sh.NBv, v, 1) % min(35, sh.NBv - 20)
    head = np.concatenate([[0.0], -3.0 - 0.1 * np.arange(1, h)])
    tail = -8.0 - 0.01 * np.arange(sh.NBv - h - m)
    x, cols = _place(sh, [head, np.full(m, -6.0), tail], _plateau_cols(sh, v), v, 2)
    off = _offset(sh, v, 3)
    return Row("B", v, _scores(sh, x, off), _txt(sh, -4.0, off), dict(plateau=cols[1], head=h))


def _crossing(sh: Shape, s_vis, s_txt, p=P_REMAIN) -> int:
    """Sorted position of the first element whose sequential sum exceeds p (len: none does)."""
    pr = model_probs(s_vis, s_txt, sh.scale, sh.block)
    c = np.cumsum(pr[np.lexsort((np.arange(len(pr)), -pr))], dtype=np.float32)
    return int((c <= F32(p)).sum())


def row_C(sh: Shape, v: int) -> Row:
    K = (sh.KPL, 4)[(v // 2) % 2] if sh.long else sh.KPL
    last = v % 2 == 1
    target = next(t for t in range(12, 400) if t % K == (K - 1 if last else 0))
    h = 3 if (v // 4) % 2 == 0 else 0
    m = min(sh.NBv - h - 8, 4 * target - 4)
    head = -0.02 * np.arange(h)
    ntail = sh.NBv - h - m
    off = _offset(sh, v, 5)

    def build(xt):
        x, cols = _place(sh, [head, np.full(m, -0.5 if h else 0.0), xt - 0.01 * np.arange(ntail)], _plateau_cols(sh, v), v, 6)
        return _scores(sh, x, off), cols
    txt = _txt(sh, -30.0, off)
    lo, hi = -40.0, -0.6                                  # the crossing moves to later positions as the tail gains weight
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        pos = _crossing(sh, build(mid)[0], txt)
        if pos == target:
            break
        lo, hi = (mid, hi) if pos < target else (lo, mid)
    s_vis, cols = build(mid)
    assert _crossing(sh, s_vis, txt) == target, (sh.name, v, target)
    return Row("C", v, s_vis, txt, dict(plateau=cols[1], head=h, crossing=target, lane_keys=K, lane_last=last))


def row_A(sh: Shape, v: int) -> Row:
    if v == 0:      # A1: the whole row, text tokens included, at one score
        c = (1.0, -2.5, 0.0, 7.0)[_h(sh.NBv, 7) % 4]
        return Row("A", v, np.full(sh.NBv, c, np.float32), np.full(sh.n_txt, c, np.float32), dict(whole=True))
    kmax = int(np.log2(sh.NBv))
    k = min(kmax, (5, 6, 7, 8, 10)[(v - 1) % 5]) if sh.NBv >= 64 else 5
    m = 1 << k
    x, cols = _place(sh, [np.zeros(0), np.zeros(m), np.full(sh.NBv - m, -95.0)], _plateau_cols(sh, v), v, 8)
    off = (0.5, 2.0, -1.0)[_h(sh.NBv, v, 9) % 3]           # (not 0: a score of 0 pins its GAPR byte to 1)
    return Row("A", v, _scores(sh, x, off), _scores(sh, np.full(sh.n_txt, -95.0), off), dict(whole=False, plateau=cols[1], k=k))


def row_F(sh: Shape, v: int) -> Row:
    """t scores at the maximum (Z ~ t), `nn` normal values, `ns` in the zone that x / Z turns subnormal, zeros behind."""
    t, nn, ns = ((4, 10, 20), (4, 2, 20), (2, 1, 2))[v % 3]
    ns = min(ns, sh.NBv - t - nn - 6)
    zone_lo, zone_hi = -87.30, -87.336 + np.log(t) - 0.02          # exp() is 0 below -87.3365; exp() / t is subnormal below zone_hi
    u = lambda n, tag: (_mix(np.arange(n), sh.NBv, v, tag) % np.uint64(10007)).astype(np.float64) / 10007.0
    normal = -60.0 - 24.0 * u(nn, 1)
    sub = zone_lo + (zone_hi - zone_lo) * u(ns, 2)
    nz = sh.NBv - t - nn - ns
    zeros = -88.0 - 12.0 * u(nz, 3)
    x, cols = _place(sh, [np.zeros(t), np.zeros(0), normal, sub, zeros], [], v, 4)
    off = _offset(sh, v, 12)
    want = ("normal", "subnormal", "zero")[v % 3]
    return Row("F", v, _scores(sh, x, off), _txt(sh, -20.0, off), dict(cut=want, zeros=cols[4]))


D_COUNTS = (128, 127, 256, 257)


def row_D(sh: Shape, v: int) -> Row:
    if v < 4:           # the values above the second plateau number exactly T
        T = D_COUNTS[v]
        h = 20
        m1 = T - h
        m2 = min(200, sh.NBv - T)
        head = np.concatenate([[0.0], -3.0 - 0.05 * np.arange(1, h)])
        tail = -9.0 - 0.01 * np.arange(sh.NBv - T - m2)
        x, cols = _place(sh, [head, np.full(m1, -6.0), np.full(m2, -7.0), tail], _plateau_cols(sh, v), v, 21)
        info = dict(count=T, plateau=cols[1], second=cols[2])
    else:               # a distinct head of 100, then a plateau that jumps the window
        h = 100
        m = min(300, sh.NBv - h)
        head = np.concatenate([[0.0], -3.0 - 0.02 * np.arange(1, h)])
        x, cols = _place(sh, [head, np.full(m, -6.0), -9.0 - 0.01 * np.arange(sh.NBv - h - m)], _plateau_cols(sh, v), v, 22)
        info = dict(count=None, plateau=cols[1], jump=(h, h + m))
    off = _offset(sh, v, 23)
    return Row("D", v, _scores(sh, x, off), _txt(sh, -12.0, off), info)


def row_E(sh: Shape, v: int) -> Row:
    """Near-flat distinct values within 0.5 of the maximum (there one ulp of the score moves the probability by at most one ulp);
    the element just behind the cut is then moved, bit pattern by bit pattern, until its probability is the float below the
    probability of the element just before the cut -- in the lower column of the two (variants 0, 1: what a tie rule applied to
    near-ties would get wrong) or in the higher one (variants 2, 3)."""
    at_topk = v % 2 == 0
    nflat = 12 if at_topk else sh.NBv              # top_k's cut: 12 near-flat values carry the row, the sum passes 0.25 at the third
    step = 0.03 if at_topk else 0.45 / sh.NBv
    flat = -step * np.arange(nflat)
    x, cols = _place(sh, [flat, np.zeros(0), -30.0 - 0.001 * np.arange(sh.NBv - nflat)], [], v, 31)
    txt = _txt(sh, -30.0, 0.0)
    s = _scores(sh, x)
    pr = model_probs(s, txt, sh.scale, sh.block)
    order = np.lexsort((np.arange(len(pr)), -pr))
    cut = TOP_K if at_topk else _crossing(sh, s, txt) + 1         # the first sorted position that is NOT kept
    a, b = int(order[cut - 1]), int(order[cut])
    hi_higher = v < 2                               # the larger probability into the higher column (variants 2, 3: the lower)
    if (a < b) == hi_higher:
        s[a], s[b] = s[b], s[a]
        a, b = b, a
    s[b] = s[a]
    for _ in range(400):
        s[b] = np.nextafter(s[b], F32(-np.inf))
        pr = model_probs(s, txt, sh.scale, sh.block)
        if pr[b] != pr[a]:
            break
    return Row("E", v, s, txt, dict(cut="top_k" if at_topk else "p_remain", hi=a, lo=b, hi_higher=hi_higher))


BUILDERS = dict(A=(row_A, 6), B=(row_B, 6), C=(row_C, 8), D=(row_D, 5), E=(row_E, 4), F=(row_F, 3))


def classes(sh: Shape) -> str:
    return "BCAFDE" if sh.long else "BCAF"


@functools.lru_cache(maxsize=None)
def _row(sh: Shape, cls: str, v: int) -> Row:
    return BUILDERS[cls][0](sh, v)


@dataclasses.dataclass
class Case:
    sh: Shape
    rows: List[Row]              # head 0: row r of the launch
    scores: np.ndarray           # [2, NBv, NBv + n_txt] fp32: head 1 = head 0's rows permuted
    unrel: np.ndarray            # [2, NBv, NBv] u8
    perm: np.ndarray             # head 1's row r is head 0's row perm[r]

    def row_of(self, bh: int, r: int) -> Row:
        return self.rows[r if bh == 0 else int(self.perm[r])]


@functools.lru_cache(maxsize=None)
def case(sh: Shape) -> Case:
    cl = classes(sh)
    P = len(cl)
    rows = [_row(sh, cl[r % P], (r // P) % BUILDERS[cl[r % P]][1]) for r in range(sh.NBv)]
    sc0 = np.stack([np.concatenate([r.s_vis, r.s_txt]) for r in rows]).astype(np.float32)
    perm = _perm(sh.NBv, 77)
    scores = np.stack([sc0, sc0[perm]])
    bh, i, j = np.meshgrid(np.arange(2), np.arange(sh.NBv), np.arange(sh.NBv), indexing="ij")
    unrel = (_mix(bh, i, j, 5) % np.uint64(3) == 0).astype(np.uint8)           # hashed GAPR bytes, a third of them set ...
    unrel |= (scores[:, :, :sh.NBv] == 0).astype(np.uint8)                       # ... and where s == 0: !(0 > 0) = 1
    return Case(sh, rows, scores, unrel, perm)


def reference(sh: Shape, pname: str, bh: int = 0, nbr: bool = True) -> dict:
    """The oracle's selection of one head of the case under one parameter set ([NBv, ...]), with or without the neighbour list; made
    once, read-only."""
    return _reference(sh, pname, bh, nbr)


@functools.lru_cache(maxsize=None)
def _reference(sh: Shape, pname: str, bh: int, nbr: bool) -> dict:
    c = case(sh)
    top_k, p = param_sets(sh)[pname]
    nv = sh.NBv
    ref = orc.select_rows_from_scores(c.scores[bh][:, :nv], c.scores[bh][:, nv:], c.unrel[bh], sh.layout(), top_k, p,
                                      sh.neighbor(nbr), D=sh.D, block=sh.block)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def probs_of(sh: Shape, r: int) -> np.ndarray:
    """The model's probabilities of head 0's row r."""
    row = case(sh).rows[r]
    pr = model_probs(row.s_vis, row.s_txt, sh.scale, sh.block)
    pr.setflags(write=False)
    return pr


def model_case_row(sh: Shape, bh: int, r: int, pname: str, mut: str = "", nbr_on: bool = True):
    """model_row on row r of head bh under a parameter set."""
    c = case(sh)
    top_k, p = param_sets(sh)[pname]
    src = r if bh == 0 else int(c.perm[r])
    nbr = sh.neighbor(nbr_on)
    return model_row(probs_of(sh, src), c.unrel[bh, r], None if nbr is None else nbr[r], sh, r, top_k, p, mut,
                     _MEMO.setdefault((sh, src), {}))


_MEMO: Dict[tuple, dict] = {}
