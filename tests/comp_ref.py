"""Designed inputs, references and numpy models for K4, comp = w . vbar (compensation_kernel<D>, the fp32 MFMA chain, and
compensation_split_kernel<D>, bf16 hi / lo planes with three MFMAs per product, in rsa_stats.hip).

K4 reads w [BH, NBv, L] and vbar [BH, NB_total, D] and writes comp [BH, NBv, D]; L = NBv + (n_txt > 0).  Everything here is written
straight into those two buffers, so any fp32 pattern can be reached.

Exact classes (exact_case).  Every operand is an integer times a power of two (2^-e per row of w, 2^f per channel of vbar), and the
integers are so short that sum_j |w_ij vbar_jd| < 2^24 quanta for every (i, d): every partial sum under any order and any rounding is
representable, so comp is known to the bit.  The split form is exact only while lo . lo = 0:
    X1  w has 9 .. 12 significant bits (always odd, so lo != 0), vbar at most 8, signed: pins  al . bh8
    X2  w at most 8 bits, vbar 9 .. 12, signed:                                         pins  ah . bl8
Rows of at most 129 columns are dense; longer ones hold at most 64 non-zeros, at hashed columns that always include the chunk edges.
Row kinds (KINDS, rotated from tile to tile so that each kind meets several accumulator rows): one-hot rows e_j at the chunk edges of
both forms (comp[i] = vbar[j] 2^-e to the bit), a row whose only weight is the text column, dense rows, an all-zero row, a pair of
rows that differ in column L - 1 only.  The second and third head hold the first head's rows permuted inside each 32-row tile and a
vbar of their own.  vbar rows j >= L are large finite decoys, and so is what lies behind w, vbar (flat(): the buffers as the device
gets them, with a decoy tail) -- a mis-guarded tail gives a wrong number, not a fault.

Bound class (bound_case).  Full 24-bit operands: w = random^6 2^-e per row (rows of 1, 2, 3, 8 non-zeros, dense rows, a subnormal
row), vbar normal 2^f per channel.  bounds() is the per-element reference: fp64 product, S = sum |w| |vbar|, n = non-zero products,
    chain  |got - ref| <= (n + 1) u S + floor                        u = 2^-24: the dot-product bound, any order, fused or not
    split  |got - ref| <= (2^-15 (1 + 2^-7) + 6 n u) S + floor       x = hi + lo + rest, |x - hi| <= 2^-8 |x|, |rest| <= 2^-17 |x|:
           the dropped lo . lo + rest . v + w . rest is at most 2^-15 (1 + 2^-7) per product; 3 n exact products, each addition
           allowed a whole ulp (2u) of a partial sum of at most S
    floor = n 2^-126 max_j |vbar_jd|   (operands a pipe may flush, sums that underflow)

Models.  staged() restates the kernels' index arithmetic (head strides, clamped rows, the guarded tail chunk) as gathers into the
tile operands A [H, rows, J], B [H, J, D]; product() multiplies them -- exactly (fp64: an exact class has one answer), or in float32
under an accumulation order; stored() is the accumulator-to-row map.  MUTANTS are flags of these three stages: the ways a
correct-looking kernel goes wrong exactly where the designed rows look."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, Tuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24
HEADS = 3
W_TAIL = 128          # decoy floats behind w
V_TAIL_ROWS = 64      # decoy rows behind vbar
C_TAIL_ROWS = 32      # guard rows behind comp (a tile is 32 rows)
EDGES = (0, 1, 30, 31, 32, 33, 62, 63, 64, 65)   # and L - 2, L - 1


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Shape:
    """wan: no text.  hunyuan: a 256-token text tail, 40 of it valid (NB_total = L + 1 at 128-token blocks, L + 3 at 64).
    flux: 512 text tokens (NB_total = L + 3)."""
    NBv: int
    kind: str = "wan"
    block: int = 128

    @property
    def text_blocks(self) -> int:
        return {"wan": 0, "hunyuan": 256 // self.block, "flux": 512 // self.block}[self.kind]

    @property
    def n_txt(self) -> int:
        return {"wan": 0, "hunyuan": 40, "flux": 512}[self.kind]

    @property
    def L(self) -> int:
        return self.NBv + (1 if self.n_txt else 0)

    @property
    def NB_total(self) -> int:
        return self.NBv + self.text_blocks

    @property
    def S(self) -> int:
        return self.NB_total * self.block

    @property
    def name(self) -> str:
        return f"{self.kind}{self.NBv}" + (f"/b{self.block}" if self.block != 128 else "")

    @property
    def dense(self) -> bool:
        return self.L <= 129

    @property
    def nnz(self) -> int:
        return self.L if self.dense else 64


SHAPES = tuple([Shape(n) for n in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 520)] +
               [Shape(n, "hunyuan") for n in (31, 32, 63, 64, 127, 256)] +
               [Shape(5, "flux"), Shape(40, "flux"), Shape(70, "hunyuan", 64), Shape(1029, "hunyuan")])
THRESHOLD_SHAPES = (Shape(255), Shape(256))
DS = (64, 128)

KINDS = ("dense", "hot:0", "text", "pair_a", "pair_b", "zero", "hot:L-1", "hot:1", "hot:L-2", "dense", "hot:31", "hot:32", "hot:63",
         "hot:64", "hot:30", "hot:33", "hot:62", "hot:65") + ("dense",) * 14
assert len(KINDS) == 32


def kind_of(sh: Shape, i: int) -> str:
    """The kind of row i of the first head; a kind the shape cannot hold (no text, a column past L) is a dense row."""
    k = KINDS[(i + 7 * (i // 32)) % 32]
    if k == "text" and not sh.n_txt:
        return "dense"
    if k.startswith("hot:") and not 0 <= _col(sh, k) < sh.L:
        return "dense"
    if k == "pair_b" and (i == 0 or KINDS[(i - 1 + 7 * ((i - 1) // 32)) % 32] != "pair_a"):
        return "dense"
    return k


def _col(sh: Shape, k: str) -> int:
    c = k[4:]
    return sh.L - int(c[2:]) if c.startswith("L-") else int(c)


def bits(sh: Shape) -> Tuple[int, int]:
    """(bits of the split side, bits of the narrow side): nnz 2^bs 2^bn <= 2^24."""
    lg = int(np.ceil(np.log2(sh.nnz))) if sh.nnz > 1 else 0
    bs = 12 if sh.nnz <= 64 else 10
    return bs, min(8, 24 - lg - bs)


def head_perm(sh: Shape, h: int) -> np.ndarray:
    """Rows of head h in terms of the first head's: inside each 32-row tile reversed (h = 1) or rotated."""
    idx = np.arange(sh.NBv)
    if h == 0:
        return idx
    out = idx.copy()
    for t0 in range(0, sh.NBv, 32):
        n = min(32, sh.NBv - t0)
        out[t0:t0 + n] = t0 + (np.arange(n)[::-1] if h == 1 else (np.arange(n) + n // 2 + 1) % n)
    return out


# ---- bf16 ------------------------------------------------------------------------------------------------------------------
def bf16_rne(x: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bfloat16 (ties to even), as float32.  Finite inputs only."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + ((u >> 16) & 1) + 0x7FFF) & 0xFFFF0000).astype(np.uint32).view(F32)


def bf16_trunc(x: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def split(x: np.ndarray, mut: str = ""):
    """k4_split2: hi = bf16(x), lo = bf16(x - hi)."""
    hi = bf16_trunc(x) if mut == "hi_trunc" else bf16_rne(x)
    lo = bf16_rne(x) if mut == "lo_from_x" else bf16_rne((x - hi).astype(F32))
    return hi, lo


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    sh: Shape
    D: int
    cls: str
    w: np.ndarray        # [HEADS, NBv, L] float32
    vbar: np.ndarray     # [HEADS, NB_total, D] float32
    ref: np.ndarray      # [HEADS, NBv, D]: float32 bits (exact classes) or float64 (bound class)
    kinds: list          # kinds[h][i]
    info: dict

    def flat(self, heads: int):
        """(w, vbar) of the first `heads` heads as flat float32 arrays with their decoy tails: what the device gets."""
        g = np.random.default_rng(99)
        wt = (F32(3.0) * F32(2.0) ** 30 * (1 + g.random(W_TAIL))).astype(F32)
        vt = (-F32(5.0) * F32(2.0) ** 28 * (1 + g.random(V_TAIL_ROWS * self.D))).astype(F32)
        return np.concatenate([self.w[:heads].ravel(), wt]), np.concatenate([self.vbar[:heads].ravel(), vt])


def _columns(sh: Shape, g) -> np.ndarray:
    """The non-zero columns of a long row: the chunk edges of both forms and hashed ones, 64 at most."""
    L = sh.L
    fixed = {c for c in EDGES + (L - 2, L - 1, (L - 1) // 32 * 32, (L - 1) // 32 * 32 - 1, (L - 1) // 64 * 64, (L - 1) // 64 * 64 - 1)
             if 0 <= c < L}
    rest = np.setdiff1d(np.arange(L), sorted(fixed))
    extra = g.choice(rest, 64 - len(fixed), replace=False)
    return np.sort(np.concatenate([np.array(sorted(fixed), np.int64), extra]))


def _ints(g, n, lo_bits, hi_bits, odd):
    """n integers of lo_bits .. hi_bits significant bits (odd: the lowest bit set, so the value needs all of them)."""
    b = g.integers(lo_bits, hi_bits + 1, n)
    v = g.integers(0, 1 << 62, n) % (1 << (b - 1)) + (1 << (b - 1))
    return (v | 1) if odd else v


@functools.lru_cache(maxsize=None)
def exact_case(sh: Shape, D: int, cls: str) -> Case:
    assert cls in ("X1", "X2")
    bs, bn = bits(sh)
    NBv, L, NB = sh.NBv, sh.L, sh.NB_total
    g = np.random.default_rng([NBv, NB, D, sh.block, cls == "X1"])
    w_bits, v_bits = ((9, bs, True), (1, bn, False)) if cls == "X1" else ((1, bn, False), (9, bs, True))
    W = np.zeros((NBv, L), np.int64)
    kinds0 = [kind_of(sh, i) for i in range(NBv)]
    for i, k in enumerate(kinds0):
        if k == "zero":
            continue
        if k.startswith("hot:"):
            W[i, _col(sh, k)] = 1
        elif k == "text":
            W[i, NBv] = _ints(g, 1, *w_bits)[0]
        elif k == "pair_b":
            W[i] = W[i - 1]
            W[i, L - 1] = W[i - 1, L - 1] + 2      # (stays odd, stays inside the bit budget: see the assertion below)
        else:
            cols = np.arange(L) if sh.dense else _columns(sh, g)
            W[i, cols] = _ints(g, cols.size, *w_bits)
            if k == "pair_a":                     # room for pair_b's + 2
                W[i, L - 1] = (1 << (w_bits[1] - 1)) | 1
    e = (np.arange(NBv) * 7 + 3) % 12
    for i, k in enumerate(kinds0):
        if k == "pair_b":
            e[i] = e[i - 1]
    f =(np.arange(D) * 5 + 2) % 9 - 4
    w = np.empty((HEADS, NBv, L), F32)
    vbar = np.empty((HEADS, NB, D), F32)
    ref = np.empty((HEADS, NBv, D), F32)
    kinds, smax = [], 0
    for h in range(HEADS):
        perm = head_perm(sh, h)
        Wh, eh = W[perm], e[perm]
        V = _ints(g, NB * D, *v_bits).reshape(NB, D) * g.choice((-1, 1), (NB, D))
        V[L:] = (3 + 4 * g.integers(0, 1 << 10, (NB - L, D))) << 28        # decoy rows: large, finite
        S = np.abs(Wh) @ np.abs(V[:L])
        assert (S < 1 << 24).all(), (sh.name, D, cls, int(S.max()))       # the budget, per element
        smax = max(smax, int(S.max()))
        w[h] = np.ldexp(Wh.astype(np.float64), -eh[:, None])
        vbar[h] = np.ldexp(V.astype(np.float64), f[None, :])
        assert np.array_equal(w[h].astype(np.float64), np.ldexp(Wh.astype(np.float64), -eh[:, None]))
        assert np.array_equal(vbar[h].astype(np.float64), np.ldexp(V.astype(np.float64), f[None, :]))
        exact = np.ldexp((Wh @ V[:L]).astype(np.float64), f[None, :] - eh[:, None])
        ref[h] = exact
        assert np.array_equal(ref[h].astype(np.float64), exact)
        assert len({r.tobytes() for r in V[:L]}) == L and (L < 4 or len({c.tobytes() for c in V[:L].T}) == D)
        kinds.append([kinds0[p] for p in perm])
    # the split side keeps a lo, the other side has none, and hi + lo is the operand: lo . lo = 0 and nothing is dropped
    side, other = (w, vbar[:, :L]) if cls == "X1" else (vbar[:, :L], w)
    hi, lo = split(side)
    assert np.array_equal(hi.astype(np.float64) + lo, side.astype(np.float64))
    assert not split(other)[1].any()
    nz = side != 0
    share = float((lo[nz] != 0).mean())
    return Case(sh, D, cls, w, vbar, ref, kinds, dict(bits=(bs, bn), budget=smax / float(1 << 24), lo_share=share,
                                                      nonzero=int(nz.sum())))


BOUND_KINDS = ("nz1", "dense", "nz2", "nz3", "nz8", "subnormal", "dense", "nz1")


@functools.lru_cache(maxsize=None)
def bound_case(sh: Shape, D: int) -> Case:
    NBv, L, NB = sh.NBv, sh.L, sh.NB_total
    g = np.random.default_rng([NBv, NB, D, sh.block, 7])
    w = np.zeros((HEADS, NBv, L), F32)
    vbar = np.empty((HEADS, NB, D), F32)
    kinds = []
    for h in range(HEADS):
        kh = []
        for i in range(NBv):
            k = BOUND_KINDS[(i + 3 * h) % len(BOUND_KINDS)]
            kh.append(k)
            row = (g.random(L) ** 6 * 2.0 ** -((i * 7 + h) % 12)).astype(F32)
            if k.startswith("nz"):
                keep = g.choice(L, min(L, int(k[2:])), replace=False)
                if i % 3 == 0:
                    keep[0] = L - 1
                m = np.zeros(L, bool)
                m[keep] = True
                row = np.where(m, np.maximum(row, F32(2.0 ** -40)), F32(0))
            elif k == "subnormal":
                row = (g.random(L) * 2.0 ** -128).astype(F32)           # below 2^-126: subnormal in fp32 and in bf16
            w[h, i] = row
        kinds.append(kh)
        vbar[h] = (g.standard_normal((NB, D)) * 2.0 ** ((np.arange(D) * 5 + 2) % 9 - 4)[None, :]).astype(F32)
        vbar[h, L:] = (F32(2.0) ** 30 * (1 + g.random((NB - L, D)))).astype(F32)
    ref = w.astype(np.float64) @ vbar[:, :L].astype(np.float64)
    return Case(sh, D, "B", w, vbar, ref, kinds, {})


def bounds(w: np.ndarray, vbar: np.ndarray, L: int) -> Dict[str, np.ndarray]:
    """Per element of comp [H, NBv, D]: ref (fp64), and the chain and split bounds of the module docstring."""
    w64, v64 = w.astype(np.float64), vbar[:, :L].astype(np.float64)
    ref = w64 @ v64
    S = np.abs(w64) @ np.abs(v64)
    n = (w64 != 0).astype(np.float64) @ (v64 != 0).astype(np.float64)
    floor = n * 2.0 ** -126 * np.abs(v64).max(1)[:, None, :]
    return dict(ref=ref, S=S, n=n, floor=floor, chain=(n + 1) * U * S + floor,
                split=(2.0 ** -15 * (1 + 2.0 ** -7) + 6 * n * U) * S + floor)


# ---- the kernels' index arithmetic -----------------------------------------------------------------------------------------
TJ = {"chain": 32, "split": 64}
INDEX_MUTANTS = ("guard_w", "guard_v", "guard_both", "skip_last", "v_stride", "w_stride", "no_text", "swap1_w", "swap1_v", "swap8_w",
                 "swap8_v")
STORE_MUTANTS = ("wv1", "no4h", "clamp_store")
SPLIT_MUTANTS = ("drop_lohi", "drop_hilo", "lo_from_x", "hi_trunc")     # the bound class must see these too (see hi_trunc below)
MUTANTS = INDEX_MUTANTS + STORE_MUTANTS + SPLIT_MUTANTS


def staged(wflat, vflat, sh: Shape, D: int, heads: int, form: str, mut: str = ""):
    """The operands as a workgroup stages them: A [heads, tiles * 32, J] (row i of a tile reads row min(i, NBv - 1)), B [heads, J, D],
    J = the chunks walked; elements at j >= L are 0 unless a mutant takes the guard off."""
    NBv, NB = sh.NBv, sh.NB_total
    L = NBv if mut == "no_text" else sh.L
    tj = TJ[form]
    nch = (L + tj - 1) // tj
    if mut == "skip_last" and nch > 1:
        nch -= 1
    J = nch * tj
    rows = np.minimum(np.arange((NBv + 31) // 32 * 32), NBv - 1)
    j = np.arange(J)
    ws = NBv * NBv if mut == "w_stride" else NBv * L
    vs = L * D if mut == "v_stride" else NB * D
    aw = np.arange(heads)[:, None, None] * ws + rows[None, :, None] * L + j[None, None, :]
    av = np.arange(heads)[:, None, None] * vs + j[None, :, None] * D + np.arange(D)[None, None, :]
    A = wflat[np.minimum(aw, wflat.size - 1)]
    B = vflat[np.minimum(av, vflat.size - 1)]
    assert mut in ("guard_w", "guard_v", "guard_both") or (aw[..., j < L].max() < wflat.size and av[:, j < L].max() < vflat.size)
    if mut not in ("guard_w", "guard_both"):
        A = np.where(j[None, None, :] < L, A, F32(0))
    if mut not in ("guard_v", "guard_both"):
        B = np.where(j[None, :, None] < L, B, F32(0))
    if mut in ("swap1_w", "swap8_w"):
        A = A[:, :, j ^ (1 if mut == "swap1_w" else 8)]
    if mut in ("swap1_v", "swap8_v"):
        B = B[:, j ^ (1 if mut == "swap1_v" else 8)]
    return np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)


def stored(acc: np.ndarray, sh: Shape, mut: str = "") -> np.ndarray:
    """Accumulators [heads, tiles * 32, D] -> comp [heads, NBv, D]; what no lane writes stays NaN."""
    H, R, D = acc.shape
    comp = np.full((H, sh.NBv, D), np.nan, acc.dtype)
    if mut == "wv1":
        acc = acc[:, :, np.arange(D) ^ 32]
    for i in range(R):                                  # ascending: of two lanes that write one address the later row wins
        t = i - 4 if (mut == "no4h" and i & 4) else i
        if mut == "clamp_store":
            t = min(t, sh.NBv - 1)
        if t < sh.NBv:
            comp[:, t] = acc[:, i]
    return comp


ORDERS = {"chain": ("seq_fused", "seq_unfused", "pairwise"), "split": ("seq", "planes", "pairwise")}


def _tree(p: np.ndarray) -> np.ndarray:
    """Pairwise float32 sum over axis 2 of p [H, R, J, D]."""
    J = p.shape[2]
    n2 = 1 << max(0, int(np.ceil(np.log2(J)))) if J > 1 else 1
    if n2 != J:
        p = np.concatenate([p, np.zeros(p.shape[:2] + (n2 - J,) + p.shape[3:], F32)], 2)
    while p.shape[2] > 1:
        p = (p[:, :, 0::2] + p[:, :, 1::2]).astype(F32)
    return p[:, :, 0]


def product(A: np.ndarray, B: np.ndarray, form: str, order: str, mut: str = "") -> np.ndarray:
    """A . B as the form computes it.  order "exact": in fp64 (an exact class has one answer under every order, and a mutant's
    answer only has to differ); otherwise float32 accumulators: j-sequential (the chain fused as the MFMA is, or unfused), the split
    form's planes lo.hi, hi.lo, hi.hi per 16-column step, or a pairwise tree over the products."""
    H, R, J = A.shape
    D = B.shape[2]
    if form == "split":
        ah, al = split(A, mut)
        bh, bl = split(B, mut)
        terms = [t for t, name in (((al, bh), "drop_lohi"), ((ah, bl), "drop_hilo"), ((ah, bh), None)) if name is None or name != mut]
    else:
        terms = [(A, B)]
    if order == "exact":
        with np.errstate(over="ignore", invalid="ignore"):
            return sum(a.astype(np.float64) @ b.astype(np.float64) for a, b in terms).astype(F32)
    acc = np.zeros((H, R, D), F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if order == "pairwise":
            for r0 in range(0, R, 32):
                for a, b in terms:                       # (bf16 x bf16 is exact in float32; the chain's product is rounded)
                    acc[:, r0:r0 + 32] = (acc[:, r0:r0 + 32] + _tree(a[:, r0:r0 + 32, :, None] * b[:, None, :, :])).astype(F32)
            return acc
        if order in ("seq_fused", "seq_unfused"):
            a, b = terms[0]
            for j in range(J):
                if order == "seq_fused":
                    acc = (acc.astype(np.float64) + a[:, :, j, None].astype(np.float64) * b[:, None, j, :].astype(np.float64)).astype(F32)
                else:
                    acc = acc + a[:, :, j, None] * b[:, None, j, :]
            return acc
        if order == "seq":
            for j in range(J):
                for a, b in terms:
                    acc = acc + a[:, :, j, None] * b[:, None, j, :]
            return acc
        assert order == "planes"
        for j0 in range(0, J, 16):
            for a, b in terms:
                for j in range(j0, j0 + 16):
                    acc = acc + a[:, :, j, None] * b[:, None, j, :]
        return acc


def model(case: Case, heads: int, form: str, order: str = "exact", mut: str = "", tiles=None) -> np.ndarray:
    """comp [heads, NBv, D] of the model.  tiles: the 32-row tiles to compute (the rows of the others stay NaN)."""
    wflat, vflat = case.flat(heads)
    A, B = staged(wflat, vflat, case.sh, case.D, heads, form, mut if mut in INDEX_MUTANTS else "")
    if tiles is None:
        acc = product(A, B, form, order, mut if mut in SPLIT_MUTANTS else "")
    else:
        acc = np.full(A.shape[:2] + (case.D,), np.nan, F32)
        for t in tiles:
            acc[:, 32 * t:32 * t + 32] = product(A[:, 32 * t:32 * t + 32], B, form, order, mut if mut in SPLIT_MUTANTS else "")
    return stored(acc, case.sh, mut if mut in STORE_MUTANTS else "")


def exemption(sh: Shape, D: int, form: str, mut: str):
    """The printed rule under which a shape cannot hold a mutant, or None."""
    if mut in ("v_stride", "w_stride", "no_text") and not sh.n_txt:
        return "a shape without text cannot hold the text mutants"
    if mut == "skip_last" and sh.L <= 32:
        return "L <= 32 cannot hold a second chunk"
    if mut == "skip_last" and form == "split" and sh.L <= 64:
        return "L <= 64 cannot hold a second chunk of the split form"
    if mut in ("swap1_w", "swap1_v") and sh.L == 1:
        return "one-column rows cannot hold pair swaps"
    if mut in ("guard_w", "guard_v"):
        return "no shape: the other operand's guarded zeros annihilate a finite tail, only both guards off can show"
    if mut == "guard_both" and sh.L % TJ[form] == 0:
        return "a row that ends on a chunk edge has no tail to guard"
    if mut == "no4h" and sh.NBv == 1:
        return "one query-block row: every row of the tile is a copy of row 0"
    if mut == "clamp_store":
        return "no shape: rows past NBv are staged as copies of row NBv - 1, so the clamped store writes that row's own bits again"
    if mut in SPLIT_MUTANTS and form == "chain":
        return "the chain form has no planes"
    if mut == "hi_trunc":
        return "exact classes: hi + lo = x under either rounding of hi, and the other operand has no lo"
    return None
