"""Exact witnesses for the masked and dropout dense attention kernel (rsa_attn_masked.hip: dense_masked_kernel behind
rsa_dense_masked_fwd and rsa_dense_dropout_fwd, reached through _core.dense_attention_masked, _core.dense_attention_dropout
and fullattn's "torch" / "vanilla" modes).  The counterpart of tests/visibility.py and tests/weights.py for the one kernel
whose keys differ from row to row.

Every q . k is exactly 0 (visibility.zero_score_qk) and V is visibility.witness_v (0 / 1: probes, key census, tile census),
so a row's output only says which keys it summed and with what weight.  Four classes of case:

    A   visibility: bool masks and additive masks of 0 / -inf, every weight is 1.
    B   integer weights: the kernel computes x = 0 + 1.44269504f * bias in fp32.  For every integer n in -12 .. 12 there is a
        float32 b with fl(1.44269504f * b) == n exactly (EXACT_BIAS, found by enumerating the neighbours of n / 1.44269504; a
        contracted fma(c, b, 0) rounds the same exact product once).  Through the float32 mask kind every exp2(x - m), every
        rescale factor and every weight is then a power of two, and numerator, denominator and every l * alpha + psum are
        exact in fp32 as long as sum_j 2^(n_j - n_min) < 2^24 over a row's visible keys (budget()).  The 2-byte mask kind
        cannot reach this: a bf16 / fp16 b times the 24-bit constant is never an integer (other than 0).
    C   2-byte additive masks with finite values: not exact, held to 1.5 ulp (bound_c()).
    D   dropout: keep_np() is a numpy twin of the kernel's drop_hash.  It PINS the stream that the docstring of
        _core.dense_attention_dropout declares -- a counter-based hash of (seed, b * H + h, row, key): a change of the hash in
        the kernel has to change the twin in the same commit.  A weight is dropped iff hash < thresh(p); kept weights are
        multiplied by c = round_to_type(1 / (1 - p)) (the kernel's keep_scale after P is rounded to the 2-byte type); the row
        sum keeps every weight.  With the budget tightened to 2^13 the products c * 2^k still sum exactly.

The reference is per row, from a bool vis[BH, Sq, Sk] and an integer n[BH, Sq, Sk] (0 in class A), all in float64:

    out = c * (keep o w) @ v / sum_j w,     w = 2^n where visible, else 0

(the denominator runs over every visible key, kept or not).  A row without a visible key is 0 (empty_rows_nan=False, fullattn
"torch") or NaN (True, "vanilla").  Bound for A, B and D: visibility's, |got - ref| <= ULP |ref| + FLOOR max|ref|, zeros exact.
The causal rule is the top-left triangle j <= i (rsa_attn_masked.hip, attn.py), unlike every other kernel of the library.

The model mutants of insensitive() are numpy only; the rescale mutants run on walk(), which steps through 32-key tiles with a
running maximum as the kernel does.  They apply to the cases that have integer weights: in class A every alpha is 1 by
construction, so a lost rescale is not a fault those inputs could show -- class B witnesses it.

A plain helper module: the case tables live here so that the CPU test can walk them without a device."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional

import numpy as np

import visibility as vis
from visibility import FLOOR, SENSITIVITY, ULP, tolerance, violations  # noqa: F401  (the bound is visibility's, not restated)

LOG2E = np.float32(1.44269504)        # the constant of rsa_attn_masked.hip, not log2(e) to full precision
TILE = 32                             # keys per tile of dense_masked_kernel
WAVE = 32                             # query rows per wave
N_RANGE = 12                          # EXACT_BIAS covers -12 .. 12
SHAPES = [(1, 1), (33, 31), (129, 32), (1, 129), (200, 333), (257, 257), (130, 300), (300, 130)]
FORMS = [(64, "bf16"), (64, "fp16"), (128, "bf16"), (128, "fp16")]
C_VALUES = np.array([-4.0, -2.75, -1.5, -0.625, 0.0, 0.875, 2.25, 4.0], np.float32)     # exact in bf16 and in fp16


# ---- number formats ------------------------------------------------------------------------------------------------------
def round_dt(x, dt: str) -> np.ndarray:
    """x (float32) rounded to nearest-even in bf16 / fp16, widened back to float32."""
    x = np.asarray(x, np.float32)
    if dt == "fp16":
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def _exact_bias() -> Dict[int, np.float32]:
    """{n: a float32 b with fl32(1.44269504f * b) == n}: of the 64 float32 neighbours either side of n / 1.44269504 the one
    nearest to it that qualifies (n = 0: b = 0)."""
    table = {}
    for n in range(-N_RANGE, N_RANGE + 1):
        b0 = np.float32(n / float(LOG2E))
        up = down = b0
        cands = [b0]
        for _ in range(64):
            up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
            cands += [up, down]
        hits = [b for b in cands if np.float32(LOG2E * b) == np.float32(n)]
        assert hits, f"no float32 bias gives the integer {n}"
        table[n] = hits[0]
    return table


EXACT_BIAS = _exact_bias()


# ---- dropout: the twin of drop_hash ------------------------------------------------------------------------------------------
def drop_hash_np(seed: int, bh, row, key) -> np.ndarray:
    """uint64 arrays (broadcast together) -> the kernel's 24-bit hash: SplitMix64's finaliser over the packed coordinates,
    in np.uint64, which wraps around as the kernel's 64-bit arithmetic does."""
    u = np.uint64
    bh, row, key = (np.asarray(x).astype(np.uint64) for x in (bh, row, key))
    with np.errstate(over="ignore"):
        z = u(seed & 0xFFFFFFFFFFFFFFFF) + u(0x9E3779B97F4A7C15) * ((bh << u(42)) ^ (row << u(21)) ^ key)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
    return z >> u(40)


def thresh(p: float) -> int:
    """The launcher's threshold: int(float64(float32(p)) * 2^24 + 0.5), at least 1 for p > 0, 0 = no dropout."""
    if not p > 0:
        return 0
    return max(1, int(float(np.float32(p)) * 16777216.0 + 0.5))


def keep_np(seed: int, p: float, BH: int, Sq: int, Sk: int, order="row,key", with_bh=True) -> np.ndarray:
    """bool [BH, Sq, Sk]: the weights the kernel keeps.  order / with_bh: the mutants of insensitive()."""
    bh = np.arange(BH)[:, None, None] * (1 if with_bh else 0)
    r, j = np.arange(Sq)[None, :, None], np.arange(Sk)[None, None, :]
    h = drop_hash_np(seed, bh, r, j) if order == "row,key" else drop_hash_np(seed, bh, j, r)
    return np.broadcast_to(h >= np.uint64(thresh(p)), (BH, Sq, Sk))


def keep_scale(p: float, dt: str) -> float:
    """c: the kernel's float32 keep_scale = 1 / (1 - p) (0 for p = 1) once P * keep_scale is rounded to the 2-byte type."""
    if not p > 0:
        return 1.0
    p32 = np.float32(p)
    ks = np.float32(1) / (np.float32(1) - p32) if p32 < 1 else np.float32(0)
    return float(round_dt(ks, dt))


# ---- masks ---------------------------------------------------------------------------------------------------------------
def _edges(Sk: int) -> List[int]:
    """The 32-key tile edges that designed rows' masks end on: the first and the last edge inside the keys."""
    last = TILE * ((Sk - 1) // TILE)
    return sorted({e for e in (TILE, last) if 0 < e < Sk})


def probes_of(c: dict) -> List[int]:
    Sk = c["Sk"]
    p = [0, Sk - 2, Sk - 1]
    for e in _edges(Sk):
        p += vis.around(e)
    if c.get("causal"):
        p += vis.around(min(c["Sq"], Sk) // 2 + 1)          # around the diagonal of a middle row
    return sorted({k for k in p if 0 <= k < (min(Sk, c["Sq"]) if c.get("causal") else Sk)})


def logical_mask(c: dict) -> Optional[np.ndarray]:
    """bool, in the mask's own (2 to 4 dim) shape: random at density 0.6, and in every 32-row wave designed rows -- rows 0 and 1
    of the wave with about 8 keys and the last one (a tail wave of one row must show every mutant by itself), 3 without any key,
    7 empty in its first tiles and keys later, 11 keys in the first tile only, 13 exactly one key, the last, 17 and 19 every key
    up to a tile edge (the last and the first).  None: the case has no mask."""
    shape = c.get("mshape")
    if shape is None:
        return None
    Sq, Sk = c["Sq"], c["Sk"]
    rng = np.random.default_rng(c["mseed"])
    m = rng.random(shape) < 0.6
    if shape[-2] == 1 and Sq > 1:            # a key mask in additive form: [B, 1, 1, Sk]
        m[..., Sk - 1] = True
        return m
    j = np.arange(Sk)
    edges = _edges(Sk)
    for r in range(Sq):
        w = r % WAVE
        if w < 2:
            m[..., r, :] = rng.random(shape[:-2] + (Sk,)) < 8.0 / Sk
            m[..., r, Sk - 1] = True
        elif w == 3:
            m[..., r, :] = False
        elif w == 7 and Sk > TILE:
            m[..., r, :] &= j >= min(2 * TILE, TILE * ((Sk - 1) // TILE))
            m[..., r, Sk - 1] = True
        elif w == 11:
            m[..., r, :] &= j < TILE
            m[..., r, 0] = True
        elif w == 13:
            m[..., r, :] = j == Sk - 1
        elif w == 17 and edges:
            m[..., r, :] = j < edges[-1]
        elif w == 19 and edges:
            m[..., r, :] = j < edges[0]
    return m


def _mix(*xs) -> np.ndarray:
    h = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for x in xs:
            h = (h ^ np.asarray(x).astype(np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            h = h ^ (h >> np.uint64(31))
        h = h * np.uint64(0x94D049BB133111EB)
        return h ^ (h >> np.uint64(29))


PROFILES = ("flat", "first", "late", "stairs", "last", "hidden", "diag", "focus")      # the profile of row r is PROFILES[r % 8]


def integer_n(c: dict, m4: np.ndarray) -> np.ndarray:
    """int64 in the 4-dim shape of the mask m4: n[.., r, j] = offset(r) + base + profile (class B).  Every run of 8 rows, so
    every 32-row wave, holds rows of every profile:
        flat     base only (0 .. base-1, hashed)
        first    the maximum in the first tile, falling off
        late     amp on three keys of the last full tile
        stairs   +3 per 32-key tile on two keys of each of the tiles 1 .. 3
        last     amp on the last key, in the ragged tile
        hidden   amp on a key the mask hides (it must not be seen at all)
        diag     amp on the key just above the diagonal (causal cases; it must not be seen at all)
        focus    amp on the first key and on one hashed key of every fourth tile (which fourth by r // 8: the focus rows of a
                 wave cover all four), so that every tile is the main weight of some row
    offset(r) = -12 + 7 r mod (25 - amp) moves the row's integers over -12 .. 12 without changing its weights.  base + profile <= amp:
    the spread of a row stays <= amp (10: P stays normal in fp16)."""
    Sq, Sk = c["Sq"], c["Sk"]
    amp, base = c.get("amp", 10), c.get("base", 3)
    bb = np.arange(m4.shape[0])[:, None, None, None]
    hh = np.arange(m4.shape[1])[None, :, None, None]
    r = np.arange(Sq)[None, None, :, None]
    j = np.arange(Sk)[None, None, None, :]
    n = np.broadcast_to((_mix(bb, hh, r, j, 1) % np.uint64(base)).astype(np.int64), m4.shape[:2] + (Sq, Sk)).copy()
    prof = r % 8
    tile = j // TILE

    def put(where, value):
        np.maximum(n, np.where(where, value, 0), out=n)
    put((prof == 1) & (j < TILE), np.maximum(0, amp - 1 - j // 3))
    lt = max(Sk // TILE - 1, 0)
    put((prof == 2) & (tile == lt) & (j % TILE >= 5) & (j % TILE < 8), amp)
    put((prof == 3) & (tile >= 1) & (tile <= 3) & (j % TILE >= 7) & (j % TILE < 9), 3 * np.minimum(tile, 3))
    put((prof == 4) & (j == Sk - 1), amp)
    put((r % WAVE < 2) & (j == Sk - 1), 4)          # the sparse rows of logical_mask(): a last key that counts
    hidden = ~np.broadcast_to(m4, n.shape)
    first_hidden = hidden & (np.cumsum(hidden & (j >= min(40, Sk - 1)), axis=-1) == 1) & (j >= min(40, Sk - 1))
    put((prof == 5) & first_hidden, amp)
    put((prof == 6) & (j == r + 1), amp)
    t0 = 8 + (_mix(bb, hh, r, tile, 2) % np.uint64(16)).astype(np.int64)
    put((prof == 7) & (tile % 4 == (r // 8) % 4) & ((j % TILE == t0) | (j % TILE == 0)), amp)
    assert n.min() >= 0 and n.max() <= amp
    n += -N_RANGE + (7 * r) % (2 * N_RANGE + 1 - amp)
    assert n.min() >= -N_RANGE and n.max() <= N_RANGE
    return n


# ---- the model of a case ---------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Model:
    c: dict
    logical: Optional[np.ndarray]        # the mask as the caller hands it over: bool, or the float32 bias; None = no mask
    mvis: np.ndarray                     # bool [B, H, Sq, Sk]: what the mask admits (all True without one)
    n: np.ndarray                        # int64 [B, H, Sq, Sk]: the integer that comes with the mask element (0: classes A, C)
    svis: np.ndarray                     # bool [Sq, Sk]: what the shape admits (the causal triangle)
    v: np.ndarray                        # [Sk, D]
    keep: Optional[np.ndarray]           # bool [BH, Sq, Sk], None = no dropout
    cval: float                          # c
    bias: Optional[np.ndarray] = None    # class C: float32 [B, H, Sq, Sk], the finite biases
    seed: int = 0

    @property
    def BH(self):
        return self.c["B"] * self.c["H"]


def _to4(a: np.ndarray) -> np.ndarray:
    return a.reshape((1,) * (4 - a.ndim) + a.shape)


def model(c: dict, seed: Optional[int] = None) -> Model:
    """seed: the dropout seed when it is not the case's own (the fullattn cases draw it from torch's generator)."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    full = (B, H, Sq, Sk)
    lm = logical_mask(c)
    m4 = _to4(lm) if lm is not None else np.ones((1, 1, 1, 1), bool)
    n4 = np.zeros((1, 1, 1, 1), np.int64)
    logical, bias = lm, None
    if c["cls"] in ("B", "DB"):
        n4 = integer_n(c, m4)
        table = np.array([EXACT_BIAS[i] for i in range(-N_RANGE, N_RANGE + 1)], np.float32)
        logical = np.where(np.broadcast_to(m4, n4.shape), table[n4 + N_RANGE], np.float32(-np.inf)).astype(np.float32)
        logical = logical.reshape(n4.shape[4 - lm.ndim:])
    elif c["cls"] == "C":
        rng = np.random.default_rng(c["mseed"] + 1)
        b4 = C_VALUES[rng.integers(0, len(C_VALUES), m4.shape)]
        logical = np.where(m4, b4, np.float32(-np.inf)).astype(np.float32).reshape(lm.shape)
        bias = np.broadcast_to(b4, full)
    elif c.get("mkind") in ("add2", "add32"):
        logical = np.where(lm, np.float32(0), np.float32(-np.inf)).astype(np.float32)
    i, j = np.arange(Sq)[:, None], np.arange(Sk)[None, :]
    svis = (j <= i) if c.get("causal") else np.ones((Sq, Sk), bool)
    p = c.get("p", 0.0)
    seed = c.get("seed", 0) if seed is None else seed
    keep = keep_np(seed, p, B * H, Sq, Sk) if p > 0 else None
    return Model(c, logical, np.broadcast_to(m4, full), np.broadcast_to(n4, full), svis, vis.witness_v(Sk, D, probes_of(c)),
                 keep, keep_scale(p, c["dt"]), bias, seed)


def _flat(a: np.ndarray, m: Model) -> np.ndarray:
    return np.ascontiguousarray(np.broadcast_to(a, (m.c["B"], m.c["H"]) + a.shape[-2:])).reshape(m.BH, *a.shape[-2:])


def finish(m: Model, num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """num [BH, Sq, D] / den [BH, Sq] or [BH, Sq, D]; a zero denominator is the empty row's 0 or NaN."""
    den = den if den.ndim == 3 else den[..., None]
    empty = np.nan if m.c.get("empty_nan") else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), empty)


def reference(m: Model, mvis=None, n=None, svis=None, keep=None, cval=None, v=None, den_keep=False, halves=False,
              extra_key=False, parts=False) -> np.ndarray:
    """float64 [BH, Sq, D] (module docstring).  The arguments replace parts of the model: the mutants of insensitive().
    den_keep: dropout applied to the row sum as well; halves: the two half-wave row sums not combined (the lanes of half hh hold
    the keys with bit 2 of the key index == hh and write the channels with bit 2 of the channel index == hh); extra_key: Sk + 1,
    one more key of score 0 and V = 0 (what the kernel stages past the end), with the mask element of the last key, seen by every
    row the triangle lets; parts: (numerator, denominator) instead of the output."""
    mvis = m.mvis if mvis is None else mvis
    n = m.n if n is None else n
    svis = m.svis if svis is None else svis
    keep = m.keep if keep is None else keep
    cval = m.cval if cval is None else cval
    v = m.v if v is None else v
    seen = _flat(mvis, m) & svis
    if m.bias is not None:
        b = _flat(m.bias, m).astype(np.float64)
        top = np.where(seen, b, -np.inf).max(-1, keepdims=True, initial=-np.inf)
        w = np.where(seen, np.exp(b - np.where(np.isfinite(top), top, 0.0)), 0.0)
    else:
        w = np.where(seen, np.ldexp(1.0, _flat(n, m).astype(np.int64)), 0.0)
    wk = w if keep is None else w * keep
    num = cval * (wk @ v.astype(np.float64))
    if halves:
        odd = (np.arange(w.shape[-1]) // 4) % 2 == 1
        d_odd = (np.arange(v.shape[1]) // 4) % 2 == 1
        den = np.where(d_odd, (w * odd).sum(-1)[..., None], (w * ~odd).sum(-1)[..., None])
    else:
        den = (wk if den_keep else w).sum(-1)
    if extra_key:
        Sq, Sk = m.c["Sq"], m.c["Sk"]
        den = den + w[..., Sk - 1] * (np.arange(Sq) >= Sk if m.c.get("causal") else np.ones(Sq, bool))
    if parts:
        return num, den
    return finish(m, num, den)


def budget(m: Model) -> float:
    """max over rows of sum 2^(n - n_min) over the row's visible keys: below 2^24 (2^13 under dropout) every sum is exact."""
    seen = _flat(m.mvis, m) & m.svis
    n = _flat(m.n, m)
    lo = np.where(seen, n, 99).min(-1, keepdims=True)
    return float(np.where(seen, np.ldexp(1.0, n - lo), 0.0).sum(-1).max())


def spread(m: Model) -> int:
    seen = _flat(m.mvis, m) & m.svis
    n = _flat(m.n, m)
    return int((np.where(seen, n, -99).max(-1) - np.where(seen, n, 99).min(-1))[seen.any(-1)].max(initial=0))


def bound_c(ref: np.ndarray, ulp: float) -> np.ndarray:
    """Class C (derived): visibility's bound plus 0.5 ulp.  P is rounded to the 2-byte type, 2^-9 relative in bf16 and 2^-12 in
    fp16 = ULP / 4; every V is >= 0, so that carries over to the sum.  The fp32 terms (the product with the constant, the
    hardware exp2, the row sum) are <= 1e-5 relative and fit the spare quarter."""
    return 1.5 * ulp * np.abs(ref) + FLOOR * float(np.abs(ref).max())


# ---- the kernel's walk, for the mutants that only a walk has ---------------------------------------------------------------
def walk(m: Model, skip_O=False, skip_l=False, skip_dtile: Optional[int] = None) -> np.ndarray:
    """The online softmax of dense_masked_kernel over 32-key tiles in float64 (exact: powers of two): running maximum m_run,
    alpha = 2^(m_run - m_new) applied to O and to l, l kept in two halves.  skip_*: alpha not applied to O, to l, or to the
    32-channel d-tile skip_dtile of O."""
    seen = _flat(m.mvis, m) & m.svis
    x = np.where(seen, _flat(m.n, m).astype(np.float64), -np.inf)
    BH, Sq, Sk = x.shape
    D = m.v.shape[1]
    keepc = m.cval * (np.ones_like(x) if m.keep is None else m.keep)
    O = np.zeros((BH, Sq, D))
    l = np.zeros((BH, Sq))
    m_run = np.full((BH, Sq), -np.inf)
    with np.errstate(invalid="ignore"):
        for k0 in range(0, Sk, TILE):
            xt = x[..., k0:k0 + TILE]
            m_new = np.maximum(m_run, xt.max(-1))
            none = np.isneginf(m_new)
            alpha = np.where(none | np.isneginf(m_run), np.where(none, 1.0, 0.0), np.exp2(m_run - np.where(none, 0.0, m_new)))
            p = np.where(none[..., None], 0.0, np.exp2(xt - np.where(none, 0.0, m_new)[..., None]))
            l = l * (1.0 if skip_l else alpha) + p.sum(-1)
            m_run = m_new
            a_O = np.broadcast_to((np.ones_like(alpha) if skip_O else alpha)[..., None], O.shape).copy()
            if skip_dtile is not None:
                a_O[..., 32 * skip_dtile:32 * skip_dtile + 32] = 1.0
            O = O * a_O + (p * keepc[..., k0:k0 + TILE]) @ m.v[k0:k0 + TILE].astype(np.float64)
    return finish(m, O, l)


# ---- the mutants -------------------------------------------------------------------------------------------------------------
def _swapped_v(m: Model, bit: int) -> np.ndarray:
    """V with keys j and j ^ bit exchanged: the score side (mask, bias, dropout) of a tile attached to its partner's V.  A
    partner past Sk is the zero row the kernel stages there."""
    Sk = m.c["Sk"]
    j = np.arange(Sk) ^ bit
    return np.where((j < Sk)[:, None], m.v[np.minimum(j, Sk - 1)], 0).astype(np.float32)


def mutants(m: Model):
    """(kind, name, "ref" or "walk", the arguments of reference() / walk() that make the mutant)."""
    c = m.c
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    j = np.arange(Sk)
    # visibility
    if m.logical is not None:             # (a case without a mask has no element to flip: Sk and the diagonal are its limits)
        for p in probes_of(c):
            yield "visibility", f"mask flipped at key {p}", "ref", dict(mvis=m.mvis ^ (j == p))
    yield "visibility", "Sk-1", "ref", dict(svis=m.svis & (j < Sk - 1))
    if m.logical is not None and _to4(m.logical).shape[2] == Sq:
        # (without a row mask no row is short enough for one more key of V = 0 to show: the row-masked cases witness Sk + 1)
        yield "visibility", "Sk+1", "ref", dict(extra_key=True)
    if c.get("causal"):
        i = np.arange(Sq)[:, None]
        for d in (-1, 1):
            yield "visibility", f"diagonal{d:+d}", "ref", dict(svis=j[None, :] <= i + d)
    # mask addressing
    if m.logical is not None:
        shape4 = _to4(m.logical).shape

        def moved(axis, step):
            size = m.mvis.shape[axis]
            idx = np.arange(size) + step
            idx = np.where(idx >= size, idx - 2 * step if axis >= 2 else idx - size, idx)
            return dict(mvis=np.take(m.mvis, idx, axis), n=np.take(m.n, idx, axis))
        for axis, name in ((2, "row"), (0, "batch item"), (1, "head")):
            if shape4[axis] > 1:
                yield "addressing", f"mask of the next {name}", "ref", moved(axis, 1)
        yield "addressing", "mask one key further on", "ref", moved(3, 1)
        if Sk > TILE:
            yield "addressing", "mask one tile further on", "ref", moved(3, TILE)
    # lane-to-key map
    for bit in (4, 8):
        yield "lane map", f"keys j and j ^ {bit} swapped on the score side", "ref", dict(v=_swapped_v(m, bit))
    # rescale (the cases with integer weights: module docstring)
    if c["cls"] in ("B", "DB"):
        yield "rescale", "alpha not applied to O", "walk", dict(skip_O=True)
        yield "rescale", "alpha not applied to l", "walk", dict(skip_l=True)
        yield "rescale", "alpha not applied to d-tile 1", "walk", dict(skip_dtile=1)
    # row sum
    yield "row sum", "half-wave row sums not combined", "ref", dict(halves=True)
    # dropout
    if m.keep is not None and thresh(c["p"]) < 1 << 24:
        p = c["p"]
        yield "dropout", "keyed by (key, row)", "ref", dict(keep=keep_np(m.seed, p, B * H, Sq, Sk, order="key,row"))
        yield "dropout", "keyed without bh", "ref", dict(keep=keep_np(m.seed, p, B * H, Sq, Sk, with_bh=False))
        yield "dropout", "keyed without the seed", "ref", dict(keep=keep_np(0, p, B * H, Sq, Sk))
        yield "dropout", "applied to the row sum as well", "ref", dict(den_keep=True)
        yield "dropout", "keep_scale left out", "ref", dict(cval=1.0)


RULES = ("equivalent in the wave", "only dropped weights touched")


def insensitive(m: Model):
    """-> (missed, exempt, total): for every mutant and every wave (bh, 32 rows) of the case, does the mutant move some element
    of the wave by SENSITIVITY tolerances (or turn a number into NaN or back)?  missed: the (kind, name, bh, block) that do not.
    exempt {(kind, rule): count}, by two rules (RULES):
        equivalent in the wave         the mutant's exact output equals the reference's in the whole wave (it touches no visible
                                       key there, or swaps two keys of equal weight that set the same V channels): no output
                                       could show it
        only dropped weights touched   a visibility mutant under dropout whose exact numerator c (keep o w) @ v is unchanged in
                                       the wave -- every weight it adds or removes there is a dropped one -- so that only row
                                       sums move, by one key among hundreds
    total {kind: count} of triples."""
    base = reference(m)
    if m.bias is None:
        assert np.array_equal(np.nan_to_num(base, nan=-1.0), np.nan_to_num(walk(m), nan=-1.0)), "walk() and reference() differ"
    num0 = reference(m, parts=True)[0]
    tol = tolerance(np.nan_to_num(base), ULP[m.c["dt"]])
    BH, Sq, D = base.shape
    nb = -(-Sq // WAVE)
    pad = nb * WAVE - Sq
    missed, exempt, total = [], {}, {}

    def per_wave(a):
        return np.pad(a, ((0, 0), (0, pad), (0, 0))).reshape(BH, nb, WAVE * D).any(-1)
    for kind, name, fn, kw in mutants(m):
        mut = reference(m, **kw) if fn == "ref" else walk(m, **kw)
        nan_differs = np.isnan(mut) != np.isnan(base)
        with np.errstate(invalid="ignore"):
            diff = np.abs(np.nan_to_num(mut, posinf=1e30) - np.nan_to_num(base))
        same = ~per_wave((diff != 0) | nan_differs)
        hit = per_wave((diff >= SENSITIVITY * tol) | nan_differs)
        dropped = np.zeros_like(same)
        if kind == "visibility" and m.keep is not None:
            dropped = ~per_wave(reference(m, parts=True, **kw)[0] != num0) & ~same
        total[kind] = total.get(kind, 0) + BH * nb
        for rule, where in zip(RULES, (same, dropped & ~hit)):
            exempt[kind, rule] = exempt.get((kind, rule), 0) + int(where.sum())
        for bh, blk in np.argwhere(~hit & ~same & ~dropped):
            missed.append((kind, name, int(bh), int(blk)))
    return missed, exempt, total


# ---- the case tables -------------------------------------------------------------------------------------------------------
def _case(cls, idx, D, dt, Sq, Sk, entry="masked", B=2, H=3, **kw):
    kw.setdefault("empty_nan", bool(idx % 2))
    if kw.get("mshape") is not None:
        kw.setdefault("mseed", 1000 + 17 * idx + Sq + Sk)
        kw.setdefault("mem", "contig")
    tags = [cls, f"D{D}", dt, f"{Sq}x{Sk}", entry]
    if kw.get("mshape") is not None:
        tags += [kw["mkind"], "x".join(str(s) for s in kw["mshape"]), kw["mem"]]
    tags += [t for t, on in (("causal", kw.get("causal")), ("bshd", kw.get("bshd")), ("nan", kw["empty_nan"])) if on]
    if "p" in kw:
        tags.append(f"p{kw['p']}")
    if "mode" in kw:
        tags.append(kw["mode"])
    return dict(id="-".join(tags), cls=cls, D=D, dt=dt, Sq=Sq, Sk=Sk, B=B, H=H, entry=entry, **kw)


def _cases() -> List[dict]:
    B, H = 2, 3
    out = []
    idx = 0

    def add(cls, D, dt, Sq, Sk, **kw):
        nonlocal idx
        out.append(_case(cls, idx, D, dt, Sq, Sk, **kw))
        idx += 1
    # ---- A: visibility.  Every mask form at all four (D, type) on the ragged main shape
    Sq, Sk = 200, 333
    main = [("bool", (B, 1, Sq, Sk), "contig"), ("bool", (1, H, Sq, Sk), "transpose"), ("bool", (B, H, Sq, Sk), "slice"),
            ("bool", (1, 1, Sq, Sk), "contig"), ("bool", (Sq, Sk), "transpose"), ("bool", (B, 1, Sq, Sk), "expand"),
            ("add2", (B, H, Sq, Sk), "contig"), ("add32", (1, 1, Sq, Sk), "slice"), ("add2", (B, 1, 1, Sk), "contig"),
            ("add32", (B, 1, Sq, Sk), "transpose"), ("add2", (Sq, Sk), "expand")]
    for D, dt in FORMS:
        for kind, shape, mem in main:
            add("A", D, dt, Sq, Sk, mkind=kind, mshape=shape, mem=mem)
        add("A", D, dt, Sq, Sk, mkind="bool", mshape=(B, H, Sq, Sk), bshd=True)
    # ... the other shapes, the forms by turns
    for i, (Sq, Sk) in enumerate(s for s in SHAPES if s != (200, 333)):
        D, dt = FORMS[i % 4]
        add("A", D, dt, Sq, Sk, mkind="bool", mshape=(B, H, Sq, Sk), mem="slice")
        D, dt = FORMS[(i + 1) % 4]
        add("A", D, dt, Sq, Sk, mkind="add32", mshape=(1, H, Sq, Sk), mem="transpose")
    # ... causal, through the dropout entry at rate 0: Sq == Sk, Sq < Sk, Sq > Sk
    for D, dt in FORMS:
        for Sq, Sk in ((257, 257), (130, 300), (300, 130)):
            add("A", D, dt, Sq, Sk, entry="dropout", causal=True, p=0.0)
    for i, (Sq, Sk) in enumerate(((33, 31), (1, 129), (129, 32), (1, 1))):
        D, dt = FORMS[i % 4]
        add("A", D, dt, Sq, Sk, entry="dropout", causal=True, p=0.0)
    for D, dt in FORMS[1:3]:
        add("A", D, dt, 130, 300, entry="dropout", causal=True, p=0.0, mkind="bool", mshape=(B, 1, 130, 300))
    # ... fullattn's routing, on the smallest shape with more than one tile edge to miss
    for i, mode in enumerate(("torch", "vanilla")):
        D, dt = FORMS[i + 1]
        add("A", D, dt, 33, 31, entry="fullattn", mode=mode, empty_nan=mode == "vanilla", mkind="bool", mshape=(B, H, 33, 31))
        add("A", D, dt, 33, 31, entry="fullattn", mode=mode, empty_nan=mode == "vanilla", mkind="add2", mshape=(33, 31))
    # ---- B: integer weights through the float32 mask kind
    for D, dt in FORMS:
        add("B", D, dt, 200, 333, mkind="add32", mshape=(B, H, 200, 333))
        add("B", D, dt, 130, 300, entry="dropout", p=0.0, mkind="add32", mshape=(1, H, 130, 300), mem="slice")
        add("B", D, dt, 257, 257, entry="dropout", p=0.0, causal=True, mkind="add32", mshape=(1, 1, 257, 257))
        add("B", D, dt, 300, 130, mkind="add32", mshape=(B, 1, 300, 130), mem="transpose")
    for i, (Sq, Sk) in enumerate(((33, 31), (1, 129), (129, 32))):
        D, dt = FORMS[(i + 2) % 4]
        add("B", D, dt, Sq, Sk, mkind="add32", mshape=(B, H, Sq, Sk))
    # ---- C: 2-byte additive masks with finite values
    for D, dt in FORMS:
        add("C", D, dt, 200, 333, mkind="add2", mshape=(B, H, 200, 333), empty_nan=False)
        add("C", D, dt, 130, 300, mkind="add2", mshape=(1, 1, 130, 300), mem="slice", empty_nan=False)
    # ---- D: dropout
    rates = (0.5, 0.75, 0.25)
    for i, (D, dt) in enumerate(FORMS):
        for p in rates:
            add("D", D, dt, 200, 333, entry="dropout", p=p, seed=0x1234567 + 977 * idx)
        add("D", D, dt, 130, 300, entry="dropout", p=rates[i % 3], seed=(1 << 61) + idx, mkind="bool", mshape=(B, 1, 130, 300))
        add("D", D, dt, 130, 300, entry="dropout", p=rates[(i + 1) % 3], seed=31 * idx, causal=True)
        add("D", D, dt, 300, 130, entry="dropout", p=rates[(i + 2) % 3], seed=(1 << 40) + idx, causal=True)
        add("DB", D, dt, 200, 333, entry="dropout", p=rates[(i + 2) % 3], seed=7 + idx, mkind="add32", mshape=(B, H, 200, 333),
            amp=9, base=2)
    add("D", 64, "bf16", 130, 300, entry="dropout", p=1.0, seed=5)
    add("D", 128, "fp16", 33, 31, entry="dropout", p=1.0, seed=6, mkind="bool", mshape=(B, H, 33, 31), empty_nan=False)
    add("D", 128, "bf16", 130, 300, entry="dropout", p=0.0, seed=5)
    add("D", 64, "fp16", 130, 300, entry="dropout", p=0.0, seed=6, mkind="bool", mshape=(B, H, 130, 300), same_as_masked=True)
    for i, mode in enumerate(("torch", "vanilla")):
        D, dt = FORMS[2 * i + (1 - i)]          # (64, fp16), (128, bf16)
        add("D", D, dt, 33, 31, entry="fullattn", mode=mode, empty_nan=mode == "vanilla", p=0.5, torch_seed=1234 + i, seed=991 + i,
            mkind="bool", mshape=(B, 1, 33, 31))
    return out


CASE_LIST = _cases()
CASES: Dict[str, dict] = {c["id"]: c for c in CASE_LIST}
assert len(CASES) == len(CASE_LIST), "case ids collide"
EXACT_CLASSES = ("A", "B", "D", "DB")


def by_class(*classes) -> List[str]:
    return [c["id"] for c in CASE_LIST if c["cls"] in classes]


@functools.lru_cache(maxsize=8)
def cached_model(cid: str) -> Model:
    return model(CASES[cid])
