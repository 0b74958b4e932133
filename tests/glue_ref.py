"""References and case tables for the producers either side of the path (csrc/rsa_glue.hip): permute_tokens, qk_norm_rope
(RMSNorm and LayerNorm forms), norm_rope_across_heads and rel_l1.  The models are numpy on the CPU; the torch functions at the
end restate the module calls the kernels replace (CPU tensors) for tests/test_glue_ref_cpu.py and for the statistics of
tests/test_gpu_glue_exact.py.

The interval reference of the norm + RoPE kernels
-------------------------------------------------
The kernels' comments state the chain operation by operation, and the file is built with -ffp-contract=off, so every step
but two is a pure function of its inputs: exact widening of the 2-byte input; n = fl32(v * r); rounding to the storage type;
fl32(n * w) and a second rounding; the RoPE products and sums, each rounded to fp32 (rope_kind 1: fp64 products and
difference, then (float), then the storage type).  The two free steps are the fp32 sum behind r (and behind LayerNorm's mean)
and rsqrtf.  So r is taken as an interval r_true * (1 +- delta), r_true in float64 from the exactly widened inputs, rounded
OUTWARD to fp32, and the chain is evaluated at its ends: every later step is monotone in each argument, so a normalised
element lies between the two end results and a rotated element inside the hull over the four corners of its pair.  The
assertion is lo <= got <= hi per element, in fp32 (-0 equals 0, NaN fails); where lo == hi the kernel must give that value.

delta (u = 2^-24, the unit roundoff of fp32; all summands are non-negative, so relative errors add and never amplify):
  per-head RMSNorm   v*v rounded: 1u.  A summand passes through 8 sequential adds in its lane and log2(D/8) <= 4 shuffle
                     levels: <= 12u.  * (1/D) is exact (a power of two); + eps: 1u.  The argument of rsqrt is off by <= 14u,
                     x^(-1/2) halves that: 7u.  rsqrtf within 1 ulp of the true value: <= 2u.  Total 9u; DELTA_HEAD = 16u =
                     2^-20, about twice the count.
  across heads       8 * nch sequential adds (nch = ceil(C / 512) chunks per lane; the padded chunks add exact zeros) and 6
                     shuffle levels, the rounded square, the division by C (correctly rounded: 1u) and + eps:
                     (8 nch + 9)u, halved, + 2u for rsqrtf = (4 nch + 6.5)u; delta_across(nch) = (4 nch + 7)u, the bound
                     itself -- 71u = 2^-17.85 at the widest row (nch = 16).
  LayerNorm          mean: the errors of one level of adds cover disjoint sets of summands, so each of the 8 + log2(D/8)
                     levels contributes <= u * sum|v|: |mean - mean_true| <= depth * u * mean|v| (/ D is exact).  rstd:
                     fl32(v - mean) 1u, squared 2u, the rounded square 1u, 12u of adds, + eps 1u: 16u, halved, + 2u = 10u;
                     DELTA_HEAD again.  The mean's error e enters the variance exactly as + e^2 (the cross term vanishes),
                     which widens the lower end of rstd explicitly.  Corners over (mean, rstd), one rounding.
All of this supposes rsqrtf within 1 ulp on the device and fp32 denormals kept (the default of the HIP toolchain).

rel_l1: a and b hold only -1, 0, 1, so both sums are integers below 2^24 in any order and the device must return the count.
permute_tokens: a counter viewed as the 2-byte type (NaN payloads, -0 and subnormals among it), compared bit for bit.
"""
import functools
import itertools

import numpy as np

U = 2.0 ** -24
DELTA_HEAD = 2.0 ** -20
CAP_HEAD_RMS, CAP_WIDE = 0.01, 0.05       # largest share of elements with lo != hi a case may have
FILL = 0x5A3C                              # what a mutant that leaves elements unwritten leaves there (the pre-fill)


def delta_across(nch):
    return (4 * nch + 7) * U


# ---- number formats -----------------------------------------------------------------------------------------------
def widen(bits, dt):
    """uint16 -> the float32 holding the same value"""
    bits = np.ascontiguousarray(bits, np.uint16)
    if dt == "bf16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def to_bits(x, dt):
    """float32 -> uint16 of the storage type, round to nearest even (no NaN handling: the norm cases hold none)"""
    x = np.ascontiguousarray(x, np.float32)
    if dt == "bf16":
        u = x.view(np.uint32)
        return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    with np.errstate(over="ignore"):
        return x.astype(np.float16).view(np.uint16)


def rnd(x, dt):
    """float32 -> float32 holding the storage-type rounding of x"""
    return widen(to_bits(x, dt), dt)


def f32_down(x):
    y = np.asarray(x, np.float64).astype(np.float32)
    return np.where(y.astype(np.float64) > x, np.nextafter(y, np.float32(-np.inf)), y).astype(np.float32)


def f32_up(x):
    y = np.asarray(x, np.float64).astype(np.float32)
    return np.where(y.astype(np.float64) < x, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


# ---- hashed inputs ------------------------------------------------------------------------------------------------
def hashed(seed, n):
    """n 64-bit hashes of (seed, index): splitmix64's finaliser"""
    x = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15 + 0x1234567) % 2 ** 64)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def uniform(seed, n):
    return ((hashed(seed, n) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normal(seed, shape):
    n = int(np.prod(shape))
    return (np.sqrt(-2.0 * np.log(uniform(2 * seed + 1, n))) * np.cos(2 * np.pi * uniform(2 * seed + 2, n))).reshape(shape)


def pick(k, salt, seq):
    return seq[int(hashed(k * 64 + salt, 1)[0] % np.uint64(len(seq)))]


EDGE_KINDS = ("zero", "one_nonzero", "max_finite", "eps_scale", "subnormal", "neg_zero")


def plant_edge_rows(rows, dt, seed):
    """rows float64 [R, L] -> (rows with every fifth one (4, 9, ...) replaced by an edge row, kind per row (-1: none)).
    max_finite is +-65504 in fp16; in bf16 +-2^50, whose 8192 squares (the widest row) still sum in fp32."""
    R, L = rows.shape
    kinds = np.full(R, -1)
    sign = np.where(hashed(seed + 77, R * L).reshape(R, L) & np.uint64(1), -1.0, 1.0)
    for n, j in enumerate(range(4, R, 5)):
        kind = n % len(EDGE_KINDS)
        kinds[j] = kind
        if kind == 0:
            rows[j] = 0.0
        elif kind == 1:
            rows[j] = 0.0
            rows[j, (7 * j + 3) % L] = -1.5
        elif kind == 2:
            rows[j] = sign[j] * (65504.0 if dt == "fp16" else 2.0 ** 50)
        elif kind == 3:
            rows[j] = rows[j] * (1e-3 / 1.7)
        elif kind == 4:
            tiny, top = (2.0 ** -24, 1023) if dt == "fp16" else (2.0 ** -133, 127)
            rows[j] = sign[j] * tiny * (1 + (hashed(seed + 78, L) % np.uint64(top)).astype(np.float64))
        else:
            rows[j, ::3] = -0.0
    return rows, kinds


# ---- the models ---------------------------------------------------------------------------------------------------
def _r_interval(arg_lo, arg_hi, delta):
    """fp32 interval of rsqrt over an exact argument in [arg_lo, arg_hi] (float64) computed to relative delta"""
    with np.errstate(divide="ignore"):
        return f32_down((1 - delta) / np.sqrt(arg_hi)), f32_up((1 + delta) / np.sqrt(arg_lo))


def _rms_chain(v, r, w, dt, mut):
    with np.errstate(invalid="ignore", over="ignore"):
        n = v * r
        if w is not None:
            if mut != "no_preround":
                n = rnd(n, dt)
            n = n * w
        return rnd(n, dt)


def _hull(parts):
    lo, hi = parts[0], parts[0]
    for p in parts[1:]:
        lo, hi = np.minimum(lo, p), np.maximum(hi, p)
    bad = np.zeros(lo.shape, bool)
    for p in parts:
        bad |= np.isnan(p)
    return np.where(bad, np.float32(np.nan), lo), np.where(bad, np.float32(np.nan), hi)


def _rms(v, var, eps, delta, w, dt, mut):
    """v float32 [..., L]; var float64 [..., 1], the exact mean of squares the row is divided by"""
    e = 0.0 if mut == "no_eps" else float(np.float32(eps))
    rlo, rhi = _r_interval(var + e, var + e, delta)
    if w is not None and mut == "w_nbr":
        w = np.roll(w, 1)
    return _hull([_rms_chain(v, rlo, w, dt, mut), _rms_chain(v, rhi, w, dt, mut)])


def _layernorm(v, eps, w, b, dt, mut):
    D = v.shape[-1]
    v64 = v.astype(np.float64)
    mean = v64.mean(-1, keepdims=True)
    depth = 8 + int(np.log2(D // 8))
    em = depth * U * np.abs(v64).mean(-1, keepdims=True)
    mlo, mhi = f32_down(mean - em), f32_up(mean + em)
    var = ((v64 - mean) ** 2).sum(-1, keepdims=True) / (D - 1 if mut == "ln_unbiased" else D)
    e = 0.0 if mut == "no_eps" else float(np.float32(eps))
    rlo, rhi = _r_interval(var + e, var + em * em + e, DELTA_HEAD)
    if w is not None and mut == "w_nbr":
        w = np.roll(w, 1)
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for m in (mlo, mhi):
            for r in (rlo, rhi):
                n = (v - m) * r
                if mut == "bias_first" and w is not None and b is not None:
                    n = (n + b) * w
                else:
                    if w is not None:
                        n = n * w
                    if b is not None:
                        n = n + b
                parts.append(rnd(n, dt))
    return _hull(parts)


def _rotate(lo, hi, cos, sin, dt, wide, mut):
    """out[j] = fl(fl(x[j] * cos[j]) + fl(sg[j] * x[j ^ 1] * sin[j])), sg = -1 on even j; x [B, S, H, D], cos / sin
    [S, D] already expanded per channel; wide: float64 arithmetic, then (float).  Hull over the four corners."""
    D = lo.shape[-1]
    j = np.arange(D)
    partner, sg = j ^ 1, np.where(j % 2 == 0, -1.0, 1.0)
    if mut == "pair_half":
        partner, sg = (j + D // 2) % D, np.where(j < D // 2, -1.0, 1.0)
    if mut == "rot_sign":
        sg = -sg
    if mut == "cos_sin_swap":
        cos, sin = sin, cos
    if mut == "cos_nbr":
        cos = np.roll(cos, 1, axis=-1)
    if mut == "sin_nbr":
        sin = np.roll(sin, 1, axis=-1)
    if mut in ("tok_prev", "tok_next"):
        cos, sin = (np.roll(t, 1 if mut == "tok_prev" else -1, axis=0) for t in (cos, sin))
    ft = np.float64 if wide and mut != "rope1_fp32" else np.float32
    cos, sin = cos.astype(ft)[None, :, None, :], (sin.astype(ft) * sg.astype(ft))[None, :, None, :]
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in (lo, hi):
            for b in (lo, hi):
                o = a.astype(ft) * cos + b[..., partner].astype(ft) * sin
                parts.append(rnd(o.astype(np.float32), dt))
    return _hull(parts)


def qk_model(x, dt, norm=None, rope=None, s_rope=0, mut=None):
    """The per-head kernel.  x uint16 [B, S, H, D]; norm None | ("rms", w, eps) | ("ln", w, b, eps), w / b float32 [D] or
    None; rope None | (cos, sin) float32 [S, D]; tokens < s_rope are rotated.  -> lo, hi float32 [B, S, H, D]."""
    B, S, H, D = x.shape
    if mut == "head_next":
        x = np.roll(x, -1, axis=2)
    if mut == "group_prev":
        x = np.concatenate([x[:, :, :8], x[:, :, :H - 8]], axis=2)
    v = widen(x, dt)
    if norm is None:
        lo = hi = rnd(v, dt)
    elif norm[0] == "rms":
        v64 = v.astype(np.float64)
        var = (v64 * v64).mean(-1, keepdims=True)
        if mut == "var_other":
            var = np.broadcast_to((v64 * v64).mean((-2, -1), keepdims=True), var.shape)
        lo, hi = _rms(v, var, norm[2], DELTA_HEAD, norm[1], dt, mut)
    else:
        lo, hi = _layernorm(v, norm[3], norm[1], norm[2], dt, mut)
    if rope is not None:
        n_rot = s_rope + (mut == "rope_extra") - (mut == "rope_short")
        rlo, rhi = _rotate(lo, hi, rope[0][:S], rope[1][:S], dt, False, mut)
        rot = (np.arange(S) < n_rot)[None, :, None, None]
        lo, hi = np.where(rot, rlo, lo), np.where(rot, rhi, hi)
    if mut == "last_group":
        lo, hi = lo.copy(), hi.copy()
        lo[:, :, 8 * ((H - 1) // 8):] = hi[:, :, 8 * ((H - 1) // 8):] = widen(np.uint16(FILL), dt)
    return lo, hi


def across_model(x, dt, H, norm=None, kind=0, tables=None, mut=None):
    """The across-heads kernel.  x uint16 [B, S, H * D]; norm None | (w float32 [C] | None, eps); kind 0 none, 1 tables =
    complex128 [S, D / 2], 2 tables = (cos, sin) float32 [S, D] with cos of pair p at [2p] and sin at [2p + 1].
    -> lo, hi float32 [B, S, H, D]."""
    B, S, C = x.shape
    D = C // H
    v = widen(x, dt)
    if mut == "head_next":
        v = np.roll(v.reshape(B, S, H, D), -1, axis=2).reshape(B, S, C)
    if norm is None:
        lo = hi = rnd(v, dt)
    else:
        v64 = v.astype(np.float64)
        var = (v64 * v64).mean(-1, keepdims=True)
        if mut == "var_other":
            var = np.repeat((v64 * v64).reshape(B, S, H, D).mean(-1), D, axis=-1)
        lo, hi = _rms(v, var, norm[1], delta_across(-(-C // 512)), norm[0], dt, mut)
    lo, hi = lo.reshape(B, S, H, D), hi.reshape(B, S, H, D)
    if kind == 1:
        cos, sin = np.repeat(tables.real, 2, axis=1), np.repeat(tables.imag, 2, axis=1)
        lo, hi = _rotate(lo, hi, cos, sin, dt, True, mut)
    elif kind == 2:
        cos, sin = np.repeat(tables[0][:, 0::2], 2, axis=1), np.repeat(tables[1][:, 1::2], 2, axis=1)
        lo, hi = _rotate(lo, hi, cos, sin, dt, False, mut)
    return lo, hi


def ambiguous_share(lo, hi):
    return float(np.mean(lo != hi))


def inside(got, lo, hi):
    """bool per element: lo <= got <= hi in fp32 (NaN on either side is outside)"""
    return (lo <= got) & (got <= hi)


def escapes(mlo, mhi, lo, hi):
    """True if a mutant's whole interval lies outside the reference's on some element: a kernel that computed the mutant
    could not pass."""
    with np.errstate(invalid="ignore"):
        return bool(np.any((mhi < lo) | (mlo > hi) | np.isnan(mlo) | np.isnan(mhi)))


# ---- tables and inputs shared by the norm + RoPE cases ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(D):
    import helpers
    cos, sin = helpers.rope_tables(4096, D)
    fr = helpers.wan_freqs(4096, D)[0, 0]
    c22, s22 = helpers.wan22_rope(4096, D)
    return cos.numpy(), sin.numpy(), fr.numpy(), c22[0, :, 0].numpy(), s22[0, :, 0].numpy()


def _positions(seed, S):
    return (1 + hashed(seed, S) % np.uint64(4095)).astype(np.int64)      # never position 0: no identity rotation


def head_tables(seed, S, D):
    """(cos, sin) float32 [S, D] in the interleaved-pair convention: helpers.rope_tables rows at hashed positions, the odd
    channels from a second set of positions so that every channel of a token has its own cos and sin"""
    cos, sin = _tables(D)[:2]
    p0, p1 = _positions(seed, S), _positions(seed + 1, S)
    c, s = cos[p0].copy(), sin[p0].copy()
    c[:, 1::2], s[:, 1::2] = cos[p1][:, 1::2], sin[p1][:, 1::2]
    return c, s


def wan21_table(seed, S, D):
    """complex128 [S, D / 2]: helpers.wan_freqs rows at hashed positions.  Pair 0 of token 0 is built so that an fp32
    rotation of x = (1, 1) rounds to another 2-byte value than the fp64 one in both storage types: 1 + 2^-8 + 0.8 * 2^-23
    becomes 1 + 2^-8 + 2^-23 as a float (above the bf16 tie), while fp32 products give 1 + 2^-8 (the tie, to even);
    fp16 has the same tie three bits lower."""
    fr = _tables(D)[2][_positions(seed, S)].copy()
    return fr


def craft_rope1(fr, x, dt):
    """plant the fp32-versus-fp64 witness of wan21_table's docstring at token 0, head 0, pair 0 of batch 0 (x [B, S, C])"""
    t = 2.0 ** (-8 if dt == "bf16" else -11)
    fr[0, 0] = complex(1 + t + 0.4 * 2.0 ** -23, -0.4 * 2.0 ** -23)
    x[0, 0, 0:2] = to_bits(np.array([1.0, 1.0], np.float32), dt)


def wan22_tables(seed, S, D):
    """(cos, sin) float32 [S, D] as Wan2.2 hands them over, at hashed positions; the entries the rotation never reads
    (cos at odd channels, sin at even ones) are moved away so that reading them shows"""
    _, _, _, c, s = _tables(D)
    p = _positions(seed, S)
    c, s = c[p].copy(), s[p].copy()
    c[:, 1::2] += 0.25
    s[:, 0::2] -= 0.25
    return c, s


def _weights(lo_, hi_, n, dt):
    return rnd(np.linspace(lo_, hi_, n, dtype=np.float32), dt)      # representable, so a 2-byte module holds them


# ---- qk_norm_rope cases -----------------------------------------------------------------------------------------
QK_H, QK_S = (1, 3, 8, 9, 16, 24, 30), (1, 15, 16, 17, 33)
QK_NORMS = {"rms": ("rms_w", "rms_w", "rms_now", "none"), "ln": ("ln_wb", "ln_w", "ln_b", "ln_plain")}
QK_LAYOUTS = ("contig", "q", "k", "v", "bstride")


@functools.lru_cache(maxsize=None)
def qk_cases():
    """dicts: id, B, S, H, D, dt, norm (a name of QK_NORMS), rope (bool), s_rope, layout, concat (bool), seed"""
    out = []
    for i, (H, S) in enumerate(itertools.product(QK_H, QK_S)):
        for f, fam in enumerate(("rms", "ln")):
            k = 2 * i + f
            c = dict(B=2, S=S, H=H, seed=1000 + k, D=(64, 128)[(i + f) % 2], dt=("bf16", "fp16")[(i // 2 + f) % 2],
                     norm=QK_NORMS[fam][(i + i // 4) % 4], rope=pick(k, 1, (True, True, False)),
                     layout=QK_LAYOUTS[(i + 2 * f) % 5], concat=bool((i // 3 + f) % 2))
            c["s_rope"] = (0, 1, S - 1, S)[(i + i // 5 + f) % 4]
            out.append(c)
    # the production head counts with everything on, and the plain strided copy at a ragged last group
    out.append(dict(B=2, S=33, H=24, seed=1900, D=128, dt="bf16", norm="rms_w", rope=True, layout="q", concat=True, s_rope=32))
    out.append(dict(B=2, S=17, H=30, seed=1901, D=64, dt="bf16", norm="ln_wb", rope=True, layout="k", concat=True, s_rope=16))
    out.append(dict(B=2, S=17, H=30, seed=1902, D=128, dt="fp16", norm="rms_w", rope=True, layout="v", concat=False, s_rope=17))
    out.append(dict(B=2, S=16, H=9, seed=1903, D=64, dt="fp16", norm="none", rope=False, layout="bstride", concat=True, s_rope=0))
    for c in out:
        c["id"] = "H{H}-S{S}-D{D}-{dt}-{norm}-{r}-{layout}{cc}".format(
            r="rope%d" % c["s_rope"] if c["rope"] else "norope", cc="-concat" if c["concat"] else "", **c)
    assert len({c["id"] for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def qk_inputs(cid):
    """-> dict: x uint16 [B, S, H, D], norm / rope as qk_model takes them, kinds (edge kind per row of x.reshape(-1, D))"""
    c = next(c for c in qk_cases() if c["id"] == cid)
    B, S, H, D, dt = c["B"], c["S"], c["H"], c["D"], c["dt"]
    rows = normal(c["seed"], (B * S * H, D)) * 1.7
    if c["norm"].startswith("ln"):
        rows += 0.3
    rows, kinds = plant_edge_rows(rows, dt, c["seed"])
    x = to_bits(rows.astype(np.float32), dt).reshape(B, S, H, D)
    w, b = _weights(0.8, 1.2, D, dt), _weights(-0.2, 0.2, D, dt)
    norm = {"none": None, "rms_w": ("rms", w, 1e-6), "rms_now": ("rms", None, 1e-6), "ln_wb": ("ln", w, b, 1e-6),
            "ln_w": ("ln", w, None, 1e-6), "ln_b": ("ln", None, b, 1e-5), "ln_plain": ("ln", None, None, 1e-5)}[c["norm"]]
    rope = head_tables(c["seed"], S, D) if c["rope"] else None
    return dict(x=x, norm=norm, rope=rope, kinds=kinds)


def qk_reference(cid, mut=None):
    c = next(c for c in qk_cases() if c["id"] == cid)
    i = qk_inputs(cid)
    return qk_model(i["x"], c["dt"], i["norm"], i["rope"], c["s_rope"], mut)


QK_MUTANTS = ("w_nbr", "cos_nbr", "sin_nbr", "cos_sin_swap", "rot_sign", "pair_half", "tok_prev", "tok_next", "rope_extra",
              "rope_short", "head_next", "group_prev", "last_group", "no_eps", "no_preround", "var_other", "ln_unbiased",
              "bias_first")


def qk_mutant_rule(c, kinds, mut):
    """None if the case can hold the mutant, else the rule that exempts it"""
    norm, rot = c["norm"], c["rope"] and c["s_rope"] > 0
    if mut in ("cos_nbr", "sin_nbr", "cos_sin_swap", "rot_sign", "pair_half") and not rot:
        return "rope mutants need a rotated token"
    if mut in ("tok_prev", "tok_next") and not (rot and c["S"] >= 2):
        return "a neighbouring table row needs rotation and two tokens"
    if mut == "rope_extra" and not (c["rope"] and c["s_rope"] < c["S"]):
        return "rotating token S_rope needs tables and S_rope < S"
    if mut == "rope_short" and not rot:
        return "rope mutants need a rotated token"
    if mut == "w_nbr" and norm not in ("rms_w", "ln_wb", "ln_w"):
        return "weight mutants need a weight"
    if mut == "no_preround" and norm != "rms_w":
        return "the rounding before the weight exists only in RMSNorm with a weight"
    if mut == "head_next" and c["H"] < 2:
        return "head mutants need two heads"
    if mut in ("group_prev", "last_group") and c["H"] <= 8:
        return "group mutants need a second head group"
    if mut == "no_eps" and (norm == "none" or not np.isin(kinds, (0, 3, 4)).any()):
        return "eps shows only on a zero, eps-scale or subnormal row of a normalised case"
    if mut == "var_other" and (not norm.startswith("rms") or c["H"] < 2):
        return "the variance over H*D needs RMSNorm and two heads"
    if mut == "ln_unbiased" and not norm.startswith("ln"):
        return "the unbiased variance needs LayerNorm"
    if mut == "bias_first" and norm != "ln_wb":
        return "bias before weight needs both"
    return None


# ---- norm_rope_across_heads cases -------------------------------------------------------------------------------------
# (H, D): ceil(H * D / 512) = 1, 3, 4, 6, 7, 10, 11, 16 (the kernel is instantiated for 3, 6, 10 and 16 chunks per lane)
AH_SHAPES = ((3, 64), (10, 128), (16, 128), (24, 128), (26, 128), (40, 128), (42, 128), (64, 128), (5, 32), (5, 256),
             (20, 64))
AH_S = (1, 3, 4, 5, 9)


@functools.lru_cache(maxsize=None)
def across_cases():
    """dicts: id, B, S, H, D, dt, norm ("w", "now", "none"), kind, layout ("contig", "cols", "bstride"), seed"""
    out = []
    for i, (H, D) in enumerate(AH_SHAPES):
        for f in range(2):
            k = 2 * i + f
            out.append(dict(B=2, S=AH_S[(i + 2 * f) % 5], H=H, D=D, seed=3000 + k, kind=(k + i // 3) % 3,
                            dt=("bf16", "fp16")[(i + f) % 2],
                            norm=("w", "now", "w", "none")[(i + 3 * f) % 4], layout=("contig", "cols", "bstride")[k % 3]))
    for c in out:
        c["id"] = "H{H}-D{D}-S{S}-{dt}-{norm}-kind{kind}-{layout}".format(**c)
    assert len({c["id"] for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def across_inputs(cid):
    c = next(c for c in across_cases() if c["id"] == cid)
    B, S, H, D, dt = c["B"], c["S"], c["H"], c["D"], c["dt"]
    C = H * D
    rows, kinds = plant_edge_rows(normal(c["seed"], (B * S, C)) * 1.3, dt, c["seed"])
    x = to_bits(rows.astype(np.float32), dt).reshape(B, S, C)
    norm = {"none": None, "w": (_weights(0.8, 1.2, C, dt), 1e-6), "now": (None, 1e-6)}[c["norm"]]
    tables = None
    if c["kind"] == 1:
        tables = wan21_table(c["seed"], S, D)
        if norm is None:
            craft_rope1(tables, x, dt)
    elif c["kind"] == 2:
        tables = wan22_tables(c["seed"], S, D)
    return dict(x=x, norm=norm, tables=tables, kinds=kinds)


def across_reference(cid, mut=None):
    c = next(c for c in across_cases() if c["id"] == cid)
    i = across_inputs(cid)
    return across_model(i["x"], c["dt"], c["H"], i["norm"], c["kind"], i["tables"], mut)


AH_MUTANTS = ("w_nbr", "cos_nbr", "sin_nbr", "cos_sin_swap", "rot_sign", "pair_half", "tok_prev", "tok_next", "head_next",
              "no_eps", "no_preround", "var_other", "rope1_fp32")


def across_mutant_rule(c, kinds, mut):
    if mut in ("cos_nbr", "sin_nbr", "cos_sin_swap", "rot_sign", "pair_half") and c["kind"] == 0:
        return "rope mutants need a rotation"
    if mut in ("tok_prev", "tok_next") and (c["kind"] == 0 or c["S"] < 2):
        return "a neighbouring table row needs rotation and two tokens"
    if mut in ("w_nbr", "no_preround") and c["norm"] != "w":
        return "weight mutants need a weight"
    if mut == "no_eps" and (c["norm"] == "none" or not np.isin(kinds, (0, 3, 4)).any()):
        return "eps shows only on a zero, eps-scale or subnormal row of a normalised case"
    if mut == "var_other" and c["norm"] == "none":
        return "the variance needs a norm"
    if mut == "rope1_fp32" and not (c["kind"] == 1 and c["norm"] == "none"):
        return "fp32 and fp64 rotations round alike but on about 2^-16 of the elements: held where the built pair is exact"
    return None


# ---- permute_tokens ---------------------------------------------------------------------------------------------------
PERMUTE_C = (8, 504, 512, 520, 2040, 2048, 2056, 3072, 5120)
PERMUTE_N = (1, 2, 3, 5, 9)


@functools.lru_cache(maxsize=None)
def permute_cases():
    """dicts: id, B, S (source rows), C, n (= len(order)), dt, idx ("int64" | "int32"), layout, seed"""
    out = []
    for i, C in enumerate(PERMUTE_C):
        for f in range(2):
            k = 2 * i + f
            out.append(dict(B=2, S=7, C=C, n=PERMUTE_N[(i + 3 * f) % 5], dt=("bf16", "fp16")[(i + f) % 2],
                            idx=("int64", "int32")[(i // 2 + f) % 2], layout=("contig", "cols", "bstride")[k % 3], seed=5000 + k))
    for c in out:
        c["id"] = "C{C}-n{n}-{dt}-{idx}-{layout}".format(**c)
    return out


def permute_inputs(c):
    """x uint16 [B, S, C]: a counter (so every 16-bit pattern class is present and every element names its place), and an
    order with repeats whenever it has room for one"""
    B, S, C, n = c["B"], c["S"], c["C"], c["n"]
    x = ((np.arange(B * S * C, dtype=np.uint64) * np.uint64(40503) + np.uint64(c["seed"])) & np.uint64(0xFFFF)).astype(np.uint16)
    order = (hashed(c["seed"], n) % np.uint64(S)).astype(np.int64)
    if n >= 3:
        order[-1] = order[0]
    return x.reshape(B, S, C), order


def permute_reference(x, order, skip_chunk=None):
    """x[:, order]; skip_chunk (b, row, chunk): the mutant that leaves one 16-byte chunk of one row unwritten"""
    out = x[:, order].copy()
    if skip_chunk is not None:
        b, r, ch = skip_chunk
        out[b, r, 8 * ch:8 * ch + 8] = FILL
    return out


# ---- rel_l1 -------------------------------------------------------------------------------------------------------
RL1_CLAMP = 1024 * 2048                        # 16-byte chunks at which the grid reaches its 1024 workgroups
REL_L1_SIZES = tuple(range(10)) + tuple(8 * n16 + t for n16 in (255, 256, 257, 2048, 2049, 1380, 6844) for t in (0, 5)) + \
    tuple(8 * n16 + t for n16 in (RL1_CLAMP, RL1_CLAMP + 1) for t in (0, 7))
# 1380: one workgroup, the second trip of its loop has slot 0 full, slot 1 partly live, slots 2 and 3 dead;
# 6844: four workgroups (a trip covers 4096 chunks), the second trip has slots 0 and 1 full and slot 2 partly live


@functools.lru_cache(maxsize=1)
def _rel_l1_pool():
    n = 8 * (RL1_CLAMP + 1) + 8
    ha, hb = hashed(901, n), hashed(902, n)
    a = np.where(ha % np.uint64(8) == 0, 1, np.where(ha % np.uint64(8) == 1, -1, 0)).astype(np.int8)
    b = np.where(hb % np.uint64(8) == 0, 1, np.where(hb % np.uint64(8) == 1, -1, 0)).astype(np.int8)
    # every 16-byte chunk holds one element with b = +-1 and a = 0, so that no chunk can go missing (or count twice)
    # without changing BOTH integers
    slot = np.arange(0, n, 8) + (hashed(903, n // 8) % np.uint64(8)).astype(np.int64)
    b[slot] = np.where(hashed(904, n // 8) & np.uint64(1), 1, -1)
    a[slot] = 0
    return a, b


def rel_l1_inputs(n):
    """(a, b) int8 of length n over {-1, 0, 1}, non-zero differences on the first element, on the last element of the last
    full chunk and on the last element"""
    a, b = (t[:n].copy() for t in _rel_l1_pool())
    for j in {0, (n // 8) * 8 - 1, n - 1}:
        if 0 <= j < n:
            a[j], b[j] = 1, -1
    return a, b


def rel_l1_counts(a, b):
    """(sum |a - b|, sum |b|) as python ints"""
    return int(np.abs(a.astype(np.int64) - b).sum()), int(np.abs(b.astype(np.int64)).sum())


# ---- what the kernels replace, in torch on the CPU --------------------------------------------------------------------
def _tdt(dt):
    import torch
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _tensor(bits, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(_tdt(dt))


def _t(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dt is None else t.to(_tdt(dt))


def torch_norm_module(norm, dt, n):
    """the module a processor would hold for `norm` (qk_model's tuple), in the storage type: helpers.RMS or
    torch.nn.LayerNorm; None for no norm"""
    import helpers
    import torch
    if norm is None:
        return None
    with torch.no_grad():
        if not (isinstance(norm[0], str) and norm[0] == "ln"):
            w, eps = norm[-2], norm[-1]
            m = helpers.RMS(n, eps=eps).to(_tdt(dt))
            if w is None:
                m.weight = None
                m.forward = lambda x: (x * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)
            else:
                m.weight.copy_(_t(w))
            return m
        _, w, b, eps = norm
        m = torch.nn.LayerNorm(n, eps=eps, elementwise_affine=w is not None or b is not None, bias=b is not None).to(_tdt(dt))
        if w is not None:
            m.weight.copy_(_t(w))
        if b is not None:
            m.bias.copy_(_t(b))
        return m


def torch_qk(cid):
    """float32 numpy [B, S, H, D]: norm module, then _operator.rotary on the first s_rope tokens"""
    import torch
    from rectified_spaattn_amd import _operator as op
    c = next(c for c in qk_cases() if c["id"] == cid)
    i = qk_inputs(cid)
    with torch.no_grad():
        q = _tensor(i["x"], c["dt"]).transpose(1, 2)                     # [B, H, S, D]
        m = torch_norm_module(i["norm"], c["dt"], c["D"])
        if m is not None:
            q = m(q)
        if i["rope"] is not None and c["s_rope"] > 0:
            n = c["s_rope"]
            tab = tuple(_t(t[:n]) for t in i["rope"])
            q = torch.cat([op.rotary(q[:, :, :n], tab), q[:, :, n:]], dim=2)
        return q.transpose(1, 2).float().numpy()


def torch_across(cid):
    """float32 numpy [B, S, H, D]: RMSNorm over H * D, then Wan2.1's complex or Wan2.2's cos / sin rotation"""
    import torch
    from rectified_spaattn_amd import rectified_wan21_attn as w21, rectified_wan22_attn as w22
    c = next(c for c in across_cases() if c["id"] == cid)
    i = across_inputs(cid)
    with torch.no_grad():
        x = _tensor(i["x"], c["dt"])
        m = torch_norm_module(i["norm"], c["dt"], c["H"] * c["D"])
        if m is not None:
            x = m(x)
        x = x.unflatten(2, (c["H"], -1))                                  # [B, S, H, D]
        if c["kind"] == 1:
            x = w21._complex_rope(x.transpose(1, 2), _t(i["tables"])[None, None]).transpose(1, 2)
        elif c["kind"] == 2:
            x = w22._cos_sin_rope(x, *(_t(t)[None, :, None, :] for t in i["tables"]))
        return x.float().numpy()
