"""References of merge_partials (rsa_merge_partials), numpy only.

    merge_ref    the contract in fp64: over the live entries of a row (lse > -inf; the sink last, its out zero),
                 out = sum_i exp(lse_i - m) out_i / sum_i exp(lse_i - m), lse = m + ln sum_i exp(lse_i - m); no live entry: 0 / -inf.
                 The out of an entry that is not live is never read (it may hold NaN).
    merge_twin   the kernel's operation order in fp32: w_i = exp2((lse_i - m) * log2 e) from one subtraction and one multiplication,
                 acc = fma(w_i, out_i, acc) and l = l + w_i over the live partials in ascending order, the sink's weight into l alone,
                 out = acc / l rounded once to the output type, lse = m + ln 2 * log2 l.  numpy's exp2 / log2 stand for the
                 hardware's: both are within an ulp or two, which is what the bound below allows for.
    bound        what the twin and the kernel are held to against merge_ref:
                 out: half a unit in the last place of the output type at the reference value + 2^-20 max_i |out_i|;
                 lse: 2^-20 max(1, |lse|).
                 At most 9 weighted terms; each weight is within a few fp32 ulps (the rounding of the exp2 argument included: the
                 argument's error is 2^-24 |x| log2 e, and x e^-x <= 0.37 keeps the weighted error below 2^-24 of the largest term);
                 fmaf and the sum of l add at most 9 half-ulps; the division one more: in all below 2^-20 of max_i |out_i|, and
                 the one rounding to the output type adds its half ulp.  lse: log2 l with l in [1, 9] to a few ulps of at most
                 3.2, one multiplication and one addition.
    make_case    random partials for both tests: outs representable in the output type, a share of the (partial, row) pairs dead
                 (lse = -inf, out NaN), some rows dead in every entry.

Formats: "bf16" (8 significant bits, least normal exponent -126) and "fp16" (11, -14)."""
import numpy as np

LOG2E = np.float32(1.44269504088896340736)
LN2 = np.float32(0.69314718055994530942)
FORMATS = {"bf16": (8, -126), "fp16": (11, -14)}
OUT_FLOOR = 2.0 ** -20
LSE_TOL = 2.0 ** -20


def ulp(x, kind):
    """The unit in the last place of the 2-byte type at x (fp64 in, fp64 out); the subnormal spacing below the least normal."""
    bits, emin = FORMATS[kind]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                                  # |x| = m 2^e, 0.5 <= m < 1 (frexp(0) says e = 0: taken out below)
    return np.ldexp(1.0, np.maximum(np.where(x == 0.0, emin + 1, e), emin + 1) - bits)


def round_to(x, kind):
    """x (fp64) rounded once, to nearest even, to the 2-byte type; returned as fp64."""
    u = ulp(x, kind)
    return np.rint(np.asarray(x, np.float64) / u) * u


def to_bits(x, kind):
    """Values representable in the type -> its 16-bit patterns (uint16)."""
    if kind == "fp16":
        return np.asarray(x, np.float64).astype(np.float16).view(np.uint16)
    return (np.asarray(x, np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _entries(outs, lses, sink):
    outs, lses = np.asarray(outs), np.asarray(lses)
    assert outs.shape[:-1] == lses.shape and outs.ndim >= 2
    if sink is not None:        # (one value per row: make_case's sink_rows)
        sink = np.asarray(sink)
    return outs, lses, sink


def merge_ref(outs, lses, sink=None):
    """outs [N, ..., D], lses [N, ...], sink None or broadcastable to lses[0] -> (out [..., D], lse [...]) in fp64."""
    outs, lses, sink = _entries(outs, lses, sink)
    lses = lses.astype(np.float64)
    live = lses > -np.inf
    x = np.where(live[..., None], outs.astype(np.float64), 0.0)        # (where: a dead entry's NaN is never multiplied)
    every = lses
    if sink is not None:
        every = np.concatenate([lses, np.broadcast_to(sink.astype(np.float64), lses.shape[1:])[None]], 0)
    m = every.max(0)
    some = m > -np.inf
    ms = np.where(some, m, 0.0)
    w = np.where(every > -np.inf, np.exp(np.where(every > -np.inf, every, 0.0) - ms), 0.0)
    l = w.sum(0)
    acc = (w[:len(lses), ..., None] * x).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(some[..., None], acc / np.where(some, l, 1.0)[..., None], 0.0)
        lse = np.where(some, ms + np.log(np.where(some, l, 1.0)), -np.inf)
    return out, lse


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64, the sum is rounded there and once more to fp32
    (a double rounding that can differ from the fused result in the last bit, rarely; the bound has room for it)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def merge_twin(outs, lses, sink=None, kind="bf16"):
    """The kernel's order of operations in fp32 -> (out rounded to the type, as fp64; lse fp32)."""
    outs, lses, sink = _entries(outs, lses, sink)
    outs, lses = outs.astype(np.float32), lses.astype(np.float32)
    live = lses > -np.inf
    m = np.where(live, lses, -np.inf).max(0).astype(np.float32)
    if sink is not None:
        sk = np.broadcast_to(sink.astype(np.float32), m.shape)
        m = np.maximum(m, np.where(sk > -np.inf, sk, -np.inf)).astype(np.float32)
    some = m > -np.inf
    ms = np.where(some, m, np.float32(0))
    acc = np.zeros(outs.shape[1:], np.float32)
    l = np.zeros(m.shape, np.float32)

    def weight(v, on):
        return np.where(on, np.exp2((np.where(on, v, np.float32(0)) - ms) * LOG2E), np.float32(0)).astype(np.float32)
    for i in range(len(lses)):
        w = weight(lses[i], live[i])
        x = np.where(live[i][..., None], outs[i], np.float32(0))
        acc = np.where(live[i][..., None], fma32(np.broadcast_to(w[..., None], x.shape), x, acc), acc)
        l = np.where(live[i], l + w, l).astype(np.float32)
    if sink is not None:
        l = np.where(sk > -np.inf, l + weight(sk, sk > -np.inf), l).astype(np.float32)
    safe = np.where(some, l, np.float32(1))
    out = np.where(some[..., None], (acc / safe[..., None]).astype(np.float32), np.float32(0))
    lse = np.where(some, ms + (LN2 * np.log2(safe)).astype(np.float32), np.float32(-np.inf)).astype(np.float32)
    return round_to(out.astype(np.float64), kind), lse


def bound(outs, lses, ref_out, ref_lse, kind):
    """(the largest |out - ref| allowed per element, the largest |lse - ref| per row) for these partials and their fp64 merge."""
    outs, lses = np.asarray(outs, np.float64), np.asarray(lses, np.float64)
    big = np.where((lses > -np.inf)[..., None], np.abs(outs), 0.0).max(0)
    with np.errstate(invalid="ignore"):
        lse_tol = LSE_TOL * np.maximum(1.0, np.where(np.isfinite(ref_lse), np.abs(ref_lse), 0.0))
    return 0.5 * ulp(ref_out, kind) + OUT_FLOOR * big, lse_tol


def worst_ratios(got_out, got_lse, outs, lses, sink, kind):
    """|got - merge_ref| over the bound, the largest per output -> (out ratio, lse ratio); rows without a live entry must be 0 / -inf
    exactly and count as ratio 0 (inf where they are not)."""
    ref_out, ref_lse = merge_ref(outs, lses, sink)
    tol_out, tol_lse = bound(outs, lses, ref_out, ref_lse, kind)
    got_out, got_lse = np.asarray(got_out, np.float64), np.asarray(got_lse, np.float64)
    dead = ~np.isfinite(ref_lse)
    with np.errstate(invalid="ignore"):
        r_out = np.abs(got_out - ref_out) / tol_out
        r_lse = np.where(dead, np.where(got_lse == -np.inf, 0.0, np.inf), np.abs(got_lse - np.where(dead, 0.0, ref_lse)) / tol_lse)
    r_out = np.where(np.isnan(r_out), np.inf, r_out)
    r_out = np.where(dead[..., None], np.where(got_out == 0.0, 0.0, np.inf), r_out)
    return float(r_out.max()), float(np.where(np.isnan(r_lse), np.inf, r_lse).max())


def make_case(seed, N, shape, kind, spread=3.0, mag=1.0, dead=0.2, sink=False, dead_rows=True):
    """Random partials: outs fp32 [N, *shape] representable in the type, of magnitude mag; lses fp32 [N, *shape[:-1]] spread over
    `spread` around a per-row centre; `dead` of the (partial, row) pairs not live: lse -inf and the out row NaN; with dead_rows every
    seventh row dead in every entry (beside a sink: that head's sink is then -inf too, for head 0 only).  sink: fp32 [H] or None, H
    = shape[1].  -> dict(outs, lses, sink, sink_rows: the sink broadcast to a row's shape or None)."""
    rng = np.random.default_rng(seed)
    rows = tuple(shape[:-1])
    outs = round_to(mag * rng.standard_normal((N,) + tuple(shape)), kind).astype(np.float32)
    centre = 4.0 * rng.standard_normal(rows)
    lses = (centre[None] + spread * (rng.random((N,) + rows) - 0.5)).astype(np.float32)
    off = rng.random((N,) + rows) < dead
    sk = sk_rows = None
    H = shape[1]                # [B, H, S, D] and packed [T, H, D] alike
    hshape = [1] * len(rows)
    hshape[-2 if len(rows) == 3 else -1] = H
    if sink:
        sk = (spread * (rng.random(H) - 0.5)).astype(np.float32)
    if dead_rows:
        flat = np.zeros(int(np.prod(rows)), bool)
        flat[3::7] = True
        gone = flat.reshape(rows)
        if sink:                # a row is dead only where its head's sink is: head 0's sink is -inf, the other heads keep theirs
            sk[0] = -np.inf
            gone = gone & (np.arange(H).reshape(hshape) == 0)
        off = off | gone[None]
    lses[off] = -np.inf
    outs[off] = np.nan
    if sink:
        sk_rows = np.broadcast_to(sk.reshape(hshape), rows)
    return dict(outs=outs, lses=lses, sink=sk, sink_rows=sk_rows)
