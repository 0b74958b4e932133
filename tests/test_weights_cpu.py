"""The exact-weight tests' own ground (tests/weights.py), checked without a device, for every case of its tables: the inputs are
exact in the case's type, round_dt(a * qk_scale) is the target with room to the next rounding tie, the scores of the rounded
operands are the integers n, every row of every head fits the 2^24 budget (fp16: a spread of at most 10), every spike key "just
outside a limit" is outside it and beside a visible key, the weighted-count reference equals a brute-force fp64 masked softmax
(on the heads and query blocks of _sample: all of a small case, a sample of the large ones, as the sensitivity check), and every model mutant -- a row with another row's scores, a class on another K channel,
the weights of a sub-step permuted, a rescale that skips O, l, a d-tile or a 32-row half, pieces merged without their weights,
a query head on its neighbour's K or V head, a key seen beyond a limit -- moves some output element of the query block it
touches by visibility.SENSITIVITY tolerances.  The exemptions (three rules) and the limit mutants left to the visibility tests are printed with their counts; any other
insensitive mutant fails.

The e4m3 and pv cases have a test of their own for the first half: the operands are checked on the block-scaled images the oracle's
byte-exact contract makes of them (the scaled Q one-hot with a power of two, mu / 8 integral, K - mu = 8 (n - mu / 8) and V exact in
their images, two distinct K and V exponents among the blocks some row sees), the spread of every row against the code map's own
constants, the budget with the code map's factor 1.5 and V's block gains in it, and the reference against a brute-force fp64 softmax
of the DEQUANTISED operands.  The mutant test runs on them with the fp8 forms' own mutants added."""
import numpy as np
import pytest

import weights as w

ALL = [cid for cid, c in w.CASES.items() if not w.form_of(c)]
FP8 = [c["id"] for c in w.FP8_CASES]


def _sample(c):
    """(heads, every): all heads of a small case; of the large ones (the tail split, the long rectified layouts) the first and
    the last head and every seventh query block and the last three (the text rows among them)."""
    if c["family"] == "gqa":
        return None, 1
    big = c.get("mask") == "tail" or c.get("layout") in ("hunyuan_tsplit", "hunyuan_tail")
    if big:
        return sorted({0, c["H"] - 1}), 7
    return min(c["H"], 2 if c["family"] in ("plain", "ranged") else 1), 1


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(cid):
        if cid not in cache:
            cache.clear()           # (one at a time: the large cases hold tens of megabytes)
            cache[cid] = w.model(w.CASES[cid])
        return cache[cid]
    return get


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_exactly_one_value_of_q_gives_the_target_at_the_default_scale(dt, D):
    a, margin = w.find_a(dt, float(D) ** -0.5)
    print(f"{dt} D {D}: a = {a.tolist()}, {margin:.3f} ulp from a tie")
    assert len(a) == 1 and margin >= 0.05
    assert w.round_dt(np.float32(a[0]) * w.qk_scale(float(D) ** -0.5), dt) == w.TARGET
    assert w.round_dt(a, dt)[0] == a[0]


def test_the_explicit_scale_makes_qk_scale_one_eighth_and_a_one():
    one, margin = w.find_a("bf16", w.TARGET / w.LOG2E)
    assert one.tolist() == [1.0] and float(w.qk_scale(w.TARGET / w.LOG2E)) == 0.125 and margin >= 0.05


@pytest.mark.parametrize("cid", ALL)
def test_inputs_are_exact_and_the_reference_is_the_masked_softmax(cid, models):
    c = w.CASES[cid]
    m = models(cid)
    heads, every = _sample(c)
    _, margin = w.find_a(m.dt, m.scale)
    assert margin >= 0.05
    q, k, v = m.q(), m.k(), m.v
    for x in (q, k, v):
        assert np.array_equal(w.round_dt(x, m.dt), x), "an input is not exact in the case's type"
    assert set(np.unique(v)) <= {0.0, 1.0} and k.max() <= 256 and np.array_equal(k, np.round(k))
    worst, spread = w.budget(m)          # every row of every head: the exactness argument rests on it
    assert not w.misplaced_outside_keys(m), w.misplaced_outside_keys(m)
    print(f"{cid}: largest sum 2^(n - n_min) {worst:.0f}, largest spread {spread}; {w.exercised(m, heads, every)}")
    assert worst < 2 ** 24
    assert m.dt != "fp16" or spread <= 10
    # the operands as the kernels see them: Q * qk_scale rounded to the type, in fp64 from there on
    qs = w.round_dt(q * w.qk_scale(m.scale), m.dt).astype(np.float64)
    want = w.reference(m, heads, every=every)
    ref = m.ref
    for bh in m.heads(heads):
        h = bh % m.H
        kk, vv = k[m.kvh(h)].astype(np.float64), v[m.kvh(h)].astype(np.float64)
        vbh = ref.vis[bh if ref.vis.shape[0] > 1 else 0]
        for qb in m.blocks(every):
            rows = np.arange(qb * m.qrows, min((qb + 1) * m.qrows, m.Sq))
            g = ref.r2g[rows]
            s = qs[bh // m.H, h][rows] @ kk.T
            assert np.array_equal(s, m.n[m.kvh(h)][:, w.cls(rows, h, m.D)].T), "a score is not its integer n"
            seen = vbh[np.maximum(g, 0)] & (g >= 0)[:, None]
            s = np.where(seen, s * np.log(2.0), -np.inf)
            mx = np.where(seen.any(1), s.max(1, initial=-np.inf), 0.0)
            e = np.where(seen, np.exp(s - mx[:, None]), 0.0)
            den = e.sum(1, keepdims=True)
            o = np.where(den > 0, e @ vv / np.where(den > 0, den, 1.0), 0.0)
            if ref.R is not None:
                o = np.where((g >= 0)[:, None], ref.R[bh][np.maximum(g, 0)][:, None] * o + ref.comp[bh][np.maximum(g, 0)], 0.0)
            assert np.abs(o - want[bh, rows]).max() <= 1e-12, (cid, bh, qb)


def test_the_code_map_turns_an_integer_distance_into_an_exact_power_of_two():
    """PMap<true> (U, BIAS, OFFSET, THRESH as oracle.py restates them): a score d above its reference (d <= THRESH by the move rule)
    or below it arrives as the code 108 + 8 d, mantissa field 4: 1.5 * 2^(d + 6) down to d = -max_spread(), the subnormal 2^-7 one
    further down -- which is why every visible key of a row must lie within max_spread() = 12 of the row's maximum."""
    from oracle import oracle as orc
    U, BIAS, OFFSET, THRESH = w.pmap()
    val = orc.e4m3_code_values()
    assert w.max_spread() == 12
    for d in range(-w.max_spread(), int(THRESH) + 1):
        code = U * (d + OFFSET) + BIAS
        assert code == int(code) and 8 <= code <= 124 and val[int(code)] == 1.5 * 2.0 ** (d + 6), d
    below = int(U * (-w.max_spread() - 1 + OFFSET) + BIAS)
    assert below == 4 and val[below] == 2.0 ** -7 != 1.5 * 2.0 ** (-w.max_spread() - 1 + 6)


@pytest.mark.parametrize("D", [64, 128])
def test_the_scaled_q_of_the_fp8_forms(D):
    """pv: one bf16 value a with round(a * (float)(sm_scale * 1.44269504 * 8)) == 1, the launcher's own expression; e4m3: the image
    is taken of Q * oracle.fp8_qk_const, the 2-byte kernels' qk_scale (the power of two itself is asserted on the image per case)."""
    from oracle import oracle as orc
    sm = float(D) ** -0.5
    assert np.float32((1.0 / np.sqrt(float(D))) * 1.44269504 * 8.0) == w.qk_scale(8.0 * sm)
    assert orc.fp8_qk_const(D) == w.qk_scale(sm)
    a, margin = w.find_a("bf16", 8.0 * sm, 1.0)
    print(f"pv D {D}: a = {a.tolist()}, {margin:.3f} ulp from a tie")
    assert len(a) == 1 and margin >= 0.05
    assert w.round_dt(np.float32(a[0]) * w.qk_scale(8.0 * sm), "bf16") == 1.0


def _oracle_layout(c):
    from oracle import oracle as orc
    import visibility as vis
    ctor, args = vis.RECT_LAYOUTS[c["layout"]]
    return getattr(orc, f"layout_{ctor}")(*args)


@pytest.mark.parametrize("cid", FP8)
def test_fp8_operands_are_exact_and_the_reference_is_the_softmax_of_the_dequantised_images(cid, models):
    from oracle import oracle as orc
    c = w.CASES[cid]
    m = models(cid)
    heads, every = _sample(c)
    _, margin = w.find_a(m.dt, *m.q_target)
    assert margin >= 0.05
    for x in (m.q(), m.k(), m.v):
        assert np.array_equal(w.round_dt(x, m.dt), x), "an input is not exact in the case's type"
    faults = w.fp8_image_faults(m)
    assert not faults, faults
    im = w.fp8_images(m)
    worst, spread = w.budget(m)          # every row of every head
    assert not w.misplaced_outside_keys(m), w.misplaced_outside_keys(m)
    print(f"{cid}: largest sum 2^(n - n_min) {worst:.0f}, largest spread {spread}, mu / 8 in {sorted(set((im['mu'] / 8).ravel().tolist()))}, "
          f"exponents K {np.unique(im['ek']).tolist()} V {np.unique(im['ev']).tolist()} Q {np.unique(im['eq']).tolist()}; "
          f"{w.exercised(m, heads, every)}")
    assert spread <= w.max_spread()
    assert 3 * 2 ** max(w.V_GAINS) * worst < 2 ** 24
    qd, kd, vd = (im[x].astype(np.float64) for x in ("qd", "kd", "vd"))
    if c["family"] == "rect":            # the same images through the oracle's own entry point
        B, H = m.B, m.H
        q4 = m.q()
        k4, v4 = (np.broadcast_to(x[None], (B,) + x.shape) for x in (m.k(), m.v))
        q8, k8, v8, _ = orc.fp8_dequantized_qkv(q4, k4, v4, _oracle_layout(c))
        assert np.array_equal(v8[0], im["vd"])
        if m.fp8 is True:
            assert np.array_equal(k8[0], im["kd"])
            assert np.abs(q8[0] * np.float64(orc.fp8_qk_const(m.D)) - im["qd"]).max() <= 1e-6 * im["qunit"]
    want = w.reference(m, heads, every=every)
    ref = m.ref
    u = im["mu"].astype(np.float64) / w.KSCALE
    for bh in m.heads(heads):
        h = bh % m.H
        vbh = ref.vis[bh if ref.vis.shape[0] > 1 else 0]
        for qb in m.blocks(every):
            rows = np.arange(qb * m.qrows, min((qb + 1) * m.qrows, m.Sq))
            g = ref.r2g[rows]
            s = qd[h][rows] @ kd[h].T / (8.0 * im["qunit"])
            cl = w.cls(rows, h, m.D)
            seen = vbh[np.maximum(g, 0)] & (g >= 0)[:, None]
            assert np.array_equal(np.where(seen, s, 0), np.where(seen, m.n[h][:, cl].T - u[h][cl][:, None], 0)), "a score is not n - mu / 8"
            s = np.where(seen, s * np.log(2.0), -np.inf)
            mx = np.where(seen.any(1), s.max(1, initial=-np.inf), 0.0)
            e = np.where(seen, np.exp(s - mx[:, None]), 0.0)
            den = e.sum(1, keepdims=True)
            o = np.where(den > 0, e @ vd[h] / np.where(den > 0, den, 1.0), 0.0)
            if ref.R is not None:
                o = np.where((g >= 0)[:, None], ref.R[bh][np.maximum(g, 0)][:, None] * o + ref.comp[bh][np.maximum(g, 0)], 0.0)
            assert np.abs(o - want[bh, rows]).max() <= 1e-12 * max(1.0, float(np.abs(want).max())), (cid, bh, qb)


@pytest.mark.parametrize("cid", ALL + FP8)
def test_every_model_mutant_would_break_the_bound(cid, models):
    c = w.CASES[cid]
    heads, every = _sample(c)
    missed, exempt = w.insensitive(models(cid), heads, w.limit_mutants(c), every)
    print(f"{cid}: exempt by rule: {exempt}")
    assert not missed, f"{cid}: the bound would not notice {len(missed)} mutants: {missed[:12]}"


def test_the_sensitivity_check_notices_equal_exponents_and_a_flat_v_tile():
    """The fp8 mutants' check itself: with one V gain everywhere a neighbour's V exponent cannot show (it must be exempt by its
    rule, not missed), and with every V row of a tile equal the swapped k-slots cannot show, and the check must say so."""
    c = w.CASES["dense-e4m3-D64-300x520-whole"]
    m = w.model(c)
    missed, exempt = w.insensitive(m, 1)
    assert not missed
    m.v = m.v / np.exp2(np.repeat(m.extra["gains"], 128, axis=1)[:, :m.Sk, None]).astype(np.float32)
    m.extra["gains"][:] = 0
    m.extra.pop(("v", 0))
    missed, flat = w.insensitive(m, 1)
    assert not missed and flat["neighbouring block with the same exponent"] > exempt["neighbouring block with the same exponent"]
    m = w.model(c)
    m.v[:] = m.v[:, :1]
    missed, _ = w.insensitive(m, 1)
    assert any("k-slots" in x for x in missed)


def test_the_sensitivity_check_notices_uniform_weights():
    """The check itself: with every score equal (the zero-score witness's weights) the permutations inside a sub-step and the
    wrong K channel cannot show, and the check must say so."""
    c = w.CASES["plain-bf16-D64-b64-kv337_165"]
    assert not w.insensitive(w.model(c), 1)[0]
    m = w.model(c)
    m.n[:] = 0
    missed, _ = w.insensitive(m, 1)
    assert any("classes read K channel" in x for x in missed) and any("weights of sub-step" in x for x in missed)
