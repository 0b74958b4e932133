"""The exact-weight tests' own ground (tests/weights.py), checked without a device, for every case of its tables: the inputs are
exact in the case's type, round_dt(a * qk_scale) is the target with room to the next rounding tie, the scores of the rounded
operands are the integers n, every row of every head fits the 2^24 budget (fp16: a spread of at most 10), every spike key "just
outside a limit" is outside it and beside a visible key, the weighted-count reference equals a brute-force fp64 masked softmax
(on the heads and query blocks of _sample: all of a small case, a sample of the large ones, as the sensitivity check), and every model mutant -- a row with another row's scores, a class on another K channel,
the weights of a sub-step permuted, a rescale that skips O, l, a d-tile or a 32-row half, pieces merged without their weights,
a query head on its neighbour's K or V head, a key seen beyond a limit -- moves some output element of the query block it
touches by visibility.SENSITIVITY tolerances.  The exemptions (three rules) and the limit mutants left to the visibility tests are printed with their counts; any other
insensitive mutant fails."""
import numpy as np
import pytest

import weights as w

ALL = list(w.CASES)


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


@pytest.mark.parametrize("cid", ALL)
def test_every_model_mutant_would_break_the_bound(cid, models):
    c = w.CASES[cid]
    heads, every = _sample(c)
    missed, exempt = w.insensitive(models(cid), heads, w.limit_mutants(c), every)
    print(f"{cid}: exempt by rule: {exempt}")
    assert not missed, f"{cid}: the bound would not notice {len(missed)} mutants: {missed[:12]}"


def test_the_sensitivity_check_notices_uniform_weights():
    """The check itself: with every score equal (the zero-score witness's weights) the permutations inside a sub-step and the
    wrong K channel cannot show, and the check must say so."""
    c = w.CASES["plain-bf16-D64-b64-kv337_165"]
    assert not w.insensitive(w.model(c), 1)[0]
    m = w.model(c)
    m.n[:] = 0
    missed, _ = w.insensitive(m, 1)
    assert any("classes read K channel" in x for x in missed) and any("weights of sub-step" in x for x in missed)
