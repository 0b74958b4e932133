"""The masked / dropout witness's own ground (tests/masked_witness.py), checked without a device: the bias table gives exact
integers, the budgets that make every fp32 sum exact hold, the dropout twin equals a plain-integer version of the hash, every
reference equals a brute-force float64 masked softmax built from the documented rule, and every case meets the sensitivity
condition: each model mutant (a mask element flipped, Sk or the diagonal moved, the mask read from the neighbouring row / batch
item / head / key / tile, two keys of a tile swapped on the score side, a lost rescale, half a row sum, a dropout stream keyed
wrongly or applied to the row sum, a lost keep_scale) moves some element of every 32-row wave by eight tolerances."""
import functools
import math

import numpy as np
import pytest

import masked_witness as mw
import visibility as vis

EXACT = mw.by_class(*mw.EXACT_CLASSES)


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def test_the_bias_table_gives_every_integer_exactly():
    """np.float32(1.44269504) * b == n in float32, and in float64 rounded once (what a contracted fma(c, b, 0) computes), for every
    n the cases use: -12 .. 12.  The enumeration finds nothing for 13 and 15, which is why the range ends at 12."""
    used = set()
    for cid in mw.by_class("B", "DB"):
        m = mw.cached_model(cid)
        seen = m.mvis & m.svis
        used |= set(np.unique(m.n[seen]).tolist())
    assert used == set(range(-mw.N_RANGE, mw.N_RANGE + 1)), sorted(used)
    for n, b in mw.EXACT_BIAS.items():
        assert b.dtype == np.float32
        assert mw.LOG2E * b == np.float32(n)
        exact = float(mw.LOG2E) * float(b)                       # 24 x 24 bits: exact in float64
        assert np.float32(exact) == np.float32(n)
        assert abs(float(b) - n * math.log(2.0)) <= 1e-7 * abs(n) + 0.0, (n, b)    # b is n ln 2 to float32's precision
    c = float(mw.LOG2E)
    for n in (13, 15, -13, -15):
        b = np.float32(n / c)
        cands = [b]
        up = down = b
        for _ in range(64):
            up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
            cands += [up, down]
        assert not any(mw.LOG2E * x == np.float32(n) for x in cands), n


@pytest.mark.parametrize("cid", mw.by_class("B", "DB"))
def test_budget_and_spread_of_the_integer_weight_cases(cid):
    """sum 2^(n - n_min) < 2^24 per row (2^13 under dropout: times c's 11 significant bits it is still below 2^24), the spread of
    a row <= 10 (P stays normal in fp16), and the float32 mask holds the table's bias or -inf."""
    m = mw.cached_model(cid)
    b = mw.budget(m)
    print(f"{cid}: budget {b:.0f} = 2^{math.log2(b):.2f}, spread {mw.spread(m)}")
    assert b < (2.0 ** 13 if m.keep is not None else 2.0 ** 24)
    assert mw.spread(m) <= 10
    lg = m.logical
    assert lg.dtype == np.float32 and (np.isneginf(lg) | np.isin(lg, list(mw.EXACT_BIAS.values()))).all()
    assert np.array_equal(np.isneginf(lg), ~mw.logical_mask(m.c))


def test_keep_scale_is_what_the_type_holds():
    for dt, bits in (("bf16", 8), ("fp16", 11)):
        assert mw.keep_scale(0.5, dt) == 2.0 and mw.keep_scale(0.75, dt) == 4.0
        assert mw.keep_scale(1.0, dt) == 0.0 and mw.keep_scale(0.0, dt) == 1.0
        c = mw.keep_scale(0.25, dt)
        scaled = c * 2.0 ** (bits - 1)
        assert scaled == int(scaled) and int(scaled) % 2 == 1, (dt, c)       # the full significand of the type
        assert abs(c - 4.0 / 3.0) <= 2.0 ** -bits * 4.0 / 3.0 * 2
    assert mw.thresh(0.5) == 1 << 23 and mw.thresh(1.0) == 1 << 24 and mw.thresh(0.0) == 0 and mw.thresh(1e-9) == 1
    assert mw.thresh(0.25) == 1 << 22 and mw.thresh(0.3) == int(float(np.float32(0.3)) * 2 ** 24 + 0.5)


@pytest.mark.parametrize("cid", mw.by_class("D", "DB"))
def test_dropout_cases_sum_exactly(cid):
    """c * 2^k with c of at most 11 significant bits: the sums stay exact when sum 2^(n - n_min) < 2^13."""
    m = mw.cached_model(cid)
    assert mw.budget(m) < 2.0 ** 13
    assert m.cval == float(mw.round_dt(np.float32(m.cval), m.c["dt"]))


# ---- the hash twin ---------------------------------------------------------------------------------------------------------------
def _hash_int(seed, bh, row, key):
    M = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * ((bh << 42) ^ (row << 21) ^ key)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return z >> 40


def test_the_hash_twin_equals_plain_integer_arithmetic():
    rng = np.random.default_rng(5)
    n = 4000
    bh, row, key = rng.integers(0, 65535, n), rng.integers(0, 1 << 20, n), rng.integers(0, 1 << 20, n)
    for seed in (0, 1, (1 << 62) - 1, 0xFFFFFFFFFFFFFFFF, 0x1234567):
        got = mw.drop_hash_np(seed, bh, row, key)
        want = [_hash_int(seed, int(a), int(b), int(c)) for a, b, c in zip(bh, row, key)]
        assert got.tolist() == want
        assert int(got.max()) < 1 << 24
    for p in (0.25, 0.5, 0.75):
        keep = mw.keep_np(77, p, 5, 100, 200)                    # 10^5 draws
        share = keep.mean()
        sigma = math.sqrt(p * (1 - p) / keep.size)
        print(f"p = {p}: kept share {share:.5f}, {abs(share - (1 - p)) / sigma:.2f} sigma from 1 - p")
        assert abs(share - (1 - p)) <= 3 * sigma
    assert mw.keep_np(77, 1.0, 2, 9, 9).sum() == 0


# ---- the references against a brute-force masked softmax ---------------------------------------------------------------------------
def _brute(m, bias_of):
    """softmax(q k^T / sqrt(D) + bias [+ the top-left causal triangle]) with dropout on the weights, times v, in float64 with
    exp: the rule that the docstrings of _core.dense_attention_masked / dense_attention_dropout and attn.py state."""
    c = m.c
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    q, k = vis.qk_inputs(B, H, Sq, Sk, D)
    s = np.einsum("bhid,bhjd->bhij", q.astype(np.float64), k.astype(np.float64)) / math.sqrt(D)
    assert not s.any(), "the scores are not exactly zero"
    if m.logical is not None:
        lg = m.logical
        s = s + (np.where(lg, 0.0, -np.inf) if lg.dtype == bool else bias_of(lg.astype(np.float64)))
    if c.get("causal"):
        s = np.where(np.tril(np.ones((Sq, Sk), bool)), s, -np.inf)
    s = s.reshape(B * H, Sq, Sk)
    top = s.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(s), 0.0, np.exp(s - np.where(np.isneginf(top), 0.0, top)))
    den = e.sum(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = e / den                                              # an empty row: 0 / 0 = NaN, an explicit softmax's answer
    if m.keep is not None:
        p32 = np.float32(c["p"])
        scale = float(mw.round_dt(np.float32(1) / (np.float32(1) - p32), c["dt"])) if p32 < 1 else 0.0
        w = np.where(m.keep, w * scale, 0.0 * w)
    out = w @ m.v.astype(np.float64)
    if not c.get("empty_nan"):
        out = np.where(den > 0, out, 0.0)                        # the fused SDPA's answer for an empty row
    return out


@pytest.mark.parametrize("cid", EXACT + mw.by_class("C"))
def test_reference_equals_a_masked_softmax(cid):
    m = mw.cached_model(cid)
    ref = mw.reference(m)
    assert np.array_equal(np.isnan(ref), np.isnan(ref[..., :1]) & np.ones_like(ref, bool))
    if m.c["cls"] in ("B", "DB"):
        # (i) on the ideal biases n ln 2, which the table's float32 values stand for: the weights are 2^n
        with np.errstate(invalid="ignore"):
            out = _brute(m, lambda b: np.where(np.isneginf(b), b, np.rint(b * float(mw.LOG2E)) * math.log(2.0)))
        tol = 1e-12
        # (ii) on the float32 biases themselves: e^b is 2^n only to |n| ln 2 (2^-24 + 6.2e-10) <= 5.1e-7, twice that in a weight
        out2 = _brute(m, lambda b: b)
        assert np.nanmax(np.abs(out2 - ref), initial=0.0) <= 2e-6 * np.nanmax(np.abs(ref))
    else:
        out = _brute(m, lambda b: b)
        tol = 1e-12
    assert np.array_equal(np.isnan(out), np.isnan(ref)), cid
    assert np.nanmax(np.abs(out - ref), initial=0.0) <= tol, cid
    empty = ~(mw._flat(m.mvis, m) & m.svis).any(-1)
    if m.c.get("empty_nan"):
        assert np.array_equal(np.isnan(ref[..., 0]), empty)
    else:
        assert not ref[empty].any()


def test_the_designed_rows_are_there():
    """Every wave of a row-masked case holds a row without keys, one that is empty in its first tiles only, one with keys in the
    first tile only, one with exactly the last key, and rows that end on a tile edge."""
    m = mw.cached_model(next(c["id"] for c in mw.CASE_LIST if c["cls"] == "A" and c["Sq"] == 200 and c["mshape"] == (2, 3, 200, 333)))
    seen = m.mvis.reshape(m.BH, 200, 333)
    assert not seen[:, 3::32].any()
    assert not seen[:, 7::32, :64].any() and seen[:, 7::32, 64:].any(-1).all()
    assert not seen[:, 11::32, 32:].any() and seen[:, 11::32, 0].all()
    assert (seen[:, 13::32].sum(-1) == 1).all() and seen[:, 13::32, 332].all()
    assert (seen[:, 17::32].sum(-1) == 320).all() and (seen[:, 19::32].sum(-1) == 32).all()
    probes = mw.probes_of(m.c)
    assert {30, 31, 32, 33, 318, 319, 320, 321, 331, 332} <= set(probes)


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sensitivity(cid):
    return mw.insensitive(mw.model(mw.CASES[cid]))


@pytest.mark.parametrize("cid", EXACT)
def test_every_case_meets_the_sensitivity_condition(cid):
    missed, exempt, total = _sensitivity(cid)
    print(f"{cid}: {sum(total.values())} (wave, mutant) pairs, exempt: { {k: v for k, v in exempt.items() if v} }")
    assert not missed, f"{cid}: the bound would not notice {len(missed)} (mutant, head, wave): {missed[:8]}"


def test_exemptions_stay_within_the_cap():
    """Two rules exempt (masked_witness.RULES, each printed with its count): the mutant's exact output equals the reference's in
    the whole wave; a visibility mutant under dropout that touches only dropped weights of the wave.  At most 5 % of all (case,
    wave, mutant) triples, and no mutant kind exempt in every case."""
    tot, ex, always = {}, {}, {}
    for cid in EXACT:
        _, exempt, total = _sensitivity(cid)
        for k in total:
            tot[k] = tot.get(k, 0) + total[k]
            mine = sum(v for (kind, _), v in exempt.items() if kind == k)
            always[k] = always.get(k, True) and mine == total[k]
        for k, v in exempt.items():
            ex[k] = ex.get(k, 0) + v
    share = sum(ex.values()) / sum(tot.values())
    print(f"exempt: {sum(ex.values())} of {sum(tot.values())} (case, wave, mutant) triples = {100 * share:.2f} %")
    for rule in mw.RULES:
        print(f"  rule '{rule}': {sum(v for (_, r), v in ex.items() if r == rule)}")
        for k in tot:
            print(f"    {k:12s} {ex.get((k, rule), 0):6d} of {tot[k]:7d} = {100 * ex.get((k, rule), 0) / tot[k]:.2f} %")
    assert share <= 0.05
    assert set(tot) == {"visibility", "addressing", "lane map", "rescale", "row sum", "dropout"}
    assert not any(always.values()), always


def test_the_sensitivity_check_notices_a_blind_witness():
    """The check itself: with a V that cannot tell keys apart it must report the case."""
    cid = next(c["id"] for c in mw.CASE_LIST if c["cls"] == "B" and c["Sq"] == 33)
    m = mw.model(mw.CASES[cid])
    assert not mw.insensitive(m)[0]
    m.v = np.zeros_like(m.v)
    m.v[:, 0] = 1
    assert mw.insensitive(m)[0]
