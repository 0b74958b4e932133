"""The visibility tests' own ground (tests/visibility.py), checked without a device: the counting references equal a brute-force
fp64 masked softmax on the same inputs, the scores of the orthogonal-support inputs are exactly zero -- also on the e4m3
operands -- and every case of the tables meets the sensitivity condition: one key on the wrong side of any limit, or one
64-key tile dropped or counted twice, would move some output element by at least eight times its tolerance."""
import numpy as np
import pytest

import visibility as vis

ALL = list(vis.CASES)
H_CPU = {"plain": 2, "dense": 1, "rect": 1}      # heads the CPU checks build (the tail cases' masks differ by head: 2 of 9)


def _expanded(ref):
    """bool [BH | 1, Sq, Sk]: the keys of every row."""
    out = np.zeros((ref.vis.shape[0], ref.r2g.shape[0], ref.vis.shape[2]), bool)
    has = ref.r2g >= 0
    out[:, has] = ref.vis[:, ref.r2g[has]]
    return out


def _sample_rows(ref, limit=1 << 21):
    """Every row of a small case; of a large one the first and last row of every group and the rows either side of a change."""
    Sq, Sk = ref.r2g.shape[0], ref.vis.shape[2]
    if Sq * Sk <= limit:
        return np.arange(Sq)
    edge = np.nonzero(np.diff(ref.r2g))[0]
    return np.unique(np.clip(np.concatenate([[0, Sq - 1], edge, edge + 1]), 0, Sq - 1))


@pytest.mark.parametrize("cid", ALL)
def test_counting_reference_equals_a_masked_softmax(cid):
    c = vis.CASES[cid]
    H = min(c["H"], H_CPU[c["family"]])
    ref = vis.reference(c, H)
    B = c["B"] if c["family"] != "dense" else 1
    Sq, (Sk, D) = ref.r2g.shape[0], ref.v.shape
    q, k = vis.qk_inputs(B, H, Sq, Sk, D)
    rows = _sample_rows(ref)
    want = ref.rows()[:, rows]
    BH = ref.vis.shape[0]
    for bh in range(BH):
        qq, kk = q.reshape(-1, Sq, D)[bh][rows].astype(np.float64), k.reshape(-1, Sk, D)[bh].astype(np.float64)
        s = qq @ kk.T * float(D) ** -0.5
        assert not s.any(), "the scores are not exactly zero"
        seen = ref.vis[bh][ref.r2g[rows]] & (ref.r2g[rows] >= 0)[:, None]
        s = np.where(seen, s, -np.inf)
        m = np.where(seen.any(1), s.max(1, initial=-np.inf), 0.0)
        e = np.where(seen, np.exp(s - m[:, None]), 0.0)
        den = e.sum(1, keepdims=True)
        o = np.where(den > 0, e @ ref.v.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)
        if ref.R is not None:
            g = ref.r2g[rows]
            o = np.where((g >= 0)[:, None], ref.R[bh][g][:, None] * o + ref.comp[bh][g], 0.0)
        assert np.abs(o - want[bh]).max() <= 1e-12, cid


@pytest.mark.parametrize("cid", ALL)
def test_every_case_meets_the_sensitivity_condition(cid):
    c = vis.CASES[cid]
    missed = vis.insensitive(c, vis.case_ulp(c), min(c["H"], H_CPU[c["family"]]))
    assert not missed, f"{cid}: the bound would not notice: {missed}"


def test_the_sensitivity_check_notices_a_blind_witness():
    """The check itself: with a V that cannot tell keys apart (every key in the same channels) it must report the case."""
    c = vis.CASES["plain-bf16-D64-b64-kv64_165"]
    real = vis.witness_v
    try:
        def blind(Sk, D, probes):
            v = np.zeros((Sk, D), np.float32)
            v[:, 0] = 1
            return v
        vis.witness_v = blind
        assert vis.insensitive(c, vis.ULP["bf16"])
    finally:
        vis.witness_v = real
    assert not vis.insensitive(c, vis.ULP["bf16"])


def test_witness_v_is_exact_in_every_format():
    from oracle import oracle as orc
    v = vis.witness_v(700, 64, vis.around(300) + [0, 699])
    assert set(np.unique(v)) == {0.0, 1.0} and (v.sum(1) == 2).all()
    assert np.array_equal(orc.round_bf16(v), v) and np.array_equal(orc.round_fp16(v), v)
    assert np.array_equal(orc.dequantize_e4m3(orc.quantize_e4m3(v)), v)
    for p, key in enumerate(sorted(set(vis.around(300) + [0, 699]))):
        assert v[key, p] == 1 and v[:, p].sum() == 1, "a probe channel belongs to one key"
    q, k = vis.zero_score_qk(1, 1, 2, 50, 70, 64)
    for x in (q, k):
        assert np.array_equal(orc.round_bf16(x), x) and np.array_equal(orc.round_fp16(x), x)
        assert (np.abs(x).reshape(-1, 64).max(0) > 0).sum() == 32


FP8_RECT = [c["id"] for c in vis.RECT_CASES if c["fp8"] and c["layout"] != "hunyuan_tail"]


@pytest.mark.parametrize("cid", FP8_RECT)
def test_scores_stay_zero_on_the_e4m3_operands_of_the_rectified_call(cid):
    """oracle.fp8_operands: Q * qk_const, K minus its "smooth K" mean, block-scaled and rounded to e4m3 -- zero channels stay
    zero, so every score of the dequantised operands is exactly 0; V's 0 / 1 come back unchanged."""
    from oracle import oracle as orc
    c = vis.CASES[cid]
    sp = vis.spec_numbers(vis.rect_spec(c))
    lay = orc.Layout(sp.S, sp.NB_total, sp.NBv, sp.n_txt, sp.kv_valid, sp.pool_valid, 0, 0, sp.q_text_valid, sp.kv_text_valid)
    ref = vis.reference(c, 1)
    q, k = vis.qk_inputs(1, 1, sp.S, sp.S, c["D"])
    v = ref.v[None, None]
    qd, kd, vd, ops = orc.fp8_dequantized_qkv(q, k, v, lay)
    assert np.abs(ops["kmean"][0, :c["D"] // 2]).max() == 0 and np.abs(ops["kmean"][0, c["D"] // 2:]).max() > 0
    s = qd[0, 0].astype(np.float64) @ kd[0, 0].astype(np.float64).T
    assert not s.any()
    assert np.abs(qd).max() > 0 and np.abs(kd).max() > 0
    n = min(sp.S, sp.pool_valid)
    assert np.array_equal(vd[0, 0, :n], ref.v[:n])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", vis.DENSE_SHAPES)
def test_scores_stay_zero_on_the_e4m3_operands_of_the_dense_call(Sq, Sk, D):
    """oracle.fp8_block_images as rsa_dense_fwd_fp8 applies them: over all Sq / Sk rows, K minus fp8_kmean over its Sk rows."""
    from oracle import oracle as orc
    q, k = vis.qk_inputs(1, 1, Sq, Sk, D)
    q, k = q[0, 0], k[0, 0]
    pad = lambda n: -(-n // 128) * 128                                           # noqa: E731
    mu = orc.fp8_kmean(k, Sk)
    assert not mu[:D // 2].any()
    deq = []
    for x, n, pre, km in ((q, Sq, "q", None), (k, Sk, "k", mu)):
        img, ex = orc.fp8_block_images(x, n, pad(n), pre, km)
        val = orc.dequantize_e4m3(img).astype(np.float64) * np.exp2(np.repeat(ex.astype(np.int64) - 127, 128))[:, None]
        assert np.abs(val).max() > 0
        deq.append(val[:n])
    assert not (deq[0] @ deq[1].T).any()
