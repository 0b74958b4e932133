"""The references of tests/glue_ref.py held against torch on the CPU, and against themselves: every case's interval contains
what the replaced module calls give (helpers.RMS, torch.nn.LayerNorm, _operator.rotary, the Wan rotations), few elements are
ambiguous, and every way of getting the kernel subtly wrong that the list below names leaves the interval somewhere in every
case that can hold it.  The exemptions are rules of glue_ref.*_mutant_rule, printed, never a case that happened to miss."""
import numpy as np
import pytest
import torch

import glue_ref as g

QK_IDS = [c["id"] for c in g.qk_cases()]
AH_IDS = [c["id"] for c in g.across_cases()]


def _case(cases, cid):
    return next(c for c in cases if c["id"] == cid)


def test_case_tables_reach_every_path():
    qk = g.qk_cases()
    assert {c["H"] for c in qk} == set(g.QK_H) and {c["S"] for c in qk} == set(g.QK_S)
    for fam in ("rms", "ln"):
        mine = [c for c in qk if c["norm"] in g.QK_NORMS[fam]]
        assert {c["norm"] for c in mine} == set(g.QK_NORMS[fam])
        for key, want in (("D", {64, 128}), ("dt", {"bf16", "fp16"}), ("layout", set(g.QK_LAYOUTS)), ("concat", {False, True}),
                          ("rope", {False, True}), ("H", set(g.QK_H)), ("S", set(g.QK_S))):
            assert {c[key] for c in mine} == want, (fam, key)
        rot = [c for c in mine if c["rope"]]
        assert {0, 1} <= {c["s_rope"] for c in rot} and any(c["s_rope"] == c["S"] > 1 for c in rot)
        assert any(c["s_rope"] == c["S"] - 1 > 1 for c in rot)
        assert any(c["H"] == 30 and c["rope"] and c["s_rope"] > 0 for c in mine)      # rotation on the ragged last group
    assert any(c["norm"] == "none" and not c["rope"] for c in qk)                       # the plain strided copy
    assert any(c["norm"] == "none" and c["rope"] and c["s_rope"] > 0 for c in qk)       # rope only
    kinds = np.concatenate([g.qk_inputs(c["id"])["kinds"] for c in qk])
    assert set(kinds.tolist()) == set(range(-1, len(g.EDGE_KINDS)))
    ah = g.across_cases()
    assert {-(-c["H"] * c["D"] // 512) for c in ah} >= {1, 3, 4, 6, 7, 10, 11, 16}
    assert any((c["H"] * c["D"] // 8) % 64 for c in ah) and {32, 256} <= {c["D"] for c in ah}
    assert {c["S"] for c in ah} == set(g.AH_S) and {c["kind"] for c in ah} == {0, 1, 2}
    assert {c["norm"] for c in ah} == {"w", "now", "none"} and {c["layout"] for c in ah} == {"contig", "cols", "bstride"}
    assert all(512 % c["D"] == 0 and c["H"] * c["D"] <= 8192 for c in ah)
    pm = g.permute_cases()
    assert {c["C"] for c in pm} == set(g.PERMUTE_C) and {c["n"] for c in pm} == set(g.PERMUTE_N)
    assert {c["idx"] for c in pm} == {"int64", "int32"} and {c["layout"] for c in pm} == {"contig", "cols", "bstride"}
    assert any(len(set(g.permute_inputs(c)[1].tolist())) < c["n"] for c in pm)          # an order with repeats


def _check(lo, hi, ref, cap, what):
    share = g.ambiguous_share(lo, hi)
    ok = g.inside(ref, lo, hi)
    print(f"{what}: {lo.size} elements, ambiguous {share:.5f}, torch inside {int(ok.sum())}")
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
    assert share <= cap, (what, share)


def _mutants(names, rule, reference, lo, hi):
    missed = []
    for m in names:
        why = rule(m)
        if why is not None:
            print(f"  exempt {m}: {why}")
            continue
        if not g.escapes(*reference(m), lo, hi):
            missed.append(m)
    assert not missed, missed


@pytest.mark.parametrize("cid", QK_IDS)
def test_qk_interval_holds_torch_and_drops_the_mutants(cid):
    c = _case(g.qk_cases(), cid)
    lo, hi = g.qk_reference(cid)
    cap = g.CAP_HEAD_RMS if not c["norm"].startswith("ln") else g.CAP_WIDE
    _check(lo, hi, g.torch_qk(cid), cap, cid)
    kinds = g.qk_inputs(cid)["kinds"]
    _mutants(g.QK_MUTANTS, lambda m: g.qk_mutant_rule(c, kinds, m), lambda m: g.qk_reference(cid, m), lo, hi)


@pytest.mark.parametrize("cid", AH_IDS)
def test_across_interval_holds_torch_and_drops_the_mutants(cid):
    c = _case(g.across_cases(), cid)
    lo, hi = g.across_reference(cid)
    _check(lo, hi, g.torch_across(cid), g.CAP_WIDE, cid)
    kinds = g.across_inputs(cid)["kinds"]
    _mutants(g.AH_MUTANTS, lambda m: g.across_mutant_rule(c, kinds, m), lambda m: g.across_reference(cid, m), lo, hi)


def test_delta_follows_the_documented_count():
    assert g.DELTA_HEAD == 16 * g.U >= ((1 + 8 + 4 + 1) / 2 + 2) * g.U
    for nch in (1, 3, 6, 10, 16):
        assert g.delta_across(nch) >= ((1 + 8 * nch + 6 + 1 + 1) / 2 + 2) * g.U
    assert g.delta_across(16) == 71 * g.U


def test_rounding_helpers_match_torch():
    x = (g.normal(5, (4096,)) * np.exp(g.normal(6, (4096,)) * 20)).astype(np.float32)
    x[:4] = [0.0, -0.0, 65520.0, 1e-41]
    for dt, tdt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        want = torch.from_numpy(x).to(tdt)
        assert np.array_equal(g.to_bits(x, dt).view(np.int16), want.view(torch.int16).numpy())
        assert np.array_equal(g.widen(g.to_bits(x, dt), dt), want.float().numpy(), equal_nan=True)
    y = np.array([1.0 + 2.0 ** -30, -(1.0 + 2.0 ** -30), 1e-50, 0.5])
    assert np.all(g.f32_down(y).astype(np.float64) <= y) and np.all(g.f32_up(y).astype(np.float64) >= y)
    assert np.all(np.nextafter(g.f32_down(y), np.float32(np.inf)).astype(np.float64) >= y)


@pytest.mark.parametrize("c", g.permute_cases(), ids=lambda c: c["id"])
def test_permute_reference_is_torch_indexing(c):
    x, order = g.permute_inputs(c)
    want = g.permute_reference(x, order)
    t = torch.from_numpy(x.view(np.int16))
    assert np.array_equal(t[:, torch.from_numpy(order)].numpy().view(np.uint16), want)
    C16 = c["C"] // 8
    for b, r, ch in {(0, 0, 0), (1, c["n"] - 1, C16 - 1), (1, c["n"] // 2, C16 // 2), (0, c["n"] - 1, min(C16 - 1, 64 * 3))}:
        assert not np.array_equal(g.permute_reference(x, order, (b, r, ch)), want), (b, r, ch)


@pytest.mark.parametrize("n", g.REL_L1_SIZES)
def test_rel_l1_counts_are_exact_and_every_chunk_counts(n):
    a, b = g.rel_l1_inputs(n)
    sd, sb = g.rel_l1_counts(a, b)
    assert set(np.unique(a).tolist()) | set(np.unique(b).tolist()) <= {-1, 0, 1}
    assert 0 <= sb < 2 ** 24 and 0 <= sd < 2 ** 24            # fp32 holds every partial sum of either, in any order
    if n:
        assert 0.2 < np.mean(b != 0) < 0.45 or n < 64
    for tdt in (torch.bfloat16, torch.float16):
        ta, tb = torch.from_numpy(a).to(tdt), torch.from_numpy(b).to(tdt)
        assert float((ta.double() - tb.double()).abs().sum()) == sd and float(tb.double().abs().sum()) == sb
    # the mutants: any one 16-byte chunk dropped or counted twice moves both integers
    n16 = n // 8
    d8 = np.abs(a[:8 * n16].astype(np.int64) - b[:8 * n16]).reshape(n16, 8).sum(1)
    b8 = np.abs(b[:8 * n16].astype(np.int64)).reshape(n16, 8).sum(1)
    assert (d8 > 0).all() and (b8 > 0).all()
    for j in {0, (n // 8) * 8 - 1, n - 1}:
        if 0 <= j < n:
            assert a[j] != b[j] and b[j] != 0


def test_rel_l1_sizes_reach_the_grid_paths():
    n16 = {n // 8 for n in g.REL_L1_SIZES}
    assert {0, 255, 256, 257, 2048, 2049, g.RL1_CLAMP, g.RL1_CLAMP + 1} <= n16
    nwg = lambda k: min(max(-(-k // 2048), 1), 1024)
    assert nwg(2048) == 1 and nwg(2049) == 2 and nwg(g.RL1_CLAMP) == 1024 and -(-(g.RL1_CLAMP + 1) // 2048) > 1024
    for k, live in ((1380, (256, 100, 0, 0)), (6844, (1024, 1024, 700, 0))):
        stride = nwg(k) * 256
        last = (k - 1) // (4 * stride) * 4 * stride
        assert k in n16 and tuple(min(max(k - last - u * stride, 0), stride) for u in range(4)) == live
