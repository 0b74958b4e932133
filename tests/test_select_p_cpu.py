"""The top-p selection without a GPU: the vectorised reference of tests/select_p_ref.py against its naive
loop, the Python and C refusals (every C check precedes the first HIP call), the routing of top_p=None to the top-k entries, and
mutants of the reference, each of which must change the expected output of an exact-class case of tests/test_gpu_select_p.py."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import select_p_ref as pref
import select_ref as ref

NAMES = ("rsa_block_select_p_bytes", "rsa_block_select_p", "rsa_block_select_pooled_p_bytes", "rsa_block_select_pooled_p")


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_vectorised_reference_is_the_naive_loop_on_tie_heavy_grids(seed):
    """Scores from {-3 .. 0} (c = 1: weights 1, 1/2, 1/4, 1/8 of 2^18), random visible prefixes and forced sets, every p16 class."""
    g = np.random.default_rng(seed)
    B, Hl, NQ, NK = 2, 3, 4, (5, 37, 64, 130)[seed]
    t = g.integers(-3, 1, (B, Hl, NQ, NK)).astype(np.float64)
    nvis = g.integers(0, NK + 1, (B, NQ))
    vis = np.arange(NK)[None, None, :] < nvis[..., None]
    frc = vis & (g.random((B, NQ, NK)) < 0.1)
    u = pref.weights(t, vis, frc, np.float32(1.0))
    assert set(np.unique(u)) <= {0, pref.ONE, pref.ONE // 2, pref.ONE // 4, pref.ONE // 8}
    differ = 0
    for p16 in (0, 1, 13107, 32768, 58982, 65535, 65536):
        for top_k in (0, 1, 7, NK, NK + 5):
            a = pref.kept_vectorised(t, vis, frc, top_k, u, p16)
            b = pref.kept_naive(t, vis, frc, top_k, u, p16)
            assert np.array_equal(a, b), (p16, top_k)
            assert not (a & ~np.broadcast_to(vis[:, None], a.shape)).any() and not (frc[:, None] & ~a).any()
            for mut in pref.MUTANTS[:4] + pref.MUTANTS[5:]:       # (the t_max mutant acts in weights())
                am, bm = (f(t, vis, frc, top_k, u, p16, mut) for f in (pref.kept_vectorised, pref.kept_naive))
                assert np.array_equal(am, bm), (p16, top_k, mut)
                differ += int((am != a).any())
    assert differ > 0


def test_weights_are_the_contract():
    t = np.array([0.0, -1.0, -17.0, -18.0, -19.0, -20.0, -200.0, 5.0]).reshape(1, 1, 1, 8)
    vis = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool).reshape(1, 1, 8)
    u = pref.weights(t, vis, np.zeros_like(vis), np.float32(1.0))[0, 0, 0]
    assert u.tolist() == [1 << 18, 1 << 17, 2, 1, 1, 0, 0, 0]        # 2^-19 * 2^18 + 0.5 = 1; 2^-20 * 2^18 + 0.5 < 1
    assert pref.c_of(pref.SCALE_EXACT) == np.float32(1.0)
    assert pref.p16_of(0.0) == 0 and pref.p16_of(1.0) == 65536 and pref.p16_of(0.5) == 32768
    m = pref.mass_of(np.array([1, 1, 0, 0, 0, 0, 0, 0], bool).reshape(1, 1, 1, 8), u.reshape(1, 1, 1, 8))
    assert m.dtype == np.float32 and m[0, 0, 0] == np.float32(3 << 17) / np.float32((3 << 17) + 4)
    assert pref.mass_of(np.zeros((1, 1, 1, 8), bool), np.zeros((1, 1, 1, 8), np.int64))[0, 0, 0] == 0


_INPUTS = {}


def _reference(c, params, mut=""):
    if c["seed"] not in _INPUTS:        # (made once per case, read-only)
        q, k = pref.exact_inputs(c["B"], c["H"], c["Hkv"], c["Sq"], c["Sk"], c["D"], c["blk"], c["heads"], c["seed"])
        _INPUTS[c["seed"]] = (q, k, ref.scores(q, k, c["lens"], c["blk"], c["heads"]))
    q, k, t = _INPUTS[c["seed"]]
    top_p, tk, kf, kl = params
    return pref.select(q, k, pref.exact_top_k(tk, c["NK"]), top_p, score_scale=pref.SCALE_EXACT, blk=c["blk"], lens=c["lens"],
                       causal=c["causal"], keep_first=kf, keep_local=kl, mask_heads=c["heads"], t=t, mut=mut)


def test_every_mutant_changes_an_exact_class_case():
    changed = {m: 0 for m in pref.MUTANTS}
    for c in pref.exact_cases():
        for params in pref.EXACT_PARAMS:
            want = _reference(c, params)["mask"]
            for m in pref.MUTANTS:
                changed[m] += int((_reference(c, params, m)["mask"] != want).any(-1).sum())
    assert all(n > 0 for n in changed.values()), changed


def test_the_exact_class_holds_every_case_the_contract_names():
    """Counted on the reference: exact landings, plateaus of 6 .. 40 cut by ceil(rem / u_T) short of their end, forced blocks that
    alone pass the target, a cap that binds and one that does not, a tail of zero weights at top_p = 1, top_p = 0."""
    seen = dict(landing=0, plateau=0, forced_pass=0, cap_binds=0, cap_free=0, zero_tail=0, p_zero=0, blind=0)
    for c in pref.exact_cases():
        for params in pref.EXACT_PARAMS:
            r = _reference(c, params)
            top_p, tk, kf, kl = params
            vis, frc = (np.broadcast_to(a[:, None], r["mask"].shape) for a in (r["vis"], r["frc"]))
            u, kept = r["u"], r["mask"]
            total, fmass, got = u.sum(-1), np.where(frc, u, 0).sum(-1), np.where(kept, u, 0).sum(-1)
            target = (total * pref.p16_of(top_p) + 65535) >> 16
            n_k = np.maximum(pref.exact_top_k(tk, c["NK"]) - frc.sum(-1), 0)
            taken = (kept & ~frc).sum(-1)
            open_ = (fmass < target) & (total > 0)
            seen["landing"] += int((open_ & (got == target) & (taken > 0)).sum())
            seen["forced_pass"] += int(((fmass >= target) & (target > 0) & ((vis & ~frc).sum(-1) > 0)).sum())
            seen["cap_binds"] += int((open_ & (got < target) & (taken == n_k)).sum())
            seen["cap_free"] += int((open_ & (got >= target) & (taken < n_k)).sum())
            seen["p_zero"] += int(top_p == 0.0 and np.array_equal(kept, frc) and bool(frc.any()))
            seen["blind"] += int((vis.sum(-1) == 0).sum())
            if top_p == 1.0:
                seen["zero_tail"] += int(((vis & ~kept & (u == 0)).any(-1) & (got == total) & (total > 0)).sum())
            # a plateau across the cut: kept and dropped unforced blocks at one score, 6 .. 40 of them
            tt = np.where(vis & ~frc, r["t"], np.nan)
            low = np.nanmin(np.where(kept & ~frc, tt, np.nan), axis=-1, initial=np.inf, where=kept & ~frc)
            tie = (tt == low[..., None]) & ~frc & vis
            seen["plateau"] += int(((tie & ~kept).any(-1) & (tie.sum(-1) >= 6) & (tie.sum(-1) <= 40) & (got >= target)).sum())
    assert all(n > 0 for n in seen.values()), seen


def test_top_p_one_over_nonzero_weights_is_top_k():
    """Where every visible block has weight >= 1, top_p = 1 keeps the forced blocks and the best min(n_k, nunf) unforced ones, ties
    to the lower index: select_ref's mask.  On the reference alone; tests/test_gpu_select_p.py holds the kernels to it."""
    inputs = {}
    cases = ties = everything = 0
    for c in pref.plateau_cases():
        key = (c["blk"], c["NK"], c["Hkv"], c["heads"], c["Sq"])
        if key not in inputs:
            q, k = pref.plateau_inputs(c["B"], c["H"], c["Hkv"], c["Sq"], c["Sk"], c["D"], c["blk"], c["heads"], c["seed"])
            inputs[key] = (q, k, ref.scores(q, k, c["lens"], c["blk"], c["heads"]))
        q, k, t = inputs[key]
        for tk, kf, kl in pref.PLATEAU_BUDGETS:
            top_k = pref.exact_top_k(tk, c["NK"])
            kw = dict(blk=c["blk"], lens=c["lens"], causal=c["causal"], keep_first=kf, keep_local=kl, mask_heads=c["heads"])
            by_k = ref.select(q, k, top_k, **kw)
            by_p = pref.select(q, k, top_k, 1.0, score_scale=pref.SCALE_EXACT, t=t, **kw)
            what = (c, tk, kf, kl)
            assert np.array_equal(by_k["mask"], by_p["mask"]), what
            vis, frc = (np.broadcast_to(a[:, None], by_p["mask"].shape) for a in (by_p["vis"], by_p["frc"]))
            assert (by_p["u"][vis] >= 1).all(), what
            kept, cand = by_k["mask"], vis & ~frc
            low = np.where(kept & cand, by_k["t"], np.inf).min(-1, keepdims=True)    # the lowest kept unforced score of a row
            ties += int((cand & ~kept & (by_k["t"] == low)).any())
            everything += int(vis.any() and np.array_equal(kept, vis))
            cases += 1
    assert cases == 432 and ties > 0 and everything > 0, (cases, ties, everything)


# ---- 2. the Python refusals --------------------------------------------------------------------------------------------------------
def _q(Sq=3):
    return torch.zeros(2, 8, Sq, 64, dtype=torch.bfloat16)


def _calls():
    from rectified_spaattn_amd import select_blocks, select_blocks_pooled
    k, cache = torch.zeros(2, 2, 700, 64, dtype=torch.bfloat16), torch.zeros(2, 2, 6, 64)
    return [lambda **kw: select_blocks(_q(), k, 3, **kw), lambda **kw: select_blocks_pooled(_q(), cache, 3, **kw)]


def test_python_refusals_name_the_argument():
    for call in _calls():
        for bad in (-0.01, 1.01, float("nan"), "0.5", True, [0.5]):
            with pytest.raises(ValueError, match="top_p"):
                call(top_p=bad)
        for bad in (0.0, -1.0, float("inf"), float("nan"), "1", True, 1e-60, 1e39):
            with pytest.raises(ValueError, match="score_scale"):
                call(top_p=0.5, score_scale=bad)
        with pytest.raises(ValueError, match="score_scale"):
            call(score_scale=0.1)
        with pytest.raises(ValueError, match="return_mass"):
            call(return_mass=True)
        with pytest.raises(ValueError, match="keep_local"):        # (today's refusals stand beside top_p)
            call(top_p=0.5, keep_local=-1)


@pytest.mark.parametrize("kw", [dict(top_p=0.0), dict(top_p=1, return_mass=True), dict(top_p=0.9, score_scale=0.25, as_lists=True,
                                                                                        return_scores=True, return_mass=True)])
def test_a_well_formed_call_on_cpu_tensors_reaches_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib
    for call in _calls():
        with pytest.raises(_lib.RsaError):
            call(**kw)


# ---- 3. routing ------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands for the loaded library: records the entries that are called, returns RSA_OK."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.mark.parametrize("pooled", [False, True])
def test_top_p_none_runs_the_top_k_entries_and_top_p_the_new_ones(monkeypatch, pooled):
    from rectified_spaattn_amd import _core, _lib, block_sparse
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(_core, "_require_device", lambda *ts: None)
    monkeypatch.setattr(_core, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    call = _calls()[int(pooled)]
    old = "rsa_block_select_pooled" if pooled else "rsa_block_select"
    out = call(return_scores=True)
    assert [n for n, _ in rec.calls] == [old + "_bytes", old, "rsa_lists_to_block_mask"]
    assert isinstance(out, tuple) and len(out) == 2
    n_old = len(rec.calls[1][1])
    rec.calls.clear()
    out = call(top_p=0.5, return_scores=True, return_mass=True, as_lists=True)
    assert [n for n, _ in rec.calls] == [old + "_p_bytes", old + "_p"]
    args = rec.calls[1][1]
    assert len(args) == n_old + 3 and args[-4] == 32768 and args[-2] == out[2].data_ptr()
    g_l = 4                                             # H = 8 over Hl = Hkv = 2
    assert args[-3] == (1.0 / (g_l * 8.0)) * pref.LOG2_E     # score_scale defaults to 1 / (g_l sqrt(D)), D = 64
    assert set(out[0]) == {"bitmask", "cols", "counts"} and out[1].shape == (2, 2, 1, 6) and out[2].shape == (2, 2, 1)
    assert out[2].dtype == torch.float32
    rec.calls.clear()
    call(top_p=1.0, score_scale=0.5, mask_heads="q")
    args = rec.calls[1][1]
    assert args[-4] == 65536 and args[-3] == 0.5 * pref.LOG2_E and args[-2] is None


# ---- 4. the C entries ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_exported_and_the_version_stays():
    _lib, L = _lib_or_skip()
    assert all(n in _lib.EXPORTED and hasattr(L, n) for n in NAMES)
    at = [_lib.EXPORTED.index(n) for n in NAMES]
    assert at == list(range(at[0], at[0] + 4))
    assert L.rsa_version() == 601 and _lib.HEADER_VERSION == 601


def test_workspace_sizes_are_the_top_k_entries():
    _, L = _lib_or_skip()
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for new, old in ((L.rsa_block_select_p_bytes, L.rsa_block_select_bytes),
                     (L.rsa_block_select_pooled_p_bytes, L.rsa_block_select_pooled_bytes)):
        for shape in ((2, 2, 2, 128, 1, 6), (1, 8, 32, 128, 1, 1024), (3, 2, 2, 16, 5, 8192), (0, 2, 2, 128, 1, 6), (2, 2, 2, 96, 1, 6)):
            assert new(*shape, ctypes.byref(a)) == old(*shape, ctypes.byref(b)) and a.value == b.value
        assert new(2, 2, 2, 128, 1, 6, None) == -1


def test_c_entries_check_the_budget_and_everything_their_counterparts_check():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks
    big = 1 << 30

    def pooled(B=2, H=8, Hkv=2, Hl=2, Sq=1, D=128, dt=0, blk=128, NQ=1, NK=6, q=t, pk=p, kv=None, kvv=700, causal=0, top_k=2, kf=0,
               kl=0, splits=0, ws=p, wsb=big, bitmask=p, cols=p, counts=p, scores=None, p16=32768, c=1.0, mass=None):
        return L.rsa_block_select_pooled_p(B, H, Hkv, Hl, Sq, D, dt, blk, NQ, NK, q, pk, kv, kvv, causal, top_k, kf, kl, splits, ws,
                                           wsb, bitmask, cols, counts, scores, p16, c, mass, None)

    def plain(B=2, H=8, Hkv=2, Hl=2, Sq=1, Sk=700, D=128, dt=0, blk=128, NQ=1, NK=6, q=t, k=t, kv=None, kvv=700, causal=0, top_k=2,
              kf=0, kl=0, ws=p, wsb=big, bitmask=p, cols=p, counts=p, scores=None, p16=32768, c=1.0, mass=None):
        return L.rsa_block_select_p(B, H, Hkv, Hl, Sq, Sk, D, dt, blk, NQ, NK, q, k, kv, kvv, causal, top_k, kf, kl, ws, wsb,
                                    bitmask, cols, counts, scores, p16, c, mass, None)

    for call in (pooled, plain):
        for base in (dict(), dict(mass=p), dict(p16=0), dict(p16=65536, c=1e-30), dict(scores=p, kv=p)):
            f = lambda **kw: call(**{**base, **kw})   # noqa: E731
            # the budget
            assert f(p16=-1) == BAD and f(p16=65537) == BAD
            for c in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
                assert f(c=c) == BAD, c
            assert f(mass=ctypes.c_void_p(4098)) == BAD
            # the counterparts' refusals
            assert f(blk=96) == UNS and f(D=96) == UNS and f(dt=7) == UNS
            assert f(B=0) == BAD and f(Sq=0) == BAD and f(Hl=4) == BAD and f(NQ=2) == BAD
            assert f(top_k=-1) == BAD and f(kf=-1) == BAD and f(kl=-1) == BAD
            assert f(ws=None) == BAD and f(bitmask=None) == BAD and f(cols=None) == BAD and f(counts=None) == BAD
            assert f(cols=ctypes.c_void_p(4098)) == BAD and f(scores=ctypes.c_void_p(4098)) == BAD
            assert f(q=_lib.RsaTensor4(4100, 8 * 128, 128, 128)) == BAD
            assert f(wsb=0) == WS
            if "kv" not in base:
                assert f(kvv=-1) == BAD
    assert pooled(NK=8193) == UNS and pooled(splits=257) == BAD and pooled(pk=ctypes.c_void_p(4104)) == BAD
    assert plain(NK=7) == BAD and plain(Sk=8193 * 128, NK=8193) == UNS
