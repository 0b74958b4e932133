"""The ragged calls without a device: the rule of tests/ragged_ref.py -- the existing rule per truncated
item, embedded -- against its direct form and a naive loop; mutants of the rule and of the selection contract, each of which must
move a witness element by visibility.SENSITIVITY tolerances or change a kept list; the Python and C refusals; and that q_len changes
neither the workspace nor the default split."""
import contextlib
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import extend_ref as eref
import ragged_ref as ref
import visibility as vis
from rectified_spaattn_amd import block_sparse_decode as dec
from rectified_spaattn_amd import block_sparse_extend as ext
from rectified_spaattn_amd import select_blocks, select_blocks_pooled

B, SQ, SK = ref.B, ref.SQ, ref.SK
ENTRIES = ("rsa_block_sparse_extend_ragged", "rsa_block_sparse_extend_ragged_kv8", "rsa_block_select_ragged",
           "rsa_block_select_pooled_ragged")


# ---- the visibility rule ---------------------------------------------------------------------------------------------------------
RULE_CASES = [(128, ref.QLENS[0], True), (64, ref.QLENS[0], True), (128, ref.QLENS[1], True), (64, ref.QLENS[1], False),
              (128, ref.clamp(ref.RAW_QLEN, SQ), True)]


@pytest.mark.parametrize("blk,q_lens,causal", RULE_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_rule_is_the_truncated_calls_and_the_naive_loop(blk, q_lens, causal):
    H, Hl = 2, 2
    lens = [SK, 40, 333, 129]
    assert any(ln < n for ln, n in zip(lens, q_lens)), "one item is shorter than its chunk"
    NQ, NK = -(-SQ // blk), -(-SK // blk)
    mask = np.random.default_rng(blk + sum(q_lens)).random((B, Hl, NQ, NK)) < 0.6
    emb = ref.visible(mask, lens, q_lens, SQ, SK, blk, H, causal)
    assert np.array_equal(emb, ref.visible_direct(mask, lens, q_lens, SQ, SK, blk, H, causal))
    assert np.array_equal(emb, ref.visible_naive(mask, lens, q_lens, SQ, SK, blk, H, causal))
    for b, n in enumerate(q_lens):
        assert not emb[b, :, n:].any()
    # q_len = Sq everywhere is the existing rule
    full = ref.visible(mask, lens, [SQ] * B, SQ, SK, blk, H, causal)
    assert np.array_equal(full, eref.visible(mask, lens, SQ, SK, blk, H, causal))


def test_clamp_and_the_sets():
    assert ref.clamp(ref.RAW_QLEN, SQ) == [128, 129, SQ, 0]
    for c in ref.gpu_combos():
        ns = ref.clamp(ref.combo_qlens(c), SQ)
        lens = ref.combo_lens(c, ns)
        assert any(ln < n for ln, n in zip(lens, ns)) and max(lens) == SK and all(ln >= 0 for ln in lens)


@pytest.mark.parametrize("c", ref.WITNESS_CASES, ids=lambda c: c["id"])
def test_witness_cases_are_well_formed(c):
    inp = ref.witness_inputs(c)
    out, lse = ref.witness_reference(c, inp)
    out2, lse2 = ref.witness_reference(c, inp, mut="")
    assert np.array_equal(out, out2) and np.array_equal(lse, lse2)
    for b, n in enumerate(c["q_lens"]):
        assert (out[b, :, n:] == 0).all() and np.isneginf(lse[b, :, n:]).all()
    assert len(ref.witness_probes(c)) >= 6
    assert (out != 0).any()


@pytest.mark.parametrize("mut", ref.MUTANTS)
def test_rule_mutants_move_a_witness_element(mut):
    """Each mutation of the rule moves some element of some witness case by at least visibility.SENSITIVITY tolerances."""
    worst = 0.0
    for c in ref.WITNESS_CASES:
        inp = ref.witness_inputs(c)
        out = ref.witness_reference(c, inp)[0]
        got = ref.witness_reference(c, inp, mut=mut)[0]
        worst = max(worst, float((np.abs(got - out) / vis.tolerance(out, vis.ULP[c["dt"]])).max()))
        if worst >= vis.SENSITIVITY:
            break
    assert worst >= vis.SENSITIVITY, (mut, worst)


# ---- the selection ---------------------------------------------------------------------------------------------------------------
def _select_inputs(seed, H=4, Hkv=2, D=32):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, H, SQ, D))
    k = rng.standard_normal((B, Hkv, SK, D)) + 0.5 * rng.standard_normal((B, Hkv, SK // 50 + 1, D)).repeat(50, 2)[:, :, :SK]
    return q, k


SELECT_KW = [dict(top_k=3, blk=128, causal=True, keep_first=1, keep_local=1), dict(top_k=4, blk=64, causal=True),
             dict(top_k=2, blk=128, causal=False, mask_heads="q"), dict(top_k=6, top_p=0.6, blk=64, causal=True, keep_first=1, keep_local=1),
             dict(top_k=5, top_p=0.8, blk=128, causal=False)]


@pytest.mark.parametrize("kw", SELECT_KW, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
@pytest.mark.parametrize("qset", range(3))
def test_selection_contract_with_n_is_the_truncated_selection(kw, qset):
    kw = dict(kw)
    top_k = kw.pop("top_k")
    q_lens = ref.clamp((ref.QLENS + (ref.RAW_QLEN,))[qset], SQ)
    lens = [SK, 40, 333, 129]
    q, k = _select_inputs(7 + qset)
    q_nan = q.copy()
    for b, n in enumerate(q_lens):
        q_nan[b, :, n:] = np.nan        # (the truncated reference never sees them; the direct form zeroes them)
    a = ref.select(q_nan, k, top_k, q_lens, lens=lens, **kw)
    d = ref.select_direct(q_nan, k, top_k, q_lens, lens=lens, **kw)
    assert np.array_equal(a["mask"], d["mask"])
    assert np.array_equal(np.isneginf(a["t"]), np.isneginf(d["t"]))
    fin = np.isfinite(a["t"])
    assert np.allclose(a["t"][fin], d["t"][fin], rtol=1e-12, atol=1e-12)
    if a["mass"] is not None:
        assert np.array_equal(a["mass"], d["mass"])
    blk = kw["blk"]
    for b, n in enumerate(q_lens):
        nq = ref.live_blocks(n, blk)
        assert not a["mask"][b, :, nq:].any() and np.isneginf(a["t"][b, :, nq:]).all()
        assert a["mass"] is None or (a["mass"][b, :, nq:] == 0).all()


@pytest.mark.parametrize("mut", ref.SELECT_MUTANTS)
def test_selection_mutants_change_a_kept_list(mut):
    """The divisor of the pooled mean scales a row's scores by one positive factor, which no top-k ranking sees: the top-p budget
    does (its weights are exp2 of score differences).  The two others move the visible and forced sets."""
    changed = 0
    for qset in range(3):
        q_lens = ref.clamp((ref.QLENS + (ref.RAW_QLEN,))[qset], SQ)
        q, k = _select_inputs(7 + qset)
        for kw in SELECT_KW:
            kw = dict(kw)
            if (mut == "mean over the full block") != ("top_p" in kw) or (mut != "mean over the full block" and not kw["causal"]):
                continue
            top_k = kw.pop("top_k")
            if "top_p" in kw:
                kw["top_k"] = top_k
                args = (q * 8.0, k, kw.pop("top_k"))       # (larger logits: the budget binds before the cap)
            else:
                args = (q, k, top_k)
            want = ref.select_direct(*args, q_lens, lens=[SK, 40, 333, 129], **kw)["mask"]
            got = ref.select_direct(*args, q_lens, lens=[SK, 40, 333, 129], mut=mut, **kw)["mask"]
            changed += int(not np.array_equal(want, got))
    assert changed >= 1, mut


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def _qkv(Bn=B, H=8, Hkv=2, Sq=SQ, Sk=SK, D=64, dt=torch.bfloat16):
    return (torch.zeros(Bn, H, Sq, D, dtype=dt), torch.zeros(Bn, Hkv, Sk, D, dtype=dt), torch.zeros(Bn, Hkv, Sk, D, dtype=dt))


def test_q_len_is_a_keyword_of_three_calls_and_not_of_decode():
    for fn in (ext, select_blocks, select_blocks_pooled):
        par = inspect.signature(fn).parameters["q_len"]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert "q_len" not in inspect.signature(dec).parameters
    q, k, v = _qkv(Sq=1)
    with pytest.raises(TypeError, match="q_len"):
        dec(q, k, v, torch.ones(B, 2, 1, 6, dtype=torch.bool), q_len=[1] * B)
    assert "block_sparse_extend" in dec.__doc__ and "q_len" in dec.__doc__


def test_python_refusals_in_kv_lens_wording():
    q, k, v = _qkv()
    m = torch.ones(B, 2, 3, 6, dtype=torch.bool)
    pooled = torch.zeros(B, 2, 6, 64)
    calls = (lambda **kw: ext(q, k, v, m, **kw), lambda **kw: select_blocks(q, k, 2, **kw),
             lambda **kw: select_blocks_pooled(q, pooled, 2, **kw))
    for call in calls:
        for bad in (SQ + 1, -1, [1, 2, 3], [1, 2, 3, SQ + 1], torch.tensor([1, 2, 3]), (0, 0, 0, -1)):
            with pytest.raises(ValueError, match="q_len"):
                call(q_len=bad)
        with pytest.raises(ValueError, match=rf"q_len \[.*\] outside \[0, {SQ}\]"):
            call(q_len=SQ + 1)
        with pytest.raises(ValueError, match=f"q_len: 3 values for a batch of {B}"):
            call(q_len=[1, 2, 3])
        with pytest.raises(ValueError, match="kv_len"):      # (kv_len is still checked, and first)
            call(kv_len=-1, q_len=-1)


class _Recorder:
    """Stands for the loaded library: records the entries that are called, returns RSA_OK."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def rec(monkeypatch):
    from rectified_spaattn_amd import _core, _lib
    r = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: r)
    monkeypatch.setattr(_core, "_require_device", lambda *ts: None)
    monkeypatch.setattr(_core, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return r


def test_routing_none_and_full_lengths_run_the_existing_entries(rec):
    q, k, v = _qkv()
    lists = dict(cols=torch.zeros(B * 2, 3, 6, dtype=torch.int32), counts=torch.zeros(B * 2, 3, dtype=torch.int32))
    pooled = torch.zeros(B, 2, 6, 64)
    k8 = k.to(torch.float8_e4m3fn)

    def names(fn):
        rec.calls.clear()
        fn()
        return [n for n, _ in rec.calls], [len(a) for _, a in rec.calls]
    for q_len, sfx in ((None, ""), ([SQ] * B, ""), (SQ, ""), ([SQ, 1, 0, 5], "_ragged"), (7, "_ragged"),
                       (torch.tensor([300, 1, 0, 5]), "_ragged")):
        n, a = names(lambda: ext(q, k, v, lists, q_len=q_len, blocks_per_split=2))
        assert n == ["rsa_block_sparse_extend_bytes", "rsa_block_sparse_extend" + sfx], (q_len, n)
        assert a[1] == 28 + bool(sfx)
        n8, a8 = names(lambda: ext(q, k8, k8, lists, q_len=q_len, k_scale=1.0, v_scale=1.0))
        assert n8[1] == "rsa_block_sparse_extend" + sfx + "_kv8" and a8[1] == 30 + bool(sfx)
        assert a[0] == 10 and a8[0] == 10           # the workspace query never sees q_len
        for top_p, old in ((None, ""), (0.5, "_p")):
            n, a = names(lambda: select_blocks(q, k, 2, q_len=q_len, top_p=top_p, as_lists=True))
            assert n == ["rsa_block_select" + old + "_bytes", "rsa_block_select" + (sfx or old)]
            assert a[1] == (30 if sfx else 26 + 3 * bool(old))
            n, a = names(lambda: select_blocks_pooled(q, pooled, 2, q_len=q_len, top_p=top_p, as_lists=True))
            assert n == ["rsa_block_select_pooled" + old + "_bytes", "rsa_block_select_pooled" + (sfx or old)]
            if sfx:      # p16 = -1 names plain top-k
                assert (rec.calls[1][1][25] == -1) == (top_p is None)


def test_workspace_and_default_split_do_not_depend_on_q_len(rec):
    from rectified_spaattn_amd.block_sparse import extend_default_split, extend_row_groups
    assert "q_len" not in inspect.signature(extend_row_groups).parameters
    assert "q_len" not in inspect.signature(extend_default_split).parameters
    q, k, v = _qkv()
    lists = dict(cols=torch.zeros(B * 2, 3, 6, dtype=torch.int32), counts=torch.zeros(B * 2, 3, dtype=torch.int32))
    seen = []
    for q_len in (None, [1, 0, 0, 1], 1, torch.tensor([1])):
        for bps in (None, 2):
            rec.calls.clear()
            ext(q, k, v, lists, q_len=q_len, blocks_per_split=bps)
            (_, size_args), (_, args) = rec.calls
            seen.append((bps, size_args[:9], args[22], args[24]))       # the size query, blocks_per_split, ws_bytes
    for bps in (None, 2):
        assert len({s[1:] for s in seen if s[0] == bps}) == 1


# ---- the C entries -----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_declared_exported_and_the_version_stays():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and name in _lib.EXPORTED
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    # the ragged prototypes are their counterparts' with one pointer in front of the stream
    P = _lib.PROTOTYPES
    for new, old in zip(ENTRIES, ("rsa_block_sparse_extend", "rsa_block_sparse_extend_kv8", "rsa_block_select_p",
                                  "rsa_block_select_pooled_p")):
        assert P[new] == (P[old][0], P[old][1][:-1] + [_lib.vp, _lib.vp])
    _, L = _lib_or_skip()
    assert all(hasattr(L, name) for name in ENTRIES) and L.rsa_version() == 601


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_extend_entries_check_q_len_and_everything_the_extend_entries_check(entry):
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    kv8 = entry.endswith("_kv8")
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    o = _lib.RsaOut4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks

    def call(Bn=4, Sq=300, blk=128, NK=6, kv=None, kvv=700, bps=0, wsb=1 << 40, ql=p, D=128):
        tail = (p, p) if kv8 else ()
        return getattr(L, entry)(Bn, 8, 2, 2, Sq, 700, D, 0, blk, NK, kv, kvv, 1, 0.1, t, t, t, None, 6, 0, p, p, bps, p, wsb, o, None,
                                 *tail, ql, None)
    n = ctypes.c_size_t(0)
    for ql in (p, None):
        assert call(ql=ql, wsb=0) == WS             # every argument passes, with row counts and without
        assert call(ql=ql, Bn=0) == BAD and call(ql=ql, Sq=0) == BAD and call(ql=ql, NK=7) == BAD and call(ql=ql, kvv=701) == BAD
        assert call(ql=ql, blk=96) == UNS and call(ql=ql, D=32) == UNS
        for bps in (0, 1, 4):       # the workspace is the extend call's: exactly what its query reports, not a byte less
            assert L.rsa_block_sparse_extend_bytes(4, 8, 2, 2, 300, 128, 128, 6, bps, ctypes.byref(n)) == 0
            assert call(ql=ql, bps=bps, wsb=n.value - 1) == WS
    for bad in (4097, 4098, 4099):
        assert call(ql=ctypes.c_void_p(bad), wsb=0) == BAD


@pytest.mark.parametrize("entry", ENTRIES[2:])
def test_select_entries_check_q_len_the_budget_and_everything_their_counterparts_check(entry):
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    pooled = "pooled" in entry
    t = _lib.RsaTensor4(4096, 8 * 128 * 300, 128 * 300, 128)
    tk = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    p = ctypes.c_void_p(4096)

    def call(Bn=4, Sq=300, D=128, blk=128, NQ=3, NK=6, kvv=700, top_k=2, wsb=1 << 30, p16=-1, c=0.0, mass=None, ql=p):
        if pooled:
            return getattr(L, entry)(Bn, 8, 2, 2, Sq, D, 0, blk, NQ, NK, t, p, None, kvv, 1, top_k, 0, 0, 0, p, wsb, p, p, p, None,
                                     p16, c, mass, ql, None)
        return getattr(L, entry)(Bn, 8, 2, 2, Sq, 700, D, 0, blk, NQ, NK, t, tk, None, kvv, 1, top_k, 0, 0, p, wsb, p, p, p, None,
                                 p16, c, mass, ql, None)
    for ql in (p, None):
        assert call(ql=ql, wsb=0) == WS                                 # plain top-k: c and mass are not looked at
        assert call(ql=ql, wsb=0, c=float("nan"), mass=ctypes.c_void_p(4098)) == WS
        assert call(ql=ql, wsb=0, p16=32768, c=1.0) == WS and call(ql=ql, wsb=0, p16=0, c=1.0, mass=p) == WS
        for kw in (dict(p16=-2, c=1.0), dict(p16=65537, c=1.0), dict(p16=1, c=0.0), dict(p16=1, c=float("inf")),
                   dict(p16=1, c=1.0, mass=ctypes.c_void_p(4098)), dict(Bn=0), dict(Sq=0), dict(NQ=2), dict(NK=5), dict(top_k=-1),
                   dict(kvv=-1)):
            assert call(ql=ql, **kw) == BAD, kw
        assert call(ql=ql, blk=96) == UNS and call(ql=ql, D=48) == UNS
    for bad in (4097, 4098, 4099):
        assert call(ql=ctypes.c_void_p(bad), wsb=0) == BAD
