"""The packed calls without a device: the rule of tests/packed_ref.py -- the existing extend rule per item
at the rows a sanitised cu_seqlens_q gives it -- against its direct form and a naive loop, malformed cu_seqlens_q included; the
bound QP on the row groups of a launch against the true maximum; mutants of the rule and of the selection, each of which must move
a witness element by visibility.SENSITIVITY tolerances or change a kept list; the Python and C refusals; and that workspace and
split depend on (T, B, M) alone."""
import contextlib
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import extend_ref as eref
import packed_ref as ref
import ragged_ref as rref
import visibility as vis
from rectified_spaattn_amd import append_kv_e4m3, select_blocks, select_blocks_pooled
from rectified_spaattn_amd import block_sparse_extend as ext

B, T, SK = ref.B, ref.T, ref.SK
ENTRIES = ("rsa_block_sparse_extend_packed", "rsa_block_sparse_extend_packed_kv8", "rsa_block_select_pooled_packed",
           "rsa_kv8_append_packed", "rsa_block_sparse_extend_packed_bytes")
LENS = [SK, 40, 333, 129]


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_sanitise_orders_clamps_and_caps():
    for cu, M in [ref.malformed(kind) for kind in ref.MALFORMED] + [(ref.cu_of(ls, gap), M) for ls, M, gap in ref.LSETS]:
        s, ns = ref.sanitise(cu, T, M)
        assert s == sorted(s) and 0 <= s[0] and s[-1] <= T and all(0 <= n <= M for n in ns)
        item, row = ref.row_items(cu, T, M)
        for b, n in enumerate(ns):      # disjoint ranges: every row belongs to one item at most
            assert (item[s[b]:s[b] + n] == b).all() and (item == b).sum() == n
    assert ref.sanitise(ref.malformed("a decreasing pair")[0], T, 128) == ([0, 100, 100, 200, 290], [100, 0, 100, 90])
    assert ref.sanitise(ref.malformed("a value above T")[0], T, 150) == ([5, 70, 300, 300, 300], [65, 150, 0, 0])
    assert ref.sanitise(ref.malformed("a negative value")[0], T, 128) == ([0, 0, 64, 65, 193], [0, 64, 1, 128])
    assert ref.sanitise(ref.malformed("an item longer than M")[0], T, 100) == ([0, 10, 250, 251, 300], [10, 100, 1, 49])
    for ls, M, gap in ref.LSETS:
        assert ref.sanitise(ref.cu_of(ls, gap), T, M)[1] == list(ls) and gap + sum(ls) <= T


RULE_CASES = [(blk, ref.cu_of(ls, gap), M, causal) for blk in (128, 64) for (ls, M, gap), causal in zip(ref.LSETS, (True, True, blk == 64))]
RULE_CASES += [(blk, *ref.malformed(kind), True) for blk, kind in zip((128, 64, 128, 64), ref.MALFORMED)]


@pytest.mark.parametrize("blk,cu,M,causal", RULE_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_rule_is_the_truncated_calls_the_direct_form_and_the_naive_loop(blk, cu, M, causal):
    H, Hl = 2, 2
    s, ns = ref.sanitise(cu, T, M)
    NQ, NK = -(-M // blk), -(-SK // blk)
    mask = np.random.default_rng(blk + sum(ns)).random((B, Hl, NQ, NK)) < 0.6
    emb = ref.visible(mask, LENS, cu, T, M, SK, blk, H, causal)
    assert np.array_equal(emb, ref.visible_direct(mask, LENS, cu, T, M, SK, blk, H, causal))
    assert np.array_equal(emb, ref.visible_naive(mask, LENS, cu, T, M, SK, blk, H, causal))
    item, _ = ref.row_items(cu, T, M)
    assert not emb[item < 0].any()
    # the padded copy: the ragged rule with q_len = n_b, row for row
    padded = rref.visible(mask, LENS, ns, M, SK, blk, H, causal)
    for b, n in enumerate(ns):
        assert np.array_equal(emb[s[b]:s[b] + n], padded[b, :, :n].transpose(1, 0, 2))


def test_one_length_set_has_an_item_shorter_than_its_chunk():
    for ls, M, gap in ref.LSETS[::2]:
        assert any(ln < n for ln, n in zip(LENS, ls))


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def _group_shapes():
    out = set()
    for H, Hkv in eref.GROUPS:
        for Hl in (H, Hkv, 1):
            out.add(H // max(Hl, Hkv))
    return sorted(out)


@pytest.mark.parametrize("blk", (64, 128))
def test_no_sanitised_cu_seqlens_asks_for_more_row_groups_than_the_bound(blk):
    """For every (gh, qg) extend_ref.GROUPS produces, M in {1, 21, 64, 128, 200}, every T <= 3 * block and B <= 4: the maximum of
    sum pieces(n_b) over all length vectors with n_b <= M and sum n_b <= T (dynamic programming: one pass gives every T, one
    round more every B) is <= QP, and QP <= B * pieces(M)."""
    from rectified_spaattn_amd.block_sparse import packed_row_groups
    Tmax = 3 * blk
    seen = set()
    tight = 0
    for gu in _group_shapes():
        for M in (1, 21, 64, 128, 200):
            gh, qg, cpb = ref.groups_of(gu, M, blk)
            if (qg, M) in seen:
                continue
            seen.add((qg, M))
            p = np.array([ref.pieces(n, blk, qg, cpb) for n in range(min(M, Tmax) + 1)])
            best = np.zeros(Tmax + 1, np.int64)
            for Bn in range(1, 5):
                new = best.copy()
                for n in range(1, len(p)):
                    new[n:] = np.maximum(new[n:], best[:Tmax + 1 - n] + p[n])
                best = new
                for Tn in range(M, Tmax + 1):
                    qp = ref.qp_bound(Tn, Bn, M, qg, blk)
                    assert best[Tn] <= qp <= Bn * ref.pieces(M, blk, qg, cpb), (gu, M, Bn, Tn, int(best[Tn]), qp)
                    tight += int(best[Tn] == qp)
            if M == 21:         # (the vectorised passes above against the plain form)
                assert int(best[Tmax]) == ref.max_pieces(Tmax, 4, M, qg, blk)
    assert tight > 0        # (the bound is met somewhere: it is not vacuous)
    # the published form and the library's agree with the reference
    for H, Hkv in eref.GROUPS:
        for Hl in (H, Hkv, 1):
            for Tn, Bn, M in ((300, 4, 150), (8, 8, 1), (576, 8, 512), (300, 4, 128)):
                g = packed_row_groups(Tn, Bn, H, Hkv, Hl, M, blk)
                gh, qg, cpb = ref.groups_of(H // max(Hl, Hkv), M, blk)
                assert (g["gh"], g["qg"], g["pieces_per_block"]) == (gh, qg, cpb)
                assert g["pieces"] == ref.qp_bound(Tn, Bn, M, qg, blk)
                assert g["groups"] == g["pieces"] * max(Hl, Hkv) * g["head_chunks"]
    assert packed_row_groups(8, 8, 32, 8, 8, 1, 128)["pieces"] == 8 and packed_row_groups(8, 8, 32, 8, 8, 1, 128)["qg"] == 1


# ---- mutants -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.WITNESS_CASES, ids=lambda c: c["id"])
def test_witness_cases_are_well_formed(c):
    inp = ref.witness_inputs(c)
    out, lse = ref.witness_reference(c, inp)
    out2, lse2 = ref.witness_reference(c, inp, mut="")
    assert np.array_equal(out, out2) and np.array_equal(lse, lse2)
    item, _ = ref.row_items(c["cu"], T, c["M"])
    assert (out[item < 0] == 0).all() and np.isneginf(lse[item < 0]).all() and (item < 0).any()
    assert len(ref.witness_probes(c)) >= 6 and (out != 0).any()


@pytest.mark.parametrize("mut", ref.MUTANTS)
def test_rule_mutants_move_a_witness_element(mut):
    worst = 0.0
    for c in ref.WITNESS_CASES:
        inp = ref.witness_inputs(c)
        out = ref.witness_reference(c, inp)[0]
        got = ref.witness_reference(c, inp, mut=mut)[0]
        worst = max(worst, float((np.abs(got - out) / vis.tolerance(out, vis.ULP[c["dt"]])).max()))
        if worst >= vis.SENSITIVITY:
            break
    assert worst >= vis.SENSITIVITY, (mut, worst)


SELECT_KW = [dict(top_k=3, blk=128, causal=True, keep_first=1, keep_local=1), dict(top_k=4, blk=64, causal=True),
             dict(top_k=6, top_p=0.6, blk=64, causal=True, keep_first=1, keep_local=1)]


def _select_inputs(seed, H=4, Hkv=2, D=32):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((T, H, D))
    k = rng.standard_normal((B, Hkv, SK, D)) + 0.5 * rng.standard_normal((B, Hkv, SK // 50 + 1, D)).repeat(50, 2)[:, :, :SK]
    return q, k


def test_selection_is_the_ragged_selection_on_the_padded_copy():
    for (ls, M, gap), kw in zip(ref.LSETS, SELECT_KW):
        kw = dict(kw)
        top_k = kw.pop("top_k")
        cu = ref.cu_of(ls, gap)
        q, k = _select_inputs(11 + M)
        item, _ = ref.row_items(cu, T, M)
        q[item < 0] = np.nan
        got = ref.select(q, k, top_k, cu, T, M, lens=LENS, **kw)
        want = rref.select(ref.pad(q, cu, T, M), k, top_k, list(ls), lens=LENS, **kw)
        assert np.array_equal(got["mask"], want["mask"]) and got["mask"].any()


@pytest.mark.parametrize("mut", ref.SELECT_MUTANTS)
def test_selection_mutants_change_a_kept_list(mut):
    changed = 0
    for (ls, M, gap) in ref.LSETS:
        cu = ref.cu_of(ls, gap)
        q, k = _select_inputs(11 + M)
        for kw in SELECT_KW:
            kw = dict(kw)
            top_k = kw.pop("top_k")
            want = ref.select(q, k, top_k, cu, T, M, lens=LENS, **kw)["mask"]
            got = ref.select(q, k, top_k, cu, T, M, lens=LENS, mut=mut, **kw)["mask"]
            changed += int(not np.array_equal(want, got))
    assert changed >= 1, mut


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def _ops(H=8, Hkv=2, D=64, dt=torch.bfloat16):
    return (torch.zeros(T, H, D, dtype=dt), torch.zeros(B, Hkv, SK, D, dtype=dt), torch.zeros(B, Hkv, SK, D, dtype=dt))


CU = torch.tensor(ref.cu_of(*ref.LSETS[0][::2]), dtype=torch.int32)


def test_the_keywords():
    for fn in (ext, select_blocks_pooled):
        for name in ("cu_seqlens_q", "max_q_len"):
            par = inspect.signature(fn).parameters[name]
            assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert inspect.signature(append_kv_e4m3).parameters["cu_seqlens"].default is None
    assert "cu_seqlens_q" not in inspect.signature(select_blocks).parameters        # the prefill tool stays padded


def test_python_refusals():
    q, k, v = _ops()
    m = torch.ones(B, 2, 2, 6, dtype=torch.bool)
    pooled = torch.zeros(B, 2, 6, 64)
    q4 = torch.zeros(B, 8, 150, 64, dtype=torch.bfloat16)
    calls = (lambda q=q, **kw: ext(q, k, v, m, **kw), lambda q=q, **kw: select_blocks_pooled(q, pooled, 2, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="packed"):         # a 4-d q with cu_seqlens_q, a 3-d q without
            call(q=q4, cu_seqlens_q=CU, max_q_len=150)
        with pytest.raises(ValueError, match="4-d tensors"):
            call()
        with pytest.raises(ValueError, match="q_len belongs to a padded q"):
            call(cu_seqlens_q=CU, max_q_len=150, q_len=[1] * B)
        for bad in (0, T + 1, None, 1.0, True):
            with pytest.raises(ValueError, match="max_q_len"):
                call(cu_seqlens_q=CU, max_q_len=bad)
        for bad in (CU.to(torch.int64), CU[:-1], torch.cat([CU, CU]), CU.tolist(), CU.float()):
            with pytest.raises(ValueError, match="cu_seqlens_q: a device int32 tensor of B \\+ 1 = 5 values"):
                call(cu_seqlens_q=bad, max_q_len=150)
        with pytest.raises(ValueError, match="max_q_len belongs to cu_seqlens_q"):
            call(q=q4, max_q_len=150)
    kc = torch.zeros(B, 2, SK, 64, dtype=torch.float8_e4m3fn)
    kn = torch.zeros(T, 2, 64, dtype=torch.bfloat16)
    kw = dict(start=0, k_scale=1.0, v_scale=1.0)
    with pytest.raises(ValueError, match="n_new belongs to a padded k_new"):
        append_kv_e4m3(kn, kn, kc, kc, cu_seqlens=CU, n_new=1, **kw)
    with pytest.raises(ValueError, match="4-d tensors"):
        append_kv_e4m3(kn, kn, kc, kc, **kw)
    with pytest.raises(ValueError, match="packed"):
        append_kv_e4m3(kn[None], kn[None], kc, kc, cu_seqlens=CU, **kw)
    with pytest.raises(ValueError, match="cu_seqlens: a device int32 tensor of B \\+ 1 = 5 values"):
        append_kv_e4m3(kn, kn, kc, kc, cu_seqlens=CU[:-1], **kw)


class _Recorder:
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


def test_routing_and_that_workspace_and_split_see_host_values_alone(rec):
    q, k, v = _ops()
    lists = dict(cols=torch.zeros(B * 2, 2, 6, dtype=torch.int32), counts=torch.zeros(B * 2, 2, dtype=torch.int32))
    pooled = torch.zeros(B, 2, 6, 64)
    k8 = k.to(torch.float8_e4m3fn)
    seen = set()
    for cu in (CU, torch.zeros(B + 1, dtype=torch.int32), torch.tensor([9, -4, 10 ** 6, 3, 3], dtype=torch.int32)):
        rec.calls.clear()
        ext(q, k, v, lists, cu_seqlens_q=cu, max_q_len=150, blocks_per_split=None)
        (n0, a0), (n1, a1) = rec.calls
        assert (n0, n1) == ("rsa_block_sparse_extend_packed_bytes", "rsa_block_sparse_extend_packed")
        assert a0[:10] == (T, B, 8, 2, 2, 150, 64, 128, 6, 0) and len(a1) == 30 and a1[:6] == (T, B, 8, 2, 2, 150)
        seen.add((a0[:10], a1[23], a1[25]))         # the size query, blocks_per_split, ws_bytes
        rec.calls.clear()
        ext(q, k8, k8, lists, cu_seqlens_q=cu, max_q_len=150, k_scale=1.0, v_scale=1.0)
        assert rec.calls[1][0] == "rsa_block_sparse_extend_packed_kv8" and len(rec.calls[1][1]) == 32
        for top_p in (None, 0.5):
            rec.calls.clear()
            select_blocks_pooled(q, pooled, 2, cu_seqlens_q=cu, max_q_len=150, top_p=top_p, as_lists=True)
            (n0, a0), (n1, a1) = rec.calls
            assert n0 == "rsa_block_select_pooled" + ("_p" if top_p else "") + "_bytes" and a0[:6] == (B, 2, 2, 64, 2, 6)
            assert n1 == "rsa_block_select_pooled_packed" and len(a1) == 32 and (a1[26] == -1) == (top_p is None)
        rec.calls.clear()
        append_kv_e4m3(q[:, :2], q[:, :2], k8, k8, start=0, cu_seqlens=cu, k_scale=1.0, v_scale=1.0)
        assert rec.calls[0][0] == "rsa_kv8_append_packed" and len(rec.calls[0][1]) == 21 and rec.calls[0][1][:3] == (B, 2, T)
    assert len(seen) == 1
    # a view of a fused projection [T, (H + 2 Hkv) D] is read where it lies
    fused = torch.zeros(T, (8 + 4) * 64, dtype=torch.bfloat16)
    qv = fused[:, :8 * 64].view(T, 8, 64)
    rec.calls.clear()
    ext(qv, k, v, lists, cu_seqlens_q=CU, max_q_len=150)
    t4 = rec.calls[1][1][15]
    assert (t4.ptr, t4.stride_h, t4.stride_s) == (fused.data_ptr(), 64, 12 * 64)


def test_workspace_and_split_of_the_library_depend_on_T_B_M_alone():
    from rectified_spaattn_amd import _lib
    from rectified_spaattn_amd.block_sparse import extend_default_split, packed_row_groups
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    L = _lib.lib()
    assert list(inspect.signature(packed_row_groups).parameters) == ["T", "B", "H", "Hkv", "Hl", "max_q_len", "block_size"]
    n, p = ctypes.c_size_t(0), ctypes.c_int64(0)
    for (Tn, Bn, H, Hkv, Hl, M, D, blk, NK) in ((300, 4, 8, 2, 2, 150, 128, 128, 6), (576, 8, 32, 8, 8, 512, 128, 128, 256),
                                                (8, 8, 32, 8, 8, 1, 128, 128, 256), (300, 4, 72, 1, 1, 128, 64, 64, 11)):
        g = packed_row_groups(Tn, Bn, H, Hkv, Hl, M, blk)
        for bps in (0, 1, 2):
            assert L.rsa_block_sparse_extend_packed_bytes(Tn, Bn, H, Hkv, Hl, M, D, blk, NK, bps, ctypes.byref(n), ctypes.byref(p)) == 0
            assert p.value == g["pieces"]
            C = bps or extend_default_split(g["groups"], NK)
            head = (2 * (Bn + 1) * 4 + 15) // 16 * 16
            assert n.value == head + g["groups"] * -(-NK // C) * g["rows16"] * (D + 2) * 4


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
    P = _lib.PROTOTYPES
    i32, vp = _lib.i32, _lib.vp
    # the packed extend prototypes are the ragged ones with T in front; the selection has T in front and the scratch behind cu
    for new, old in zip(ENTRIES[:2], ("rsa_block_sparse_extend_ragged", "rsa_block_sparse_extend_ragged_kv8")):
        assert P[new] == (P[old][0], [i32] + P[old][1])
    old = P["rsa_block_select_pooled_ragged"]
    assert P[ENTRIES[2]] == (old[0], [i32] + old[1][:-1] + [vp, vp])
    assert _lib.EXPORTED[-3:] == ("rsa_block_sparse_extend_bytes", "rsa_block_sparse_extend", "rsa_block_sparse_extend_kv8")
    _, L = _lib_or_skip()
    assert all(hasattr(L, name) for name in ENTRIES) and L.rsa_version() == 601


@pytest.mark.parametrize("entry", ENTRIES[:2])
def test_extend_entries_refuse_before_the_first_hip_call(entry):
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    kv8 = entry.endswith("_kv8")
    tq = _lib.RsaTensor4(4096, 0, 128, 8 * 128)
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    o = _lib.RsaOut4(4096, 0, 128, 8 * 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks

    def call(Tn=300, Bn=4, M=150, blk=128, NK=6, kvv=700, bps=0, wsb=0, cu=p, D=128):
        tail = (p, p) if kv8 else ()
        return getattr(L, entry)(Tn, Bn, 8, 2, 2, M, 700, D, 0, blk, NK, None, kvv, 1, 0.1, tq, t, t, None, 6, 0, p, p, bps, p, wsb, o,
                                 None, *tail, cu, None)
    assert call() == WS             # every argument passes
    n = ctypes.c_size_t(0)
    for bps in (0, 1, 4):
        assert L.rsa_block_sparse_extend_packed_bytes(300, 4, 8, 2, 2, 150, 128, 128, 6, bps, ctypes.byref(n), None) == 0
        assert call(bps=bps, wsb=n.value - 1) == WS
    for kw in (dict(Tn=0), dict(M=0), dict(M=301), dict(Tn=149), dict(Bn=0), dict(NK=7), dict(kvv=701), dict(cu=None),
               dict(cu=ctypes.c_void_p(4097)), dict(cu=ctypes.c_void_p(4098)), dict(bps=-1)):
        assert call(**kw) == BAD, kw
    assert call(blk=96) == UNS and call(D=32) == UNS
    assert L.rsa_block_sparse_extend_packed_bytes(300, 4, 8, 2, 2, 301, 128, 128, 6, 0, ctypes.byref(n), None) == BAD
    assert L.rsa_block_sparse_extend_packed_bytes(300, 4, 8, 2, 2, 150, 128, 128, 6, 0, None, None) == BAD


def test_select_entry_refuses_before_the_first_hip_call():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    tq = _lib.RsaTensor4(4096, 0, 128, 8 * 128)
    p = ctypes.c_void_p(4096)

    def call(Tn=300, Bn=4, M=150, D=128, blk=128, NQ=2, NK=6, kvv=700, top_k=2, wsb=0, p16=-1, c=0.0, mass=None, cu=p, items=p):
        return L.rsa_block_select_pooled_packed(Tn, Bn, 8, 2, 2, M, D, 0, blk, NQ, NK, tq, p, None, kvv, 1, top_k, 0, 0, 0, p, wsb, p, p,
                                                p, None, p16, c, mass, cu, items, None)
    assert call() == WS and call(p16=32768, c=1.0) == WS
    for kw in (dict(Tn=0), dict(M=0), dict(M=301), dict(Bn=0), dict(NQ=3), dict(NK=5), dict(top_k=-1), dict(kvv=-1), dict(cu=None),
               dict(items=None), dict(cu=ctypes.c_void_p(4098)), dict(items=ctypes.c_void_p(4097)), dict(p16=-2, c=1.0),
               dict(p16=1, c=0.0)):
        assert call(**kw) == BAD, kw
    assert call(blk=96) == UNS and call(D=48) == UNS


def test_append_entry_refuses_before_the_first_hip_call():
    _lib, L = _lib_or_skip()
    BAD, UNS = -1, -2
    tn = _lib.RsaTensor4(4096, 0, 128, 2 * 128)
    oc = _lib.RsaOut4(4096, 2 * 700 * 128, 700 * 128, 128)
    p = ctypes.c_void_p(4096)

    def call(Bn=4, Tn=300, Sk=700, D=128, blk=128, start=0, cu=p, items=p, ks=p):
        return L.rsa_kv8_append_packed(Bn, 2, Tn, Sk, D, 0, blk, tn, tn, oc, oc, None, 0, 0, None, start, cu, items, ks, p, None)
    for kw in (dict(Bn=0), dict(Tn=0), dict(Sk=0), dict(start=701), dict(start=-1), dict(cu=None), dict(items=None),
               dict(cu=ctypes.c_void_p(4098)), dict(items=ctypes.c_void_p(4099)), dict(ks=None)):
        assert call(**kw) == BAD, kw
    assert call(blk=96) == UNS and call(D=32) == UNS
