"""block_sparse_extend without a GPU: the numpy reference against the ranged call's rule, a naive loop and
decode's rule; the split merge of the model per row group; what a mutated model does to the witness cases; the Python refusals;
the C entries' presence, argument refusals, workspace sizes and default split (every call fails its host checks: nothing is
launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import decode_ref as dref
import extend_ref as ref
import test_ranged_cpu as ranged
import visibility as vis
from rectified_spaattn_amd import block_sparse_extend as ext

ENTRY, ENTRY8, BYTES = "rsa_block_sparse_extend", "rsa_block_sparse_extend_kv8", "rsa_block_sparse_extend_bytes"


# ---- the rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,lens", [(129, 700, [700, 333]), (300, 700, [400, 140]), (256, 300, [300, 0]), (130, 513, [513, 100])])
def test_rule_is_the_ranged_calls_at_several_query_blocks(Sq, Sk, lens):
    blk = 128
    NQ, NK = -(-Sq // blk), -(-Sk // blk)
    assert NQ > 1
    for Hl, NKm in ((1, NK), (3, NK), (3, max(NK - 1, 1))):
        mask = np.random.default_rng(Sq + Sk + Hl).random((2, Hl, NQ, NKm)) < 0.5
        for causal in (False, True):
            lo, hi = ranged.window_ranges(Sq, lens, -1, 0 if causal else -1)
            want = ranged.visible(mask, lo, hi, lens, Sq, Sk)
            assert np.array_equal(ref.visible(mask, lens, Sq, Sk, blk, Hl, causal), want), (Hl, NKm, causal)


@pytest.mark.parametrize("H,Hl", [(4, 1), (4, 2), (4, 4)])
def test_rule_is_the_naive_loop_at_64_token_blocks(H, Hl):
    Sq, Sk, lens = 70, 200, [200, 67]       # (item 1: the first rows have r + kv_len - Sq < 0)
    for NK in (4, 3):
        mask = np.random.default_rng(H + Hl + NK).random((2, Hl, 2, NK)) < 0.5
        for causal in (False, True):
            got = ref.visible(mask, lens, Sq, Sk, 64, H, causal)
            assert np.array_equal(got, ref.visible_naive(mask, lens, Sq, Sk, 64, H, causal))
            if causal:
                assert not got[1, :, :3].any() and got[1, :, 3:].any()


@pytest.mark.parametrize("Sq,blk", [(1, 128), (8, 64), (64, 64), (128, 128)])
def test_rule_is_decodes_at_one_query_block(Sq, blk):
    Sk, lens = 300, [300, 131]
    mask = np.random.default_rng(Sq).random((2, 2, 1, -(-Sk // blk))) < 0.5
    for causal in (False, True):
        assert np.array_equal(ref.visible(mask, lens, Sq, Sk, blk, 4, causal), dref.visible(mask, lens, Sq, Sk, blk, 4, causal))


def test_fast_scores_and_parts_are_decode_refs():
    g = np.random.default_rng(2)
    q, k, v = (g.standard_normal(s).astype(np.float32) for s in ((2, 6, 5, 8), (2, 2, 40, 8), (2, 2, 40, 8)))
    seen = g.random((2, 6, 5, 40)) < 0.5
    for dt in (None, "bf16", "fp16"):
        assert np.allclose(ref.scores2(q, k, 0.3, dt), dref.scores2(q, k, 0.3, dt), rtol=1e-13, atol=1e-13)
    s2 = dref.scores2(q, k, 0.3)
    for a, b in zip(ref.parts(s2, seen, v), dref.parts(s2, seen, v)):
        assert np.allclose(a, b, rtol=1e-13, atol=1e-13)


# ---- row groups ------------------------------------------------------------------------------------------------------------------
def test_row_groups_hold_at_most_64_rows_and_cover_every_row_once():
    from rectified_spaattn_amd.block_sparse import extend_row_groups
    for gu in (1, 2, 3, 4, 8, 9, 64, 65, 72, 200):
        for Sq, blk in ((1, 128), (8, 128), (65, 128), (128, 128), (129, 128), (300, 128), (300, 64), (64, 64), (65, 64)):
            gh, qg = ref.row_groups(gu, Sq, blk)
            assert 1 <= gh * qg <= 64 and qg <= min(Sq, blk)
            first, count = ref.group_rows(gu, Sq, blk)
            assert (count >= 1).all() and (count <= qg).all() and (first // blk == np.arange(Sq) // blk).all()
            assert (first + count - 1) .max() == Sq - 1 and ((first + count - 1) // blk == first // blk).all()
            lib = extend_row_groups(1, gu, 1, 1, Sq, blk)
            assert (lib["gh"], lib["qg"]) == (gh, qg)
            assert lib["groups"] == ref.group_count(1, gu, 1, 1, Sq, blk) == len(set(first.tolist())) * -(-gu // gh)
            assert lib["rows16"] == ref.rows16(gu, Sq, blk)
    # decode's ground: one group per unit, decode's row tiles
    assert ref.row_groups(4, 8, 128) == (4, 8) and ref.group_count(2, 8, 2, 2, 8, 128) == 4
    assert ref.row_groups(72, 5, 128) == (36, 1) and ref.group_count(1, 72, 1, 1, 5, 128) == 10


# ---- the split and merge model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_merged_splits_equal_the_unsplit_result_per_row_group(causal):
    g = np.random.default_rng(5)
    H, Hkv, Hl, Sq, Sk, D, blk, lens = 4, 2, 2, 150, 300, 8, 64, [300, 130]
    q = g.standard_normal((2, H, Sq, D)).astype(np.float32)
    k, v = (g.standard_normal((2, Hkv, Sk, D)).astype(np.float32) for _ in range(2))
    k[1, :, 130:] = np.nan
    v[1, :, 130:] = np.nan
    mask = g.random((2, Hl, 3, 5)) < 0.6
    s2 = ref.scores2(q, k, 0.3)
    seen = ref.visible(mask, lens, Sq, Sk, blk, H, causal)
    out, lse = ref.attention(s2, seen, v)
    assert np.isfinite(out).all()
    first, _ = ref.group_rows(H // max(Hl, Hkv), Sq, blk)
    assert len(set(first.tolist())) == 5        # 2 heads x 32 rows: 2 + 2 + 1 groups of a unit's three query blocks
    for C in (1, 2, 3, 5):
        pieces = ref.split_parts(s2, seen, v, mask, blk, C)
        assert len(pieces) == -(-5 // C)
        o2, l2 = dref.finish(*dref.merge(pieces))
        for f in sorted(set(first.tolist())):       # per row group
            rows = first == f
            assert np.allclose(o2[:, :, rows], out[:, :, rows], rtol=1e-12, atol=1e-13)
            assert np.allclose(l2[:, :, rows], lse[:, :, rows], rtol=1e-12, atol=1e-13)


# ---- the witness cases and the mutants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ref.VIS_CASES + ref.WEIGHT_CASES, ids=lambda c: c["id"])
def test_witness_cases_are_well_formed(c):
    inp = ref.case_inputs(c)
    assert inp["mask"].shape[2] >= 2
    for name in ("q", "k", "v"):
        assert np.array_equal(ref.weights.round_dt(inp[name], c["dt"]), inp[name]), name
    s2 = ref.scores2(inp["q"], inp["k"], inp["sm_scale"], c["dt"])
    if c["kind"] == "vis":
        assert (s2 == 0).all() and set(np.unique(inp["v"])) <= {0.0, 1.0}
    else:
        total, spread = ref.weight_budget(c, inp)
        assert total < 2.0 ** 24 and spread <= dref.SPREAD


def test_witness_cases_cover_what_they_are_for():
    cs = ref.VIS_CASES
    assert {(c["H"], c["Hkv"]) for c in cs} == set(ref.GROUPS)
    assert {c["dt"] for c in cs} == {"bf16", "fp16"} and {c["blk"] for c in cs} == {64, 128} and {c["D"] for c in cs} == {64, 128}
    assert {c["causal"] for c in cs} == {False, True}
    gus = {ref.case_groups(c)[0] for c in cs}
    assert 72 in gus and 1 in gus and any(1 < g < 64 for g in gus)
    # more than one row group in a query block; a group boundary at rows 63 / 64 of a unit's block; a ragged last group
    assert any((ref.case_groups(c)[1][:c["blk"]] > 0).any() for c in cs)
    assert any(ref.case_groups(c)[1][64] == 64 and ref.case_groups(c)[1][63] == 0 for c in cs)
    assert any(len(set(ref.case_groups(c)[2].tolist())) > 1 for c in cs)
    # rows that see nothing because r + kv_len - Sq < 0
    assert any(c["causal"] and min(c["lens"]) < c["Sq"] for c in cs)
    # probes of a causal case sit on the limits of the rows either side of a group boundary
    for c in cs:
        if c["causal"] and c["D"] == 128:
            inp = ref.vis_inputs(c)
            probes = ref.vis_probes(c, inp["mask"])
            _, first, _ = ref.case_groups(c)
            for r in [r for r in range(1, c["Sq"]) if first[r] == r][:2]:
                for n in c["lens"]:
                    for key in (r - 1 + n - c["Sq"], r + n - c["Sq"], r + n - c["Sq"] + 1):
                        assert not 0 <= key < ref.SK or key in probes, (c["id"], r, key)


MUTANTS = [("the mask row taken as (r + 1) // block", dict(mask_row="next")),
           ("the mask row taken from the first row of a run of 48 rows that straddles blocks", dict(mask_row=("run", 48))),
           ("the causal offset with the block's row count for Sq", dict(sq_as="block")),
           ("the causal offset with the group's row count for Sq", dict(sq_as="group")),
           ("the row's index in its block for its index in the call", dict(row_as="block")),
           ("the row's index in its group for its index in the call", dict(row_as="group")),
           ("the group's first row's limit for all its rows", dict(group_limit="first")),
           ("kv limit + 1", dict(kv_shift=1)), ("kv limit - 1", dict(kv_shift=-1)),
           ("causal limit + 1", dict(causal_shift=1)), ("causal limit - 1", dict(causal_shift=-1))]
CAUSAL_ONLY = ("sq_as", "row_as", "group_limit", "causal_shift")


@pytest.mark.parametrize("name,mut", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_model_mutants_move_the_witness_cases(name, mut):
    """Each mutation of the numpy model moves some element of some witness case by at least visibility.SENSITIVITY tolerances (no
    kernel is built in a mutated form: this shows that the GPU tests' inputs and bounds would see the same fault)."""
    worst = 0.0
    for c in ref.VIS_CASES + ref.WEIGHT_CASES:
        if any(key in mut for key in CAUSAL_ONLY) and not c["causal"]:
            continue
        inp = ref.case_inputs(c)
        out = ref.case_reference(c, inp)[0]
        got = ref.case_reference(c, inp, **mut)[0]
        worst = max(worst, float((np.abs(got - out) / vis.tolerance(out, vis.ULP[c["dt"]])).max()))
        if worst >= vis.SENSITIVITY:
            break
    assert worst >= vis.SENSITIVITY, (name, worst)


def test_a_dropped_partial_moves_every_split_case():
    """EVERY live split of every query block of a split case is watched."""
    seen_cases = 0
    for c in ref.VIS_CASES[::2] + ref.WEIGHT_CASES[::3]:
        inp = ref.case_inputs(c)
        out, lse, pieces = ref.case_reference(c, inp, want_pieces=True)
        o2, l2 = dref.finish(*dref.merge(pieces))
        assert np.allclose(o2, out, rtol=1e-12, atol=0) and np.allclose(l2, lse, rtol=1e-12, atol=1e-12)
        tol = vis.tolerance(out, vis.ULP[c["dt"]])
        live = np.flatnonzero(np.stack([p[1] for p in pieces]).reshape(len(pieces), -1).any(1))
        if len(live) < 2:
            continue
        seen_cases += 1
        for s in live:
            got = dref.finish(*dref.merge(pieces, drop=int(s)))[0]
            assert float((np.abs(got - out) / tol).max()) >= vis.SENSITIVITY, (c["id"], int(s))
    assert seen_cases >= 3


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) -------------------------------------------
def _qkv(B=2, H=8, Hkv=2, Sq=300, Sk=700, D=64, dt=torch.bfloat16):
    return (torch.zeros(B, H, Sq, D, dtype=dt), torch.zeros(B, Hkv, Sk, D, dtype=dt), torch.zeros(B, Hkv, Sk, D, dtype=dt))


def _mask(B=2, Hl=2, NQ=3, NK=6):
    return torch.ones(B, Hl, NQ, NK, dtype=torch.bool)


def test_block_sparse_extend_is_exported_from_the_package():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import block_sparse
    assert callable(ext) and callable(block_sparse.block_sparse_extend)
    assert "block_sparse_extend" in dir(rectified_spaattn_amd)


def test_python_refusals():
    q, k, v = _qkv()
    m = _mask()
    with pytest.raises(NotImplementedError, match="block_size"):
        ext(q, k, v, m, block_size=96)
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            ext(*_qkv(D=D), m)
    with pytest.raises(ValueError, match="head dim"):
        ext(*_qkv(D=48), m)
    with pytest.raises(ValueError, match="Hkv"):
        ext(*_qkv(H=8, Hkv=3), m)
    with pytest.raises(ValueError, match="dtype"):
        ext(q, k.float(), v, m)
    with pytest.raises(ValueError, match="empty"):
        ext(q[:, :, :0], k, v, _mask(NQ=1))
    # the mask for NQ = 3 query blocks: dtype, rank, batch axis, query blocks, head axis, key blocks
    for bad in (m.float(), m[0], _mask(B=3), _mask(NQ=1), _mask(NQ=2), _mask(NQ=4)):
        with pytest.raises(ValueError, match="block_mask"):
            ext(q, k, v, bad)
    with pytest.raises(ValueError, match="block_mask"):
        ext(q, k, v, _mask(NQ=3, NK=11), block_size=64)        # 5 query blocks of 64
    with pytest.raises(ValueError, match="head axis"):
        ext(q, k, v, _mask(Hl=4))
    with pytest.raises(ValueError, match="key blocks"):
        ext(q, k, v, _mask(NK=7))
    # the lists for NQ = 3: both tensors, int32, [B * Hl, 3, NK] and [B * Hl, 3], contiguous
    cols, counts = torch.zeros(4, 3, 6, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int32)
    for bad in (dict(cols=cols), dict(cols=cols.long(), counts=counts),
                dict(cols=cols[:, :1].contiguous(), counts=counts[:, :1].contiguous()),
                dict(cols=cols, counts=counts[:, :1].contiguous()), dict(cols=cols[:3], counts=counts[:3]),
                dict(cols=cols.transpose(0, 1).contiguous().transpose(0, 1), counts=counts)):
        with pytest.raises(ValueError, match="block_mask"):
            ext(q, k, v, bad)
    # scales belong to an e4m3 cache, and an e4m3 cache needs both
    with pytest.raises(ValueError, match="scales belong"):
        ext(q, k, v, m, k_scale=1.0, v_scale=1.0)
    k8, v8 = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="required"):
        ext(q, k8, v8, m)
    with pytest.raises(ValueError, match="required"):
        ext(q, k8, v8, m, k_scale=1.0)
    with pytest.raises(ValueError, match="e4m3 cache"):
        ext(q, k8, v, m, k_scale=1.0, v_scale=1.0)
    for kv_len in (701, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="kv_len"):
            ext(q, k, v, m, kv_len=kv_len)
    for bps in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="blocks_per_split"):
            ext(q, k, v, m, blocks_per_split=bps)
    pool = torch.zeros(9, 2, 128, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block_table"):
        ext(q, pool, pool, m, block_table=torch.zeros(2, 6, dtype=torch.int64))
    with pytest.raises(ValueError, match="not copied"):
        ext(q, k.transpose(2, 3).contiguous().transpose(2, 3), v, m)


@pytest.mark.parametrize("kw", [dict(), dict(causal=True, kv_len=[700, 333], return_lse=True), dict(block_size=64, blocks_per_split=2),
                                dict(lists=True), dict(paged=True), dict(heads72=True), dict(kv8=True)],
                         ids=["plain", "causal-lens-lse", "block64-split", "lists", "paged", "72-heads-in-a-unit", "e4m3"])
def test_a_well_formed_call_on_cpu_tensors_reaches_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors.  Neither Sq = 300 nor 72 heads in a unit is refused."""
    from rectified_spaattn_amd import _lib
    kw = dict(kw)
    q, k, v = _qkv(H=72, Hkv=1) if kw.pop("heads72", False) else _qkv()
    Hl = k.shape[1]
    m = _mask(Hl=Hl, NQ=5, NK=11) if kw.get("block_size") == 64 else _mask(Hl=Hl)
    if kw.pop("lists", False):
        m = dict(cols=torch.zeros(4, 3, 6, dtype=torch.int32), counts=torch.zeros(4, 3, dtype=torch.int32))
    if kw.pop("paged", False):
        k = v = torch.zeros(15, 2, 128, 64, dtype=torch.bfloat16)
        kw["block_table"] = torch.zeros(2, 6, dtype=torch.int32)
    if kw.pop("kv8", False):
        k, v = k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)
        kw.update(k_scale=0.5, v_scale=torch.ones(2))
    with pytest.raises(_lib.RsaError):
        ext(q, k, v, m, **kw)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_declared_listed_last_and_exported_and_the_version_stays():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    for name in (ENTRY, ENTRY8, BYTES):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
    assert _lib.EXPORTED[-3:] == (BYTES, ENTRY, ENTRY8)
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    _, L = _lib_or_skip()
    assert all(hasattr(L, name) for name in (ENTRY, ENTRY8, BYTES))
    assert L.rsa_version() == 601


def test_workspace_size_query_and_the_default_split_on_both_sides_of_its_switch():
    from rectified_spaattn_amd.block_sparse import extend_default_split, extend_row_groups
    _, L = _lib_or_skip()
    n = ctypes.c_size_t(0)

    def size(B, H, Hkv, Hl, Sq, D, blk, NK, bps):
        st = L.rsa_block_sparse_extend_bytes(B, H, Hkv, Hl, Sq, D, blk, NK, bps, ctypes.byref(n))
        return n.value if st == 0 else st
    part = lambda rows16, D: rows16 * (D + 2) * 4       # noqa: E731  fp32 O, m, l per row of a partial
    # decode's ground: the decode entry's sizes at an explicit split
    for shape, bps in (((2, 8, 2, 2, 1, 128), 2), ((2, 8, 2, 8, 3, 64), 1), ((1, 8, 1, 1, 3, 64), 3), ((1, 8, 1, 1, 8, 64), 3)):
        B, H, Hkv, Hl, Sq, D = shape
        NK = 6
        assert L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hl, Sq, D, NK, bps, ctypes.byref(n)) == 0
        assert size(B, H, Hkv, Hl, Sq, D, 128, NK, bps) == n.value
    # 2 x 2 units of 4 heads, Sq = 300 at 128: 16 rows a group, 8 + 8 + 3 groups a unit; 3 splits
    assert size(2, 8, 2, 2, 300, 128, 128, 6, 2) == 4 * 19 * 3 * part(64, 128)
    assert size(2, 8, 2, 2, 300, 128, 64, 11, 11) == 4 * (4 * 4 + 3) * 1 * part(64, 128)
    # 72 heads in one unit: two chunks of 36 heads, one query row a group
    assert size(1, 72, 1, 1, 5, 64, 128, 6, 6) == 10 * part(64, 64)
    assert size(1, 72, 1, 72, 5, 64, 128, 6, 6) == 72 * part(16, 64)
    # the documented default, a function of the shapes alone: min(8, NK) below 256 row groups, one split from there on
    for shape in ((1, 32, 8, 8, 16, 128, 128, 1024), (1, 32, 8, 8, 496, 128, 128, 1024), (1, 32, 8, 8, 497, 128, 128, 1024),
                  (1, 32, 8, 8, 2048, 128, 128, 1024), (8, 32, 8, 8, 64, 128, 128, 256), (2, 8, 2, 2, 300, 64, 64, 5),
                  (1, 72, 1, 1, 127, 64, 128, 700), (1, 72, 1, 1, 128, 64, 128, 700)):
        B, H, Hkv, Hl, Sq, D, blk, NK = shape
        g = extend_row_groups(B, H, Hkv, Hl, Sq, blk)
        assert g["groups"] == ref.group_count(B, H, Hkv, Hl, Sq, blk)
        C = extend_default_split(g["groups"], NK)
        assert C == ref.default_split(g["groups"], NK) == (min(8, NK) if g["groups"] < 256 else NK)
        want = g["groups"] * -(-NK // C) * part(g["rows16"], D)
        assert size(*shape, 0) == size(*shape, C) == want, shape
    groups = [ref.group_count(*s)
              for s in ((1, 32, 8, 8, 496, 128), (1, 32, 8, 8, 497, 128), (1, 72, 1, 1, 127, 128), (1, 72, 1, 1, 128, 128))]
    assert groups == [248, 256, 254, 256]       # (both sides of the switch)
    assert L.rsa_block_sparse_extend_bytes(2, 8, 2, 2, 1, 128, 128, 6, 2, None) == -1
    for bad in ((0, 8, 2, 2, 1, 128, 128, 6, 2), (2, 8, 3, 3, 1, 128, 128, 6, 2), (2, 8, 2, 4, 1, 128, 128, 6, 2),
                (2, 8, 2, 2, 0, 128, 128, 6, 2), (2, 8, 2, 2, 1, 128, 128, 0, 2), (2, 8, 2, 2, 1, 128, 128, 8193, 2),
                (2, 8, 2, 2, 1, 128, 128, 6, -1)):
        assert size(*bad) == -1, bad
    for uns in ((2, 8, 2, 2, 1, 96, 128, 6, 2), (2, 8, 2, 2, 1, 32, 128, 6, 2), (2, 8, 2, 2, 1, 128, 96, 6, 2),
                (1 << 20, 8, 8, 8, 1 << 20, 64, 64, 6, 2),          # 2^37 row groups
                (1 << 10, 64, 1, 1, 1 << 24, 64, 128, 6, 2)):       # the merge's grid: B H Sq D / 1024 = 2^34
        assert size(*uns) == -2, uns
    assert size(1 << 10, 64, 1, 1, 1 << 14, 64, 128, 6, 6) > 0      # (2^24 row groups are served)


@pytest.mark.parametrize("entry", [ENTRY, ENTRY8])
def test_entry_checks_its_arguments(entry):
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    kv8 = entry == ENTRY8
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    o = _lib.RsaOut4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks
    big = 1 << 40

    def call(B=1, H=8, Hkv=2, Hl=2, Sq=300, Sk=700, D=128, dt=0, blk=128, NK=6, kv=None, kvv=700, causal=0, scale=0.1, q=t, k=t, v=t,
             table=None, tsb=6, pages=0, cols=p, counts=p, bps=0, ws=p, wsb=big, out=o, lse=None, ks=p, vs=p):
        tail = (ks, vs, None) if kv8 else (None,)
        return getattr(L, entry)(B, H, Hkv, Hl, Sq, Sk, D, dt, blk, NK, kv, kvv, causal, scale, q, k, v, table, tsb, pages, cols,
                                 counts, bps, ws, wsb, out, lse, *tail)

    for kw in (dict(H=0), dict(Hkv=0), dict(Hl=0), dict(Hl=-1), dict(Hkv=3, Hl=3), dict(Hl=4), dict(H=6, Hkv=4, Hl=4)):
        assert call(**kw) == BAD, kw
    for base in (dict(), dict(Hl=8), dict(Hl=1), dict(Hkv=1, Hl=1), dict(causal=1), dict(lse=p), dict(kv=p), dict(table=p, pages=20),
                 dict(bps=2), dict(Sq=1), dict(H=144, Hkv=2, Hl=2)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(D=96) == UNS
        assert c(D=32) == UNS
        assert c(dt=7) == UNS
        assert c(B=0) == BAD
        assert c(Sq=0) == BAD
        assert c(Sk=0) == BAD
        assert c(NK=0) == BAD
        assert c(NK=7) == BAD                        # more than ceil(Sk / block)
        assert c(blk=64, NK=12) == BAD
        assert c(bps=-1) == BAD
        assert c(ws=None) == BAD
        assert c(ws=ctypes.c_void_p(4104)) == BAD    # 16-byte alignment
        assert c(cols=None) == BAD
        assert c(counts=None) == BAD
        assert c(cols=ctypes.c_void_p(4098)) == BAD
        assert c(lse=ctypes.c_void_p(4098)) == BAD
        assert c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(table=p, pages=0) == BAD
        assert c(table=p, pages=20, tsb=-6) == BAD
        assert c(q=_lib.RsaTensor4(None, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(v=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        assert c(out=_lib.RsaOut4(None, 8 * 128, 128, 128)) == BAD
        assert c(out=_lib.RsaOut4(4096, 8 * 128, 130, 128)) == BAD
        assert c(wsb=0) == WS                        # every argument passes: Sq = 300 and 72 heads a unit are served
        if kv8:
            assert c(ks=None) == BAD and c(vs=ctypes.c_void_p(4098)) == BAD
        if "kv" not in base:
            assert c(kvv=-1) == BAD
            assert c(kvv=701) == BAD
    # what decode refuses is served: more than one query block, more than 64 rows per unit
    assert call(Sq=129, wsb=0) == WS and call(Sq=17, wsb=0) == WS and call(Hkv=1, Hl=1, Sq=9, wsb=0) == WS
    assert call(Sq=65, blk=64, NK=11, wsb=0) == WS
    # beyond the grid
    assert call(B=1 << 20, H=8, Hkv=8, Hl=8, Sq=1 << 20, blk=64, NK=6) == UNS
    # the workspace: exactly what the query reports is enough for the checks, one byte less is not
    n = ctypes.c_size_t(0)
    for bps in (0, 1, 4):
        assert L.rsa_block_sparse_extend_bytes(1, 8, 2, 2, 300, 128, 128, 6, bps, ctypes.byref(n)) == 0
        assert call(bps=bps, wsb=n.value - 1) == WS
        assert call(bps=bps, wsb=n.value, blk=96) == UNS
