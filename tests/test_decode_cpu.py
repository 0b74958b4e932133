"""block_sparse_decode without a GPU: the numpy reference against the ranged call's rule and a naive
loop, the split merge and the paged gather of the model, the witness cases' own preconditions and what a mutated model does to
them, the Python refusals, and the C entries' presence and argument refusals (every call fails its host checks: nothing is
launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import decode_ref as ref
import test_ranged_cpu as ranged
import visibility as vis

ENTRY, BYTES = "rsa_block_sparse_decode", "rsa_block_sparse_decode_bytes"


# ---- the rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq,Sk,lens", [(1, 700, [700, 333]), (3, 700, [129, 2]), (8, 300, [300, 0]), (128, 513, [513, 200])])
def test_rule_is_the_ranged_calls_at_one_query_block(Sq, Sk, lens):
    blk = 128
    NK = -(-Sk // blk)
    for Hl, NKm in ((1, NK), (3, NK), (3, max(NK - 1, 1))):
        mask = np.random.default_rng(Sq + Sk + Hl).random((2, Hl, 1, NKm)) < 0.5
        for causal in (False, True):
            lo, hi = ranged.window_ranges(Sq, lens, -1, 0 if causal else -1)
            want = ranged.visible(mask, lo, hi, lens, Sq, Sk)
            assert np.array_equal(ref.visible(mask, lens, Sq, Sk, blk, Hl, causal), want), (Hl, NKm, causal)


@pytest.mark.parametrize("H,Hl", [(4, 1), (4, 2), (4, 4)])
def test_rule_is_the_naive_loop_at_64_token_blocks(H, Hl):
    Sq, Sk, lens = 5, 200, [200, 67]
    for NK in (4, 3):
        mask = np.random.default_rng(H + Hl + NK).random((2, Hl, 1, NK)) < 0.5
        for causal in (False, True):
            assert np.array_equal(ref.visible(mask, lens, Sq, Sk, 64, H, causal),
                                  ref.visible_naive(mask, lens, Sq, Sk, 64, H, causal))


def _random_case(seed, H=4, Hkv=2, Hl=2, Sq=3, Sk=300, D=8, blk=64, lens=(300, 130)):
    g = np.random.default_rng(seed)
    q = g.standard_normal((2, H, Sq, D)).astype(np.float32)
    k = g.standard_normal((2, Hkv, Sk, D)).astype(np.float32)
    v = g.standard_normal((2, Hkv, Sk, D)).astype(np.float32)
    mask = g.random((2, Hl, 1, -(-Sk // blk))) < 0.6
    return q, k, v, mask, list(lens)


@pytest.mark.parametrize("causal", [False, True])
def test_merged_splits_equal_the_unsplit_result(causal):
    q, k, v, mask, lens = _random_case(5)
    k[1, :, 130:] = np.nan
    v[1, :, 130:] = np.nan
    s2 = ref.scores2(q, k, 0.3)
    seen = ref.visible(mask, lens, 3, 300, 64, 4, causal)
    out, lse = ref.attention(s2, seen, v)
    assert np.isfinite(out).all()
    for C in (1, 2, 3, 5):
        pieces = ref.split_parts(s2, seen, v, mask, 64, C)
        assert len(pieces) == -(-5 // C)
        o2, l2 = ref.finish(*ref.merge(pieces))
        assert np.allclose(o2, out, rtol=1e-12, atol=1e-13) and np.allclose(l2, lse, rtol=1e-12, atol=1e-13)
    # the log-sum-exp is the natural one
    b, h, r = 0, 1, 2
    s = s2[b, h, r][seen[b, h, r]] / ref.LOG2E
    assert np.isclose(lse[b, h, r], np.log(np.exp(s).sum()))


def test_a_row_without_a_visible_key_is_zero_and_minus_infinity():
    q, k, v, mask, _ = _random_case(6)
    lens = [2, 0]
    seen = ref.visible(mask | True, lens, 3, 300, 64, 4, True)
    assert not seen[0, :, 0].any() and seen[0, :, 1].any() and not seen[1].any()
    out, lse = ref.attention(ref.scores2(q, k, 0.3), seen, v)
    assert (out[0, :, 0] == 0).all() and np.isneginf(lse[0, :, 0]).all() and (out[1] == 0).all() and np.isneginf(lse[1]).all()
    assert np.isfinite(lse[0, :, 1:]).all()


@pytest.mark.parametrize("blk", [64, 128])
def test_paged_gather_of_a_permuted_pool_is_the_contiguous_cache(blk):
    g = np.random.default_rng(blk)
    cache = g.standard_normal((2, 2, 700, 8)).astype(np.float32)
    NK = -(-700 // blk)
    P = 2 * NK + 3
    pool, table = ref.make_pool(cache, blk, P, g.permutation(P))
    assert len(set(table.reshape(-1).tolist())) == 2 * NK
    back = ref.gather(pool, table)
    assert back.shape == (2, 2, NK * blk, 8)
    assert np.array_equal(back[:, :, :700], cache) and np.isnan(back[:, :, 700:]).all()
    spare = np.setdiff1d(np.arange(P), table.reshape(-1))
    assert len(spare) == 3 and np.isnan(pool[spare]).all()
    table[1, 2] = P + 5
    assert np.isnan(ref.gather(pool, table)[1, :, 2 * blk:3 * blk]).all()


# ---- the witness cases: their own preconditions, and what a mutated model does to them --------------------------------------------
@pytest.mark.parametrize("c", ref.VIS_CASES + ref.WEIGHT_CASES, ids=lambda c: c["id"])
def test_witness_cases_are_well_formed(c):
    inp = ref.case_inputs(c)
    rows = c["Sq"] * c["H"] // max(c["Hl"], c["Hkv"])
    assert rows <= 64
    for name in ("q", "k", "v"):        # exact in the storage type
        assert np.array_equal(ref.weights.round_dt(inp[name], c["dt"]), inp[name]), name
    s2 = ref.scores2(inp["q"], inp["k"], inp["sm_scale"], c["dt"])
    if c["kind"] == "vis":
        assert (s2 == 0).all() and set(np.unique(inp["v"])) <= {0.0, 1.0}
    else:
        total, spread = ref.weight_budget(c, inp)
        assert total < 2.0 ** 24 and spread <= ref.SPREAD
    out, lse, pieces = ref.case_reference(c, inp)
    o2, l2 = ref.finish(*ref.merge(pieces))
    assert np.allclose(o2, out, rtol=1e-12, atol=0) and np.allclose(l2, lse, rtol=1e-12, atol=1e-12)


def test_witness_cases_cover_what_they_are_for():
    cs = ref.VIS_CASES
    for H, Hkv in ref.GROUPS:
        mine = [c for c in cs if (c["H"], c["Hkv"]) == (H, Hkv)]
        assert {c["dt"] for c in mine} == {"bf16", "fp16"} and {c["blk"] for c in mine} == {64, 128}
        assert {c["D"] for c in mine} == {64, 128} and {c["causal"] for c in mine} == {False, True}
    assert any(c["Sq"] * c["H"] // max(c["Hl"], c["Hkv"]) == 64 for c in cs)
    # weights: a row whose maximum sits in the last split, one in the first, a +8 step at a split edge
    last = first = step = 0
    for c in ref.WEIGHT_CASES:
        inp = ref.weight_inputs(c)
        _, _, pieces = ref.case_reference(c, inp)
        ms = np.stack([p[0] for p in pieces])
        live = np.stack([p[1] for p in pieces]) > 0
        if len(pieces) < 2:
            continue
        top = np.where(live, ms, -np.inf)
        arg = top.argmax(0)
        nlive = live.sum(0)
        lastlive = len(pieces) - 1 - live[::-1].argmax(0)
        last += int(((arg == lastlive) & (nlive > 1) & (top.max(0) > np.sort(top, 0)[-2])).sum())
        first += int(((arg == live.argmax(0)) & (nlive > 1)).sum())
        with np.errstate(invalid="ignore"):
            step += int((np.diff(top, axis=0) == 8).sum())
    assert last > 0 and first > 0 and step > 0


MUTANTS = [("kv limit + 1", dict(kv_shift=1), None), ("kv limit - 1", dict(kv_shift=-1), None),
           ("causal top-left", dict(top_left=True), None), ("a split's partial dropped", {}, "drop"),
           ("a merge factor off by one step", {}, "bump")]


@pytest.mark.parametrize("name,mut,merge_mut", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_model_mutants_move_the_witness_cases(name, mut, merge_mut):
    """Each mutation of the numpy model moves some element of some witness case by at least visibility.SENSITIVITY tolerances
    (no kernel is built in a mutated form: this shows that the GPU tests' inputs and bounds would see the same fault)."""
    worst = 0.0
    for c in ref.VIS_CASES + ref.WEIGHT_CASES:
        if "top_left" in mut and not c["causal"]:
            continue
        inp = ref.case_inputs(c)
        out, _, pieces = ref.case_reference(c, inp)
        tol = vis.tolerance(out, vis.ULP[c["dt"]])
        if merge_mut is None:
            got = ref.case_reference(c, inp, **mut)[0]
            worst = max(worst, float((np.abs(got - out) / tol).max()))
            continue
        live = np.flatnonzero(np.stack([p[1] for p in pieces]).reshape(len(pieces), -1).any(1))
        if len(live) < 2:
            continue
        for s in live:
            got = ref.finish(*ref.merge(pieces, **{merge_mut: int(s)}))[0]
            moved = float((np.abs(got - out) / tol).max())
            assert moved >= vis.SENSITIVITY, (c["id"], int(s), moved)      # EVERY split of every split case is watched
            worst = max(worst, moved)
    assert worst >= vis.SENSITIVITY, (name, worst)


# ---- the Python refusals (CPU tensors: each is refused before the device is asked for) -------------------------------------------
def _qkv(B=2, H=8, Hkv=2, Sq=1, Sk=700, D=64, dt=torch.bfloat16):
    return (torch.zeros(B, H, Sq, D, dtype=dt), torch.zeros(B, Hkv, Sk, D, dtype=dt), torch.zeros(B, Hkv, Sk, D, dtype=dt))


def _mask(B=2, Hl=2, NK=6):
    return torch.ones(B, Hl, 1, NK, dtype=torch.bool)


def test_block_sparse_decode_is_exported_from_the_package():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import block_sparse, block_sparse_decode
    assert callable(block_sparse_decode) and callable(block_sparse.block_sparse_decode)
    assert "block_sparse_decode" in dir(rectified_spaattn_amd)


def test_python_refusals():
    from rectified_spaattn_amd import block_sparse_decode as dec
    q, k, v = _qkv()
    m = _mask()
    with pytest.raises(NotImplementedError, match="block_size"):
        dec(q, k, v, m, block_size=96)
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            dec(*_qkv(D=D), m)
    with pytest.raises(ValueError, match="head dim"):
        dec(*_qkv(D=48), m)
    with pytest.raises(ValueError, match="tensors"):
        dec(q[0], k, v, m)
    with pytest.raises(ValueError, match="Hkv"):
        dec(*_qkv(H=8, Hkv=3), m)
    with pytest.raises(ValueError, match="same K/V heads"):
        dec(q, k, v[:, :1], m)
    with pytest.raises(ValueError, match="match"):
        dec(q, k[:1], v[:1], m)
    with pytest.raises(ValueError, match="dtype"):
        dec(q, k.float(), v, m)
    with pytest.raises(ValueError, match="dtype"):
        dec(*_qkv(dt=torch.float32), m)
    with pytest.raises(ValueError, match="one query block"):
        dec(*_qkv(Sq=129), m)
    with pytest.raises(ValueError, match="one query block"):
        dec(*_qkv(Sq=65, H=2), m, block_size=64)
    with pytest.raises(ValueError, match="empty"):
        dec(q[:, :, :0], k, v, m)
    # the mask: dtype, rank, batch axis, one query block, head axis, key blocks
    for bad in (m.float(), m[0], _mask(B=3), torch.ones(2, 2, 2, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="block_mask"):
            dec(q, k, v, bad)
    with pytest.raises(ValueError, match="head axis"):
        dec(q, k, v, _mask(Hl=4))
    with pytest.raises(ValueError, match="key blocks"):
        dec(q, k, v, _mask(NK=7))
    # more than 64 rows share a K/V head and a list row
    with pytest.raises(NotImplementedError, match="block_sparse_attention"):
        dec(*_qkv(Sq=17, H=8, Hkv=2), m)
    with pytest.raises(NotImplementedError, match="block_sparse_attention"):
        dec(*_qkv(Sq=9, H=8, Hkv=1), _mask(Hl=1))
    for kv_len in (701, -1, [1, 2, 3]):
        with pytest.raises(ValueError, match="kv_len"):
            dec(q, k, v, m, kv_len=kv_len)
    for bps in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="blocks_per_split"):
            dec(q, k, v, m, blocks_per_split=bps)
    # the paged form: the table's type and shape, pools of block_size rows
    pool = torch.zeros(9, 2, 128, 64, dtype=torch.bfloat16)
    for table in (torch.zeros(2, 6, dtype=torch.int64), torch.zeros(3, 6, dtype=torch.int32), torch.zeros(12, dtype=torch.int32),
                  [[0] * 6] * 2):
        with pytest.raises(ValueError, match="block_table"):
            dec(q, pool, pool, m, block_table=table)
    with pytest.raises(ValueError, match="page pools"):
        dec(q, pool[:, :, :64], pool[:, :, :64], m, block_table=torch.zeros(2, 6, dtype=torch.int32))
    with pytest.raises(ValueError, match="key blocks"):
        dec(q, pool, pool, m, block_table=torch.zeros(2, 5, dtype=torch.int32))
    # a cache is never copied: strides that would need a copy are refused
    with pytest.raises(ValueError, match="not copied"):
        dec(q, k.transpose(2, 3).contiguous().transpose(2, 3), v, m)
    # a lists dict: one query block, int32, contiguous
    cols, counts = torch.zeros(4, 1, 6, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.int32)
    for bad in (dict(cols=cols), dict(cols=cols.long(), counts=counts), dict(cols=torch.zeros(4, 2, 6, dtype=torch.int32), counts=counts),
                dict(cols=torch.zeros(3, 1, 6, dtype=torch.int32), counts=counts[:3])):
        with pytest.raises(ValueError, match="block_mask"):
            dec(q, k, v, bad)


@pytest.mark.parametrize("kw", [dict(), dict(causal=True, kv_len=[700, 333], return_lse=True), dict(block_size=64, blocks_per_split=2),
                                dict(lists=True), dict(paged=True)], ids=["plain", "causal-lens-lse", "block64-split", "lists", "paged"])
def test_a_well_formed_call_on_cpu_tensors_reaches_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib, block_sparse_decode as dec
    kw = dict(kw)
    q, k, v = _qkv()
    m = _mask(NK=11 if kw.get("block_size") == 64 else 6)
    if kw.pop("lists", False):
        m = dict(cols=torch.zeros(4, 1, 6, dtype=torch.int32), counts=torch.zeros(4, 1, dtype=torch.int32))
    if kw.pop("paged", False):
        k = v = torch.zeros(15, 2, 128, 64, dtype=torch.bfloat16)
        kw["block_table"] = torch.zeros(2, 6, dtype=torch.int32)
    with pytest.raises(_lib.RsaError):
        dec(q, k, v, m, **kw)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------
def _lib_or_skip():
    from rectified_spaattn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("librsa_hip.so is not built")
    return _lib, _lib.lib()


def test_entries_are_declared_listed_and_exported_and_the_version_stays():
    from rectified_spaattn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    for name in (ENTRY, BYTES):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr)
        assert name in _lib.EXPORTED
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    mk = open(os.path.join(root, "rectified_spaattn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^rsa_decode\.o:", mk, re.M) and re.search(r"^\.\./librsa_hip\.so:.*\brsa_decode\.o\b", mk, re.M)
    _, L = _lib_or_skip()
    assert hasattr(L, ENTRY) and hasattr(L, BYTES)
    assert L.rsa_version() == 601
    assert L.rsa_abi_check(601, ctypes.sizeof(_lib.RsaBuffers), ctypes.sizeof(_lib.RsaLayout)) == 0


def test_workspace_size_query_and_the_default_split():
    _, L = _lib_or_skip()
    n = ctypes.c_size_t(0)

    def size(B, H, Hkv, Hl, Sq, D, NK, bps):
        st = L.rsa_block_sparse_decode_bytes(B, H, Hkv, Hl, Sq, D, NK, bps, ctypes.byref(n))
        return n.value if st == 0 else st
    part = lambda rows16, D: rows16 * (D + 2) * 4       # noqa: E731  fp32 O, m, l per row of a partial
    # 2 x 2 units of 4 rows; 6 key blocks, 2 entries per split: 3 splits
    assert size(2, 8, 2, 2, 1, 128, 6, 2) == 4 * 3 * part(16, 128)
    assert size(2, 8, 2, 2, 1, 128, 6, 6) == 4 * 1 * part(16, 128) == size(2, 8, 2, 2, 1, 128, 6, 100)
    assert size(2, 8, 2, 8, 3, 64, 11, 1) == 16 * 11 * part(16, 64)
    assert size(1, 8, 1, 1, 3, 64, 6, 3) == 1 * 2 * part(32, 64)        # 24 rows: two row tiles
    assert size(1, 8, 1, 1, 8, 64, 6, 3) == 1 * 2 * part(64, 64)        # 64 rows: four
    # the default: 8 entries per split (the measured choice), a function of the shapes alone
    assert size(1, 32, 8, 8, 1, 128, 1024, 0) == size(1, 32, 8, 8, 1, 128, 1024, 8)
    assert size(8, 32, 8, 8, 1, 128, 256, 0) == size(8, 32, 8, 8, 1, 128, 256, 8)
    assert size(2, 8, 2, 2, 1, 128, 6, 0) == size(2, 8, 2, 2, 1, 128, 6, 6)
    assert size(2, 8, 2, 2, 1, 128, 1, 0) == size(2, 8, 2, 2, 1, 128, 1, 1)
    assert L.rsa_block_sparse_decode_bytes(2, 8, 2, 2, 1, 128, 6, 2, None) == -1
    for bad in ((0, 8, 2, 2, 1, 128, 6, 2), (2, 8, 3, 3, 1, 128, 6, 2), (2, 8, 2, 4, 1, 128, 6, 2), (2, 8, 2, 2, 0, 128, 6, 2),
                (2, 8, 2, 2, 1, 128, 0, 2), (2, 8, 2, 2, 1, 128, 8193, 2), (2, 8, 2, 2, 1, 128, 6, -1)):
        assert size(*bad) == -1, bad
    for uns in ((2, 8, 2, 2, 1, 96, 6, 2), (2, 8, 2, 2, 1, 32, 6, 2), (2, 8, 2, 2, 17, 128, 6, 2), (1, 8, 1, 1, 9, 128, 6, 2)):
        assert size(*uns) == -2, uns


def test_entry_checks_its_arguments():
    _lib, L = _lib_or_skip()
    BAD, UNS, WS = -1, -2, -3
    t = _lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 128)
    o = _lib.RsaOut4(4096, 8 * 128, 128, 128)
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its host checks
    big = 1 << 30

    def call(B=1, H=8, Hkv=2, Hl=2, Sq=1, Sk=700, D=128, dt=0, blk=128, NK=6, kv=None, kvv=700, causal=0, scale=0.1, q=t, k=t, v=t,
             table=None, tsb=6, pages=0, cols=p, counts=p, bps=0, ws=p, wsb=big, out=o, lse=None):
        return getattr(L, ENTRY)(B, H, Hkv, Hl, Sq, Sk, D, dt, blk, NK, kv, kvv, causal, scale, q, k, v, table, tsb, pages, cols,
                                 counts, bps, ws, wsb, out, lse, None)

    for kw in (dict(H=0), dict(H=-8), dict(Hkv=0), dict(Hkv=-2), dict(Hl=0), dict(Hl=-1), dict(Hkv=3, Hl=3), dict(Hkv=16, Hl=16),
               dict(Hl=4), dict(Hl=16), dict(H=6, Hkv=4, Hl=4)):
        assert call(**kw) == BAD, kw
    for base in (dict(), dict(Hl=8), dict(Hl=1), dict(Hkv=8, Hl=8), dict(Hkv=1, Hl=1), dict(causal=1, Sq=3), dict(lse=p), dict(kv=p),
                 dict(table=p, pages=20), dict(bps=2)):
        c = lambda **kw: call(**{**base, **kw})   # noqa: E731
        assert c(blk=96) == UNS
        assert c(blk=32) == UNS
        assert c(D=96) == UNS
        assert c(D=32) == UNS
        assert c(D=16) == UNS
        assert c(dt=7) == UNS
        assert c(B=0) == BAD
        assert c(Sq=0) == BAD
        assert c(Sk=0) == BAD
        assert c(Sq=-5) == BAD
        assert c(NK=0) == BAD
        assert c(NK=7) == BAD                        # more than ceil(Sk / block)
        assert c(blk=64, NK=12) == BAD
        assert c(Sk=8193 * 128, NK=8193, kvv=700) == BAD
        assert c(Sq=129, H=2, Hkv=2, Hl=2) == BAD    # more than one query block
        assert c(Sq=65, H=2, Hkv=2, Hl=2, blk=64) == BAD
        assert c(bps=-1) == BAD
        assert c(ws=None) == BAD
        assert c(ws=ctypes.c_void_p(4104)) == BAD    # 16-byte alignment
        assert c(cols=None) == BAD
        assert c(counts=None) == BAD
        assert c(cols=ctypes.c_void_p(4098)) == BAD
        assert c(counts=ctypes.c_void_p(4097)) == BAD
        assert c(lse=ctypes.c_void_p(4098)) == BAD
        assert c(kv=ctypes.c_void_p(4098)) == BAD
        assert c(table=ctypes.c_void_p(4098), pages=20) == BAD
        assert c(table=p, pages=0) == BAD
        assert c(table=p, pages=-3) == BAD
        assert c(table=p, pages=20, tsb=-6) == BAD
        assert c(q=_lib.RsaTensor4(None, 8 * 128, 128, 128)) == BAD
        assert c(q=_lib.RsaTensor4(4100, 8 * 128, 128, 128)) == BAD
        assert c(k=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, 132)) == BAD
        assert c(v=_lib.RsaTensor4(4096, 2 * 128 * 700, 128 * 700, -128)) == BAD
        assert c(out=_lib.RsaOut4(None, 8 * 128, 128, 128)) == BAD
        assert c(out=_lib.RsaOut4(4100, 8 * 128, 128, 128)) == BAD
        assert c(out=_lib.RsaOut4(4096, 8 * 128, 130, 128)) == BAD
        assert c(out=_lib.RsaOut4(4096, 8 * 128, 128, -128)) == BAD
        assert c(wsb=0) == WS
        assert c(Sk=8192 * 128, NK=8192, kvv=700, wsb=0) == WS      # (the limit itself is served)
        if "kv" not in base:                         # the host limit: 0 .. Sk (a device limit is clamped on the device)
            assert c(kvv=-1) == BAD
            assert c(kvv=701) == BAD
    # more than 64 rows per unit
    assert call(Sq=17) == UNS and call(Sq=16, wsb=0) == WS
    assert call(Hkv=1, Hl=1, Sq=9) == UNS and call(Hkv=1, Hl=1, Sq=8, wsb=0) == WS
    assert call(Hkv=1, Hl=8, Sq=65) == UNS and call(Hkv=1, Hl=8, Sq=64, wsb=0) == WS
    # the workspace: exactly what the query reports is enough for the checks, one byte less is not
    n = ctypes.c_size_t(0)
    for bps in (0, 1, 4):
        assert L.rsa_block_sparse_decode_bytes(1, 8, 2, 2, 1, 128, 6, bps, ctypes.byref(n)) == 0
        assert call(bps=bps, wsb=n.value - 1) == WS
        assert call(bps=bps, wsb=n.value, blk=96) == UNS
