"""merge_partials without a GPU: the fp64 reference of tests/merge_ref.py against a naive softmax over the
concatenated keys and against itself merged in pairs; the fp32 twin of the kernel's operation order inside the stated bound; the
entry in the header, the prototype table and the library; every refusal of rsa_merge_partials through ctypes (its checks run
before the first HIP call) and the Python argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import merge_ref as ref
from rectified_spaattn_amd import merge_partials as merge

ENTRY = "rsa_merge_partials"


# ---- the references ---------------------------------------------------------------------------------------------------------------
def _naive(seed, counts, rows=6, D=8, sink=False, empty=()):
    """Partials made from real keys: partial i holds counts[i] scores and values per row (none for the rows in `empty`: lse -inf and
    a NaN out); and the softmax over the concatenation, the sink as one more score whose value is zero."""
    rng = np.random.default_rng(seed)
    outs, lses, sc, va = [], [], [], []
    for i, n in enumerate(counts):
        s, v = 3.0 * rng.standard_normal((rows, n)), rng.standard_normal((rows, n, D))
        if i in empty:
            s = np.full_like(s, -np.inf)
        sc.append(s)
        va.append(v)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = s.max(1, keepdims=True)
            p = np.exp(s - m)
            outs.append(np.where(np.isfinite(m)[..., None], np.einsum("rn,rnd->rd", p, v)[:, None] / p.sum(1)[:, None, None], np.nan)[:, 0])
            lses.append(np.where(np.isfinite(m[:, 0]), m[:, 0] + np.log(p.sum(1)), -np.inf))
    sk = rng.standard_normal(rows) if sink else None
    s, v = np.concatenate(sc, 1), np.concatenate(va, 1)
    if sink:
        s, v = np.concatenate([s, sk[:, None]], 1), np.concatenate([v, np.zeros((rows, 1, D))], 1)
    m = s.max(1, keepdims=True)
    p = np.exp(s - m)
    whole = np.einsum("rn,rnd->rd", p, v) / p.sum(1)[:, None]
    return np.stack(outs), np.stack(lses), sk, whole, m[:, 0] + np.log(p.sum(1))


@pytest.mark.parametrize("counts,sink,empty", [((5,), False, ()), ((3, 4), False, ()), ((1, 7, 2), True, ()), ((4, 4, 4, 4, 4, 4, 4, 4), False, ()),
                                               ((3, 4, 5), False, (1,)), ((2, 2), True, (0,)), ((6,), True, ())])
def test_reference_is_the_softmax_over_the_concatenation(counts, sink, empty):
    outs, lses, sk, whole, whole_lse = _naive(len(counts) + 10 * sink, counts, sink=sink, empty=empty)
    out, lse = ref.merge_ref(outs, lses, sk)
    assert np.abs(out - whole).max() < 1e-13 and np.abs(lse - whole_lse).max() < 1e-13
    if empty:
        assert np.isnan(outs[list(empty)]).all()         # (the dead partial's NaN did not reach the result)


def test_reference_rows_without_a_live_entry_are_zero_and_minus_inf():
    outs, lses = np.full((3, 4, 8), np.nan), np.full((3, 4), -np.inf)
    outs[1, 2], lses[1, 2] = 1.5, 0.25
    for sk in (None, np.full(4, -np.inf)):
        out, lse = ref.merge_ref(outs, lses, sk)
        assert (out[[0, 1, 3]] == 0).all() and (lse[[0, 1, 3]] == -np.inf).all()
        assert (out[2] == 1.5).all() and lse[2] == 0.25
        t_out, t_lse = ref.merge_twin(outs, lses, sk)
        assert np.array_equal(t_out, out) and np.array_equal(t_lse.astype(np.float64), lse)     # one live entry: its bytes


def test_merging_is_associative_in_fp64():
    """Merged pairs, merged again, equal the N-way merge; so does a left fold.  (In fp64: a merge of 2-byte partials rounds.)"""
    c = ref.make_case(3, 8, (5, 3, 16), "bf16", spread=6.0, dead=0.3, dead_rows=False)
    outs, lses = c["outs"].astype(np.float64), c["lses"].astype(np.float64)
    whole = ref.merge_ref(outs, lses)
    pairs = [ref.merge_ref(outs[i:i + 2], lses[i:i + 2]) for i in range(0, 8, 2)]
    quads = [ref.merge_ref(np.stack([a[0], b[0]]), np.stack([a[1], b[1]])) for a, b in (pairs[:2], pairs[2:])]
    tree = ref.merge_ref(np.stack([quads[0][0], quads[1][0]]), np.stack([quads[0][1], quads[1][1]]))
    fold = (outs[0], lses[0])
    for i in range(1, 8):
        # (a dead accumulator holds 0, not NaN, from here on; merge_ref does not read it either way)
        fold = ref.merge_ref(np.stack([fold[0], outs[i]]), np.stack([fold[1], lses[i]]))
    for got in (tree, fold):
        assert np.abs(got[0] - whole[0]).max() < 1e-13
        both = np.isfinite(whole[1])
        assert np.array_equal(np.isfinite(got[1]), both) and np.abs(got[1][both] - whole[1][both]).max() < 1e-13


@pytest.mark.parametrize("kind", ["bf16", "fp16"])
@pytest.mark.parametrize("N", [1, 2, 3, 5, 8])
def test_the_fp32_twin_stays_within_the_bound(N, kind):
    worst = [0.0, 0.0]
    for si, spread in enumerate((0.01, 3.0, 40.0)):
        for mi, mag in enumerate((1e-3, 1.0, 50.0)):
            for sink in (False, True):
                c = ref.make_case(100 * N + 10 * si + mi, N, (4, 3, 50, 16), kind, spread=spread, mag=mag, dead=0.2, sink=sink)
                out, lse = ref.merge_twin(c["outs"], c["lses"], c["sink_rows"], kind)
                assert not np.isnan(out).any() and not np.isnan(lse).any()
                r = ref.worst_ratios(out, lse, c["outs"], c["lses"], c["sink_rows"], kind)
                worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"N = {N}, {kind}: worst |twin - fp64| / bound: out {worst[0]:.4f}, lse {worst[1]:.4f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_rounding_helpers():
    assert ref.ulp(1.0, "bf16") == 2.0 ** -7 and ref.ulp(1.0, "fp16") == 2.0 ** -10 and ref.ulp(0.75, "bf16") == 2.0 ** -8
    assert ref.ulp(0.0, "fp16") == 2.0 ** -24 and ref.ulp(2.0 ** -20, "fp16") == 2.0 ** -24
    assert ref.round_to(1.0 + 2.0 ** -8, "bf16") == 1.0 and ref.round_to(1.0 + 3 * 2.0 ** -8, "bf16") == 1.0 + 2.0 ** -6   # ties to even
    x = np.random.default_rng(0).standard_normal(1000)
    assert np.array_equal(ref.round_to(x, "fp16"), x.astype(np.float16).astype(np.float64))
    t = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(ref.round_to(x, "bf16"), t.double().numpy())
    assert np.array_equal(ref.to_bits(ref.round_to(x, "bf16"), "bf16"), t.view(torch.int16).numpy().view(np.uint16))


# ---- the entry ----------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_and_exported_and_the_version_stays():
    import rectified_spaattn_amd
    from rectified_spaattn_amd import _lib, block_sparse
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsa.h")).read()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(", hdr)
    assert "#define RSA_HEADER_VERSION 601" in hdr and _lib.HEADER_VERSION == 601
    assert ENTRY in _lib.PROTOTYPES and ENTRY in _lib.EXPORTED[:-3]
    assert _lib.EXPORTED[-3:] == ("rsa_block_sparse_extend_bytes", "rsa_block_sparse_extend", "rsa_block_sparse_extend_kv8")
    assert ENTRY + "_bytes" not in _lib.PROTOTYPES       # no workspace: no size query
    L = _lib.lib()
    assert hasattr(L, ENTRY) and L.rsa_version() == 601
    assert callable(merge) and merge is rectified_spaattn_amd.merge_partials and callable(block_sparse.merge_partials)


def test_entry_checks_its_arguments():
    """Every refusal, with its status; and a call of no rows that passes every check returns RSA_OK without a launch."""
    from rectified_spaattn_amd import _lib
    L = _lib.lib()
    OK, BAD, UNS = 0, -1, -2
    B, H, S, D = 2, 3, 5, 128
    T4, O4 = _lib.RsaTensor4, _lib.RsaOut4
    span = B * H * S * D * 2           # bytes of one out; the lse of partial i lies behind the outs
    o_at = lambda i: 0x10000 + i * 0x10000         # noqa: E731  (never dereferenced: the zero-row call launches nothing)
    l_at = lambda i: 0x200000 + i * 0x1000         # noqa: E731
    assert span < 0x10000

    H0, S0, D0, SB, SH = H, S, D, H * S * D, S * D      # the views' strides stay those of [2, 3, 5, 128] whatever sizes a call passes

    def call(N=2, B=B, H=H, S=S, D=D, dt=0, outs="default", lses="default", ls="default", sink=None, out=None, lse=None,
             es=(H * S, S, 1), edit=None, n_arr=None):
        n = max(N, 1) if n_arr is None else n_arr
        n = min(n, 9)
        ts = [T4(o_at(i), SB, SH, D0) for i in range(n)]
        ps = [l_at(i) for i in range(n)]
        st = [H0 * S0, S0, 1] * n
        if edit:
            edit(ts, ps, st)
        a = (T4 * n)(*ts) if outs == "default" else outs
        p = (ctypes.c_void_p * n)(*ps) if lses == "default" else lses
        s = (ctypes.c_int64 * (3 * n))(*st) if ls == "default" else ls
        o = O4(0x100000, SB, SH, D0) if out is None else out
        return L.rsa_merge_partials(N, B, H, S, D, dt, a, p, s, sink, o, lse, *es, None)

    def edit_t(i, **kw):
        def f(ts, ps, st):
            for k, v in kw.items():
                setattr(ts[i], k, v)
        return f

    def edit_l(i, ptr="kept", strides=None):
        def f(ts, ps, st):
            if ptr != "kept":
                ps[i] = ptr
            if strides is not None:
                st[3 * i:3 * i + 3] = strides
        return f
    lse_ok = ctypes.c_void_p(0x300000)
    # the witness that a well-formed call passes every check: no rows, no launch
    for kw in (dict(B=0), dict(H=0), dict(S=0)):
        for more in (dict(), dict(N=1), dict(N=8), dict(lse=lse_ok), dict(sink=ctypes.c_void_p(0x400000)), dict(D=64), dict(dt=1)):
            assert call(**kw, **more) == OK, (kw, more)
    for base in (dict(), dict(B=0), dict(lse=lse_ok), dict(sink=ctypes.c_void_p(0x400000), lse=lse_ok), dict(N=8), dict(N=1, D=64, dt=1)):
        c = lambda **kw: call(**{**base, **kw})        # noqa: E731
        assert c(N=0) == BAD and c(N=9, n_arr=9) == BAD and c(N=-1) == BAD
        assert c(B=-1) == BAD and c(H=-1) == BAD and c(S=-1) == BAD
        for D_ in (0, 32, 96, 256):
            assert c(D=D_) == UNS
        assert c(dt=2) == UNS and c(dt=-1) == UNS
        assert c(outs=None) == BAD and c(lses=None) == BAD and c(ls=None) == BAD
        assert c(out=O4(None, H * S * D, S * D, D)) == BAD
        last = base.get("N", 2) - 1
        for i in {0, last}:
            assert c(edit=edit_t(i, ptr=None)) == BAD
            assert c(edit=edit_l(i, ptr=None)) == BAD
            assert c(edit=edit_t(i, ptr=o_at(i) + 4)) == BAD              # 8-byte aligned pointers
            assert c(edit=edit_t(i, ptr=o_at(i) + 2)) == BAD
            assert c(edit=edit_l(i, ptr=l_at(i) + 2)) == BAD              # 4-byte aligned
            assert c(edit=edit_t(i, stride_s=D + 2)) == BAD               # strides: multiples of 4 elements
            assert c(edit=edit_t(i, stride_h=S * D + 1)) == BAD
            assert c(edit=edit_t(i, stride_b=H * S * D + 6)) == BAD
            assert c(edit=edit_t(i, stride_s=-D)) == BAD
            assert c(edit=edit_l(i, strides=[H * S, S, -1])) == BAD
        assert c(out=O4(0x100004, H * S * D, S * D, D)) == BAD
        assert c(out=O4(0x100000, H * S * D, S * D, D + 2)) == BAD
        assert c(out=O4(0x100000, H * S * D, S * D + 4, -D)) == BAD
        assert c(lse=ctypes.c_void_p(0x300002)) == BAD
        assert c(sink=ctypes.c_void_p(0x400002)) == BAD
    # what is served: the 8-byte form's alignment, lse strides of any kind, a broadcast partial
    assert call(B=0, edit=edit_t(1, ptr=o_at(1) + 8, stride_s=D + 4)) == OK
    assert call(B=0, edit=edit_l(0, strides=[0, 1, 7])) == OK
    assert call(B=0, edit=edit_t(0, stride_b=0)) == OK
    # a result is written once: no broadcast axis of more than one entry (a zero-row call has none, so these have rows)
    assert call(out=O4(0x100000, 0, S * D, D)) == BAD and call(out=O4(0x100000, H * S * D, 0, D)) == BAD
    assert call(out=O4(0x100000, H * S * D, S * D, 0)) == BAD
    assert call(lse=lse_ok, es=(0, S, 1)) == BAD and call(lse=lse_ok, es=(H * S, S, 0)) == BAD
    assert call(lse=lse_ok, es=(H * S, -S, 1)) == BAD
    # overlap: the result may be one partial exactly; anything else that meets a partial, the sink or the other result is refused
    for i in (0, 1):
        same = O4(o_at(i), H * S * D, S * D, D)
        assert call(B=0, out=same) == OK                                              # (no rows: nothing to meet)
        assert call(out=O4(o_at(i) + 16, H * S * D, S * D, D)) == BAD                 # shifted into partial i
        assert call(out=O4(o_at(i), H * S * D + 8, S * D, D)) == BAD                  # the same pointer, other strides
        assert call(out=O4(o_at(i) - 16, H * S * D, S * D, D)) == BAD                 # its tail meets the partial's head
        assert call(out=O4(l_at(i), H * S * D, S * D, D)) == BAD                      # over an lse
        assert call(lse=ctypes.c_void_p(l_at(i) + 4)) == BAD
        assert call(lse=ctypes.c_void_p(l_at(i)), es=(H * S, 1, H)) == BAD            # the same pointer, other strides
        assert call(lse=ctypes.c_void_p(o_at(i) + 64)) == BAD
    assert call(lse=ctypes.c_void_p(0x100000 + 32)) == BAD                            # lse inside out
    assert call(sink=ctypes.c_void_p(0x100000 + 8)) == BAD                            # the sink inside out
    assert call(lse=lse_ok, sink=ctypes.c_void_p(0x300000 + 4)) == BAD
    # beyond the 32-bit row index
    assert call(B=1 << 16, H=1 << 10, S=1 << 5) == UNS and call(B=1 << 20, H=1 << 20, S=0) == UNS


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def _parts(N=2, shape=(2, 3, 5, 64), dtype=torch.bfloat16):
    return [torch.zeros(shape, dtype=dtype) for _ in range(N)], [torch.zeros(shape[:-1]) for _ in range(N)]


def test_python_refusals():
    o, l = _parts()
    with pytest.raises(ValueError, match="outs"):
        merge([], [])
    with pytest.raises(ValueError, match="outs"):
        merge(*_parts(N=9))
    with pytest.raises(ValueError, match="outs"):
        merge(None, l)
    with pytest.raises(ValueError, match="outs"):
        merge(torch.zeros(3, 64, dtype=torch.bfloat16), torch.zeros(3))         # a stacked tensor has 4 or 5 axes
    with pytest.raises(ValueError, match="lses"):
        merge(o, l[:1])
    with pytest.raises(ValueError, match="lses"):
        merge(o, torch.zeros(2, 3, dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        merge([t.float() for t in o], l)
    with pytest.raises(ValueError, match=r"outs\[1\]"):
        merge([o[0], o[1].to(torch.float16)], l)
    with pytest.raises(ValueError, match=r"outs\[1\]"):
        merge([o[0], o[1][:, :, :4]], l)
    with pytest.raises(ValueError, match=r"lses\[1\]"):
        merge(o, [l[0], l[1].double()])
    with pytest.raises(ValueError, match=r"lses\[0\]"):
        merge(o, [l[0][:1], l[1]])
    for D in (16, 32):
        with pytest.raises(NotImplementedError, match="head dim"):
            merge(*_parts(shape=(2, 3, 5, D)))
    with pytest.raises(ValueError, match="head dim"):
        merge(*_parts(shape=(2, 3, 5, 48)))
    with pytest.raises(ValueError, match="empty"):
        merge(*_parts(shape=(2, 3, 0, 64)))
    # the stride contract: a tensor outside it is named, not copied
    wide = torch.zeros(2, 3, 5, 70, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"outs\[0\].*not copied"):
        merge([wide[..., 2:66], o[1]], l)                                       # pointer 4 bytes off
    with pytest.raises(ValueError, match=r"outs\[1\].*not copied"):
        merge([o[0], torch.zeros(2, 3, 5, 66, dtype=torch.bfloat16)[..., :64]], l)     # row stride 66
    with pytest.raises(ValueError, match=r"outs\[0\].*not copied"):
        merge([torch.zeros(2, 3, 64, 5, dtype=torch.bfloat16).transpose(2, 3), o[1]], l)   # head dim not contiguous
    with pytest.raises(ValueError, match=r"out:.*not copied"):
        merge(o, l, out=torch.zeros(2, 3, 5, 66, dtype=torch.bfloat16)[..., :64])
    for bad in (torch.zeros(2, 3, 5, 64), torch.zeros(2, 3, 4, 64, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="out:"):
            merge(o, l, out=bad)
    with pytest.raises(ValueError, match="out:.*positive"):
        merge(o, l, out=torch.zeros(1, 3, 5, 64, dtype=torch.bfloat16).expand(2, -1, -1, -1))
    with pytest.raises(ValueError, match="lse:"):
        merge(o, l, lse=torch.zeros(2, 3, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="lse:.*positive"):
        merge(o, l, lse=torch.zeros(2, 3, 1).expand(-1, -1, 5))
    with pytest.raises(ValueError, match="return_lse"):
        merge(o, l, lse=torch.zeros(2, 3, 5), return_lse=False)
    # overlap that is not an exact alias
    stack = torch.zeros(2, 2, 3, 5, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"out: overlaps outs\[0\]"):
        merge(stack, torch.zeros(2, 2, 3, 5), out=stack.view(-1)[64:64 + 2 * 3 * 5 * 64].view(2, 3, 5, 64))
    base = torch.zeros(64)
    with pytest.raises(ValueError, match=r"lse: overlaps lses\[1\]"):
        merge(stack, base[:60].view(2, 2, 3, 5), lse=base[31:61].view(2, 3, 5))
    # the sink
    for bad in (float("inf"), float("nan"), True, "0", torch.zeros(3, dtype=torch.float64), torch.zeros(2)):
        with pytest.raises(ValueError, match="sink"):
            merge(o, l, sink=bad)


@pytest.mark.parametrize("kw", [dict(), dict(sink=0.5), dict(sink=float("-inf")), dict(sink=torch.zeros(3)), dict(sink=torch.zeros(1)),
                                dict(stacked=True), dict(packed=True, sink=torch.zeros(3)), dict(alias=True), dict(views=True), dict(return_lse=False),
                                dict(N=1), dict(N=8, fp16=True)],
                         ids=["plain", "sink-float", "sink-minus-inf", "sink-heads", "sink-one", "stacked", "packed", "in-place", "views",
                              "no-lse", "one", "eight-fp16"])
def test_a_well_formed_call_on_cpu_tensors_reaches_the_device_check(kw):
    """... and no further: there is no fallback for CPU tensors."""
    from rectified_spaattn_amd import _lib
    kw = dict(kw)
    shape = (37, 3, 64) if kw.pop("packed", False) else (2, 3, 5, 64)
    o, l = _parts(N=kw.pop("N", 2), shape=shape, dtype=torch.float16 if kw.pop("fp16", False) else torch.bfloat16)
    if kw.pop("stacked", False):
        o, l = torch.stack(o), torch.stack(l)
    if kw.pop("alias", False):
        kw.update(out=o[0], lse=l[1])
    if kw.pop("views", False):         # head-strided views of a wider buffer, an lse with odd strides
        buf = torch.zeros(2, 5, 2 * 3 * 64 + 4, dtype=torch.bfloat16)
        o = [buf[:, :, i * 192:(i + 1) * 192].view(2, 5, 3, 64).permute(0, 2, 1, 3) for i in range(2)]
        o[1] = buf[:, :, 196:388].view(2, 5, 3, 64).permute(0, 2, 1, 3)        # 4 elements off: the 8-byte form
        l = [torch.zeros(2, 5, 3, 7)[..., 3].permute(0, 2, 1) for _ in range(2)]
    with pytest.raises(_lib.RsaError, match="device tensors"):
        merge(o, l, **kw)
