"""K4, comp = w . vbar, in both forms (k4_split = 0: compensation_kernel, the fp32 MFMA chain; 2: compensation_split_kernel, bf16
hi / lo planes) on the designed inputs of tests/comp_ref.py.

Injected launches: the workspace is allocated as a StagedCall allocates it, w and vbar are written directly -- as views of larger
buffers whose tails hold finite decoys -- and rsa_compensation (rsa_compensation_ex at 64-token blocks) runs alone.  comp is a view
too: it is filled with a NaN pattern before every launch and followed by a guard of one tile; afterwards every element of comp is
written, the guard and the bitmask buffer (the workspace buffer behind comp) are byte-identical.
  exact classes X1 / X2: comp must EQUAL the reference by bit pattern (the all-zero rows by value), in both forms;
  bound class:           |comp - fp64| within the per-element bound of each form (comp_ref.bounds), the largest ratio printed;
  the dispatch rule:     k4_split = 1 gives the chain form's bytes at NBv = 255 and the split form's at 256;
  end to end:            StagedCall.select() on five small layouts hands K4 the right L, NB_total and buffers."""
import ctypes

import numpy as np
import pytest
import torch

import comp_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {sh.name: sh for sh in cr.SHAPES + cr.THRESHOLD_SHAPES}
NAN_PATTERN = 0x7FC12345                 # a quiet NaN no kernel produces
MASK_PATTERN = 0x5A5AA5A5
FORMS = {"chain": 0, "split": 2}
_WS = {}


def _spec(sh):
    from rectified_spaattn_amd import _core
    if sh.kind == "wan":
        spec = _core.LayoutSpec.wan(sh.S, 0, block=sh.block)
    elif sh.kind == "hunyuan":
        spec = _core.LayoutSpec.hunyuan(sh.S, sh.NBv * sh.block + sh.n_txt, block=sh.block)
    else:
        spec = _core.LayoutSpec.flux(sh.S, sh.n_txt, block=sh.block)
    assert (spec.NBv, spec.NB_total, spec.L) == (sh.NBv, sh.NB_total, sh.L)
    return spec


def _workspace(spec, H, D):
    """The buffers of the layout, with w, vbar and comp as views of pools that carry a tail (decoys behind w and vbar, a guard
    behind comp).  One per geometry: K4 only reads w and vbar."""
    from rectified_spaattn_amd import _core
    key = (spec.NBv, spec.NB_total, spec.block, spec.n_txt, H, D)
    if key not in _WS:
        bufs = _core.alloc_buffers(spec, 1, H, D, DEV)
        pools = {}
        for n, tail in (("w", cr.W_TAIL), ("vbar", cr.V_TAIL_ROWS * D), ("comp", cr.C_TAIL_ROWS * D)):
            shape = bufs[n].shape
            pools[n] = torch.empty(bufs[n].numel() + tail, dtype=torch.float32, device=DEV)
            bufs[n] = pools[n][:bufs[n].numel()].view(shape)
        _WS[key] = (bufs, pools)
    return _WS[key]


def _run_k4(spec, H, D, wflat, vflat, form):
    """comp [H, NBv, D] (numpy) of rsa_compensation alone on the injected buffers, after the written / guard / bitmask checks."""
    from rectified_spaattn_amd import _core, _lib
    bufs, pools = _workspace(spec, H, D)
    assert wflat.size == pools["w"].numel() and vflat.size == pools["vbar"].numel()
    pools["w"].copy_(torch.from_numpy(wflat))
    pools["vbar"].copy_(torch.from_numpy(vflat))
    pools["comp"].view(torch.int32).fill_(NAN_PATTERN)
    bufs["bitmask"].fill_(MASK_PATTERN)
    cb = _core._c_buffers(bufs)
    L = _lib.lib()
    if spec.block == 128:
        fn, lay = L.rsa_compensation, spec.to_c(1, H, D, torch.bfloat16)
    else:
        fn, lay = L.rsa_compensation_ex, spec.to_c_ex(1, H, D, torch.bfloat16)
    assert L.rsa_set_tuning(b"k4_split", form) == 0
    try:
        _lib.check(fn(ctypes.byref(lay), ctypes.byref(cb), _core._stream()), "rsa_compensation")
        torch.cuda.synchronize()
    finally:
        L.rsa_set_tuning(b"k4_split", 1)
    pool = pools["comp"].view(torch.int32).cpu().numpy()
    n = bufs["comp"].numel()
    assert (pool[n:] == NAN_PATTERN).all(), "a store past the last row of the last head"
    assert not (pool[:n] == NAN_PATTERN).any(), "an element of comp was never written"
    assert bool((bufs["bitmask"] == MASK_PATTERN).all()), "the buffer behind comp changed"
    return pool[:n].view(np.float32).reshape(H, spec.NBv, D)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("cls", ["X1", "X2"])
@pytest.mark.parametrize("name,D", [(sh.name, D) for sh in cr.SHAPES for D in cr.DS])
def test_exact_classes_equal_the_reference(name, D, cls, H, form):
    sh = SHAPES[name]
    c = cr.exact_case(sh, D, cls)
    got = _run_k4(_spec(sh), H, D, *c.flat(H), FORMS[form])
    zero = np.array([[k == "zero" for k in kh] for kh in c.kinds[:H]])
    eq = _bits(got) == _bits(c.ref[:H])
    eq[zero] = got[zero] == 0                                    # +0 or -0
    bad = np.argwhere(~eq.all(2))
    assert bad.size == 0, (name, D, cls, H, form, "rows (head, row, kind)", [(int(h), int(i), c.kinds[h][i]) for h, i in bad[:12]],
                           "first", got[tuple(bad[0])][:4].tolist(), c.ref[tuple(bad[0])][:4].tolist())


def _check_bound(got, w, vbar, L, form, where, kinds=None):
    b = cr.bounds(w, vbar, L)
    err = np.abs(got.astype(np.float64) - b["ref"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b[form] > 0, err / b[form], np.where(err > 0, np.inf, 0.0))
    note = ""
    if kinds is not None:
        sub = np.array([[k == "subnormal" for k in kh] for kh in kinds])
        if sub.any():
            note = f"; subnormal rows: {int((got[sub] != 0).sum())} of {int((b['ref'][sub] != 0).sum())} non-zero elements arrived non-zero"
    print(f"K4 {form} {where}: {got.size} elements, largest |got - ref| / bound {ratio.max():.4f} (n = {int(b['n'].flat[ratio.argmax()])}){note}")
    bad = np.argwhere(err > b[form])
    assert bad.size == 0, (where, form, "elements (head, row, d)", bad[:8].tolist(), float(ratio.max()))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("name,D", [(sh.name, D) for sh in cr.SHAPES for D in cr.DS])
def test_bound_class_per_element(name, D, H, form):
    sh = SHAPES[name]
    c = cr.bound_case(sh, D)
    got = _run_k4(_spec(sh), H, D, *c.flat(H), FORMS[form])
    _check_bound(got, c.w[:H], c.vbar[:H], sh.L, form, f"{name} D={D} H={H}", c.kinds[:H])


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", cr.DS)
def test_dispatch_rule_at_the_threshold(D, H):
    """k4_split = 1: the form is a function of NBv alone -- the chain form below 256 visual blocks, the split form from 256."""
    for sh, want in zip(cr.THRESHOLD_SHAPES, ("chain", "split")):
        c = cr.bound_case(sh, D)
        spec = _spec(sh)
        forced = {f: _run_k4(spec, H, D, *c.flat(H), v).copy() for f, v in FORMS.items()}
        assert not np.array_equal(_bits(forced["chain"]), _bits(forced["split"])), "the canary: the two forms must differ in bytes"
        got = _run_k4(spec, H, D, *c.flat(H), 1)
        assert np.array_equal(_bits(got), _bits(forced[want])), (sh.name, D, H, "dispatched form is not the", want, "form")


E2E = {"wan 40 blocks, ragged": dict(kind="wan", S=39 * 128 + 57, D=128, block=128),
       "hunyuan 70 blocks + text": dict(kind="hunyuan", S=72 * 128, aux=70 * 128 + 40, D=128, block=128),
       "flux 5 blocks + 512 text": dict(kind="flux", S=9 * 128, aux=512, D=128, block=128),
       "cogvideo D=64": dict(kind="cogvideo", S=20 * 128 + 226, aux=226, D=64, block=128),
       "wan 64-token blocks": dict(kind="wan", S=50 * 64 - 13, D=128, block=64)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(E2E))
def test_end_to_end_small_layouts(name, form):
    """select() on a small layout: comp equals rsa_compensation alone on copies of the call's own w and vbar in a fresh workspace,
    byte for byte, and meets the per-element bound against fp64 of them."""
    from rectified_spaattn_amd import _core, _lib
    from bench import gen_qkv
    cfg = E2E[name]
    S, D, H = cfg["S"], cfg["D"], 2
    spec = {"wan": lambda: _core.LayoutSpec.wan(S, 2, block=cfg["block"]), "hunyuan": lambda: _core.LayoutSpec.hunyuan(S, cfg["aux"]),
            "flux": lambda: _core.LayoutSpec.flux(S, cfg["aux"]), "cogvideo": lambda: _core.LayoutSpec.cogvideo(S, cfg["aux"])}[cfg["kind"]]()
    q, k, v = gen_qkv(H, 0, S, S, D, torch.device(DEV), seed=41)
    L = _lib.lib()
    assert L.rsa_set_tuning(b"k4_split", FORMS[form]) == 0
    try:
        call = _core.StagedCall(q, k, v, spec, 4, 0.1, None, reuse_buffers=False)
        call.bufs["comp"].view(torch.int32).fill_(NAN_PATTERN)
        call.select()
        torch.cuda.synchronize()
    finally:
        L.rsa_set_tuning(b"k4_split", 1)
    w, vbar = call.bufs["w"].cpu().numpy(), call.bufs["vbar"].cpu().numpy()
    comp = call.bufs["comp"].cpu().numpy()
    assert (w != 0).any() and not np.isnan(comp).any()
    g = np.random.default_rng(5)
    wflat = np.concatenate([w.ravel(), (g.random(cr.W_TAIL) * 2.0 ** 30).astype(np.float32)])
    vflat = np.concatenate([vbar.ravel(), (g.random(cr.V_TAIL_ROWS * D) * 2.0 ** 30).astype(np.float32)])
    alone = _run_k4(spec, H, D, wflat, vflat, FORMS[form])
    assert np.array_equal(_bits(comp), _bits(alone)), (name, form)
    _check_bound(comp, w, vbar, spec.L, form, name)
