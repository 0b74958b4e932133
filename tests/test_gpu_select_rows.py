"""K3 against the oracle on the designed rows of tests/select_rows.py (ties, exact cuts, one-ulp neighbours, subnormal and zero
probabilities, threshold extremes, unions on tied rows), bit for bit, and three end-to-end calls whose pooled scores tie exactly.

Injected rows: the workspace is allocated as a StagedCall allocates it, the unscaled scores and the GAPR bytes are written
directly, and rsa_select_mask (rsa_select_mask_ex at 64-token blocks) runs alone -- as dispatched, with the sorted-head path off
(k3_prefix = 0), through the workgroup-per-row kernel (k3_long = 1), with a second head whose rows are the first head's
permuted, and without the neighbour list (every shape has one otherwise).  probs, the bitmask, counts, cols[:count], R and w must EQUAL oracle.select_rows_from_scores on every row."""
import ctypes

import numpy as np
import pytest
import torch

import select_rows as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {sh.name: sh for sh in sr.SHAPES}
# way -> (tuning key, value, value to restore) | None, heads, with the neighbour list
WAYS = {"dispatched": (None, 1, True), "k3_prefix=0": ((b"k3_prefix", 0, 1), 1, True), "k3_long=1": ((b"k3_long", 1, 0), 1, True),
        "two heads": (None, 2, True), "no neighbour list": (None, 1, False)}
_DEVICE = {}


def _spec(sh):
    from rectified_spaattn_amd import _core
    if sh.n_txt:
        return _core.LayoutSpec.hunyuan(sh.S, sh.num_true, block=sh.block)
    return _core.LayoutSpec.wan(sh.S, sh.ffb, block=sh.block)


def _on_device(sh, heads):
    """The workspace of the shape with the case's scores and GAPR bytes in it (made once per shape and head count; K3 only reads them)."""
    from rectified_spaattn_amd import _core
    key = (sh, heads)
    if key not in _DEVICE:
        c = sr.case(sh)
        spec = _spec(sh)
        assert (spec.NBv, spec.n_txt, spec.NB_total, spec.L, spec.text_end_block) == \
            (sh.NBv, sh.n_txt, sh.NB_total, sh.L, sh.layout().text_end_block)
        bufs = _core.alloc_buffers(spec, 1, heads, sh.D, DEV)
        bufs["scores"].copy_(torch.from_numpy(c.scores[:heads]))
        bufs["unrel"].copy_(torch.from_numpy(c.unrel[:heads]))
        nbr = sh.neighbor()
        _DEVICE[key] = (spec, bufs, torch.from_numpy(np.array(nbr)).to(DEV))
    return _DEVICE[key]


def _run_k3(sh, heads, top_k, p, tuning, nbr_on=True):
    from rectified_spaattn_amd import _core, _lib
    spec, bufs, nbr = _on_device(sh, heads)
    if not nbr_on:
        nbr = None
    L = _lib.lib()
    bufs["probs"].fill_(float("nan")); bufs["w"].fill_(float("nan")); bufs["R"].fill_(float("nan"))
    bufs["bitmask"].fill_(-1); bufs["cols"].fill_(-1); bufs["counts"].fill_(-1)
    cb = _core._c_buffers(bufs)
    if spec.block == 128:
        fn, lay = L.rsa_select_mask, spec.to_c(1, heads, sh.D, torch.bfloat16)
    else:
        fn, lay = L.rsa_select_mask_ex, spec.to_c_ex(1, heads, sh.D, torch.bfloat16)
    if tuning is not None:
        assert L.rsa_set_tuning(tuning[0], tuning[1]) == 0
    try:
        _lib.check(fn(ctypes.byref(lay), nbr.data_ptr() if nbr is not None else None, int(top_k), float(p), ctypes.byref(cb),
                      _core._stream()), "rsa_select_mask")
        torch.cuda.synchronize()
    finally:
        if tuning is not None:
            L.rsa_set_tuning(tuning[0], tuning[2])
    out = {n: bufs[n].cpu().numpy() for n in ("probs", "w", "R", "cols", "counts")}
    out["kept"] = _core.unpack_bitmask(bufs["bitmask"], spec.NB_total).cpu().numpy()
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name,pname", [(n, k) for n, sh in SHAPES.items() for k in sr.param_sets(sh)])
def test_injected_rows_equal_the_oracle(name, pname, way):
    sh = SHAPES[name]
    tuning, heads, nbr_on = WAYS[way]
    top_k, p = sr.param_sets(sh)[pname]
    got = _run_k3(sh, heads, top_k, p, tuning, nbr_on)
    assert not (got["counts"] == -1).any(), "a row the sorted-head pass left to the full sort was never redone"
    for bh in range(heads):
        ref = sr.reference(sh, pname, bh, nbr_on)
        where = (name, pname, way, bh)
        # float outputs by bit pattern: a subnormal must arrive as that subnormal, a zero as +0
        for n_ in ("probs", "w", "R"):
            bad = np.nonzero(np.atleast_2d(_bits(got[n_][bh]) != _bits(ref[n_])).reshape(sh.NBv, -1).any(1))[0]
            assert bad.size == 0, (where, n_, "rows", bad[:8].tolist(), [sr.case(sh).row_of(bh, int(r)).cls for r in bad[:8]])
        kept = got["kept"][bh].astype(np.uint8)
        bad = np.nonzero((kept != ref["kept"]).any(1))[0]
        assert bad.size == 0, (where, "bitmask", "rows", bad[:8].tolist(), [sr.case(sh).row_of(bh, int(r)).cls for r in bad[:8]])
        cnt = ref["kept"].sum(1)
        assert np.array_equal(got["counts"][bh], cnt), (where, "counts")
        valid = np.arange(sh.NB_total)[None, :] < cnt[:, None]
        want_cols = np.full((sh.NBv, sh.NB_total), -1, np.int64)
        rr, cc = np.nonzero(ref["kept"])
        want_cols[valid] = cc                                           # (np.nonzero is row-major: ascending columns row after row)
        assert np.array_equal(np.where(valid, got["cols"][bh], -1), want_cols), (where, "cols")


# ---- end to end: K1 and K2 deliver ties as ties, and the whole call follows --------------------------------------------------
B_PERIOD = (3.0, 1.0, 4.0, 1.5, 5.0, 2.5, 2.0)       # key block j holds b_j = B_PERIOD[j % 7] ("repeated frames")
A_CYCLE = (1.0, 2.0, 0.5, 0.0, -1.0)                 # query block i holds a_i: 0 = a whole-row plateau, -1 reverses the order
E2E = {"wan 40 blocks, ragged": dict(kind="wan", nb=40, D=128, top_k=5, p=0.3, ragged=57),
       "hunyuan 70 blocks + text": dict(kind="hunyuan", nb=70, D=64, top_k=9, p=0.25, ragged=0),
       "wan 300 blocks (two-pass)": dict(kind="wan", nb=300, D=64, top_k=20, p=0.3, ragged=101)}


def _e2e_inputs(cfg):
    from rectified_spaattn_amd import _core
    from oracle import oracle as orc
    nb, D = cfg["nb"], cfg["D"]
    if cfg["kind"] == "wan":
        S = (nb - 1) * 128 + cfg["ragged"]
        spec, lay = _core.LayoutSpec.wan(S, 3), orc.layout_wan(S, 3)
    else:
        S = (nb + 2) * 128
        spec, lay = _core.LayoutSpec.hunyuan(S, nb * 128 + 40), orc.layout_hunyuan(S, nb * 128 + 40)
    blk = np.arange(S) // 128
    g = np.random.default_rng(11 + nb)
    q = np.zeros((S, D), np.float32)
    k = np.zeros((S, D), np.float32)
    q[:, 0] = np.asarray(A_CYCLE)[blk % 5]
    k[:, 0] = np.asarray(B_PERIOD)[blk % 7]
    if cfg["kind"] == "hunyuan":       # text tokens: four distinct keys, repeated
        k[nb * 128:, 0] = np.asarray((0.5, 1.0, 3.0, 6.0))[np.arange(S - nb * 128) % 4]
        q[nb * 128:] = orc.round_bf16(g.standard_normal((S - nb * 128, D)).astype(np.float32))
    v = orc.round_bf16(g.standard_normal((S, D)).astype(np.float32))
    return spec, lay, q, k, v


@pytest.mark.parametrize("name", list(E2E))
def test_end_to_end_ties(name):
    """Q and K constant over each 128-token block (a_i e_0, b_j e_0, b periodic, a zero-padded ragged tail): pooled means are exact,
    s_ij = qbar_i . kbar_j exactly, the mean-abs-deviation of every full block is 0, and rows repeat their probabilities every 7 columns."""
    from rectified_spaattn_amd import _core, _lib
    from oracle import oracle as orc
    cfg = E2E[name]
    spec, lay, q, k, v = _e2e_inputs(cfg)
    D = cfg["D"]
    qd, kd, vd = (torch.from_numpy(x).to(DEV).to(torch.bfloat16).view(1, 1, lay.S, D) for x in (q, k, v))
    out, parts = _core.rectified_attention(qd, kd, vd, spec, cfg["top_k"], cfg["p"], None, return_parts=True)
    torch.cuda.synchronize()
    # the scores, exactly: means of constant blocks (the ragged one: value * valid / 128) and one exact product each
    kz = k.copy()
    kz[lay.pool_valid:] = 0
    nv = lay.NBv
    qbar = np.add.reduceat(q[:nv * 128, 0].astype(np.float64), np.arange(0, min(lay.S, nv * 128), 128)) / 128.0
    kbar = np.add.reduceat(kz[:nv * 128, 0].astype(np.float64), np.arange(0, min(lay.S, nv * 128), 128)) / 128.0
    want = np.concatenate([qbar[:, None] * kbar[None, :], qbar[:, None] * kz[nv * 128: nv * 128 + lay.n_txt, 0][None, :]], 1)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    vz = np.where(np.arange(lay.S)[:, None] < lay.pool_valid, v, 0).astype(np.float32)
    sel = orc.select_head(q, kz, vz, lay, cfg["top_k"], cfg["p"], None)
    # a full constant block has mean-abs-deviation 0, so its GAPR byte is !(|s| > 0); the ragged block's is the oracle's
    full = min(lay.S // 128, nv)
    assert np.array_equal(sel["unrel"][:full, :full] != 0, want[:full, :full] == 0) and np.array_equal(sel["s_vis"], want[:, :nv])
    L = _lib.lib()
    try:
        for form in (0, 32, 16):
            assert L.rsa_set_tuning(b"k2_dma", form) == 0
            call = _core.StagedCall(qd, kd, vd, spec, cfg["top_k"], cfg["p"], None, reuse_buffers=False)
            call.bufs["scores"].fill_(float("nan"))
            call.select()
            torch.cuda.synchronize()
            assert np.array_equal(call.bufs["scores"][0].cpu().numpy(), want.astype(np.float32)), (name, "k2_dma", form)
            assert np.array_equal(call.bufs["unrel"][0].cpu().numpy(), sel["unrel"]), (name, "GAPR bytes", form)
    finally:
        L.rsa_set_tuning(b"k2_dma", 0)
    # the selection on every row, bit for bit
    assert any(len(set(sel["probs"][i][:nv].tolist())) == 1 for i in range(nv)), "no whole-row plateau among the rows"
    assert all(len(set(sel["probs"][i][:nv].tolist())) <= 8 for i in range(nv))
    kept = _core.unpack_bitmask(parts["bitmask"], lay.NB_total).cpu().numpy()[0].astype(np.uint8)
    assert np.array_equal(kept, sel["kept"])
    cnt = sel["kept"].sum(1)
    assert np.array_equal(parts["counts"][0].cpu().numpy(), cnt)
    cols = parts["cols"][0].cpu().numpy()
    for i in range(nv):
        assert np.array_equal(cols[i, :cnt[i]], np.nonzero(sel["kept"][i])[0]), i
    for n_ in ("probs", "w", "R"):
        assert np.array_equal(_bits(parts[n_][0].cpu().numpy()), _bits(sel[n_])), (name, n_)
    # O on sampled rows within the operator's bound
    rows = sorted({0, 1, 3, 4, nv // 2, nv - 2, nv - 1})
    ref = orc.sparse_attention_head(q, kz, vz, lay, sel["kept"][rows], rows)
    ref = ref * sel["R"][rows][:, None, None] + sel["comp"][rows][:, None, :]
    o = out.view(1, lay.S, 1, D)
    for a_, i in enumerate(rows):
        nrow = max(0, min(128, lay.S - i * 128))
        err = np.abs(o[0, i * 128:i * 128 + nrow, 0].float().cpu().numpy() - ref[a_][:nrow])
        assert err.max() <= 2e-2 and err.mean() <= 2e-3, (name, i, float(err.max()), float(err.mean()))
