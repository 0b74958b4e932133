"""numpy reference of block_sparse_attention_backward: a plain helper module, no device.

    visible        extend_ref.visible: row r of (b, h) sees key j iff mask[b, hl(h), r // block, j // block] and j < kv_len[b] and,
                   with causal, j <= r + kv_len[b] - Sq
    grads          fp64 (out, dq, dk, dv) of the dense-masked expression softmax(sm_scale q k^T | seen) v, K/V heads shared by their
                   query heads' group; a row that sees nothing is 0 and gives no gradient; keys nobody sees are never multiplied
    model          the kernels' numeric contract in numpy: scaled-and-rounded Q, log2 domain, P and dS rounded to the storage type for
                   the products they feed, one rounding per output element -- with the mutations the CPU test applies
    case tables    FP64_CASES, EXACT_CASES, VIS_CASES and their inputs (the witness constructions)"""
from __future__ import annotations

import itertools

import numpy as np

import extend_ref as eref
import weights

visible = eref.visible
SK = 400                        # keys of the fp64 and visibility cases: four 128-blocks or seven 64-blocks, the last one ragged
B = 2


# ---- fp64 gradients --------------------------------------------------------------------------------------------------------------
def _clean(x):
    return np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=0.0, neginf=0.0)


def _group_sum(x, Hkv):
    """[B, H, Sk, D] -> [B, Hkv, Sk, D]: the sum over the query heads of a K/V head's group."""
    Bn, H, Sk, D = x.shape
    return x.reshape(Bn, Hkv, H // Hkv, Sk, D).sum(2)


def grads(q, k, v, dout, seen, sm_scale: float):
    """fp64 (out, dq, dk, dv).  q, dout [B, H, Sq, D]; k, v [B, Hkv, Sk, D] (NaN where no row sees the key is ignored); seen bool
    [B, H, Sq, Sk]."""
    q, dout = np.asarray(q, np.float64), np.asarray(dout, np.float64)
    Hkv, g = k.shape[1], q.shape[1] // k.shape[1]
    kk, vv = (np.repeat(_clean(x), g, axis=1) for x in (k, v))
    s = np.where(seen, float(sm_scale) * np.matmul(q, kk.transpose(0, 1, 3, 2)), -np.inf)
    m = s.max(-1, keepdims=True)
    e = np.where(seen, np.exp(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
    l = e.sum(-1, keepdims=True)
    p = e / np.where(l > 0, l, 1.0)
    out = np.matmul(p, vv)
    dp = np.matmul(dout, vv.transpose(0, 1, 3, 2))
    ds = p * (dp - (dout * out).sum(-1, keepdims=True))
    dq = float(sm_scale) * np.matmul(ds, kk)
    dk = float(sm_scale) * _group_sum(np.matmul(ds.transpose(0, 1, 3, 2), q), Hkv)
    dv = _group_sum(np.matmul(p.transpose(0, 1, 3, 2), dout), Hkv)
    return out, dq, dk, dv


# ---- the contract ----------------------------------------------------------------------------------------------------------------
def model(q, k, v, out, dout, seen, sm_scale: float, dt: str, seen_kv=None, sum_group: bool = True, use_delta: bool = True):
    """(dq, dk, dv) as fp32 arrays holding values of the storage type: the kernels' contract.  Mutations: seen_kv (the visibility the
    dk / dv sweep uses, where it differs from the rows'), sum_group False (only the first query head of a group reaches dk / dv),
    use_delta False (dS = P o dP)."""
    r = lambda x: weights.round_dt(x, dt).astype(np.float64)        # noqa: E731
    q32, dout64, out64 = np.asarray(q, np.float32), np.asarray(dout, np.float64), np.asarray(out, np.float64)
    Hkv, g = k.shape[1], q32.shape[1] // k.shape[1]
    kk, vv = (np.repeat(_clean(x), g, axis=1) for x in (k, v))
    qs = r(q32 * weights.qk_scale(sm_scale))
    s2 = np.matmul(qs, kk.transpose(0, 1, 3, 2)).astype(np.float32).astype(np.float64)
    sm = np.where(seen, s2, -np.inf)
    m = sm.max(-1, keepdims=True)
    mref = np.where(np.isfinite(m), m, 0.0)
    l = np.where(seen, np.exp2(sm - mref), 0.0).sum(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        lse2 = np.where(l > 0, mref + np.log2(np.where(l > 0, l, 1.0)), 0.0).astype(np.float32).astype(np.float64)
    delta = (dout64 * out64).sum(-1, keepdims=True).astype(np.float32).astype(np.float64) if use_delta else 0.0
    dp = np.matmul(dout64, vv.transpose(0, 1, 3, 2)) - delta

    def p_ds(vis):
        p = np.where(vis, np.exp2(s2 - lse2), 0.0).astype(np.float32).astype(np.float64)
        return r(p), r((p * dp).astype(np.float32))
    _, ds_rows = p_ds(seen)
    p_kv, ds_kv = p_ds(seen if seen_kv is None else seen_kv)
    if not sum_group:
        first = (np.arange(q32.shape[1]) % g == 0)[None, :, None, None]
        p_kv, ds_kv = p_kv * first, ds_kv * first
    scale = np.float64(np.float32(sm_scale))
    dq = np.float32(scale) * np.matmul(ds_rows, kk).astype(np.float32)
    dk = np.float32(scale) * _group_sum(np.matmul(ds_kv.transpose(0, 1, 3, 2), q32.astype(np.float64)), Hkv).astype(np.float32)
    dv = _group_sum(np.matmul(p_kv.transpose(0, 1, 3, 2), dout64), Hkv).astype(np.float32)
    return tuple(weights.round_dt(x, dt) for x in (dq, dk, dv))


# ---- masks -----------------------------------------------------------------------------------------------------------------------
def random_mask(seed, Hl, NQ, NK, keep=0.6):
    """About 60 % kept, column 0 always."""
    m = np.random.default_rng(seed).random((B, Hl, NQ, NK)) < keep
    m[..., 0] = True
    return m


def case_mask(c):
    NQ, NK = -(-c["Sq"] // c["blk"]), -(-SK // c["blk"])
    if c["mask"] == "witness":
        return eref.witness_mask(B, c["Hl"], NQ, NK, c["lens"], c["blk"])
    return random_mask(c["seed"], c["Hl"], NQ, NK)


# ---- 1: fp64 cases ---------------------------------------------------------------------------------------------------------------
def _fp64_cases():
    """The full cross of heads x head dim x type x block x Sq; the mask's head axis, kv_len, the mask kind and the input scale
    rotate through it on sums of the indices, so that each varies inside every slice of the cross."""
    out = []
    pairs, dims, dts, blks, sqs = ((4, 4), (8, 2), (6, 1)), (64, 128), ("bf16", "fp16"), (128, 64), (129, 200, 300)
    for ip, iD, it, ib, iq in itertools.product(range(3), range(2), range(2), range(2), range(3)):
        (H, Hkv), D, dt, blk, Sq = pairs[ip], dims[iD], dts[it], blks[ib], sqs[iq]
        axis = ("H", "Hkv", "1")[(ip + iD + it + ib + iq) % 3]
        out.append(dict(id=f"H{H}kv{Hkv}-D{D}-{dt}-b{blk}-Sq{Sq}-m{axis}", H=H, Hkv=Hkv, D=D, dt=dt, blk=blk, Sq=Sq,
                        Hl={"H": H, "Hkv": Hkv, "1": 1}[axis], lens=[SK, 333] if (iD + iq) % 2 == 0 else [400, 140],
                        mask=("witness", "random")[(ip + it + iq) % 2], scale=(1.0, 2.0)[(ib + iD + iq) % 2],
                        seed=1000 + len(out), causals=(False, True) if blk == 128 else (False,)))
    return out


FP64_CASES = _fp64_cases()


def fp64_inputs(c):
    """N(0, 1) times the case's scale, rounded to the storage type (fp32 arrays)."""
    g = np.random.default_rng(c["seed"])
    H, Hkv, D, Sq = c["H"], c["Hkv"], c["D"], c["Sq"]
    mk = lambda *s: weights.round_dt(g.standard_normal(s).astype(np.float32) * np.float32(c["scale"]), c["dt"])   # noqa: E731
    return dict(q=mk(B, H, Sq, D), k=mk(B, Hkv, SK, D), v=mk(B, Hkv, SK, D), dout=mk(B, H, Sq, D), mask=case_mask(c),
                sm_scale=D ** -0.5)


# ---- 2: the exact gradient witness -----------------------------------------------------------------------------------------------
EXACT_SK, EXACT_SQ, EXACT_H, EXACT_HKV, EXACT_SCALE = 512, 200, 4, 2, 0.125
EXACT_CASES = [dict(id=f"{kind}-{dt}-D{D}", kind=kind, dt=dt, D=D) for kind in ("dq", "dk") for dt in ("bf16", "fp16")
               for D in (64, 128)]
_PAIRS = list(itertools.combinations(range(4), 2))


def exact_mask():
    """bool [B, H, 2, 4]: exactly two 128-blocks per (head, query block), another pair for every head and block of an item."""
    m = np.zeros((B, EXACT_H, 2, 4), bool)
    for b, h, i in itertools.product(range(B), range(EXACT_H), range(2)):
        for j in _PAIRS[(b + 2 * h + i) % 6]:
            m[b, h, i, j] = True
    return m


def _small_ints(rows, D, seed):
    r, c = np.arange(rows)[:, None], np.arange(D)[None, :]
    return ((3 * r + 5 * c + seed) % 5 - 2).astype(np.float32)


def exact_inputs(c):
    """All scores 0 (P = 2^-8 over the 256 keys every row sees), V = +-1 alternating (out = 0 and delta = 0 exactly), dout small
    integers on a lattice; case "dq": q = 0 and k small integers on a lattice, case "dk": k = 0 and q such integers."""
    D = c["D"]
    r, ch = np.arange(EXACT_SQ)[:, None], np.arange(D)[None, :]
    j = np.arange(EXACT_SK)[:, None]
    shape_q, shape_k = (B, EXACT_H, EXACT_SQ, D), (B, EXACT_HKV, EXACT_SK, D)
    v = np.broadcast_to(np.where((j + ch) % 2 == 0, 1.0, -1.0).astype(np.float32), shape_k).copy()
    dout = np.stack([np.stack([np.where((r + ch) % 16 == 0, _small_ints(EXACT_SQ, D, 7 * b + h), 0) for h in range(EXACT_H)])
                     for b in range(B)]).astype(np.float32)
    q, k = np.zeros(shape_q, np.float32), np.zeros(shape_k, np.float32)
    if c["kind"] == "dq":
        k = np.stack([np.stack([np.where((j + ch + 1) % 32 == 0, _small_ints(EXACT_SK, D, 3 * b + hk + 1), 0)
                                for hk in range(EXACT_HKV)]) for b in range(B)]).astype(np.float32)
    else:
        q = np.stack([np.stack([np.where((r + ch + 3) % 16 == 0, _small_ints(EXACT_SQ, D, 5 * b + h + 2), 0)
                                for h in range(EXACT_H)]) for b in range(B)]).astype(np.float32)
    return dict(q=q, k=k, v=v, dout=dout, mask=exact_mask(), sm_scale=EXACT_SCALE, lens=[EXACT_SK] * B)


def exact_seen(mask=None):
    return visible(exact_mask() if mask is None else mask, [EXACT_SK] * B, EXACT_SQ, EXACT_SK, 128, EXACT_H, False)


# ---- 3: visibility through dv ----------------------------------------------------------------------------------------------------
VIS_H, VIS_HKV, VIS_D, VIS_SQ, VIS_LENS = 4, 2, 64, 200, [400, 140]
VIS_CASES = [dict(id=f"b{blk}-{'causal' if causal else 'full'}-m{axis}", blk=blk, causal=causal, Sq=VIS_SQ, lens=VIS_LENS,
                  Hl={"H": VIS_H, "Hkv": VIS_HKV, "1": 1}[axis], mask="witness", seed=77)
             for blk, causal, axis in ((128, False, "Hkv"), (128, True, "H"), (64, False, "1"))]


def vis_rows(c):
    """int [g, NQ, n]: the probe rows of (head in group, query block), n = D / (g NQ) of them, by priority: the first and last row
    of the block, rows 63 / 64 and 31 / 32 of it, the rows either side of the first row that sees a key under the causal limit of
    either item and of kv_len's own edge, then the block's rows from the front."""
    g, blk, Sq = VIS_H // VIS_HKV, c["blk"], c["Sq"]
    NQ = -(-Sq // blk)
    n = VIS_D // (g * NQ)
    rows = np.zeros((g, NQ, n), np.int64)
    for hi, i in itertools.product(range(g), range(NQ)):
        r0, r1 = i * blk, min((i + 1) * blk, Sq)
        want = [r0, r1 - 1, r0 + 63, r0 + 64, r0 + 31, r0 + 32]
        for nb in c["lens"]:
            want += [Sq - nb - 1, Sq - nb, Sq - nb + 1]
        want += list(range(r0 + hi, r1))
        got = []
        for x in want:
            if r0 <= x < r1 and x not in got and len(got) < n:
                got.append(x)
        assert len(got) == n
        rows[hi, i] = got
    return rows


def vis_inputs(c):
    """q = 0 (zero scores), dout one-hot: channel ch belongs to one (head in group, query block, probe row).  Then dv[b, hk, j, ch]
    is non-zero iff that row of head hk g + hi sees key j.  k and v hold NaN at and beyond kv_len."""
    g, Sq = VIS_H // VIS_HKV, c["Sq"]
    rows = vis_rows(c)
    rng = np.random.default_rng(c["seed"])
    dout = np.zeros((B, VIS_H, Sq, VIS_D), np.float32)
    ch = 0
    owner = []
    for hi, i, x in itertools.product(range(g), range(rows.shape[1]), range(rows.shape[2])):
        for hk in range(VIS_HKV):
            dout[:, hk * g + hi, rows[hi, i, x], ch] = 1.0
        owner.append((hi, int(rows[hi, i, x])))
        ch += 1
    k = weights.round_dt(rng.standard_normal((B, VIS_HKV, SK, VIS_D)).astype(np.float32), "bf16")
    v = weights.round_dt(rng.standard_normal((B, VIS_HKV, SK, VIS_D)).astype(np.float32), "bf16")
    for b, nb in enumerate(c["lens"]):
        k[b, :, nb:] = np.nan
        v[b, :, nb:] = np.nan
    return dict(q=np.zeros((B, VIS_H, Sq, VIS_D), np.float32), k=k, v=v, dout=dout, mask=case_mask(c), sm_scale=VIS_D ** -0.5,
                owner=owner)


def vis_pattern(c, inp, seen=None):
    """bool [B, Hkv, Sk, D]: where dv must be non-zero."""
    g = VIS_H // VIS_HKV
    if seen is None:
        seen = visible(inp["mask"], c["lens"], c["Sq"], SK, c["blk"], VIS_H, c["causal"])
    want = np.zeros((B, VIS_HKV, SK, VIS_D), bool)
    for ch, (hi, row) in enumerate(inp["owner"]):
        for hk in range(VIS_HKV):
            want[:, hk, :, ch] = seen[:, hk * g + hi, row, :]
    return want
