"""numpy reference of the packed calls: block_sparse_extend / select_blocks_pooled(cu_seqlens_q=,
max_q_len=) and append_kv_e4m3(cu_seqlens=).  A plain helper module, no device.  q is [T, H, D]; the device sanitises cu_seqlens_q
(sanitise below) and item b is the existing extend call on rows [s_b, s_b + n_b), so the references are the existing ones
(extend_ref, ragged_ref) per item, placed at the item's rows; beside them stands a direct form of the rule with the mutations the
CPU test applies, and the bound QP on the row groups of a launch with its brute-force counterpart.

    sanitise           cu -> (s [B + 1], n [B]): s_b the running maximum of clamp(cu[b], 0, T), n_b = min(s_{b+1} - s_b, M)
    visible            extend_ref.visible of each truncated item at rows [s_b, s_b + n_b); every other row sees nothing
    visible_direct     the same rule per row t with s_b, n_b written in, and its mutants
    visible_naive      ... as a loop over every (t, h, j)
    pad / unpad        the padded copy [B, H, M, D] of a packed tensor and back (the ragged call's layout)
    select             ragged_ref's selection on the padded copy, and its mutants
    pieces, qp_bound   row groups of an item; the host bound on their sum; max_pieces: the true maximum by dynamic programming"""
from __future__ import annotations

import numpy as np

import extend_ref as eref
import ragged_ref as rref

B, T, SK = 4, 300, eref.SK
# (lengths, M, rows in front of the first item): T - sum(lengths) - gap rows of slack stay behind the last item
LSETS = (((150, 129, 1, 0), 150, 7), ((1, 1, 1, 1), 1, 3), ((64, 65, 128, 0), 128, 11))
MALFORMED = ("a decreasing pair", "a value above T", "a negative value", "an item longer than M")


def cu_of(lengths, gap: int = 0):
    return [gap + int(sum(lengths[:b])) for b in range(len(lengths) + 1)]


def malformed(kind: str):
    """(cu, M) of the four malformed inputs, over T = 300 rows; what the sanitised rule makes of them stands beside each."""
    return {"a decreasing pair": ([0, 100, 60, 200, 290], 128),        # s = 0 100 100 200 290: item 1 is empty, item 2 = rows 100..199
            "a value above T": ([5, 70, 4000, 4001, 4002], 150),       # s = 5 70 300 300 300: item 1 holds 230 rows, 150 of them live
            "a negative value": ([-9, -2, 64, 65, 193], 128),          # s = 0 0 64 65 193: item 0 is empty
            "an item longer than M": ([0, 10, 250, 251, 300], 100)}[kind]      # item 1: rows 10..109 live, 110..249 empty


def sanitise(cu, T: int, M: int):
    s, run = [], 0
    for x in cu:
        run = max(run, min(max(int(x), 0), T))
        s.append(run)
    return s, [min(s[b + 1] - s[b], M) for b in range(len(s) - 1)]


def row_items(cu, T: int, M: int):
    """(item [T] (-1: none), row in item [T])."""
    s, n = sanitise(cu, T, M)
    item, row = np.full(T, -1), np.zeros(T, np.int64)
    for b in range(len(n)):
        item[s[b]:s[b] + n[b]] = b
        row[s[b]:s[b] + n[b]] = np.arange(n[b])
    return item, row


def live_blocks(n: int, blk: int) -> int:
    return -(-n // blk)


# ---- the extend rule -------------------------------------------------------------------------------------------------------------
def visible(mask, lens, cu, T: int, M: int, Sk: int, blk: int, H: int, causal: bool):
    """bool [T, H, Sk]: per item the existing rule on the truncated call, at the item's rows."""
    mask = np.asarray(mask, bool)
    nb = len(lens)
    m = np.broadcast_to(mask, (nb,) + mask.shape[1:])
    s, ns = sanitise(cu, T, M)
    out = np.zeros((T, H, Sk), bool)
    for b, n in enumerate(ns):
        if n:
            one = eref.visible(m[b:b + 1, :, :live_blocks(n, blk)], [lens[b]], n, Sk, blk, H, causal)[0]
            out[s[b]:s[b] + n] = one.transpose(1, 0, 2)
    return out


MUTANTS = ("boundary row to the next item", "causal offset from M", "causal offset from T", "n of the neighbouring item",
           "list row of block i + 1")


def visible_direct(mask, lens, cu, T: int, M: int, Sk: int, blk: int, H: int, causal: bool, mut: str = ""):
    """Row t of [0, T): its item is the b with s_b <= t < s_b + n_b, r = t - s_b; it sees key j iff mask[b, hl(h), r // block,
    j // block], j < kv_len[b], j < NK * block and, with causal, j <= r + kv_len[b] - n_b.  mut: one of MUTANTS."""
    assert mut in ("",) + MUTANTS
    mask = np.asarray(mask, bool)
    nb = len(lens)
    Hl, NQ, NK = mask.shape[1:]
    m = np.broadcast_to(mask, (nb, Hl, NQ, NK))
    hl = np.arange(H) // (H // Hl)
    s, ns = sanitise(cu, T, M)
    j = np.arange(Sk)
    inside = j < NK * blk
    out = np.zeros((T, H, Sk), bool)
    for t in range(T):
        b = next((b for b in range(nb) if s[b] <= t < s[b] + ns[b]), -1)
        if mut == "boundary row to the next item":      # `<=` for `<`: row s_b - 1 is given to item b, as its row -1
            b = next((x for x in range(nb) if ns[x] and t == s[x] - 1), b)
        if b < 0:
            continue
        n = ns[(b + 1) % nb] if mut == "n of the neighbouring item" else ns[b]
        r = t - s[b]
        if r >= n:
            continue
        qb = min(max(r, 0) // blk + (mut == "list row of block i + 1"), NQ - 1)
        row = inside & (j < lens[b])
        kept = np.zeros((H, Sk), bool)
        kept[:, inside] = m[b][hl][:, qb][:, j[inside] // blk]
        if causal:
            base = {"causal offset from M": M, "causal offset from T": T}.get(mut, n)
            row = row & (j <= r + lens[b] - base)
        out[t] = kept & row[None]
    return out


def visible_naive(mask, lens, cu, T, M, Sk, blk, H, causal):
    mask = np.asarray(mask, bool)
    Hl, NQ, NK = mask.shape[1:]
    item, row = row_items(cu, T, M)
    _, ns = sanitise(cu, T, M)
    out = np.zeros((T, H, Sk), bool)
    for t in range(T):
        b = int(item[t])
        if b < 0:
            continue
        mb = mask[b if mask.shape[0] > 1 else 0]
        for h in range(H):
            lst = mb[h // (H // Hl), int(row[t]) // blk]
            for j in range(min(lens[b], NK * blk, Sk)):
                if causal and j > row[t] + lens[b] - ns[b]:
                    break
                out[t, h, j] = lst[j // blk]
    return out


# ---- packed <-> padded -------------------------------------------------------------------------------------------------------------
def pad(x, cu, T: int, M: int, fill=np.nan):
    """x [T, H, ...] -> [B, H, M, ...]: item b's n_b rows in front, `fill` behind them."""
    s, ns = sanitise(cu, T, M)
    x = np.asarray(x)
    out = np.full((len(ns), x.shape[1], M) + x.shape[2:], fill, x.dtype)
    for b, n in enumerate(ns):
        out[b, :, :n] = np.moveaxis(x[s[b]:s[b] + n], 0, 1)
    return out


def unpad(y, cu, T: int, M: int, fill=0.0):
    """y [B, H, M, ...] -> [T, H, ...]: the rows of no item hold `fill`."""
    s, ns = sanitise(cu, T, M)
    y = np.asarray(y)
    out = np.full((T, y.shape[1]) + y.shape[3:], fill, y.dtype)
    for b, n in enumerate(ns):
        out[s[b]:s[b] + n] = np.moveaxis(y[b, :, :n], 1, 0)
    return out


def attention(q, k, v, cu, T, M, mask, lens, blk, causal, sm_scale, dt=None):
    """(out [T, H, D], lse [T, H]) fp64 of the packed call: ragged_ref's attention on the padded copy, gathered back."""
    H = q.shape[1]
    _, ns = sanitise(cu, T, M)
    qp = pad(np.asarray(q, np.float32), cu, T, M)
    mask = np.asarray(mask, bool)
    m = np.broadcast_to(mask, (len(lens),) + mask.shape[1:])
    seen = rref.visible(m, lens, ns, M, k.shape[2], blk, H, causal)
    out, lse = rref.attention(qp, k, v, seen, sm_scale, dt)
    return unpad(out, cu, T, M, 0.0), unpad(lse[..., None], cu, T, M, -np.inf)[..., 0]


# ---- the selection -------------------------------------------------------------------------------------------------------------------
SELECT_MUTANTS = ("item rows from b * M", "n of the neighbouring item", "off from M")


def select(q, k, top_k, cu, T: int, M: int, mut: str = "", **kw):
    """The packed selection: ragged_ref's direct form on the padded copy of q [T, H, D] with q_len = n_b -> dict(mask [B, Hl, NQ, NK],
    t, mass).  mut: the padded copy taken from rows b * M (the padded layout's arithmetic on the packed tensor), the row counts of
    item (b + 1) % B, or the causal offset kv_len[b] - M."""
    assert mut in ("",) + SELECT_MUTANTS
    s, ns = sanitise(cu, T, M)
    nb = len(ns)
    q = np.asarray(q, np.float64)
    if mut == "item rows from b * M":
        s = [min(b * M, T) for b in range(nb + 1)]
    if mut == "n of the neighbouring item":
        ns = [ns[(b + 1) % nb] for b in range(nb)]
    qp = np.zeros((nb, q.shape[1], M, q.shape[2]))
    for b, n in enumerate(ns):
        rows = np.nan_to_num(q[s[b]:min(s[b] + n, T)])
        qp[b, :, :rows.shape[0]] = np.moveaxis(rows, 0, 1)
    return rref.select_direct(qp, k, top_k, ns, mut="off from Sq" if mut == "off from M" else "", **kw)


# ---- row groups of a launch --------------------------------------------------------------------------------------------------------
def groups_of(gu: int, M: int, blk: int):
    """(gh, qg, cpb) of the packed call: extend_ref.row_groups with M for Sq, and the groups of a full query block."""
    gh, qg = eref.row_groups(gu, M, blk)
    return gh, qg, -(-min(M, blk) // qg)


def pieces(n: int, blk: int, qg: int, cpb: int) -> int:
    return n // blk * cpb + -(-(n % blk) // qg)


def qp_bound(T: int, Bn: int, M: int, qg: int, blk: int) -> int:
    """The host's bound: min(B * pieces(M), k + (T - k) * cpb // min(M, block)) with k = min(B, T)."""
    qmax = min(M, blk)
    cpb = -(-qmax // qg)
    k = min(Bn, T)
    return min(Bn * pieces(M, blk, qg, cpb), k + (T - k) * cpb // qmax)


def max_pieces(T: int, Bn: int, M: int, qg: int, blk: int) -> int:
    """The most row groups any sanitised cu_seqlens_q can ask for: max of sum pieces(n_b) over n_b in [0, M], sum n_b <= T, by
    dynamic programming over the items."""
    cpb = -(-min(M, blk) // qg)
    p = [pieces(n, blk, qg, cpb) for n in range(min(M, T) + 1)]
    best = [0] * (T + 1)
    for _ in range(Bn):
        best = [max(best[t - n] + p[n] for n in range(min(t, len(p) - 1) + 1)) for t in range(T + 1)]
    return best[T]


# ---- the cases of tests/test_gpu_packed.py -----------------------------------------------------------------------------------------
def gpu_combos():
    """Parameters take turns over the product, as tests/test_gpu_ragged.py's: every value of every axis meets every head grouping."""
    out = []
    for gi, (H, Hkv) in enumerate(eref.GROUPS):
        for i in range(12):
            blk = (128, 64)[(i // 4) % 2]
            out.append(dict(H=H, Hkv=Hkv, D=64 if H == 72 else (64, 128)[i % 2], dt=("bf16", "fp16")[(i // 2) % 2], blk=blk,
                            axis=("H", "Hkv", "1")[(i + i // 3) % 3], causal=bool((i // 3) % 2), lset=(i + gi) % 3,
                            kv_dev=bool((i + gi // 2) % 2), bps=(None, 1, 2, -(-SK // blk))[(i + gi) % 4],
                            cache=("bf16-paged", "e4m3-paged", "contiguous")[(i // 2 + gi) % 3], seed=3000 * (gi + 1) + i))
    return out


def combo_lens(c):
    """kv_len per item, the length after the append (ragged_ref.combo_lens: one item shorter than its chunk, one at capacity)."""
    return rref.combo_lens(c, None)


# ---- witness cases: zero scores, V of 0 / 1 on a packed batch ----------------------------------------------------------------------
def _witness_cases():
    out = []
    for i, (H, Hkv, axis, D, blk, dt, lset, C) in enumerate((
            (8, 2, "Hkv", 64, 128, "bf16", 0, 2), (2, 2, "H", 64, 64, "fp16", 2, 1), (72, 1, "1", 64, 128, "fp16", 0, 6),
            (8, 8, "H", 128, 64, "bf16", 2, 3))):
        lengths, M, gap = LSETS[lset]
        c = dict(H=H, Hkv=Hkv, Hl={"H": H, "Hkv": Hkv, "1": 1}[axis], D=D, blk=blk, dt=dt, lset=lset, C=C, causal=True, seed=500 + i,
                 M=M, cu=cu_of(lengths, gap))
        c["s"], c["ns"] = sanitise(c["cu"], T, M)
        c["lens"] = [SK, 160, 333, 129] if i % 2 else [385, 140, SK, 256]     # item 1 (129 / 65 rows): its diagonal starts inside the cache
        c["id"] = f"vis-H{H}kv{Hkv}-{dt}-D{D}-b{blk}-l{lset}-m{axis}"
        out.append(c)
    return out


def witness_probes(c):
    """The probe keys, by priority, cut to D / 2 channels: either side of each item's own causal diagonal at its first and at its
    last live row; the keys that tell item b's first row from item b - 1's last (each row's own last visible key: under the other
    item's offset it would be invisible or not the last); then either side of kv_len[b]."""
    wanted = []
    for n, ln in zip(c["ns"], c["lens"]):
        if n:
            for r in (0, n - 1):
                wanted += [r + ln - n, r + ln - n + 1]
    for ln in c["lens"]:
        wanted += [ln - 1, ln]
    probes = []
    for p in wanted:
        if 0 <= p < SK and p not in probes and len(probes) < c["D"] // 2:
            probes.append(p)
    return sorted(probes)


def witness_inputs(c):
    import visibility as vis
    NQ, NK = -(-c["M"] // c["blk"]), -(-SK // c["blk"])
    mask = eref.witness_mask(B, c["Hl"], NQ, NK, c["lens"], c["blk"])
    q, k = vis.zero_score_qk(c["seed"], 1, c["H"], T, SK, c["D"])
    v = np.broadcast_to(vis.witness_v(SK, c["D"], witness_probes(c)), (B, c["Hkv"], SK, c["D"])).copy()
    k = np.broadcast_to(k[:, :c["Hkv"]], (B, c["Hkv"], SK, c["D"])).copy()
    return dict(q=np.ascontiguousarray(q[0].transpose(1, 0, 2)), k=k, v=v, mask=mask, sm_scale=c["D"] ** -0.5)


def witness_reference(c, inp, mut=None):
    """(out [T, H, D], lse [T, H]) fp64: every output element is a count over the visible keys divided by their number (K and V are
    the same for every item, so the rows are one batch item of T rows).  mut None: the per-item rule; "" or one of MUTANTS: the
    direct form."""
    args = (inp["mask"], c["lens"], c["cu"], T, c["M"], SK, c["blk"], c["H"], c["causal"])
    seen = visible(*args) if mut is None else visible_direct(*args, mut=mut)
    seen4 = np.ascontiguousarray(seen.transpose(1, 0, 2))[None]
    q4 = np.ascontiguousarray(inp["q"].transpose(1, 0, 2))[None]
    out, lse = rref.attention(q4, inp["k"][:1], inp["v"][:1], seen4, inp["sm_scale"], c["dt"])
    return np.ascontiguousarray(out[0].transpose(1, 0, 2)), np.ascontiguousarray(lse[0].T)


WITNESS_CASES = _witness_cases()
