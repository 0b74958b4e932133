"""Exact softmax-weight tests of the 2-byte, e4m3 and pv attention kernels: inputs whose softmax WEIGHTS are known exactly.

The counterpart of tests/visibility.py.  There every score is 0, which pins which keys a row sums and nothing about the weight
each key gets.  Here every score is a small non-negative integer in the kernels' own binary units, so every exp2(S - m), every
rescale factor and every merge weight of a split walk is a power of two, exact in bf16, fp16 and fp32:

    Q   row r of head h is one-hot: q[r, c] = a at c = cls(r, h) = ((37 r + 11 h) mod D) xor ((r // D) mod 4), else 0.
        a is THE value of the input type for which round_dt(fp32(a) * qk_scale) == 2^-3, found by enumerating the type
        (find_a), where qk_scale = (float)(sm_scale * 1.44269504) is what every 2-byte K5 multiplies Q by before it rounds Q
        back to the input type.
    K   k[j, c] = 8 n[kvh, j, c] with integers 0 <= n <= 15: a score is ONE product, n[j, cls(r, h)], whatever the MFMA's
        summation order.  n = base + profile: base hashed from (kvh, j, c), the profile chosen by class (KINDS below), so
        that every query block holds rows of every kind.
    V   0 / 1 and sparse (a rectified row's comp, an average of V, must not drown R * census).  Channels [0, D/2): one-hot
        digits of the key's place in its 32-key sub-step (any two keys of a sub-step differ in at least two channels), of a
        hash of the sub-step and of a hash of the key, the hashes different per K/V head.  Channels [D/2, D): the 64-key tile census of visibility.witness_v, tile t in channels D/2 + (37 t mod D/2) and D/4
        further on.

Numerator and denominator of a row are then sums of powers of two, exact in fp32 under any summation order and any lag of the
kernels' softmax reference as long as sum_j 2^(n_j - n_min) < 2^24 over the row's visible keys (budget(), asserted for every
row of every case by tests/test_weights_cpu.py; for fp16 the spread of a row is kept <= 10 so that P >= 2^-10 stays normal).
What is left is 1 / l, * R, one fma and one conversion: the bound is visibility's, |got - ref| <= ULP |ref| + FLOOR max|ref|
with visibility's ULP and FLOOR, and an element whose reference is 0 must be exactly 0.  One assumption is not derived: that
the hardware exp2 of an integer is the exact power of two (tests/test_gpu_weights.py checks torch.exp2 on the device first).

The reference is a weighted count, sum 2^n v / sum 2^n over the keys visibility's rules admit (visibility.plain_ref,
dense_ref, rect_ref and tests/test_ranged_cpu.py's rule are used as they are; only the weights are new).  The model mutants of
insensitive() live here too, all in numpy: no kernel is built in a mutated form.

The fp8 forms (a case's "fp8": True = e4m3 Q, K, V and P; "pv" = 2-byte Q . K^T, e4m3 P and V; rsa_attn_fp8_kernel.hip).  Integer
scores stay exact there under conditions that tests/test_weights_cpu.py checks for every case:
    P   the code map (PMap<true>, pmap()): a score at integer distance d from the row's reference arrives as the code 108 + 8 d,
        mantissa field 4, the value 1.5 * 2^(d + 6); the 96 cancels between P . V and the row sum.  d <= THRESH by the move rule;
        below, the last normal code is 12: every visible key of a row must lie within max_spread() = 12 of the row's maximum.  Both
        forms use the fp16 amplitudes (spread <= 10, <= 11 after balance_mu()), and the budget is 3 * 2^max(V_GAINS) * sum < 2^24.
    pv  the kernel multiplies Q by (float)(sm_scale * 1.44269504 * 8) and rounds it to the 2-byte type: a is the value that rounds
        to 1 (Model.q_target), K = 8 n as before.
    Q   e4m3: the image of a * qk_const is 2^-3 in every block (the MFMA's scale operand adds the 8).  Q's exponent is therefore
        the same in every block: NOT witnessed.
    K   e4m3: the kernel subtracts mu, the mean of up to 8 sampled full blocks of K ("smooth K", on in every case: the product's
        path).  K - mu = 8 (n - mu / 8) is exact in e4m3 only for an integral mu / 8: balance_mu() puts +-1 on base-only keys of
        the sampled rows until it is.  The key blocks QUIET_BLOCKS hold no n above QUIET, which makes their K exponent differ.
    V   0 / 2^g per 128-key block, g hashed from V_GAINS: exact, and V's block exponents differ between blocks.
fp8_image_faults() checks all of it on the images the oracle's byte-exact contract makes (fp8_kmean, fp8_block_images), among it
that two distinct K and two distinct V exponents occur among the blocks some row sees.  What is left is what is left above, and
the bound is the same.  A second assumption is not derived: that v_cvt_pk_u8_f32 of an exact integer is that integer (the fp8
cases meeting the bound on the device shows it).

Out of scope: Q's block exponent, the selection pass, and rsa_attn_masked.hip: its scale is applied in fp32, so integer SCORES cannot
be reached -- tests/masked_witness.py reaches integer weights there through the bias instead."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional

import numpy as np

import visibility as vis
from visibility import FLOOR, SENSITIVITY, ULP  # noqa: F401  (the bound is visibility's, not restated)

LOG2E = 1.44269504          # the constant of the kernels' launchers (rsa_attn.hip), not log2(e) to full precision
TARGET = 2.0 ** -3          # round_dt(a * qk_scale)
KSCALE = 8                  # k = KSCALE * n, so that a score is n
SUB = 32                    # keys per sub-step of every K5 walk
KINDS = ("flat", "fall", "step", "edge", "stairs", "spike", "focus", "focus")       # the kind of class c is KINDS[c % 8]
#   flat     base only: no reference move after the first sub-step
#   fall     the maximum sits in the first 32 keys and falls off
#   step     +9, +10 or +12 (by class) on three keys from j0 = 5 (mod 32) in an odd sub-step of the third key block: a
#            moderate jump with comparable weight on either side of it
#   edge     +8 exactly, the deferred rescale's threshold: either decision must give the same answer
#   stairs   +3 per key block on two keys of each of the key blocks 1 .. 4 (fp16: 1 .. 3), in an odd and an even sub-step by
#            turns: cumulative moves, some below and some above the threshold, each with comparable weight before it
#   spike    +12 on one key in the ragged last tile and on the key just outside each limit under test (kv_len, the causal
#            diagonal, a window edge, a chunk's end): the outside one must not be seen at all
#   focus    +12 (fp16: +9) on the first key and on one hashed key of every fourth sub-step (which fourth by class: the focus
#            rows of any 16 consecutive rows cover all four): most of the row's weight sits on single keys, so a weight
#            attached to the wrong key inside that sub-step shows, also where a limit cuts the sub-step short
#            (forced_classes() adds focus classes where a block has fewer rows or a walk too many sub-steps for that)
FOCUS_EVERY = 4
AMP = {"bf16": dict(base=4, step=(9, 10, 12), edge=8, stairs=(3, 4), spike=12, focus=12, fall=9),
       "fp16": dict(base=2, step=(9, 9, 9), edge=8, stairs=(3, 3), spike=9, focus=9, fall=9)}
STEP_KINDS = ("step", "stairs")
# the e4m3 and pv forms (module docstring, "The fp8 forms"): the fp16 amplitudes whatever the storage type
FP8_AMP = "fp16"
QUIET, QUIET_BLOCKS = 8, (1, 4, 7)     # e4m3 form: these key blocks hold no n above QUIET: |n - mu / 8| <= 7 there, 8 and more in a
                            # block with a full-height profile, and the K exponents of the two differ
V_GAINS = (0, 1)            # fp8 forms: V of key block b of K/V head kvh is 0 / 2^g, g hashed from this set


def form_of(c: dict):
    """False, True (e4m3) or "pv": the case's operand form."""
    return c.get("fp8", False)


def pmap():
    """(U, BIAS, OFFSET, THRESH) of the kernels' code-map P (rsa_attn_fp8_kernel.hip PMap<true>, as oracle.py restates it)."""
    from oracle import oracle as orc
    return orc.PCODE_U, orc.PCODE_BIAS, orc.PCODE_OFFSET, orc.PCODE_THRESH


def max_spread() -> int:
    """The largest S - m for which the code of P is still mantissa field 4 of a NORMAL e4m3 value: a score at distance d below the
    reference arrives as U (OFFSET - d) + BIAS = 108 - 8 d, and the smallest normal code is 8."""
    U, BIAS, OFFSET, _ = pmap()
    return int((U * OFFSET + BIAS - 8) // U)


# ---- the value of Q ------------------------------------------------------------------------------------------------------
def qk_scale(sm_scale: float) -> np.float32:
    """(float)(sm_scale * 1.44269504), in double as the launchers compute it."""
    return np.float32(float(sm_scale) * LOG2E)


@functools.lru_cache(maxsize=None)
def find_a(dt: str, sm_scale: float, target: float = TARGET):
    """-> (the values a of the type with round_dt(fp32(a) * qk_scale) == target, the smallest distance of such a product from a
    rounding tie in ulps of the type).  Enumerates all 2^16 values of the type on the CPU; no table."""
    import torch
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    allv = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(tdt).float()
    allv = allv[torch.isfinite(allv)]
    prod = allv * torch.tensor(float(qk_scale(sm_scale)), dtype=torch.float32)       # one fp32 product, as the kernel's
    hit = prod.to(tdt).float() == target
    a = allv[hit].double().numpy()
    ulp = ULP[dt] * target                     # the spacing of the type at target (above it; half of it below)
    p = prod[hit].double().numpy()
    tie_hi, tie_lo = target + ulp / 2, target - ulp / 4
    margin = float(np.minimum(np.abs(p - tie_hi) / ulp, np.abs(p - tie_lo) / (ulp / 2)).min()) if len(p) else 0.0
    return a, margin


def round_dt(x: np.ndarray, dt: str) -> np.ndarray:
    import torch
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    return torch.from_numpy(np.asarray(x, np.float32)).to(tdt).float().numpy()


# ---- hashing -------------------------------------------------------------------------------------------------------------
def _mix(*xs) -> np.ndarray:
    """A 64-bit mix of integer arrays (broadcast together): the inputs' only source of irregularity, fixed for ever."""
    h = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for x in xs:
            h = (h ^ np.asarray(x).astype(np.uint64)) * np.uint64(0xBF58476D1CE4E5B9)
            h = h ^ (h >> np.uint64(31))
        h = h * np.uint64(0x94D049BB133111EB)
        return h ^ (h >> np.uint64(29))


def cls(r, h, Dq):
    """The class (the one non-zero channel) of row r of head h: every class occurs once in every run of Dq rows, and rows r, r + 1,
    r + 32 and r + 64 differ at every head dim (37 * 32 and 37 * 64 are multiples of 32 and 64: the xor tells those runs apart)."""
    r = np.asarray(r)
    return ((37 * r + 11 * np.asarray(h)) % Dq) ^ ((r // Dq) % 4)


# ---- K: the integer scores -----------------------------------------------------------------------------------------------
def scores_n(dt: str, Hkv: int, Sk: int, Dq: int, key_block: int, outside=(), outside_keys=(), head_of_kv=1,
             forced=None, fp8=False, kvalid: Optional[int] = None) -> np.ndarray:
    """int8 [Hkv, Sk, Dq]: n[kvh, j, c] = base + profile_c(j) (module docstring).  outside: pairs (o, side) such that key r + o
    lies just outside a limit of row r, to the right (side = 1) or to the left (-1): the spike classes put +spike on the keys j
    with cls(j - o, h) == c, h = kvh * head_of_kv (the first query head of the K/V head).  outside_keys: keys just outside a limit
    of every row (kv_len, a chunk's end).  forced: {kvh: {c: (residue, period)}}, the classes forced_classes() turns into focus
    classes with ONE heavy key (the first) in the sub-steps s with s % period == residue.  fp8: the operand form (the fp16
    amplitudes; e4m3 form: quiet key blocks and the balance of balance_mu() over the kvalid rows the K mean is sampled from)."""
    amp = AMP[FP8_AMP if fp8 else dt]
    kvh = np.arange(Hkv)[:, None, None]
    j = np.arange(Sk)[None, :, None]
    c = np.arange(Dq)[None, None, :]
    n = (_mix(kvh, j, c, 1) % np.uint64(amp["base"])).astype(np.int64)
    n_base = n
    kind = np.broadcast_to(np.where(c % 8 == 7, 6, c % 8), (Hkv, 1, Dq)).copy()     # the index into KINDS (both focus classes: 6)
    res = np.broadcast_to((2 * (c // 8) + (c % 8 - 6)) % FOCUS_EVERY, (Hkv, 1, Dq)).copy()
    period = np.full((Hkv, 1, Dq), FOCUS_EVERY)
    single = np.zeros((Hkv, 1, Dq), bool)
    for hk, table in (forced or {}).items():
        for cc, (rr, pp) in table.items():
            kind[hk, 0, cc], res[hk, 0, cc], period[hk, 0, cc], single[hk, 0, cc] = 6, rr, pp, True
    grp = c // 8
    sub = j // SUB
    # fall
    n = n + np.where((kind == 1) & (j < SUB), np.maximum(0, amp["fall"] - j // 3), 0)
    # step and edge: three keys from j0 (step) / j0 + 64 (edge); j0 = 5 mod 32 in an odd sub-step of the third key block
    j0 = 2 * key_block + SUB + 5 + 64 * (kvh % 2)
    stepJ = np.asarray(amp["step"])[grp % 3]
    n = n + np.where((kind == 2) & (j >= j0) & (j < j0 + 3), stepJ, 0)
    n = n + np.where((kind == 3) & (j >= j0 + 64) & (j < j0 + 67), amp["edge"], 0)
    # stairs
    per, cap = amp["stairs"]
    kb = j // key_block
    at = (kb % 2) * SUB + 7
    n = n + np.where((kind == 4) & (kb >= 1) & (kb <= cap) & (j % key_block >= at) & (j % key_block < at + 2), per * np.minimum(kb, cap), 0)
    # spike
    spike = np.zeros((Hkv, Sk, Dq), bool)
    spike[:, max(Sk - 3, 0), :] = True
    for key in outside_keys:
        if 0 <= key < Sk:
            spike[:, key, :] = True
    for o, _ in outside:
        spike |= cls(j - o, kvh * head_of_kv, Dq) == c
    n = n + np.where((kind == 5) & spike, amp["spike"], 0)
    # focus: sub-steps s with s % FOCUS_EVERY == res(c), two keys of each
    t0 = 8 + (_mix(kvh, sub, c, 2) % np.uint64(16)).astype(np.int64)      # (never a partner of key 0 under the three swaps)
    n = n + np.where((kind == 6) & (sub % period == res) & ((~single & (j % SUB == t0)) | (j % SUB == 0)), amp["focus"], 0)
    # ... and the spike and focus classes +focus on the last key INSIDE such a per-row limit: the few rows that see the stub of a
    # sub-step the diagonal cuts short have most of their weight there
    inside = np.zeros((Hkv, Sk, Dq), bool)
    for o, side in outside:
        inside |= cls(j - o + side, kvh * head_of_kv, Dq) == c
    n = np.where((kind >= 5) & inside, np.maximum(n, amp["focus"] + n % amp["base"]), n)
    if fp8 is True:
        n = np.where(np.isin(j // 128, QUIET_BLOCKS), np.minimum(n, QUIET), n)
        n = balance_mu(n, n == n_base, Sk if kvalid is None else kvalid)
    assert n.min() >= 0 and n.max() <= 15
    return n.astype(np.int8)


def sampled_rows(valid: int) -> np.ndarray:
    """The rows of K that the e4m3 producer's "smooth K" mean is taken over (oracle.fp8_kmean, rsa_fp8.hip::kmean_sample_kernel):
    up to 8 evenly spaced full 128-row blocks of the first `valid` rows."""
    assert valid >= 128, "the model has no case whose only block of K is a partial one"
    nb = valid // 128
    ns = min(nb, 8)
    return np.concatenate([np.arange(128) + 128 * ((i * nb) // ns) for i in range(ns)])


def balance_mu(n: np.ndarray, base_only: np.ndarray, valid: int) -> np.ndarray:
    """n with +1 (or -1) on as many base-only keys (by a hash) of the sampled rows as it takes to make every (K/V head, channel) sum
    over those rows a multiple of their number (the nearest that the base-only keys can reach): the e4m3 kernel subtracts mu, the mean of K = 8 n over these rows, from
    K, and K - mu = 8 (n - u) is exact in e4m3 (|n - u| <= 15 has four significant bits) with an integer u = mu / 8 only then.  A
    base-only key goes from 0 / 1 to at most 2 (-1 only from 1 to 0), so a row's spread grows by at most 1."""
    rows = sampled_rows(valid)
    sub = n[:, rows, :]
    tot = sub.sum(1)                                                     # [Hkv, D]
    N = len(rows)
    near = np.maximum(np.rint(tot / N), 1).astype(np.int64) * N - tot             # to the nearest multiple, to the next one up
    above = -(-tot // N) * N - tot                                                 # where the keys that may go down are too few
    need = np.where((near < 0) & ((base_only[:, rows, :] & (sub >= 1)).sum(1) < -near), above, near)
    up = need >= 0
    cand = base_only[:, rows, :] & (up[:, None, :] | (sub >= 1))
    assert (cand.sum(1) >= np.abs(need)).all(), "too few base-only keys among the sampled rows to balance a channel's mean"
    hk, jj, cc = np.meshgrid(np.arange(n.shape[0]), rows, np.arange(n.shape[2]), indexing="ij")
    order = np.where(cand, _mix(hk, jj, cc, 6) >> np.uint64(1), np.uint64(2 ** 63))     # (candidates first, by hash)
    rank = np.argsort(np.argsort(order, axis=1, kind="stable"), axis=1, kind="stable")
    out = n.copy()
    out[:, rows, :] = sub + np.where(up, 1, -1)[:, None, :] * (rank < np.abs(need)[:, None, :])
    return out


# ---- V -------------------------------------------------------------------------------------------------------------------
def witness_v(Hkv: int, Sk: int, D: int) -> np.ndarray:
    """float32 [Hkv, Sk, D] of 0 / 1 (module docstring)."""
    half = D // 2
    assert half >= 16
    j = np.arange(Sk)
    v = np.zeros((Hkv, Sk, D), np.float32)
    low = j % SUB
    hk = np.arange(Hkv)[:, None]
    sub_hash, key_hash = _mix(hk, (j // SUB)[None, :], 3), _mix(hk, j[None, :], 4)
    # one-hot digits, (value, channels): any two keys of a sub-step differ in a digit of their place in it, so in two channels
    if half >= 64:
        digits = [(low, 32), (sub_hash % np.uint64(16), 16), (key_hash % np.uint64(half - 48), half - 48)]
    elif half >= 32:
        digits = [(low % 8, 8), (low // 8, 4), (sub_hash % np.uint64(8), 8), (key_hash % np.uint64(half - 20), half - 20)]
    else:
        digits = [(low % 8, 8), (low // 8, 4), (sub_hash % np.uint64(half - 12), half - 12)]
    ch0 = 0
    kk, jj = np.meshgrid(np.arange(Hkv), j, indexing="ij")
    for val, width in digits:
        v[kk, jj, ch0 + np.broadcast_to(np.asarray(val).astype(np.int64), (Hkv, Sk))] = 1
        ch0 += width
    assert ch0 == half
    for shift in (0, half // 2):                                   # (stride and copy: every 32-channel d-tile names tiles)
        v[:, j, half + (37 * (j // vis.TILE) + shift) % half] = 1
    return v


def v_gains(Hkv: int, Sk: int) -> np.ndarray:
    """int [Hkv, ceil(Sk / 128)]: g of each 128-key block of V in the fp8 forms (V = 0 / 2^g: exact, and the block's E8M0 exponent
    is g - 8, so that a wrong V exponent shows; the first two blocks of a head always differ)."""
    nb = -(-Sk // 128)
    hk, b = np.arange(Hkv)[:, None], np.arange(nb)[None, :]
    g = np.asarray(V_GAINS)[(_mix(hk, b, 5) % np.uint64(len(V_GAINS))).astype(np.int64)]
    if nb > 1:
        g[:, 1] = np.where(g[:, 1] == g[:, 0], np.asarray(V_GAINS)[(np.searchsorted(V_GAINS, g[:, 0]) + 1) % len(V_GAINS)], g[:, 1])
    return g


# ---- the model of a case -------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Model:
    """Everything the weighted reference needs.  ref: visibility's Ref (vis bool [BH | 1, G, Sk], r2g [Sq], R, comp; its v is not
    used)."""
    dt: str
    B: int
    H: int
    Hkv: int
    Sq: int
    Sk: int
    D: int                    # head dim of the call
    sm_scale: Optional[float]
    ref: vis.Ref
    n: np.ndarray             # int8 [Hkv, Sk, D]
    v: np.ndarray             # float32 [Hkv, Sk, D]
    qrows: int                # rows of a query block (one walk)
    key_block: int
    mask: Optional[np.ndarray] = None
    pieces: Optional[dict] = None        # (bh, query block) -> list of arrays of key blocks: the pieces of a split walk
    extra: dict = dataclasses.field(default_factory=dict)
    fp8: object = False       # False | True (e4m3 Q, K, V and P) | "pv" (2-byte Q . K^T, e4m3 P and V)

    @property
    def scale(self) -> float:
        return float(self.D) ** -0.5 if self.sm_scale is None else self.sm_scale

    @property
    def q_target(self):
        """(the scale find_a() is asked for, the value the scaled Q must round to).  The pv kernel multiplies Q by
        (float)(sm_scale * 1.44269504 * 8) before it rounds it to the 2-byte type (rsa_attn_fp8_kernel.hip, a.qk_scale), so Q
        rounds to 1 and a score arrives as 8 n, the code map's unit; the e4m3 image holds Q * (float)(sm_scale * 1.44269504), and
        the MFMA's scale operand carries the 8."""
        return (8.0 * self.scale, 1.0) if self.fp8 == "pv" else (self.scale, TARGET)

    @property
    def a(self) -> float:
        vals, _ = find_a(self.dt, *self.q_target)
        assert len(vals) >= 1, f"no value of {self.dt} gives round(a * qk_scale) == {self.q_target[1]} at sm_scale {self.scale}"
        return float(vals[0])

    def q(self) -> np.ndarray:
        """float32 [B, H, Sq, D]."""
        q = np.zeros((self.B, self.H, self.Sq, self.D), np.float32)
        r = np.arange(self.Sq)
        for h in range(self.H):
            q[:, h, r, cls(r, h, self.D)] = self.a
        return q

    def k(self) -> np.ndarray:
        """float32 [Hkv, Sk, D] (the same for every batch item)."""
        return (KSCALE * self.n.astype(np.int32)).astype(np.float32)

    def kvh(self, h: int) -> int:
        return h // (self.H // self.Hkv)

    def padded(self, what: str, head: int) -> np.ndarray:
        """n (int8) or v (float64) of one K/V head with the key axis padded to whole sub-steps, made once."""
        key = (what, head)
        if key not in self.extra:
            Skp = -(-self.Sk // SUB) * SUB
            self.extra[key] = _pad(self.n[head], 0, Skp) if what == "n" else _pad(self.v[head], 0, Skp).astype(np.float64)
        return self.extra[key]

    def n_blocks(self) -> int:
        return -(-self.Sq // self.qrows)

    def blocks(self, every: int = 1):
        """The query blocks (every: a sample for the CPU checks of the large cases, the last three always: the text rows)."""
        nb = self.n_blocks()
        return sorted(set(range(0, nb, every)) | set(range(max(nb - 3, 0), nb)))

    def heads(self, H=None) -> List[int]:
        """The (b, h) pairs as flat indices b * H + h, restricted to the first H heads, or to a list of heads (None: all)."""
        hs = range(self.H) if H is None else range(min(H, self.H)) if isinstance(H, int) else H
        return [b * self.H + h for b in range(self.B) for h in hs]


# ---- the fp8 forms: the operands as the kernels read them ------------------------------------------------------------------------
def fp8_images(m: Model) -> dict:
    """The block-scaled e4m3 images of the case's operands through the oracle's byte-exact contract (fp8_kmean, fp8_block_images),
    dequantised, made once: mu [Hkv, D] and kd [Hkv, Sk, D] = K - mu as the kernel multiplies it (e4m3 form; pv: K itself, mu = 0),
    vd [Hkv, Sk, D], qd [H, Sq, D] = the scaled Q (e4m3: the image of Q * qk_const, without the 8 the MFMA's scale operand adds; pv:
    Q * qk_scale rounded to the 2-byte type), the E8M0 exponents eq [H, .], ek, ev [Hkv, .] (minus 127) and qunit, the one
    non-zero value of a row of qd: 2^-3 (e4m3: the MFMA's scale operand adds the code map's 8) or 1 (pv: Q carries the 8), so that
    qd . kd / (8 qunit) is the score in binary units."""
    if "images" in m.extra:
        return m.extra["images"]
    from oracle import oracle as orc
    assert m.fp8 and m.Hkv == m.H
    pad = lambda x: -(-x // 128) * 128
    kvalid = m.extra["kvalid"]
    k, v, q = m.k(), m.v, m.q()[0]

    def deq(img, ex, rows):
        return (orc.dequantize_e4m3(img) * np.exp2(np.repeat(ex.astype(np.int64) - 127, 128))[:, None].astype(np.float32))[:rows]
    out = dict(mu=np.zeros((m.Hkv, m.D), np.float32), kd=[], vd=[], qd=[], ek=[], ev=[], eq=[])
    for hk in range(m.Hkv):
        img, ex = orc.fp8_block_images(v[hk], kvalid, pad(m.Sk), "v")
        out["vd"].append(deq(img, ex, m.Sk))
        out["ev"].append(ex.astype(np.int64) - 127)
        if m.fp8 is True:
            out["mu"][hk] = orc.fp8_kmean(k[hk], kvalid) if m.extra.get("smooth_k", True) else 0
            img, ex = orc.fp8_block_images(k[hk], kvalid, pad(m.Sk), "k", out["mu"][hk])
            out["kd"].append(deq(img, ex, m.Sk))
            out["ek"].append(ex.astype(np.int64) - 127)
            img, ex = orc.fp8_block_images(q[hk], m.Sq, pad(m.Sq), "q")
            out["qd"].append(deq(img, ex, m.Sq))
            out["eq"].append(ex.astype(np.int64) - 127)
        else:
            out["kd"].append(k[hk])
            out["qd"].append(round_dt(q[hk] * qk_scale(m.q_target[0]), m.dt))
    out = {key: np.stack(val) if isinstance(val, list) and len(val) else val for key, val in out.items()}
    out["qunit"] = TARGET if m.fp8 is True else 1.0
    m.extra["images"] = out
    return out


def seen_blocks(m: Model) -> np.ndarray:
    """bool [ceil(Sk / 128)]: the 128-key blocks that hold a key some row of the case sees."""
    groups = np.unique(m.ref.r2g[m.ref.r2g >= 0])
    keys = m.ref.vis[:, groups].any((0, 1))
    return _pad(keys, 0, -(-m.Sk // 128) * 128).reshape(-1, 128).any(1)


def fp8_image_faults(m: Model) -> List[str]:
    """What keeps the integer scores from being exact in the case's fp8 form (empty = nothing): the conditions of the module
    docstring, checked on the images."""
    im = fp8_images(m)
    bad = []
    kvalid = m.extra["kvalid"]
    if m.ref.vis[..., kvalid:].any():
        bad.append("a row sees a key the producer does not count")
    r = np.arange(m.Sq)
    for h in range(m.H):
        want = np.zeros((m.Sq, m.D), np.float32)
        want[r, cls(r, h, m.D)] = im["qunit"]
        if not np.array_equal(im["qd"][h], want):
            bad.append(f"head {h}: the scaled Q is not one-hot with the power of two {im['qunit']}")
    u = im["mu"].astype(np.float64) / KSCALE
    if not np.array_equal(u, np.round(u)):
        bad.append(f"mu / 8 is not integral: {u[u != np.round(u)][:4]}")
    # dequantised q . k: between any two keys of a channel it differs by exactly the difference of their n
    want_k = (KSCALE * (m.n[:, :kvalid].astype(np.float64) - u[:, None, :])).astype(np.float32)
    if not np.array_equal(im["kd"][:, :kvalid], want_k):
        bad.append("K - mu is not 8 (n - mu / 8) in the image")
    if not np.array_equal(im["vd"][:, :kvalid], m.v[:, :kvalid]):
        bad.append("V is not exact in its image")
    seen = seen_blocks(m)
    if seen.sum() == 1 and len(seen) > 1:          # (one row that sees one block: that block and its neighbour must differ)
        b = int(np.nonzero(seen)[0][0])
        seen[b + 1 if b + 1 < len(seen) else b - 1] = True
    for name in ("ev",) + (("ek",) if m.fp8 is True else ()):
        for hk in range(m.Hkv):
            if len(set(im[name][hk][:len(seen)][seen].tolist())) < 2:
                bad.append(f"K/V head {hk}: one {name[1].upper()} exponent in every block a row sees: {im[name][hk].tolist()}")
    if m.fp8 is True and len({int(e) for e in np.unique(im["eq"])}) != 1:
        bad.append(f"Q's exponent differs between blocks (the construction says it does not): {np.unique(im['eq']).tolist()}")
    return bad


def tile_walk(m: Model, t: "Terms"):
    """The walk of Terms t in the fp8 kernels' 64-key tiles, and the moves of their deferred reference (rsa_attn_fp8_kernel.hip, as
    oracle.attention_rows_pcode restates it): a row's reference starts at its first finite tile maximum and moves to the running
    maximum whenever some row of its wave (32 consecutive rows) sees a tile maximum more than THRESH above its own reference.
    -> (index of each sub-step's tile [S], num [T, R, D], den [T, R], J [T, R]: by how much the reference moves BEFORE tile t's
    P is formed, 0 at a row's first tile).  A split walk is walked as one (its pieces restart the reference; the mutants that use
    the moves are model mutants either way)."""
    tiles, idx = np.unique(t.subs // 2, return_inverse=True)
    T, R = len(tiles), len(t.rows)
    numT, denT, mxT = np.zeros((T, R, m.D)), np.zeros((T, R)), np.full((T, R), -np.inf)
    np.add.at(numT, idx, t.num)
    np.add.at(denT, idx, t.den)
    np.maximum.at(mxT, idx, t.mx)
    wave = (t.rows % 128) // 32
    thresh = pmap()[3]
    ref = np.full(R, -np.inf)
    J = np.zeros((T, R))
    with np.errstate(invalid="ignore"):
        for ti in range(T):
            grow = np.where(np.isneginf(ref), mxT[ti] > -np.inf, mxT[ti] > ref + thresh)
            gw = np.zeros(4, bool)
            np.logical_or.at(gw, wave, grow)
            new = np.where(gw[wave], np.maximum(ref, mxT[ti]), ref)
            J[ti] = np.where(np.isfinite(ref) & (new > ref), new - ref, 0.0)
            ref = new
    return idx, numT, denT, J


@dataclasses.dataclass
class Terms:
    """One query block's walk, sub-step by sub-step."""
    rows: np.ndarray          # [R] row indices
    subs: np.ndarray          # [S] indices of the 32-key sub-steps with a visible key
    W: np.ndarray             # float64 [R, S, 32]: 2^n of the visible keys, 0 of the others
    vs: np.ndarray            # float64 [S, 32, D]
    num: np.ndarray           # [S, R, D]
    den: np.ndarray           # [S, R]
    mx: np.ndarray            # [S, R] the largest visible n of the sub-step, -inf without one
    g: np.ndarray             # [R] the rows' groups (-1: written as 0)


def _pad(x: np.ndarray, axis: int, to: int) -> np.ndarray:
    if x.shape[axis] == to:
        return x
    pad = [(0, 0)] * x.ndim
    pad[axis] = (0, to - x.shape[axis])
    return np.pad(x, pad)


def terms(m: Model, bh: int, qb: int, classes=None, kn=None, kv=None, ref: Optional[vis.Ref] = None) -> Terms:
    ref = m.ref if ref is None else ref
    h = bh % m.H
    kvh = m.kvh(h)
    kn = kvh if kn is None else kn
    kv = kvh if kv is None else kv
    rows = np.arange(qb * m.qrows, min((qb + 1) * m.qrows, m.Sq))
    c = cls(rows, h, m.D) if classes is None else classes
    g = ref.r2g[rows]
    vbh = ref.vis[bh if ref.vis.shape[0] > 1 else 0]
    Skp = -(-m.Sk // SUB) * SUB
    visR = _pad(vbh[np.maximum(g, 0)] & (g >= 0)[:, None], 1, Skp)                 # [R, Skp]
    subs = np.unique(np.nonzero(visR.any(0))[0] // SUB)
    keys = subs[:, None] * SUB + np.arange(SUB)[None, :]                           # [S, 32]
    nn = m.padded("n", kn)[keys][:, :, c].astype(np.float64)                   # [S, 32, R]
    seen = visR[:, keys]                                                           # [R, S, 32]
    W = np.where(seen, np.exp2(nn).transpose(2, 0, 1), 0.0)
    vs = m.padded("v", kv)[keys]
    num = np.matmul(W.transpose(1, 0, 2), vs)
    den = W.sum(2).T
    mx = np.where(seen, nn.transpose(2, 0, 1), -np.inf).max(2, initial=-np.inf).T
    return Terms(rows, subs, W, vs, num, den, mx, g)


def finish(m: Model, bh: int, t: Terms, num: np.ndarray, den: np.ndarray, ref: Optional[vis.Ref] = None) -> np.ndarray:
    """[R, D] output rows from the whole walk's numerator [R, D] and denominator [R]."""
    ref = m.ref if ref is None else ref
    o = np.where(den[:, None] > 0, num / np.where(den > 0, den, 1.0)[:, None], 0.0)
    if ref.R is not None:
        gg = np.maximum(t.g, 0)
        o = ref.R[bh][gg][:, None] * o + ref.comp[bh][gg]
    return np.where((t.g >= 0)[:, None], o, 0.0)


def block_rows(m: Model, bh: int, qb: int, ref: Optional[vis.Ref] = None, **kw) -> np.ndarray:
    t = terms(m, bh, qb, ref=ref, **kw)
    return finish(m, bh, t, t.num.sum(0), t.den.sum(0), ref)


def reference(m: Model, H=None, ref: Optional[vis.Ref] = None, every: int = 1) -> np.ndarray:
    """float64 [B * H, Sq, D] (the heads not asked for stay 0)."""
    out = np.zeros((m.B * m.H, m.Sq, m.D))
    for bh in m.heads(H):
        for qb in m.blocks(every):
            out[bh, qb * m.qrows:(qb + 1) * m.qrows] = block_rows(m, bh, qb, ref)
    return out


def budget(m: Model, H=None, every: int = 1):
    """-> (the largest sum_j 2^(n_j - n_min) over a row's visible keys, the largest spread n_max - n_min of a row)."""
    worst, spread = 0.0, 0
    for bh in m.heads(H):
        for qb in m.blocks(every):
            t = terms(m, bh, qb)
            if not len(t.subs):
                continue
            has = t.den.sum(0) > 0
            if not has.any():
                continue
            lo = np.where(t.W > 0, np.log2(np.where(t.W > 0, t.W, 1.0)), np.inf).min((1, 2))
            hi = t.mx.max(0)
            worst = max(worst, float((t.den.sum(0)[has] / np.exp2(lo[has])).max()))
            spread = max(spread, int((hi[has] - lo[has]).max()))
    return worst, spread


def jumps(t: Terms) -> np.ndarray:
    """float64 [S, R]: by how much sub-step s raises the row's running maximum (0 for a row's first visible sub-step)."""
    if not len(t.subs):
        return np.zeros((0, len(t.rows)))
    run = np.maximum.accumulate(t.mx, 0)
    prev = np.vstack([np.full((1, t.mx.shape[1]), -np.inf), run[:-1]])
    with np.errstate(invalid="ignore"):
        J = np.where(np.isfinite(prev) & np.isfinite(t.mx), np.maximum(t.mx - prev, 0.0), 0.0)
    return J


def exercised(m: Model, H=None, every: int = 1) -> Dict[str, int]:
    """From the model: how many rows of the step and stairs classes move their reference by 9..12 / by 3..8 after their first
    sub-step, how many walks are split, and in how many of their rows the pieces' maxima differ by 3 .. 12."""
    out = dict(rows=0, step_rows_9_12=0, stairs_rows=0, edge_rows=0, merges=0, merged_rows_3_12=0)
    for bh in m.heads(H):
        h = bh % m.H
        for qb in m.blocks(every):
            t = terms(m, bh, qb)
            kinds = np.array([KINDS[c % 8] for c in cls(t.rows, h, m.D)])
            J = jumps(t)
            out["rows"] += int((t.den.sum(0) > 0).sum())
            if len(t.subs):
                out["step_rows_9_12"] += int(((kinds == "step") & (J.max(0) >= 9)).sum())
                out["stairs_rows"] += int(((kinds == "stairs") & ((J >= 3).sum(0) >= 2)).sum())
                out["edge_rows"] += int(((kinds == "edge") & (J.max(0) >= 8)).sum())
            if m.pieces and (bh, qb) in m.pieces and len(t.subs):
                out["merges"] += 1
                mi = np.array([t.mx[on].max(0) for blocks in m.pieces[bh, qb]
                               if (on := np.isin(t.subs * SUB // m.key_block, blocks)).any()])
                mi = np.where(np.isfinite(mi), mi, np.nan)
                d = np.where(np.isnan(mi).all(0), 0.0,
                             np.nan_to_num(mi, nan=-1e9).max(0) - np.nan_to_num(mi, nan=1e9).min(0))
                out["merged_rows_3_12"] += int(((d >= 3) & (d <= 12)).sum())
    return out


# ---- the sensitivity condition -------------------------------------------------------------------------------------------
PERMS = {"reversed": lambda t: SUB - 1 - t, "j^1": lambda t: t ^ 1, "j^4": lambda t: t ^ 4}


def insensitive(m: Model, H=None, vis_mutants=(), every: int = 1):
    """-> (the model mutants the bound would NOT notice, the exemptions counted by rule).  Every mutant must move some element of
    the query block it touches by SENSITIVITY tolerances:
      rows      a row uses the scores of row r + 1, r + 32 or r + 64 of its block (the shifts a block has rows for)
      channels  class c reads K channel c ^ 1, c ^ 8 or c + D / 2
      perms     for each 32-key sub-step of each walk, the weights inside it reversed, and swapped pairwise (j ^ 1, j ^ 4)
      jumps     at each sub-step where a step or stairs row moves its reference by >= 3, the keys before it too large by 2^jump
                in O only, in l only, in one 32-channel d-tile of O only, in one 32-row half only
      pieces    split walks: the pieces merged without their 2^(m_i - m)
      heads     GQA: query head h reads K, or V, of K/V head h // g +- 1
      limits    visibility's own mutants that let a row see a key beyond a limit (the spike just outside it), now with weights
    and in the fp8 forms (the walk in 64-key tiles, the reference deferred per wave of 32 rows: tile_walk())
      slots     for each 64-key tile of each walk, the k-slot of the V image (oracle.fp8_kslot_key) that holds the tile's heaviest key
                (the largest share of a row of the block) swapped with the slot of the same row's lightest key; and the whole tile
                stored in key order instead of k-slot order
      exponents each key block's V exponent, and in the e4m3 form its K exponent, replaced by the next block's
      moves     at each tile before which some row's deferred reference moves by >= 3: the rescale skips O, l or one 32-channel
                d-tile of O; the tile's own scores, computed a step ahead, are not shifted; every row rescales by the move of
                the row 32 further on or back (its neighbour wave's)
    Exempt: a sub-step without a key visible to the block (it is in no walk of the model), a rectified row with R = 0, a limit
    another limit hides, k-slots whose keys no row of the block sees, the key order in a tile of which the block sees fewer than 24 keys (keys
    0 .. 3 are their own k-slots, and the hashed heavy key of a focused sub-step is one of 8 .. 23), and a neighbouring block that has the same exponent.  Limit mutants that hide a key or move a row are not weights' to show (visibility's probes pin them): they
    are counted in the returned table under their own heading.
    """
    base = reference(m, H, every=every)
    tol = vis.tolerance(base, ULP[m.dt])
    missed: List[str] = []
    exempt = {"sub-step without a visible key": 0, "rectified row with R = 0": 0, "limit hidden by another limit": 0}
    if m.fp8:
        exempt.update({"swapped k-slots without a visible key": 0, "neighbouring block with the same exponent": 0,
                       "key order in a tile of which the block sees fewer than 24 keys": 0})
        from oracle import oracle as orc
        im = fp8_images(m)
    skipped = {"limit mutant that hides a key or moves a row (visibility's probes pin those)": 0}

    def moved(bh, t, out):
        sl = slice(t.rows[0], t.rows[-1] + 1)
        return bool((np.abs(out - base[bh, sl]) >= SENSITIVITY * tol[bh, sl]).any())

    for bh in m.heads(H):
        h = bh % m.H
        g = m.H // m.Hkv
        for qb in m.blocks(every):
            t = terms(m, bh, qb)
            where = f"bh {bh} block {qb}"
            if m.mask is not None and qb < m.mask.shape[2]:          # sub-steps of kept key blocks that hold no visible key
                mk = m.mask[bh // m.H if m.mask.shape[0] > 1 else 0, (h if m.mask.shape[1] == m.H else m.kvh(h))
                            if m.mask.shape[1] > 1 else 0, qb]
                walked = {s for kb in np.nonzero(mk)[0] for s in range(kb * m.key_block // SUB, (kb + 1) * m.key_block // SUB)}
                exempt["sub-step without a visible key"] += 3 * len(walked - set(t.subs.tolist()))
            if not len(t.subs):
                continue
            live = (t.g >= 0) & (t.den.sum(0) > 0)
            if m.ref.R is not None:
                dead = live & (m.ref.R[bh][np.maximum(t.g, 0)] == 0)
                live &= ~dead
                if dead.any() and not live.any():
                    exempt["rectified row with R = 0"] += int(dead.sum())
                    continue
            if not live.any():
                continue
            num, den = t.num.sum(0), t.den.sum(0)
            # rows and channels
            R = len(t.rows)
            c0 = cls(t.rows, h, m.D)
            for d in (1, 32, 64):
                if d < min(R, m.qrows):
                    c1 = cls(t.rows[0] + (t.rows - t.rows[0] + d) % R, h, m.D)
                    if not moved(bh, t, block_rows(m, bh, qb, classes=c1)):
                        missed.append(f"{where}: rows take the scores of row r + {d}")
            for name, c1 in (("c ^ 1", c0 ^ 1), ("c ^ 8", c0 ^ 8), ("c + D/2", (c0 + m.D // 2) % m.D)):
                if not moved(bh, t, block_rows(m, bh, qb, classes=c1)):
                    missed.append(f"{where}: classes read K channel {name}")
            # perms
            for si, s in enumerate(t.subs):
                for name, p in PERMS.items():
                    pi = p(np.arange(SUB))
                    dn = np.einsum("rt,td->rd", t.W[:, si], t.vs[si][pi] - t.vs[si])
                    if not moved(bh, t, finish(m, bh, t, num + dn, den)):
                        missed.append(f"{where}: weights of sub-step {int(s)} {name}")
            # jumps
            kinds = np.array([KINDS[c % 8] for c in c0])
            J = jumps(t)
            cn, cd = np.cumsum(t.num, 0), np.cumsum(t.den, 0)
            half_of = (t.rows % 64) // 32
            for si in range(1, len(t.subs)):
                if not (np.isin(kinds, STEP_KINDS) & (J[si] >= 3) & live).any():
                    continue
                f = np.exp2(J[si]) - 1.0
                bn, bd = cn[si - 1] * f[:, None], cd[si - 1] * f
                variants = [("in O only", num + bn, den), ("in l only", num, den + bd)]
                for dtile in range(m.D // 32):
                    sel = np.zeros(m.D, bool)
                    sel[32 * dtile:32 * dtile + 32] = True
                    variants.append((f"in d-tile {dtile} of O only", num + bn * sel, den))
                for x in (0, 1):
                    on = half_of == x
                    if (on & (J[si] > 0) & live).any():
                        variants.append((f"in 32-row half {x} only", num + bn * on[:, None], den + bd * on))
                for name, n1, d1 in variants:
                    if not moved(bh, t, finish(m, bh, t, n1, d1)):
                        missed.append(f"{where}: jump at sub-step {int(t.subs[si])}: the keys before it too large {name}")
            # pieces
            if m.pieces and (bh, qb) in m.pieces:
                n1, d1 = np.zeros_like(num), np.zeros_like(den)
                for blocks in m.pieces[bh, qb]:
                    on = np.isin(t.subs * SUB // m.key_block, blocks)
                    if not on.any():
                        continue
                    mi = t.mx[on].max(0)
                    w = np.where(np.isfinite(mi), np.exp2(-np.where(np.isfinite(mi), mi, 0.0)), 0.0)
                    n1 += t.num[on].sum(0) * w[:, None]
                    d1 += t.den[on].sum(0) * w
                if not moved(bh, t, finish(m, bh, t, n1, d1)):
                    missed.append(f"{where}: pieces merged without their 2^(m_i - m)")
            # heads
            if m.Hkv != m.H:
                for other in (m.kvh(h) - 1, m.kvh(h) + 1):
                    if 0 <= other < m.Hkv:
                        for what, kw in (("K", dict(kn=other)), ("V", dict(kv=other))):
                            if not moved(bh, t, block_rows(m, bh, qb, **kw)):
                                missed.append(f"{where}: head {h} reads {what} of K/V head {other}")
            if m.fp8:
                missed += [f"{where}: {x}" for x in _fp8_insensitive(m, bh, t, num, den, live, im, exempt, orc,
                                                                      lambda out, bh=bh, t=t: moved(bh, t, out))]
    # limits
    for name, mref in vis_mutants:
        if np.array_equal(mref.r2g, m.ref.r2g) and np.array_equal(mref.vis, m.ref.vis):
            exempt["limit hidden by another limit"] += 1
            continue
        if (m.ref.vis & ~mref.vis).any() or not np.array_equal(mref.r2g, m.ref.r2g):
            skipped[next(iter(skipped))] += 1
            continue
        if not (np.abs(reference(m, H, mref, every) - base) >= SENSITIVITY * tol).any():
            missed.append(f"limit: {name}")
    return missed, dict(exempt, **skipped)


def _fp8_insensitive(m: Model, bh: int, t: Terms, num, den, live, im, exempt, orc, moved) -> List[str]:
    """The fp8 forms' own model mutants of one walk (insensitive() has the list)."""
    out = []
    kvh = m.kvh(bh % m.H)
    idx, numT, denT, J = tile_walk(m, t)
    # slots
    vp = _pad(m.padded("v", kvh), 0, -(-m.Sk // vis.TILE) * vis.TILE)
    at = {int(s): i for i, s in enumerate(t.subs)}

    def weight(key):
        return t.W[:, at[key // SUB], key % SUB] if key // SUB in at else np.zeros(len(t.rows))
    slot_key = orc.fp8_kslot_key(np.arange(vis.TILE))
    slot_of = np.argsort(slot_key)
    share = t.W / np.where(live & (den > 0), den, np.inf)[:, None, None]
    for tile in np.unique(t.subs // 2):
        key0 = int(tile) * vis.TILE
        wt = np.stack([weight(key0 + x) for x in range(vis.TILE)], 1)                        # [R, 64]
        sh = np.stack([share[:, at[s_]] if s_ in at else np.zeros((len(t.rows), SUB)) for s_ in (2 * int(tile), 2 * int(tile) + 1)], 1)
        if not (sh > 0).any():
            exempt["swapped k-slots without a visible key"] += 2
            continue
        # (a) two slots: the tile's heaviest key (the largest share of a row of the block: where a weight on the wrong key shows) and
        #     the lightest key of the same row, an invisible one (weight 0) where the row sees only a part of the tile
        r1, k1 = np.unravel_index(np.argmax(sh.reshape(len(t.rows), -1)), (len(t.rows), vis.TILE))
        k2 = int(np.argmin(np.where(np.arange(vis.TILE) % SUB == k1 % SUB, np.inf, wt[r1])))       # (not its twin in the other sub-step)
        dn = (wt[:, k1] - wt[:, k2])[:, None] * (vp[key0 + k2] - vp[key0 + k1])[None, :]
        if not moved(finish(m, bh, t, num + dn, den)):
            out.append(f"k-slots {int(slot_of[k1])} and {int(slot_of[k2])} of the V tile {int(tile)} swapped")
        # (b) the tile stored in key order: slot p, which the MFMA takes for key fp8_kslot_key(p), holds key p
        dn = wt[:, slot_key] @ vp[key0:key0 + vis.TILE] - wt @ vp[key0:key0 + vis.TILE]
        if (wt > 0).any(0).sum() < 24:       # (keys 0 .. 3 are their own slots, and the hashed heavy key of a sub-step is one of 8 .. 23)
            exempt["key order in a tile of which the block sees fewer than 24 keys"] += 1
        elif not moved(finish(m, bh, t, num + dn, den)):
            out.append(f"the V tile {int(tile)} stored in key order, not in k-slot order")
    # exponents
    blocks = t.subs * SUB // 128
    nblk = -(-m.Sk // 128)
    for kb in np.unique(blocks):
        on = blocks == kb
        nb = int(kb) + 1 if kb + 1 < nblk else int(kb) - 1
        if nb < 0:
            continue
        d = int(m.extra["gains"][kvh, nb] - m.extra["gains"][kvh, kb])
        if d == 0:
            exempt["neighbouring block with the same exponent"] += 1
        elif not moved(finish(m, bh, t, num + t.num[on].sum(0) * (2.0 ** d - 1.0), den)):
            out.append(f"key block {int(kb)} takes the V exponent of block {nb}")
        if m.fp8 is True:
            d = int(im["ek"][kvh, nb] - im["ek"][kvh, kb])
            if d == 0:
                exempt["neighbouring block with the same exponent"] += 1
                continue
            u = (im["mu"][kvh].astype(np.float64) / KSCALE)[cls(t.rows, bh % m.H, m.D)][:, None, None]
            W0 = t.W[:, on]
            W1 = np.where(W0 > 0, np.exp2((np.log2(np.where(W0 > 0, W0, 1.0)) - u) * 2.0 ** d + u), 0.0)
            n1 = num + np.einsum("rst,std->rd", W1 - W0, t.vs[on])
            if not moved(finish(m, bh, t, n1, den + (W1 - W0).sum((1, 2)))):
                out.append(f"key block {int(kb)} takes the K exponent of block {nb}")
    # moves of the deferred reference
    cn, cd = np.cumsum(numT, 0), np.cumsum(denT, 0)
    pos = t.rows - t.rows[0]
    nbr = np.where((pos ^ 32) < len(pos), pos ^ 32, -1)
    for ti in range(1, len(J)):
        if not ((J[ti] >= 3) & live).any():
            continue
        f = np.exp2(J[ti]) - 1.0
        bn, bd = cn[ti - 1] * f[:, None], cd[ti - 1] * f
        variants = [("the rescale skips O", num + bn, den), ("the rescale skips l", num, den + bd),
                    ("the scores computed ahead are not shifted", num + numT[ti] * f[:, None], den + denT[ti] * f)]
        for dtile in range(m.D // 32):
            sel = np.zeros(m.D, bool)
            sel[32 * dtile:32 * dtile + 32] = True
            variants.append((f"the rescale skips d-tile {dtile} of O", num + bn * sel, den))
        Jn = np.where(nbr >= 0, J[ti][np.maximum(nbr, 0)], 0.0)
        if ((J[ti] != Jn) & live & (cd[ti - 1] > 0)).any():
            fw = np.exp2(J[ti] - Jn) - 1.0
            variants.append(("the waves rescale by their neighbour wave's move", num + cn[ti - 1] * fw[:, None], den + cd[ti - 1] * fw))
        for name, n1, d1 in variants:
            if not moved(finish(m, bh, t, n1, d1)):
                out.append(f"reference move at tile {ti} of the walk: {name}")
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------
def _plain_cases() -> List[dict]:
    cases = []
    for dt in ("bf16", "fp16"):
        for D, blk in ((128, 128), (64, 128), (128, 64), (64, 64), (32, 128)):
            Sk = 5 * blk + 17
            pairs = [(Sk, 2 * blk + 37), (63, Sk - 1)] if D != 32 else [(Sk, 2 * blk + 37), (65, Sk - 1)]
            for kv in pairs:
                cases.append(dict(id=f"plain-{dt}-D{D}-b{blk}-kv{kv[0]}_{kv[1]}", family="plain", dt=dt, D=D, blk=blk, B=2, H=2,
                                  Sq=300, Sk=Sk, kv_len=kv, NK=-(-Sk // blk), mask="kinds"))
    # one explicit sm_scale for which qk_scale is exactly 1/8 (a = 1), and one call on [B, S, H, D] views
    cases.append(dict(id="plain-bf16-D128-b128-sm_scale", family="plain", dt="bf16", D=128, blk=128, B=2, H=2, Sq=300, Sk=657,
                      kv_len=(657, 293), NK=6, mask="kinds", sm_scale=TARGET / LOG2E))
    cases.append(dict(id="plain-bf16-D128-b128-bshd", family="plain", dt="bf16", D=128, blk=128, B=2, H=2, Sq=300, Sk=657,
                      kv_len=(657, 293), NK=6, mask="kinds", bshd=True))
    for dt in ("bf16", "fp16"):
        cases.append(dict(vis.CASES[f"plain-{dt}-tail"], id=f"plain-{dt}-tail"))
    return cases


def _dense_cases() -> List[dict]:
    cases = []
    for dt in ("bf16", "fp16"):
        for D in (128, 64):
            for Sq, Sk in ((300, 520), (257, 257), (700, 1100)):
                qs, ks = vis.dense_splits(Sq, Sk)[1]
                for name, q_split, kv_split, causal in (("whole", None, None, False), ("causal", None, None, True),
                                                        (f"q{qs}_kv{ks}", qs, ks, False), (f"q{qs}_kv{ks}-causal", qs, ks, True)):
                    cases.append(dict(id=f"dense-{dt}-D{D}-{Sq}x{Sk}-{name}", family="dense", dt=dt, D=D, B=2, H=2, Sq=Sq, Sk=Sk,
                                      q_split=q_split, kv_split=kv_split, causal=causal))
    return cases


RANGED = {"causal": dict(causal=True), "causal_kinds": dict(causal=True), "window_100_0": dict(window=(100, 0)),
          "window_37_20": dict(window=(37, 20)), "chunk_96": dict(chunk=96)}


def _ranged_cases() -> List[dict]:
    return [dict(id=f"ranged-{dt}-D{D}-{kind}", family="ranged", dt=dt, D=D, blk=128, B=2, H=2, Sq=300, Sk=657, kind=kind)
            for dt in ("bf16", "fp16") for D in (128, 64) for kind in RANGED]


def _gqa_cases() -> List[dict]:
    cases = []
    for dt in ("bf16", "fp16"):
        for H, Hkv, axis in ((4, 2, "Hkv"), (4, 2, "H"), (6, 2, "Hkv")):
            cases.append(dict(id=f"gqa-{dt}-H{H}-Hkv{Hkv}-mask{axis}", family="gqa", dt=dt, D=128, blk=128, B=2, H=H, Hkv=Hkv, Sq=300,
                              Sk=657, axis=axis, kv_len=(657, 293)))
    cases.append(dict(id="gqa-bf16-H4-Hkv2-fused", family="gqa", dt="bf16", D=64, blk=128, B=2, H=4, Hkv=2, Sq=657, Sk=657, axis="Hkv",
                      kv_len=(657, 657), fused=True))
    return cases


def _rect_cases() -> List[dict]:
    return [c for c in vis.RECT_CASES if not c["fp8"]]


def _rect_fp8_cases() -> List[dict]:
    """visibility's rectified cases of the e4m3 and pv forms (128-token blocks: the fp8 K5 is built for no other): the four
    layouts at head dims 128 and 64, the text split (hunyuan_tsplit) in both forms, the tail split on and off (hunyuan_tail, e4m3).
    Every one runs with "smooth K" on (tuning key fp8_smooth_k = 1, the product's setting): balance_mu() found a balance in each."""
    return [c for c in vis.RECT_CASES if c["fp8"]]


def _dense_fp8_cases() -> List[dict]:
    """Every shape of visibility.DENSE_SHAPES at both head dims in both forms, with the four settings of _dense_cases()."""
    cases = []
    for fp8, form in ((True, "e4m3"), ("pv", "pv")):
        for D in (128, 64):
            for Sq, Sk in vis.DENSE_SHAPES:
                qs, ks = vis.dense_splits(Sq, Sk)[1]
                for name, q_split, kv_split, causal in (("whole", None, None, False), ("causal", None, None, True),
                                                        (f"q{qs}_kv{ks}", qs, ks, False), (f"q{qs}_kv{ks}-causal", qs, ks, True)):
                    cases.append(dict(id=f"dense-{form}-D{D}-{Sq}x{Sk}-{name}", family="dense", dt="bf16", fp8=fp8, D=D, B=2, H=2,
                                      Sq=Sq, Sk=Sk, q_split=q_split, kv_split=kv_split, causal=causal))
    return cases


PLAIN_CASES = _plain_cases()
DENSE_CASES = _dense_cases()
RANGED_CASES = _ranged_cases()
GQA_CASES = _gqa_cases()
RECT_CASES = _rect_cases()
RECT_FP8_CASES = _rect_fp8_cases()
DENSE_FP8_CASES = _dense_fp8_cases()
FP8_CASES = RECT_FP8_CASES + DENSE_FP8_CASES
_ALL_CASES = PLAIN_CASES + DENSE_CASES + RANGED_CASES + GQA_CASES + RECT_CASES + FP8_CASES
CASES: Dict[str, dict] = {c["id"]: c for c in _ALL_CASES}
assert len(CASES) == len(_ALL_CASES)


def _tail_pieces(mask: np.ndarray, H: int, NBp: int, valid_blocks: int) -> dict:
    """The tail split (rsa_attn.h::rsa_walk_map, as tests/test_gpu_ranged.py restates it) of a launch of H x NBp walks, B = 1: the
    first 512 fill one generation, the others are split 4 ways, each piece ceil(len / 4) entries of the kept list (of its
    blocks that hold a valid key).  Plain tail case: 9 x 64 = 576 walks, the last 64 every query block of the last head.
    Rectified tail case: 6 x 104 = 624 walks, the last 112 of which the visual ones are modelled here (the text rows' walk is
    the text split's)."""
    NQ = mask.shape[2]
    out = {}
    first, P = 512, 4
    for vv in range(first, H * NBp):
        h, jj = divmod(vv, NBp)
        qb = (jj & 7) * (NBp // 8) + (jj >> 3)
        if qb >= NQ:
            continue
        cols = np.nonzero(mask[0, h, qb])[0]
        cols = cols[cols < valid_blocks]
        per = -(-len(cols) // P)
        out[h, qb] = [cols[p * per:(p + 1) * per] for p in range(P) if len(cols[p * per:(p + 1) * per])]
    return out


def _text_pieces(sp, BH: int) -> Optional[dict]:
    """The text split of the rectified call (rsa_attn.hip, rsa_attn.h::rsa_walk_text): from 32 key blocks of valid text keys on,
    the walk of a text query block is cut into n // 16 pieces (at most 16) of ceil(n / pieces) key blocks each."""
    n = -(-sp.kv_text_valid // sp.block)
    if sp.q_text_valid <= 0 or n < 32:
        return None
    split = min(n // 16, 16)
    per = -(-n // split)
    cut = [np.arange(p * per, min((p + 1) * per, n)) for p in range(split) if p * per < n]
    last = (sp.NBv * sp.block + sp.q_text_valid - 1) // sp.block
    return {(bh, qb): cut for bh in range(BH) for qb in range(sp.NBv, last + 1)}


def ranged_limits(c: dict):
    """-> (keywords of the call without tensors, lo | None, hi) with lo / hi int64 [1, Sq]; the chunk's hi goes in as row_range."""
    import test_ranged_cpu as rule
    Sq, Sk = c["Sq"], c["Sk"]
    kw = RANGED[c["kind"]]
    if "chunk" in kw:
        r = np.arange(Sq, dtype=np.int64)
        return kw, None, ((r // kw["chunk"] + 1) * kw["chunk"])[None, :]
    left, right = (-1, 0) if kw.get("causal") else kw["window"]
    lo, hi = rule.window_ranges(Sq, [Sk], left, right)
    return kw, (None if left < 0 else lo), hi


LONG_WALK = 13          # focused sub-steps a forced class may hold: one heavy key each, so each keeps >= 1/14 of the row's weight


def forced_classes(ref: vis.Ref, B: int, H: int, Sq: int, Sk: int, qrows: int, D: int) -> dict:
    """{h: {c: (residue, period)}}: the classes that the shapes force into focus classes (MHA cases only: K/V head = head).
    The ordinary focus classes show every sub-step of a walk to any 16 consecutive rows, as long as the walk has at most
    4 * LONG_WALK sub-steps to share a row's weight among.  Two kinds of query block fall outside that, and there the classes of some
    of the block's own rows are made focus classes with one heavy key per focused sub-step:
      a block of fewer than 16 live rows (the one-row last block at Sq = 257, a short text block): period min(4, rows), the
        residues dealt out over its rows;
      a walk of more than 4 * LONG_WALK sub-steps (an all-kept row or the text rows of a long layout): period
        ceil(sub-steps / LONG_WALK), the residues dealt out over the block's rows of kind flat, fall, edge or spike."""
    out = {h: {} for h in range(H)}
    nb = -(-Sq // qrows)
    plain_kinds = [KINDS.index(k) for k in ("flat", "fall", "edge", "spike")]
    for h in range(H):
        blocks = []
        for b in range(B):
            vbh = ref.vis[(b * H + h) if ref.vis.shape[0] > 1 else 0]
            for qb in range(nb):
                rows = np.arange(qb * qrows, min((qb + 1) * qrows, Sq))
                g = ref.r2g[rows]
                ug = np.unique(g[g >= 0])
                if not len(ug):
                    continue
                seen = vbh[ug]
                live = rows[(g >= 0) & seen.any(1)[np.searchsorted(ug, np.maximum(g, ug[0]))]]
                T = len(np.unique(np.nonzero(seen.any(0))[0] // SUB))
                if len(live) and (len(live) < 16 or T > 4 * LONG_WALK):
                    blocks.append((len(live), T, live))
        for nlive, T, live in sorted(blocks, key=lambda x: x[0]):
            short = nlive < 16
            per = min(FOCUS_EVERY, nlive) if short and T <= 4 * LONG_WALK else max(FOCUS_EVERY, -(-T // LONG_WALK))
            cc = cls(live, h, D)
            have = {rr for x in cc if x in out[h] and out[h][x][1] == per for rr in [out[h][x][0]]}
            cand = [x for x in cc if x not in out[h] and (short or (x % 8) in plain_kinds)]
            for rr in (r_ for r_ in range(per) if r_ not in have):
                if not cand:
                    break
                out[h][int(cand.pop(0))] = (rr, per)
    return {h: t for h, t in out.items() if t}


def model(c: dict, parts=None) -> Model:
    """The case's inputs and reference.  parts: (R, comp) of a rectified call (None: visibility's model of them)."""
    fam, dt, D = c["family"], c["dt"], c["D"]
    B, H = c["B"], c["H"]
    Hkv = c.get("Hkv", H)
    fp8 = form_of(c)
    kvalid = None             # the rows of K and V the fp8 producer counts
    pieces = None
    mask = None
    outside, outside_keys = [], []
    if fam == "plain":
        ref, mask = vis.plain_ref(c)
        Sq, Sk, qrows, kb = c["Sq"], c["Sk"], c["blk"], c["blk"]
        outside_keys = list(c["kv_len"]) + [c["NK"] * c["blk"]]
        if c["mask"] == "tail":
            pieces = _tail_pieces(mask, H, mask.shape[2], -(-c["kv_len"][0] // c["blk"]))       # B = 1: bh = h
    elif fam == "dense":
        ref = vis.dense_ref(c)
        Sq, Sk, qrows, kb = c["Sq"], c["Sk"], 128, 128
        if c["causal"]:
            qs = Sq if c["q_split"] is None else c["q_split"]
            ks = Sk if c["kv_split"] is None else c["kv_split"]
            outside = [(ks - qs + 1, 1)] + ([(Sk - Sq + 1, 1)] if qs < Sq and ks - qs != Sk - Sq else [])     # (per segment)
            outside = [(o, sd) for o, sd in outside if o < Sk and o + Sq > 0]       # (a diagonal that leaves the keys has no key outside it)
        if c["kv_split"] is not None:          # (the key before the split is outside a limit only where the second segment has rows)
            outside_keys = [c["kv_split"]] + ([c["kv_split"] - 1] if c["q_split"] < Sq else [])
        kvalid = Sk
    elif fam in ("ranged", "gqa"):
        import test_ranged_cpu as rule
        Sq, Sk, qrows, kb = c["Sq"], c["Sk"], 128, 128
        NQ, NK = -(-Sq // 128), -(-Sk // 128)
        if fam == "ranged":
            lens = [Sk] * B
            mask = (np.ones((B, H, NQ, NK), bool) if c["kind"] != "causal_kinds" else vis.plain_mask(B, H, NQ, NK, 128, [Sk, 293]))
            kw, lo, hi = ranged_limits(c)
            if "chunk" in kw:
                outside_keys = sorted(set(hi[0].tolist()))
            else:
                left, right = (-1, 0) if kw.get("causal") else kw["window"]
                outside = [(Sk - Sq + right + 1, 1)] + ([(Sk - Sq - left - 1, -1)] if left >= 0 else [])
            seen = rule.visible(mask, lo, hi, lens, Sq, Sk)
        else:
            lens = list(c["kv_len"])
            mask = vis.plain_mask(B, {"H": H, "Hkv": Hkv}[c["axis"]], NQ, NK, 128, lens)
            seen = rule.visible(np.repeat(mask, H // mask.shape[1], axis=1), None, np.full((1, Sq), Sk), lens, Sq, Sk)
            outside_keys = lens
        ref = vis.Ref(seen.reshape(B * H, Sq, Sk), np.arange(Sq), None)
    else:
        sp = vis.spec_numbers(vis.rect_spec(c))
        R, comp = parts if parts is not None else (None, None)
        ref, mask = vis.rect_ref(c, sp, None, R, comp)
        Sq = Sk = sp.S
        qrows = kb = c["blk"]
        kvalid = sp.pool_valid
        outside_keys = [sp.kv_valid, sp.kv_text_valid]
        pieces = _text_pieces(sp, B * H)
        if c.get("tail_split"):
            pieces = {**(pieces or {}), **_tail_pieces(mask, H, sp.NB_total, -(-sp.kv_valid // sp.block))}
    assert not fp8 or (kvalid is not None and Hkv == H and kb == 128 and "sm_scale" not in c), "the fp8 forms: MHA, 128-token blocks"
    v = witness_v(Hkv, Sk, D)
    gains = None
    if fp8:
        gains = v_gains(Hkv, Sk)
        v = v * np.exp2(np.repeat(gains, 128, axis=1)[:, :Sk, None]).astype(np.float32)
    if fam == "rect" and parts is None:    # visibility's model of R and comp, on THIS V (head 0's) and no pooled-score model: R as there
        R, comp = vis.rect_model_parts(sp, mask, v[0])
        ref.R[:, :sp.NBv], ref.comp[:, :sp.NBv] = R, comp
    forced = forced_classes(ref, B, H, Sq, Sk, qrows, D) if Hkv == H else None
    n = scores_n(dt, Hkv, Sk, D, kb, tuple(outside), tuple(outside_keys), H // Hkv, forced, fp8, kvalid)
    return Model(dt, B, H, Hkv, Sq, Sk, D, c.get("sm_scale"), ref, n, v, qrows, kb, mask, pieces,
                 dict(outside=tuple(outside), outside_keys=tuple(outside_keys), kvalid=kvalid, gains=gains), fp8)


def misplaced_outside_keys(m: Model) -> List[str]:
    """The spike keys 'just outside a limit' that are not (empty = all in place): an offset o for which no row has the key r + o
    invisible and its neighbour on the inner side visible -- and, where every row has the same limits (one offset per side), a
    row that sees r + o at all --, a fixed key that no row has invisible right beside a visible one."""
    v = m.ref.vis
    g = np.maximum(m.ref.r2g, 0)
    has = m.ref.r2g >= 0
    r = np.arange(m.Sq)
    bad = []
    for o, side in m.extra["outside"]:
        k, inner = r + o, r + o - side
        ok = has & (k >= 0) & (k < m.Sk) & (inner >= 0) & (inner < m.Sk)
        if not (~v[:, g[ok], k[ok]] & v[:, g[ok], inner[ok]]).any():
            bad.append(f"offset {o}: no row has the key r + {o} invisible beside a visible one")
        if len({sd for _, sd in m.extra["outside"]}) == len(m.extra["outside"]) and v[:, g[ok], k[ok]].any():
            bad.append(f"offset {o}: some row sees the key r + {o}")
    for k in m.extra["outside_keys"]:
        if 0 < k < m.Sk - 1 and not (~v[..., k] & (v[..., k - 1] | v[..., k + 1])).any():
            bad.append(f"key {k}: no row has it invisible beside a visible key")
    return bad


def limit_mutants(c: dict):
    """visibility's mutants of the case's limits as (name, Ref) pairs (plain and dense cases)."""
    if c["family"] == "plain":
        return [(name, vis.plain_ref(c, **mu)[0]) for name, mu in vis.plain_mutants(c, c["H"])]
    if c["family"] == "dense":
        return [(name, vis.dense_ref(c, **mu)) for name, mu in vis.dense_mutants(c)]
    return []
