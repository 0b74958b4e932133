#!/usr/bin/env python3
"""Generator of the 64-rows-per-wave form of K5's main loop (rsa_attn_block64.h): RSA_K5W_* = head dim 128, RSA_K5V_* = head dim 64.

The text below describes head dim 128.  Head dim 64 (round 6) is the same streams on 8 + 8 MFMAs per 32-key sub-step; everything
that differs is a field of HeadDim, one immutable object per head dim, which every function here takes as its first argument.

One wave owns 64 query rows (two 32-row halves h = 0, 1) and the WHOLE register file of its SIMD (one wave per SIMD, 512
registers): every K fragment and every V^T fragment read from LDS feeds TWO MFMAs (one per row half), so the LDS operand
reads per MFMA halve against the 32-row form (24 reads per 32 MFMAs instead of per 16).  One block = one 32-key sub-step u:

    S_nxt[h]^T = K(u+1) . Q[h]^T - m[h]               16 MFMAs   ks = 0..7, h = 0, 1  (A = K rows by ds_read_b128, B = Q[h]
                                                                from the ACCUMULATOR file, C of the first = the -m block)
    P[h]       = exp2(S_cur[h])                       in place, fp32; row sums; packed to the 2-byte type
    O[h]^T    += V(u)^T . P[h]^T                      16 MFMAs   (k2, dt) = 8 V^T fragments x h (A = V^T by ds_read_b64_tr_b16,
                                                                B = packed P[h], C = D = O[h][dt] in the ACCUMULATOR file)
    mx[h]      = row max of S_nxt[h]

Register map.  Accumulator file (owned by the asm statements, never seen by the compiler as values: a "+a" operand makes
hipcc keep the tile in arch VGPRs and copy 128 registers in and out around every statement):
    O[h][dt]  a[16*(4h+dt) : +15]   (a0..a127)         Q[h][ks]  a[128 + 4*(8h+ks) : +3]   (a128..a191)
Arch VGPRs, pinned through physical-register constraints:
    SA[h] v[16h : +15]   SB[h] v[32+16h : +15]   -m[h] v[64+16h : +15]   P[h] v[96+8h : +7]   K ring v[112:127]   V ring v[128:143]
    scratch v144..v149   K read addresses v[152:159]   V read addresses v[160:167]   DMA lane offsets v[168:171] (K), v[172:175] (V)

LDS: K and V each live in a ring of FOUR 32-key half-tiles (8 KiB, image and swizzle of rsa_attn_kernel.hip); half-tile x
sits in slot x & 3, so the slot is a compile-time constant of block U = u & 3.  Block u reads K(u+1) and V(u) and stages
V(u+3) into V(u-1)'s slot and K(u+4) into K(u)'s slot: every LDS-DMA piece (global_load_lds_dwordx4, 1 KiB) has two to three
sub-steps to land, and the wait in front of block u is the constant vmcnt(16) (the 8 + 8 pieces of blocks u-2, u-1 may fly).

Schedule inside a block: the vector work is dealt into the 32 MFMA gaps by issue cost (cdna_hip_programming.md: <= 5
single-issue instructions per v_mfma_f32_32x32x16 gap, costs summing to <= 24 cycles hide) in deadline order: exponentials +
packing of the first 16 keys (needed by PV MFMA 16), of the second 16 keys (MFMA 24), row sums, then the two row maxima
interleaved with each other.  The wave's 8 DMA pieces (4 of K, 4 of V) take every fourth gap: they reach the CU's texture
addresser spread over the sub-step instead of as a burst behind the barrier (the 32-row kernel's staging point costs each wave
~450 cycles for 4 pieces: 8 waves x 4 pieces queue at one addresser, profiles/r03_k5_block.md; four pieces back to back cost
this wave ~25 cycles each, one per four MFMAs ~2 when the lines are in the CU's own cache: tools/probes/dma_issue_probe2.hip --
what a piece costs beyond that is the memory system pushing back, not the instruction).  The source bases WALK in scalar
registers -- a half-tile is 32 consecutive keys, a kept block 128 -- one step per block, re-based once per kept block, all of it
inside MFMA gaps (a scalar instruction beside an MFMA is free, between two blocks it is not); the rows of piece j come from
lane-offset register j, the LDS destination from M0 + instruction offset.  Block alone (no staging, no boundary): 1 131 .. 1 163
cycles per 32 MFMAs (round 4's block probe), in the loop with its staging ~1 330.

Two products:
  * RSA_K5W_LOOP_*: the steady-state loop as ONE asm statement: per kept 128-key block four blocks (U = 0..3), each behind
    `s_waitcnt vmcnt(16)` + `s_barrier`; list entry of the block after next read from LDS in the shadow, scalar re-basing of
    the DMA walkers, the deferred-rescale test after every block with the rescale itself out of line.  With one wave per SIMD
    nothing overlaps the instructions BETWEEN blocks (the first form of this kernel spent ~300 cycles per sub-step in hipcc's
    glue: stamps in profiles/r04_k5_w64.md), so the steady state contains none.  The loop's blocks put the row maxima ahead of
    the row sums, so the deferred-rescale test's two compares ride inside the block and only `s_or_b64` + the branch sit between
    two blocks (profiles/r06_k5_forms.txt form 23: byte-identical outputs, -0.4 % R2 / -3 % dense).  bf16 adds a second body
    without row maxima and test (the static reference, gen_loop); the 256-row dense form drops every second LDS-DMA piece.
  * RSA_K5W_BLOCK_*_U{0..3}: the same block without DMA as a statement of its own, for the sub-steps the loop does not take
    (boundary blocks: masked scores, clamped rows -- staged from C++), plus the rare-path helpers (mask, row maxima, rescale)
    and the accumulator-file housekeeping.  One statement per U: alternative statements that define the same pinned tiles make
    hipcc copy the tiles around every one of them.

The output depends on nothing but this file and the generators' shared core, k5gen.py.

usage: python3 gen_k5_block64.py > rsa_attn_block64.h        (python3 gen_k5_block64.py stats: per-gap issue costs)
"""
import sys
from dataclasses import dataclass
from types import MappingProxyType

from k5gen import CVT_PK, MFMA16, Stream, ar, clobbers, lds_dma, macro, ops_macro, pin, row_max, sr, vr

AHEAD = 4
# issue cycles of the 64-row kernel's vector work and of what rides in its gaps (the 32-row kernels' table differs)
COST64 = dict(exp=8, cvt=5, add=4, max=4, mov=4, swap=4, lds=4, wait=1, dma=24)   # (dma: the piece keeps its gap to itself at head dim 128;
                                                                                 # pricing it at 4 changes nothing measurable: r06_k5_forms.txt form 7)


@dataclass(frozen=True)
class HeadDim:
    """What depends on the head dim.  Head dim 64 (round 6): 8 + 8 MFMAs per 32-key sub-step against the same softmax; a half-tile is
    4 KiB = 4 LDS-DMA pieces (2 per wave), so the loop issues 2 + 2 pieces per sub-step."""
    D: int
    PFX: str                  # macro prefix: K5W = head dim 128, K5V = head dim 64
    DMA_GAPS: tuple           # the gaps that carry the wave's LDS-DMA pieces
    SALU_AT: MappingProxyType  # gaps of the loop's scalar bookkeeping (gen_loop)
    VMC: int                  # LDS-DMA pieces of the last two sub-steps that may still fly at a sub-step boundary
    GAPC: int                 # issue cycles of vector work dealt into one MFMA gap (head dim 64: 36 -- 16 MFMAs per sub-step cannot hide
                              # the softmax of 64 x 32 scores, the stream is paced by the vector port there)
    NEXP: int                 # exponentials per MFMA gap while there are any
    KS = property(lambda c: c.D // 16)
    DT = property(lambda c: c.D // 32)
    HALF = property(lambda c: 32 * c.D * 2)              # bytes of a 32-key half-tile
    VRING = property(lambda c: 4 * c.HALF)               # LDS offset of the V ring
    NQK = property(lambda c: 2 * c.KS)                   # MFMAs of a block: scores,
    NPV = property(lambda c: 4 * c.DT)                   # P . V,
    NMF = property(lambda c: c.NQK + c.NPV)              # all


HEAD_DIMS = (HeadDim(128, "K5W", tuple(4 * j + 1 for j in range(8)),       # every fourth gap
                     MappingProxyType(dict(k=22, k3=(22, 23, 24), v=30, h1=(2, 3))), VMC=16, GAPC=24, NEXP=2),
             HeadDim(64, "K5V", (1, 3, 9, 11),                             # K0 K1 | V0 V1: the wave's 2 + 2 pieces of the sub-step
                     MappingProxyType(dict(k=4, k3=(4, 5, 6), v=12, h1=(2, 3))), VMC=8, GAPC=36, NEXP=4))

# ---- register map ----
SA = [0, 16]
SB = [32, 48]
NM = [64, 80]
P = [96, 104]
KF, VF = 112, 128
PS = [144, 145]
T = [146, 147, 148, 149]
TH, MX = [T[0:2], T[2:4]], ["%[mx0]", "%[mx1]"]      # per row half: the row maximum's temporaries, its result
TMP0, TMP1 = 96, 150          # clobbered temporaries [TMP0, TMP1)
KA, VA = 152, 160
VOK, VOV = 168, 172           # per-lane DMA source offsets of the wave's four K pieces / four V pieces of a half-tile
# scalar registers owned by the loop statement
S_KB, S_KL, S_VB, S_VL, S_BLK, S_CNT, S_T0, S_T2, S_K128, S_V128, S_KST, S_VST = 80, 82, 84, 86, 87, 88, 90, 92, 94, 95, 96, 97
S_CLOB = list(range(80, 98))
LOOP_PRE = 24                 # issue cycles of vector work the loop's blocks put in front of their first MFMA (the boundary blocks: 64)


def AO(c, h, dt):
    return 16 * (c.DT * h + dt)


def AQ(c, h, ks):
    return 32 * c.DT + 4 * (c.KS * h + ks)


def gen_block(c, dt, U, dma, chain=None, pre=64, salu=None, loop=False, rowmax=True, halfdma=False, stats=None):
    """Block U.  dma: issue the wave's pieces from the scalar walkers (halfdma: only every second one, the 256-row form).  chain
    (the loop): the block does not open with its K reads -- the previous block issued them in its tail -- and issues the NEXT
    block's first four K reads itself, behind the lines of `chain` (the sub-step boundary: vmcnt wait, barrier, ...), which sit
    in front of MFMA 30: behind the wait for the last V^T fragment, so every LDS read of this sub-step has returned when the
    barrier releases the slots.  pre: issue cycles of vector work in front of the first MFMA.  salu: scalar lines per gap.
    loop: the row maxima go ahead of the row sums, followed by the deferred-rescale test's two compares (the loop keeps the
    branch).  rowmax=False: no row maxima at all (the static body).  stats: a list that receives the per-gap issue costs."""
    D, KS, DT, HALF, NQK, NMF = c.D, c.KS, c.DT, c.HALF, c.NQK, c.NMF
    mf, cv = MFMA16[dt], CVT_PK[dt]
    SC, SN = (SA, SB) if U % 2 == 0 else (SB, SA)
    koff = ((U + 1) & 3) * HALF
    voff = c.VRING + U * HALF
    s = Stream()
    lines = s.lines

    def k_read(ks):
        s.read(("K", ks), [f"ds_read_b128 {vr(KF + 4 * (ks % AHEAD), 4)}, {vr(KA + ks)} offset:{koff}"])

    def v_read(p):
        k2, d = divmod(p, DT)
        off = voff + k2 * 16 * D * 2
        b = VF + 4 * (p % AHEAD)
        s.read(("V", p), [f"ds_read_b64_tr_b16 {vr(b, 2)}, {vr(VA + 2 * d)} offset:{off}",
                          f"ds_read_b64_tr_b16 {vr(b + 2, 2)}, {vr(VA + 2 * d + 1)} offset:{off}"])

    # ---- vector work: an exponential stream and a stream of everything else, each item with what it waits for ----
    # exponentials in groups of four (both halves of two adjacent scores): after group g the packing of P word (g & 3) of
    # key half (g >> 2) and the row-sum adds of those scores are ready
    EXP = []
    for g in range(8):
        for h in (0, 1):
            EXP += [(h, 2 * g), (h, 2 * g + 1)]
    pos = {e: n for n, e in enumerate(EXP)}
    cvq = []           # (kind, text, exponentials that must have been issued)
    for k2 in (0, 1):
        for j in range(4):
            for h in (0, 1):
                need = max(pos[(h, 8 * k2 + 2 * j)], pos[(h, 8 * k2 + 2 * j + 1)]) + 1
                cvq.append(("cvt", f"{cv} {vr(P[h] + 4 * k2 + j)}, {vr(SC[h] + 8 * k2 + 2 * j)}, {vr(SC[h] + 8 * k2 + 2 * j + 1)}", need))
    adds = []
    for h in (0, 1):
        adds.append([("add", f"v_add_f32 {vr(PS[h])}, {vr(SC[h])}, {vr(SC[h] + 1)}", pos[(h, 1)] + 1)]
                    + [("add", f"v_add_f32 {vr(PS[h])}, {vr(PS[h])}, {vr(SC[h] + i)}", pos[(h, i)] + 1) for i in range(2, 16)]
                    + [("add", f"v_add_f32 %[l{h}], %[l{h}], {vr(PS[h])}", 32)])
    addq = [x for pair in zip(*adds) for x in pair]      # the two halves' chains interleaved
    E = NQK + 1        # S_nxt[1]'s last MFMA is MFMA NQK - 1: its readers sit two or more MFMAs behind it
    # v_permlane32_swap: 2 wait states behind the VALU write of either operand and in front of a reader of its results: the
    # other half's mov / swap and one s_nop each way ("tail": emitted as one unit, never split by other vector work)
    maxq, tail = row_max(TH, SN, MX, nop=0)
    tail = [t for _, t in tail]

    if loop:
        tail = tail + ["v_cmp_gt_f32 vcc, %[mx0], %[th0]", f"v_cmp_gt_f32 {sr(S_T2, 2)}, %[mx1], %[th1]"]
    if not rowmax:
        maxq, tail = [], []
    dcost = COST64["dma"] if D == 128 else 4
    dgaps = c.DMA_GAPS if dma else ()
    salu = salu or {}
    ei = 0             # exponentials issued
    last_exp_line = -10

    def emit_slot(cycles, gap, final=False):
        """Fill one slot: up to NEXP exponentials while there are any, then whatever is ready, by issue cost."""
        nonlocal ei, last_exp_line
        used = 0
        nexp = 0
        progress = True
        while progress and (used < cycles or final):
            progress = False
            if cvq and cvq[0][2] <= ei and len(lines) - last_exp_line >= 1 + (1 if cvq[0][2] == ei else 0):
                k, t, need = cvq.pop(0)
                lines.append(t); used += COST64[k]; progress = True
                continue
            if ei < len(EXP) and (nexp < c.NEXP or gap < 0 or final):
                h, i = EXP[ei]
                lines.append(f"v_exp_f32 {vr(SC[h] + i)}, {vr(SC[h] + i)}")
                last_exp_line = len(lines) - 1
                ei += 1; nexp += 1; used += COST64["exp"]; progress = True
                continue
            if loop and maxq and gap >= E:
                k, t = maxq.pop(0)
                lines.append(t); used += COST64[k]; progress = True
                continue
            if loop and not maxq and tail and gap >= E:
                lines.extend(tail); used += len(tail) * 4; tail.clear(); progress = True
                continue
            if addq and addq[0][2] <= ei and len(lines) - last_exp_line >= 2:
                k, t, need = addq.pop(0)
                lines.append(t); used += COST64[k]; progress = True
                continue
            if maxq and gap >= E:
                k, t = maxq.pop(0)
                lines.append(t); used += COST64[k]; progress = True
                continue
            if not maxq and not addq and not cvq and ei == len(EXP) and tail and gap >= E:
                lines.extend(tail); used += 6 * 4; tail.clear(); progress = True
        return used

    dma_j = 0

    def dma_piece():
        """Pieces in the order K0 K1 V0 V1 K2 K3 V2 V3.  One M0 value (the LDS destination) serves two pieces: the second one
        carries the instruction offset 2048, which moves BOTH its LDS destination and its source -- its lane offset register
        has the 2048 subtracted.  The source base is the half-tile's row 0 (re-based once per block); lane offset register j
        holds the rows of piece j.  One SALU instruction per two pieces instead of four per piece."""
        nonlocal dma_j
        if halfdma and (dma_j & 1):
            dma_j += 1
            return
        pair, sub = divmod(dma_j, 2)
        isv, hi = pair & 1, pair >> 1
        base, ldsw, vo = (S_VB, S_VL, VOV) if isv else (S_KB, S_KL, VOK)
        j = 2 * hi + sub
        lines.extend(lds_dma(vo + j, sr(base, 2) + (" offset:2048" if sub else ""), m0=None if sub else (sr(ldsw), 4096 * hi)))
        dma_j += 1

    if chain is None:
        for ks in range(AHEAD):
            k_read(ks)
    else:
        for ks in range(AHEAD):
            s.in_flight(("K", ks), 1)      # in flight since the previous block's tail
    emit_slot(pre, -1)
    usage = []
    for i in range(NMF):
        if i < NQK:
            ks, h = divmod(i, 2)
            if h == 0:
                s.wait_for(("K", ks))
            acc = vr(NM[h], 16) if ks == 0 else vr(SN[h], 16)
            lines.append(f"{mf} {vr(SN[h], 16)}, {vr(KF + 4 * (ks % AHEAD), 4)}, {ar(AQ(c, h, ks), 4)}, {acc}")
            fixed = 0
            if h == 1 and ks + AHEAD < KS:
                k_read(ks + AHEAD); fixed += COST64["lds"]
            if h == 0 and ks >= KS - AHEAD:   # V^T fragments 0..3 ride the last QK^T shadows (head dim 128: gaps 8, 10, 12, 14)
                v_read(ks - (KS - AHEAD)); fixed += 2 * COST64["lds"]
        else:
            p, h = divmod(i - NQK, 2)
            k2, d = divmod(p, DT)
            if h == 0:
                text = "\n".join(lines)
                for hh in (0, 1):
                    for jj in range(4):
                        assert f"{cv} {vr(P[hh] + 4 * k2 + jj)}," in text, (dt, U, "P not packed before PV", p)
                s.wait_for(("V", p))
            if chain is not None and i == NMF - 2:
                lines.extend(chain)
                nk = ((U + 2) & 3) * HALF
                lines.extend(f"ds_read_b128 {vr(KF + 4 * ks, 4)}, {vr(KA + ks)} offset:{nk}" for ks in range(AHEAD))
            lines.append(f"{mf} {ar(AO(c, h, d), 16)}, {vr(VF + 4 * (p % AHEAD), 4)}, {vr(P[h] + 4 * k2, 4)}, {ar(AO(c, h, d), 16)}")
            fixed = 0
            if h == 1 and p + AHEAD < 2 * DT:
                v_read(p + AHEAD); fixed += 2 * COST64["lds"]
        lines.extend(salu.get(i, []))      # scalar bookkeeping of the loop riding in this gap (free beside an MFMA)
        if i in dgaps:
            dma_piece(); fixed += dcost
        usage.append(fixed + emit_slot(c.GAPC - fixed, i, final=(i == NMF - 1)))
    assert ei == len(EXP) and not cvq and not addq and not maxq and not tail, (dt, U, "vector work left over")
    assert dma_j == len(dgaps)
    if stats is not None:
        stats.append((dt, U, dma, usage))
    return lines


def rowmax_lines(S):
    """mx[h] = row maximum of the 32 x 32 score tile S[h] (both halves), out of the pipelined block."""
    chain, tail = row_max(TH, S, MX, chains=1)
    return [t for _, t in chain + tail]


def gen_qk0(c, dt):
    """Prologue: S_A[h] = K(half-tile 0, slot 0) . Q[h]^T - m[h], row maxima -- the block's first half without a softmax."""
    SN, s = SA, Stream()

    def k_read(ks):
        s.read(ks, [f"ds_read_b128 {vr(KF + 4 * (ks % AHEAD), 4)}, {vr(KA + ks)}"])

    for ks in range(AHEAD): k_read(ks)
    for ks in range(c.KS):
        s.wait_for(ks)
        for h in (0, 1):
            acc = vr(NM[h], 16) if ks == 0 else vr(SN[h], 16)
            s.lines.append(f"{MFMA16[dt]} {vr(SN[h], 16)}, {vr(KF + 4 * (ks % AHEAD), 4)}, {ar(AQ(c, h, ks), 4)}, {acc}")
        if ks + AHEAD < c.KS: k_read(ks + AHEAD)
    s.lines.append("s_nop 15")     # the last MFMA's passes (8 + margin) before the maxima read S
    s.lines.append("s_nop 3")
    return s.lines + rowmax_lines(SN)


def rescale_core(c, S, al, de, ng):
    """O[h] *= al[h], S[h] -= de[h], -m[h] = ng[h] for both halves (operand names given per half)."""
    lines = ["s_nop 11"]     # the last PV MFMA of the preceding block wrote O: 12 wait states before it is read
    for h in (0, 1):
        for g in range(0, 16 * c.DT, 8):
            base = AO(c, h, 0) + g
            lines += [f"v_accvgpr_read_b32 {vr(TMP0 + j)}, {ar(base + j)}" for j in range(8)]
            lines += [f"v_mul_f32 {vr(TMP0 + j)}, {vr(TMP0 + j)}, {al[h]}" for j in range(8)]
            lines += [f"v_accvgpr_write_b32 {ar(base + j)}, {vr(TMP0 + j)}" for j in range(8)]
        lines += [f"v_sub_f32 {vr(S[h] + i)}, {vr(S[h] + i)}, {de[h]}" for i in range(16)]
        lines += [f"v_mov_b32 {vr(NM[h] + i)}, {ng[h]}" for i in range(16)]
    return lines


def rescale_decide():
    """The deferred-rescale decision of rsa_attn_kernel64.hip::half in asm (both halves): from mx[h], thr[h], m_ref[h], l[h] to
    al = v144/v145, de = v146/v147, ng = v148/v149 (and the updated thr, m_ref, l).  A half moves iff ANY of its rows exceeds its
    threshold (wave-uniform, like the C++ side's ballot); first = the row has not seen a finite score yet (thr = -inf)."""
    L = []
    mv, fin = sr(S_T0, 2), sr(S_T2, 2)
    for h in (0, 1):
        al, de, ng = vr(144 + h), vr(146 + h), vr(148 + h)
        mx, th, mr, l = f"%[mx{h}]", f"%[th{h}]", f"%[mr{h}]", f"%[l{h}]"
        L += [f"v_cmp_gt_f32 vcc, {mx}, {th}",                     # rows above their threshold
              "s_cmp_lg_u64 vcc, 0",
              f"s_cselect_b64 {mv}, -1, 0",                        # move: any row of this half (all lanes or none)
              f"v_max_f32 {de}, 0, {mx}",                          # delta = first ? mx : max(mx, 0)
              f"v_cmp_eq_f32 vcc, {th}, %[ninf]",                  # first
              f"v_cndmask_b32 {de}, {de}, {mx}, vcc",
              f"v_cmp_neq_f32 {fin}, {de}, %[ninf]",               # delta finite (not "nothing but masked keys so far")
              f"s_and_b64 {mv}, {mv}, {fin}",                      # lanes that move their reference
              f"v_cndmask_b32 {de}, 0, {de}, {mv}",                # the others: delta = 0
              f"v_exp_f32 {al}, -{de}",
              f"v_cndmask_b32 {th}, {th}, %[eight], {mv}",
              f"v_add_f32 {mr}, {mr}, {de}",
              f"v_cndmask_b32 {al}, {al}, 1.0, vcc",               # first: alpha = 1 (O and l are still zero)
              f"v_xor_b32 {ng}, 0x80000000, {mr}",
              f"v_mul_f32 {l}, {l}, {al}",
              f"v_sub_f32 {mx}, {mx}, {de}"]                      # the row maximum follows its scores to the new reference
    return L


def gen_loop_head0(t0, t1):
    """K walker -> key 0 of the next kept block (S_BLK), K pieces to LDS slot 0.., V pieces to slot 3 (block 0's V(u+3))."""
    return [f"s_mul_i32 {t0}, {sr(S_BLK)}, {sr(S_K128)}", f"s_mul_hi_u32 {t1}, {sr(S_BLK)}, {sr(S_K128)}",
            f"s_mov_b64 {sr(S_KB, 2)}, %[kb]",
            f"s_add_u32 {sr(S_KB)}, {sr(S_KB)}, {t0}", f"s_addc_u32 {sr(S_KB + 1)}, {sr(S_KB + 1)}, {t1}",
            f"s_mov_b32 {sr(S_KL)}, %[ldsk]"]


def gen_loop(c, dt, static=False, halfdma=False, stats=None):
    """The steady-state loop, one asm statement (see the file docstring).  Operands: cnt (kept blocks to process, >= 0),
    blk0 / blk1 (block index of the first one and of its successor), la (VGPR: LDS byte address of the list entry two blocks
    ahead), kb / vb (64-bit bases of this head's K / V), krow / vrow (bytes per key row), ldsk / ldsv (LDS address of the wave's
    first piece in slot 0 of the K / V ring).
    static (round 6): the statement carries a SECOND body, taken when the scalar operand `stat` is non-zero: the same four blocks
    without the row maxima and without the deferred-rescale test -- the walk then keeps the softmax reference it entered the
    loop with (rsa_attn_kernel64.hip: "optimistic static reference"; the kernel checks l and O afterwards and redoes the walk
    through the first body if anything overflowed).
    halfdma: every second LDS-DMA piece dropped, vmcnt(VMC / 2) at the sub-step boundary (the 256-row dense form)."""
    HALF, SALU_AT = c.HALF, c.SALU_AT
    t0, t1 = sr(S_T0), sr(S_T0 + 1)
    vmc = c.VMC // 2 if halfdma else c.VMC
    L = [f"s_mov_b32 {sr(S_CNT)}, %[cnt]",
         f"s_cmp_eq_u32 {sr(S_CNT)}, 0",
         "s_cbranch_scc1 .Lk5w_done_%=",
         f"s_lshl_b32 {sr(S_K128)}, %[krow], 7", f"s_lshl_b32 {sr(S_V128)}, %[vrow], 7",
         f"s_lshl_b32 {sr(S_KST)}, %[krow], 5", f"s_lshl_b32 {sr(S_VST)}, %[vrow], 5",
         f"s_mov_b32 {sr(S_BLK)}, %[blk1]",
         # V walker: the kept block being processed, its last half-tile (key 96): vb + blk0 * vrow128 + 96 * vrow
         f"s_mul_i32 {t0}, %[blk0], {sr(S_V128)}", f"s_mul_hi_u32 {t1}, %[blk0], {sr(S_V128)}",
         f"s_mov_b64 {sr(S_VB, 2)}, %[vb]",
         f"s_add_u32 {sr(S_VB)}, {sr(S_VB)}, {t0}", f"s_addc_u32 {sr(S_VB + 1)}, {sr(S_VB + 1)}, {t1}",
         f"s_mul_i32 {t0}, %[vrow], 96",
         f"s_add_u32 {sr(S_VB)}, {sr(S_VB)}, {t0}", f"s_addc_u32 {sr(S_VB + 1)}, {sr(S_VB + 1)}, 0"]
    # the first iteration's K walker and V slot (every later one is set up in block 3's gaps)
    L += gen_loop_head0(t0, t1) + [f"s_add_u32 {sr(S_VL)}, %[ldsv], {3 * HALF}"]
    # end of a sub-step: the pieces of two blocks ago have landed, every wave has finished its LDS reads
    boundary = [f"s_waitcnt vmcnt({vmc})", "s_barrier"]
    # entry: the boundary in front of the first block and its first K reads (slot 1: U = 0 reads K(u+1))
    L += boundary + [f"ds_read_b128 {vr(KF + 4 * ks, 4)}, {vr(KA + ks)} offset:{HALF}" for ks in range(AHEAD)]
    if static:
        L += ["s_cmp_lg_u32 %[stat], 0", "s_cbranch_scc1 .Lk5w_sloop_%="]
    for lname in ["loop"] + (["sloop"] if static else []):
        online = lname == "loop"
        L += [f".Lk5w_{lname}_%=:"]
        for U in range(4):
            head = []
            if U == 1:     # V walker: the next kept block, key 0; V pieces to slot 0..
                head += [f"s_mul_i32 {t0}, {sr(S_BLK)}, {sr(S_V128)}", f"s_mul_hi_u32 {t1}, {sr(S_BLK)}, {sr(S_V128)}",
                         f"s_mov_b64 {sr(S_VB, 2)}, %[vb]",
                         f"s_add_u32 {sr(S_VB)}, {sr(S_VB)}, {t0}", f"s_addc_u32 {sr(S_VB + 1)}, {sr(S_VB + 1)}, {t1}",
                         f"s_mov_b32 {sr(S_VL)}, %[ldsv]"]
            tail = list(boundary)
            if U == 1:     # list entry of the block after next: an LDS read older than every K read of block 2 (made scalar in block 3)
                tail = tail + ["ds_read_u16 %[lv], %[la]"]
            # the DMA walkers step to the next half-tile (re-based at U = 0 / 1 where a new kept block starts)
            kstep = [f"s_add_u32 {sr(S_KB)}, {sr(S_KB)}, {sr(S_KST)}", f"s_addc_u32 {sr(S_KB + 1)}, {sr(S_KB + 1)}, 0",
                     f"s_add_u32 {sr(S_KL)}, {sr(S_KL)}, {HALF}"]
            vstep = [f"s_add_u32 {sr(S_VB)}, {sr(S_VB)}, {sr(S_VST)}", f"s_addc_u32 {sr(S_VB + 1)}, {sr(S_VB + 1)}, 0",
                     f"s_add_u32 {sr(S_VL)}, {sr(S_VL)}, {HALF}"]
            nxt = [f"v_readfirstlane_b32 {sr(S_BLK)}, %[lv]", "v_add_u32 %[la], 2, %[la]"]   # (read two blocks ago) -> the next iteration's block index
            # the scalar bookkeeping rides in MFMA gaps (a scalar instruction beside an MFMA is free, between two blocks it is not:
            # one wave per SIMD).  The wave's K pieces sit in gaps 1, 5, 17, 21, its V pieces in gaps 9, 13, 25, 29: the K walker
            # steps (U = 3: is re-based on the next kept block) behind gap 21, the V walker steps behind gap 29 -- except in
            # front of block 1, which re-bases it in its own gaps 2..4, ahead of its first V piece.
            salu = {}
            g3, gh = SALU_AT["k3"], SALU_AT["h1"]
            if U == 3:
                k0 = gen_loop_head0(t0, t1)
                salu[g3[0]] = nxt[:1] + k0[:2]
                salu[g3[1]] = k0[2:5]
                salu[g3[2]] = k0[5:] + nxt[1:]
            else:
                salu[SALU_AT["k"]] = kstep
            if U != 0:                    # (block 1 re-bases the V walker itself)
                salu[SALU_AT["v"]] = vstep
            if U == 1:
                salu[gh[0]] = head[:3]
                salu[gh[1]] = head[3:]
            L += gen_block(c, dt, U, True, chain=tail, pre=LOOP_PRE, salu=salu, loop=online, rowmax=online, halfdma=halfdma, stats=stats)
            if online:    # deferred-rescale test on the scores the NEXT block consumes (S_nxt of this block; compares in the block)
                L += [f"s_or_b64 vcc, vcc, {sr(S_T2, 2)}", f"s_cbranch_vccnz .Lk5w_resc{U}_%=", f".Lk5w_back{U}_%=:"]
        L += [f"s_sub_u32 {sr(S_CNT)}, {sr(S_CNT)}, 1", f"s_cmp_lg_u32 {sr(S_CNT)}, 0", f"s_cbranch_scc1 .Lk5w_{lname}_%=",
              "s_waitcnt lgkmcnt(0)",       # (the K reads the last block issued for its successor: nothing may land behind the statement)
              "s_branch .Lk5w_done_%="]
    for U in range(4):
        S = SB if U % 2 == 0 else SA          # S_nxt of block U
        L += [f".Lk5w_resc{U}_%=:"] + rescale_decide()
        L += rescale_core(c, S, [vr(144), vr(145)], [vr(146), vr(147)], [vr(148), vr(149)])
        L += [f"s_branch .Lk5w_back{U}_%="]
    L += [".Lk5w_done_%=:"]
    return L


def header(stats=None):
    """The text of rsa_attn_block64.h: the streams of head dim 128 (RSA_K5W_*), then those of head dim 64 (RSA_K5V_*)."""
    return "\n".join(["// GENERATED by gen_k5_block64.py -- do not edit; edit the generator (its docstring says what this is).", "#pragma once", ""]
                     + [main_one(c, stats) for c in HEAD_DIMS])


def main_one(c, stats=None):
    KS, DT, R = c.KS, c.DT, f"RSA_{c.PFX}_"
    out = []
    for dt in ("bf16", "f16"):
        for U in range(4):
            out.append(macro(f"{R}BLOCK_{dt.upper()}_U{U}", gen_block(c, dt, U, False, stats=stats)))
        out.append(macro(f"{R}LOOP_{dt.upper()}", gen_loop(c, dt, static=(dt == "bf16"), stats=stats)))   # (fp16 P overflows at 2^16: no static body)
        # the 256-row dense form (four waves on one K/V ring): the same loop with every second LDS-DMA piece dropped -- each wave stages
        # 2 + 2 of a half-tile's 8 + 8 pieces (lane offset registers 0 and 2), vmcnt(8) at the sub-step boundary
        out.append(macro(f"{R}LOOP_{dt.upper()}_R256", gen_loop(c, dt, static=(dt == "bf16"), halfdma=True, stats=stats)))
        out.append(macro(f"{R}QK0_{dt.upper()}", gen_qk0(c, dt)))
    # rare paths on the pinned arch registers, as asm as well (the compiler never computes on S / -m: it then keeps every
    # pinned tile in place between statements instead of shuffling 16-register tuples around the blocks)
    for nmx, S in (("A", SA), ("B", SB)):
        out.append(macro(f"{R}ROWMAX_{nmx}", rowmax_lines(S)))
        # boundary mask: score i of lane half hh is key kfirst + 4 hh + (i & 3) + 8 (i >> 2); kept iff lo <= key < hi, tested
        # as (key - lo) <u (hi - lo): %[kb0/1] = kfirst + 4 hh - lo[h], %[sp0/1] = hi[h] - lo[h] (0 when the range is empty)
        lines = []
        for h in (0, 1):
            for i in range(16):
                off = (i & 3) + 8 * (i >> 2)
                lines.append(f"v_add_u32 {vr(T[0])}, {off}, %[kb{h}]")
                lines.append(f"v_cmp_gt_u32 vcc, %[sp{h}], {vr(T[0])}")
                lines.append(f"v_cndmask_b32 {vr(S[h] + i)}, %[ninf], {vr(S[h] + i)}, vcc")
        out.append(macro(f"{R}MASK_{nmx}", lines))
        # deferred rescale of both halves: O[h] *= al[h], S[h] -= de[h], -m[h] = ng[h] (a half that does not move gets 1, 0
        # and its old -m: exact no-ops)
        out.append(macro(f"{R}RESCALE_{nmx}", rescale_core(c, S, ["%[al0]", "%[al1]"], ["%[de0]", "%[de1]"], ["%[ng0]", "%[ng1]"])))
    out.append(macro(f"{R}NMZERO", [f"v_mov_b32 {vr(NM[0] + i)}, 0" for i in range(32)]))
    # accumulator-file housekeeping: zero O, write one Q fragment, read one O tile
    out.append(macro(f"{R}OZERO", [f"v_accvgpr_write_b32 {ar(i)}, 0" for i in range(32 * DT)]))
    # (k-steps / d tiles a head dim does not have get an empty body: the C++ side names all of them and discards by `if constexpr`)
    for h in (0, 1):
        for ks in range(8):
            out.append(macro(f"{R}QWRITE_H{h}_K{ks}",
                             [f"v_accvgpr_write_b32 {ar(AQ(c, h, ks) + j)}, {vr(TMP0 + j)}" for j in range(4)] if ks < KS else ["s_nop 0"]))
    for h in (0, 1):
        for d in range(4):
            out.append(macro(f"{R}OREAD_H{h}_D{d}",
                             [f"v_accvgpr_read_b32 {vr(TMP0 + j)}, {ar(AO(c, h, d) + j)}" for j in range(16)] if d < DT else ["s_nop 0"]))
    # operand lists
    def tiles(mod, S, name):
        return [pin(mod, S[h], 16, f"{name}[{h}]") for h in (0, 1)]
    souts = tiles("+", SA, "SA") + tiles("+", SB, "SB")
    lsum, mxo = ['[l0] "+v"(l[0])', '[l1] "+v"(l[1])'], ['[mx0] "=&v"(mx[0])', '[mx1] "=&v"(mx[1])']
    ins = tiles("", NM, "nm") + [pin("", KA, 8, "ka"), pin("", VA, 8, "va")]
    out.append(ops_macro(f"{R}OPS", souts + lsum + mxo, ins))
    nmio = tiles("+", NM, "nm")
    louts = souts + nmio + lsum + ['[mx0] "+v"(mx[0])', '[mx1] "+v"(mx[1])',
                                   '[th0] "+v"(thr[0])', '[th1] "+v"(thr[1])', '[mr0] "+v"(m_ref[0])', '[mr1] "+v"(m_ref[1])',
                                   '[la] "+v"(la)', '[lv] "=&v"(lv)']
    lins = [pin("", KA, 8, "ka"), pin("", VA, 8, "va"), pin("", VOK, 4, "vok"), pin("", VOV, 4, "vov"),
            '[cnt] "s"(cnt)', '[blk0] "s"(blk0)', '[blk1] "s"(blk1)', '[kb] "s"(kb)', '[vb] "s"(vb)', '[krow] "s"(krow)',
            '[vrow] "s"(vrow)', '[ldsk] "s"(ldsk)', '[ldsv] "s"(ldsv)', '[ninf] "v"(ninf)', '[eight] "v"(eight)', '[stat] "s"(stat)']
    out.append(ops_macro(f"{R}OPS_LOOP", louts, lins))
    out.append(ops_macro(f"{R}OPS_QK0", tiles("+", SA, "SA") + mxo, ins[:3]))
    for nmx, S in (("A", SA), ("B", SB)):
        so = tiles("+", S, f"S{nmx}")
        out.append(ops_macro(f"{R}OPS_ROWMAX_{nmx}", so + mxo, []))
        out.append(ops_macro(f"{R}OPS_MASK_{nmx}", so, ['[kb0] "v"(kb0)', '[kb1] "v"(kb1)', '[sp0] "v"(sp0)', '[sp1] "v"(sp1)', '[ninf] "v"(ninf)']))
        out.append(ops_macro(f"{R}OPS_RESCALE_{nmx}", so + nmio, [f'[{n}{h}] "v"({n}{h})' for n in ("al", "de", "ng") for h in (0, 1)]))
    out.append(ops_macro(f"{R}OPS_NMZERO", tiles("=", NM, "nm")))
    out.append(f"#define {R}CLOBBER_TMP " + clobbers("v", range(TMP0, TMP1)))
    out.append(f"#define {R}CLOBBER_O " + clobbers("a", range(32 * DT)))
    out.append(f"#define {R}CLOBBER_Q " + clobbers("a", range(32 * DT, 32 * DT + 8 * KS)))
    out.append(f"#define {R}CLOBBER_LOOP " + clobbers("s", S_CLOB) + ', "vcc", "scc"')
    out.append(f"// head dim {c.D}: O a[0:{32 * DT - 1}], Q a[{32 * DT}:{32 * DT + 8 * KS - 1}]; SA v[0:31], SB v[32:63], -m v[64:95], temporaries v[{TMP0}:{TMP1 - 1}] "
               f"(P v[96:111], K ring v[112:127], V ring v[128:143]), K addresses v[{KA}:{KA + 7}], V addresses v[{VA}:{VA + 7}], "
               f"DMA lane offsets v[{VOK}:{VOV + 1}]; the loop statement owns s[{S_CLOB[0]}:{S_CLOB[-1]}]")
    return "\n".join(out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "stats":
        stats = []
        header(stats)
        for dt, U, dma, usage in stats:
            if dt == "bf16" and U == 0:
                print(f"U{U} dma={dma}: per-gap issue cost {usage}  total {sum(usage)}")
    else:
        print(header())
