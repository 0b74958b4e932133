#!/usr/bin/env python3
"""Generator of K5's hand-placed pipelined block (rsa_attn_block.h).

The block is one sub-step of the block-sparse attention main loop of rsa_attn_kernel.hip for ONE wave (32 query rows):

    S_nxt^T = K(sub-tile u+1) . Q^T - m    KS = D/16 MFMAs  (A = K rows from LDS by ds_read_b128, B = Q fragments, registers;
                                                             the chain starts from a 16-register block holding -m)
    P       = exp2(S_cur)                  in place, fp32; row sum into l; packed to the 2-byte type
    O^T    += V(sub-tile u)^T . P^T        2 * D/32 MFMAs   (A = V^T by ds_read_b64_tr_b16, B = packed P)
    mx      = row max of S_nxt             (two v_max3 chains + one v_permlane32_swap)

hipcc schedules that as it pleases (round 2: every operand read followed by lgkmcnt(0), profiles/r03_k5_r1_vs_head.md), so
the instruction stream is written here, once, with every register named: LDS operand reads run AHEAD MFMAs ahead of their
MFMA behind counted lgkmcnt waits, and the softmax's vector instructions are dealt into the MFMA shadows by issue cost
(cdna_hip_programming.md: 4 cycles per plain VALU, 8 per v_exp_f32, an MFMA leaves about 24 issue cycles of its 32).
Registers are pinned through physical-register constraints ("{v[96:111]}"); the operand lists are generated with the
streams (RSA_K5_OPS*), so the C++ side cannot drift from the register map.

One block is generated per (D, dtype, K/V slot parity, sub-step parity); its form is a function of the head dim (negm_form):
  * RSA_K5_BLOCKN_128_*: head dim 128.  The kernel runs at the board's power cap (1.39 kW, 1.72 GHz under this loop,
    tools/clock_probe.py), so what it saves is instructions, not stalls: starting the score chain from -m removes the 16
    subtractions of a sub-step (-3.7 % time), the row maximum as two chains placed as soon as S_nxt is complete another
    0.7 % (profiles/r03_k5_block.md).  Nothing pads the statement behind its last MFMA: the only vector code that touches O
    outside the blocks (the rare rescale, the epilogue) carries the 12 wait states itself.
  * RSA_K5_BLOCK_64_*: head dim 64.  Round 2's compiled block's arithmetic operation for operation (S, then S - m by v_sub),
    which measures 4 % faster there than the -m form, with the row sums on the matrix pipe (rsm_form).

Measured and dropped: the sub-step's LDS-DMA pieces spread over the MFMA shadows (16.96 vs 16.42 ms: a piece stalls its wave
~70 cycles wherever it is issued, and inside the block that stall stops the wave's MFMA stream), 16x16x32 MFMAs (timing
probe: +-0 sparse, +3 % dense), packed f32 adds for the row sum (+0.8 % time).

The output depends on nothing but this file and the generators' shared core, k5gen.py.

usage: python3 gen_k5_block.py > rsa_attn_block.h
"""
from k5gen import CVT_PK, MFMA16, Stream, clobbers, codemap_work, lds_dma, macro, ops_macro, pin, row_max1, vr

AHEAD = 4          # LDS operand buffers per operand kind (K fragments, V^T fragments)
# issue cycles of the 32-row kernels' vector work: the 2-byte kernel, the e4m3 kernel and its pv form (the 64-row table differs)
COST32 = dict(sub=4, exp=8, cvt=4, cvt8=5, add=4, max=4, mov=4, nop=8, swap=4)


class Map:
    def __init__(self, D):
        self.D, self.KS, self.DT = D, D // 16, D // 32
        r = 0
        self.O = r; r += 16 * self.DT
        self.Q = r; r += 4 * self.KS
        self.SA = r; r += 16
        self.SB = r; r += 16
        self.NM = r
        if negm_form(D): r += 16         # the reference maximum, negated, in all 16 registers: C operand of the first QK^T MFMA
        self.tmp0 = r
        self.P = r; r += 8
        self.KF = r; r += 4 * AHEAD
        self.VF = r; r += 4 * AHEAD
        self.PS = r; r += 1
        self.T0 = r; r += 1
        self.T1 = r; r += 1
        self.tmp1 = r            # clobbered temporaries: [tmp0, tmp1)
        r = (r + 3) & ~3
        self.KA = r; r += self.KS
        self.VA = r; r += 2 * self.DT
        self.RSM = rsm_form(D)
        if self.RSM:             # row sums on the matrix pipe (head dim 64, round 5): l in four registers, the ones operand
            r = (r + 3) & ~3
            self.LACC = r; r += 4
            self.ONES = r; r += 4
        self.end = r


def negm_form(D):
    """Head dim 128: the score chain starts from -m (no subtraction in the softmax).  Head dim 64: the classic form, S then S - m."""
    return D == 128


def rsm_form(D):
    """Head dim 64: 8 MFMAs per sub-step against the same softmax make the wave vector-bound
    (profiles/r05_d64_experiments.txt: without the vector work -29 %), so the 16 row-sum additions go to the matrix pipe as two
    v_mfma_f32_16x16x32 (ones . P^T, 4 passes each): l = the row sum of the ROUNDED P, complete over both lane halves."""
    return D == 64


def gen_block(D, dt, VS, SUB):
    """The asm lines of one block variant."""
    m = Map(D)
    negm = negm_form(D)
    KS, DT = m.KS, m.DT
    mf, cv = MFMA16[dt], CVT_PK[dt]
    TILE = 64 * D * 2
    SC, SN = (m.SA, m.SB) if SUB == 0 else (m.SB, m.SA)
    kslot, ksub = (VS, 1) if SUB == 0 else (VS ^ 1, 0)
    koff = kslot * TILE + ksub * 32 * D * 2
    vbase = (2 + VS) * TILE
    s = Stream(COST32)
    lines = s.lines

    def k_read(ks):
        s.read(("K", ks), [f"ds_read_b128 {vr(m.KF + 4 * (ks % AHEAD), 4)}, {vr(m.KA + ks)} offset:{koff}"])

    def v_read(p):
        k2, d = divmod(p, DT)
        off = vbase + (2 * SUB + k2) * 16 * D * 2
        b = m.VF + 4 * (p % AHEAD)
        s.read(("V", p), [f"ds_read_b64_tr_b16 {vr(b, 2)}, {vr(m.VA + 2 * d)} offset:{off}",
                          f"ds_read_b64_tr_b16 {vr(b + 2, 2)}, {vr(m.VA + 2 * d + 1)} offset:{off}"])

    # ---- the vector work, in issue order ----
    def pair(i):   # two scores interleaved so that no instruction reads its predecessor's result
        sub = [("sub", f"v_sub_f32 {vr(SC + j)}, {vr(SC + j)}, %[m]") for j in (i, i + 1)]
        exp = [("exp", f"v_exp_f32 {vr(SC + j)}, {vr(SC + j)}") for j in (i, i + 1)]
        return exp if negm else sub + exp

    def C(j):
        return [("cvt", f"{cv} {vr(m.P + j)}, {vr(SC + 2 * j)}, {vr(SC + 2 * j + 1)}")]

    work = []
    for i in range(0, 8, 2): work += pair(i)
    work += pair(8)
    for j in range(0, 4): work += C(j)
    for i in range(10, 16, 2): work += pair(i)
    work += [("add", f"v_add_f32 {vr(m.PS)}, {vr(SC)}, {vr(SC + 1)}")]
    for i in range(2, 8): work += [("add", f"v_add_f32 {vr(m.PS)}, {vr(m.PS)}, {vr(SC + i)}")]
    for j in range(4, 8): work += C(j)
    for i in range(8, 16): work += [("add", f"v_add_f32 {vr(m.PS)}, {vr(m.PS)}, {vr(SC + i)}")]
    work += [("add", f"v_add_f32 %[l], %[l], {vr(m.PS)}")]
    if m.RSM:
        work = [w for w in work if w[0] != "add"]
    s.work, s.maxw = work, row_max1(m.T0, m.T1, SN, 8, 2 if negm else 1)     # (-m form: two chains, merged by a v_max)
    mf_rs = "v_mfma_f32_16x16x32_bf16" if dt == "bf16" else "v_mfma_f32_16x16x32_f16"
    nm = KS + 2 * DT                      # MFMAs of the block
    total = sum(COST32[k] for k, _ in s.work + s.maxw)
    pre = 72 if D == 128 else 48          # vector work issued while the first K fragments are in flight
    budget = max(24, -(-(total - pre) // nm) + 2)

    # (head dim 64: 8 MFMAs per sub-step against the same softmax, the wave is bound by vector issue, and raising its
    # priority over its partner on the SIMD costs 3-5 %: tools/perf_d64.py, profiles/r03_k5_block.md)
    if D == 128: lines.append("s_setprio 2")
    for ks in range(min(AHEAD, KS)): k_read(ks)
    s.emit_work(pre, False)
    for i in range(nm):
        if i < KS:
            s.wait_for(("K", i))
            c = (vr(m.NM, 16) if negm else "0") if i == 0 else vr(SN, 16)
            lines.append(f"{mf} {vr(SN, 16)}, {vr(m.KF + 4 * (i % AHEAD), 4)}, {vr(m.Q + 4 * i, 4)}, {c}")
            if i + AHEAD < KS: k_read(i + AHEAD)
            p = i - (KS - min(AHEAD, KS))          # V^T fragments of the first PV MFMAs ride the last QK shadows
            if 0 <= p < min(AHEAD, 2 * DT) and KS >= AHEAD: v_read(p)
            if KS < AHEAD and i == KS - 1:
                for pp in range(min(AHEAD, 2 * DT)): v_read(pp)
        else:
            p = i - KS
            k2, d = divmod(p, DT)
            text = "\n".join(lines)
            for jj in range(4):   # sanity: the half of P this MFMA reads has been packed
                assert f"{cv} {vr(m.P + 4 * k2 + jj)}," in text, (D, dt, VS, SUB, "P not packed before PV", p)
            if m.RSM and d == 0:      # l += ones . P^T over the 16 keys of half k2 (behind the conversions that packed it)
                lines.append("s_nop 1")
                lines.append(f"{mf_rs} {vr(m.LACC, 4)}, {vr(m.ONES, 4)}, {vr(m.P + 4 * k2, 4)}, {vr(m.LACC, 4)}")
            s.wait_for(("V", p))
            lines.append(f"{mf} {vr(m.O + 16 * d, 16)}, {vr(m.VF + 4 * (p % AHEAD), 4)}, {vr(m.P + 4 * k2, 4)}, {vr(m.O + 16 * d, 16)}")
            if p + AHEAD < 2 * DT: v_read(p + AHEAD)
        last = i == nm - 1
        # The row max reads S_nxt: two or more MFMAs behind the last QK MFMA (its 8 passes are over).  Classic form: it fills
        # the last two shadows and the tail, padded to the 12 wait states between the last PV MFMA and any VALU touching O.
        n0 = len(lines)
        s.emit_work(10 ** 6 if last else budget, i >= (KS + 1 if negm else max(KS + 1, nm - 2)))
        if last and not negm:
            tail = sum(int(l.split()[1]) + 1 if l.startswith("s_nop") else 1 for l in lines[n0:])
            if tail < 12: lines.append(f"s_nop {11 - tail}")
    assert not s.work and not s.maxw
    if D == 128: lines.append("s_setprio 0")
    return lines


def main():
    out = ["// GENERATED by gen_k5_block.py -- do not edit; edit the generator (its docstring says what this is).", "#pragma once", ""]
    for D in (128, 64):
        for dt in ("bf16", "f16"):
            for VS in (0, 1):
                for SUB in (0, 1):
                    out.append(macro(f"RSA_K5_BLOCK{'N' if negm_form(D) else ''}_{D}_{dt.upper()}_V{VS}_S{SUB}", gen_block(D, dt, VS, SUB)))
    # operand lists (the constraint strings carry the register map) and the clobbered temporaries
    for D in (128, 64):
        m, negm = Map(D), negm_form(D)
        outs = [pin("+", m.O + 16 * d, 16, f"o[{d}]") for d in range(m.DT)]
        outs += [pin("+", m.SA, 16, "SA"), pin("+", m.SB, 16, "SB"), pin("+", m.LACC, 4, "lacc") if m.RSM else '[l] "+v"(l)', '[mx] "=&v"(mx)']
        ins = [pin("", m.Q + 4 * k, 4, f"q[{k}]") for k in range(m.KS)]
        ins += [pin("", m.NM, 16, "nm")] if negm else ['[m] "v"(m)']
        ins += [pin("", m.KA, m.KS, "ka"), pin("", m.VA, 2 * m.DT, "va")]
        if m.RSM: ins += [pin("", m.ONES, 4, "onesv")]
        tag = f"{'N' if negm else ''}_{D}"
        out.append(ops_macro(f"RSA_K5_OPS{tag}", outs, ins))
        out.append(f"#define RSA_K5_CLOBBER{tag} " + clobbers("v", range(m.tmp0, m.tmp1)))
        out.append(f"// D = {D}{' (-m form)' if negm else ''}: O v[{m.O}:{m.Q - 1}], Q v[{m.Q}:{m.SA - 1}], SA v[{m.SA}:{m.SA + 15}], "
                   f"SB v[{m.SB}:{m.SB + 15}], " + (f"-m v[{m.NM}:{m.NM + 15}], " if negm else "")
                   + f"temporaries v[{m.tmp0}:{m.tmp1 - 1}], K addresses v[{m.KA}:{m.KA + m.KS - 1}], V addresses v[{m.VA}:{m.end - 1}]")
    main8(out)
    main8h(out)
    print("\n".join(out))


# =====================================================================================================================
# e4m3 kernel (rsa_attn_fp8_kernel.hip): one block = one 64-KEY TILE of one wave
#     S_nxt^T (two 32-key halves) = K8(tile+1) . Q8^T + (4 - m)   4 x v_mfma_scale_f32_32x32x64_f8f6f4 (chains start from MB)
#     P = exp2(S_cur) -> e4m3, packed in place into S_cur[0][0:7] 32 v_exp_f32 + 16 v_cvt_pk_fp8_f32
#     l += ones . P (row sum on the matrix pipe)                    1 x v_mfma_f32_16x16x128_f8f6f4
#     O^T += 2^ev V8^T(tile) . P                                    4 x v_mfma_scale_f32_32x32x64_f8f6f4 (V block scale: byte 1)
#     mx = row max of S_nxt
# Every A operand is 8 registers = 2 x ds_read_b128, read AHEAD8 MFMAs ahead into a ring of RING8 buffers.  K and V live in
# 4-slot LDS rings: the tile's slot (TS = tile & 3) is a compile-time constant of the block, so every LDS address is a
# loop-invariant VGPR plus an immediate (the compiled block spent ~16 v_add_u32 per tile on them).
# =====================================================================================================================
AHEAD8, RING8 = 3, 4


def operand_reads(b, reads):
    """ds_read_b128 of an A operand into v[b:...]: four registers per (address register, immediate) pair"""
    return [f"ds_read_b128 {vr(b + 4 * c2, 4)}, {vr(areg)}" + (f" offset:{off}" if off else "") for c2, (areg, off) in enumerate(reads)]
DMA8_GAPS = [0, 2, 4, 6]      # dma form: K piece 0, K piece 1, V piece 0, V piece 1 behind these MFMAs of the nine
                              # (placement: profiles/r05_pv_hand_placed.txt)


class Map8:
    def __init__(self, D8=128):
        r = 0
        self.D8, self.KS, self.DT = D8, D8 // 64, D8 // 32
        self.O = r; r += 16 * self.DT
        self.Q = r; r += 8 * self.KS
        self.SA = r; r += 32
        self.SB = r; r += 32
        self.MB = r; r += 16
        self.LACC = r; r += 4
        self.tmp0 = r
        self.OP = r; r += 8 * RING8
        self.T0 = r; r += 1
        self.T1 = r; r += 1
        self.tmp1 = r
        r = (r + 1) & ~1
        self.SC = r; r += 2          # E8M0 scale operands of the QK^T MFMAs
        self.KA = r; r += 2 * self.KS   # K read addresses [ks][chunk]
        self.VA = r; r += 2          # V read addresses [chunk]
        self.ON = r; r += 1          # address of this lane's ones / zeros pattern
        r = (r + 1) & ~1
        self.DK = r; r += 2          # LDS-DMA lane offsets of the wave's two K pieces (the second = the first + 4 096): dma form
        self.DV = r; r += 2          # ... of its two V pieces (head dim 64: one piece each)
        self.ONES = r; r += 8        # dma form: the row-sum product's ones operand in registers (as the pv block): 2 KiB fewer LDS reads per tile and wave
        self.end = r


def gen_block8(TS, codemap=False, D8=128, dma=False):
    """dma (round 5; head dim 128): the block also issues the wave's four LDS-DMA pieces -- K(tile + 3) into ring slot (TS + 3) & 3,
    V(tile + 2) into (TS + 2) & 3 -- one per MFMA shadow instead of as a burst behind the barrier (there the eight waves' pieces queue
    at the CU's one addresser: profiles/r05_pv_hand_placed.txt).  Scalar operands: %[ksrc] / %[vsrc] = first byte of the wave's
    first piece, %[ldsw] = LDS address of the wave's first piece in slot 0 of the K ring."""
    m = Map8(D8)
    SC_, SN = (m.SA, m.SB) if TS % 2 == 0 else (m.SB, m.SA)
    TILE8 = 64 * D8
    kslot = (TS + 1) & 3
    s = Stream(COST32)
    lines = s.lines
    # the A operands, in MFMA order (nine at head dim 128, five at 64): (kind, LDS reads as (address register, immediate) pairs)
    ops = []
    for sub in range(2):
        for ks in range(m.KS):
            off = kslot * TILE8 + sub * 32 * D8
            ops.append(("qk", sub, ks, [(m.KA + 2 * ks, off), (m.KA + 2 * ks + 1, off)]))
    n_qk = len(ops)
    ones_reg = dma      # (round 5: -3 % at head dim 128, profiles/r05_pv_hand_placed.txt)
    ops.append(("rs", 0, 0, [] if ones_reg else [(m.ON, 0), (m.ON, 16)]))
    for dt in range(m.DT):
        off = (4 + TS) * TILE8 + dt * 2048
        ops.append(("pv", dt, 0, [(m.VA, off), (m.VA + 1, off)]))

    def read(i):
        if ops[i][3]:
            s.read(i, operand_reads(m.OP + 8 * (i % RING8), ops[i][3]))

    # vector work: exponentials in place, the e4m3 words of P built in place in S_cur[0][0:7]
    work = []
    def exps(sub, i0):
        return [("exp", f"v_exp_f32 {vr(SC_ + 16 * sub + i)}, {vr(SC_ + 16 * sub + i)}") for i in range(i0, i0 + 4)]
    def pack(j):   # P word j = 4 * sub + w4 <- exp values 4 w4 .. 4 w4 + 3 of half `sub`
        sub, w4 = divmod(j, 4)
        e = SC_ + 16 * sub + 4 * w4
        return [("cvt", f"v_cvt_pk_fp8_f32 {vr(SC_ + j)}, {vr(e)}, {vr(e + 1)}"),
                ("cvt", f"v_cvt_pk_fp8_f32 {vr(SC_ + j)}, {vr(e + 2)}, {vr(e + 3)} op_sel:[0,0,1]")]
    # order: a group's exponentials, then the PREVIOUS group's packing (a transcendental's result is not read by the next
    # instruction); word j overwrites register j of S_cur[0], whose value the words before it have consumed
    groups = [(s_, i0) for s_ in range(2) for i0 in range(0, 16, 4)]
    if not codemap:
        for g, (s_, i0) in enumerate(groups):
            work += exps(s_, i0)
            if g >= 1: work += pack(g - 1)
        work += pack(7)
    else:
        work = codemap_work(SC_)      # (k5gen.py says what the code-map form is)
    s.work, s.maxw = work, row_max1(m.T0, m.T1, SN, 16, 2)

    lines.append("s_setprio 2")
    for i in range(AHEAD8): read(i)
    s.emit_work(64, False)
    n = len(ops)
    for i, (kind, x, y, _) in enumerate(ops):
        if kind != "qk" and s.work:   # the row sum and PV read the whole packed P
            s.emit_work(0, False, force_all=True)
        if ops[i][3]:
            s.wait_for(i)
        a = vr(m.OP + 8 * ((i if ops[i][3] else i - m.KS) % RING8), 8)
        if kind == "qk":
            c = vr(m.MB, 16) if y == 0 else vr(SN + 16 * x, 16)
            lines.append(f"v_mfma_scale_f32_32x32x64_f8f6f4 {vr(SN + 16 * x, 16)}, {a}, {vr(m.Q + 8 * y, 8)}, {c}, "
                         f"{vr(m.SC)}, {vr(m.SC + 1)} op_sel_hi:[0,0,0]")
        elif kind == "rs":
            lines.append("s_nop 1")   # the last word of P was packed just above
            lines.append(f"v_mfma_f32_16x16x128_f8f6f4 {vr(m.LACC, 4)}, {vr(m.ONES, 8) if ones_reg else a}, {vr(SC_, 8)}, {vr(m.LACC, 4)}")
        else:
            # (byte 1 of the scale registers: the V block's scale on A, 1.0 on the P operand)
            lines.append(f"v_mfma_scale_f32_32x32x64_f8f6f4 {vr(m.O + 16 * x, 16)}, {a}, {vr(SC_, 8)}, {vr(m.O + 16 * x, 16)}, "
                         f"{vr(m.SC)}, {vr(m.SC + 1)} op_sel:[1,1,0] op_sel_hi:[0,0,0]")
        if i + AHEAD8 < n: read(i + AHEAD8)
        gaps = DMA8_GAPS if D8 == 128 else [0, 2]      # head dim 64: one K piece, one V piece per wave and tile
        if dma and i in gaps:
            j = gaps.index(i)
            isv, hi = divmod(j, TILE8 // 4096)
            dst = (4 + ((TS + 2) & 3)) * TILE8 + hi * 4096 if isv else ((TS + 3) & 3) * TILE8 + hi * 4096
            lines += lds_dma((m.DV if isv else m.DK) + hi, "%[vsrc]" if isv else "%[ksrc]", m0=("%[ldsw]", dst))
        # row max of S_nxt: two MFMAs behind the last QK^T MFMA (index n_qk - 1): from the shadow of PV 0 (index n_qk + 1) on
        s.emit_work(10 ** 6 if i == n - 1 else 48, i >= n_qk + 1)
    assert not s.work and not s.maxw
    lines.append("s_setprio 0")
    return lines


def outs8(m):
    """the outputs every e4m3 / pv statement shares: O, both score tiles (two 32-key halves each), l, the row maximum"""
    return ([pin("+", m.O + 16 * d, 16, f"o[{d}]") for d in range(m.DT)]
            + [pin("+", S + 16 * h, 16, f"{n}[{h}]") for n, S in (("SA", m.SA), ("SB", m.SB)) for h in (0, 1)]
            + [pin("+", m.LACC, 4, "lacc"), '[mx] "=&v"(mx)'])


def main8(out):
    for codemap in (False, True):
        for TS in range(4):
            out.append(macro(f"RSA_K5F8_BLOCK{'C' if codemap else ''}_T{TS}", gen_block8(TS, codemap)))
    for TS in range(4):   # the product at head dim 128: code map + the wave's LDS-DMA pieces inside the block
        out.append(macro(f"RSA_K5F8_BLOCKCD_T{TS}", gen_block8(TS, True, 128, dma=True)))
    for TS in range(4):   # head dim 64 (CogVideoX): the code-map form, staging behind the barrier / inside the block (product)
        for dma in (False, True):
            out.append(macro(f"RSA_K5F8_BLOCKC{'D' if dma else ''}64_T{TS}", gen_block8(TS, True, 64, dma=dma)))
    for D8, tag in ((64, "64"), (128, "")):
        m = Map8(D8)
        ins = [pin("", m.Q + 8 * ks, 8, f"q[{ks}]") for ks in range(m.KS)]
        ins += [pin("", m.MB, 16, "mblk"), pin("", m.SC, 1, "sca"), pin("", m.SC + 1, 1, "scb"), pin("", m.KA, 2 * m.KS, "ka"),
                pin("", m.VA, 2, "va")]
        out.append(ops_macro(f"RSA_K5F8_OPS{tag}", outs8(m), ins + [pin("", m.ON, 1, "ona")]))
        insd = ins + [pin("", m.ONES, 8, "onesv"), pin("", m.DK, m.KS, "dk"), pin("", m.DV, m.KS, "dv"),
                      '[ksrc] "s"(ksrc)', '[vsrc] "s"(vsrc)', '[ldsw] "s"(ldsw)']
        out.append(ops_macro(f"RSA_K5F8_OPS{tag}D", outs8(m), insd))
        out.append(f"#define RSA_K5F8_CLOBBER{tag} " + clobbers("v", range(m.tmp0, m.tmp1)))
        out.append(f"// e4m3 kernel{', head dim 64' if D8 == 64 else ''}: O v[0:{m.Q - 1}], Q v[{m.Q}:{m.SA - 1}], SA v[{m.SA}:{m.SB - 1}], SB v[{m.SB}:{m.MB - 1}], "
                   f"{'reference block' if D8 == 64 else '4 - m'} v[{m.MB}:{m.LACC - 1}], l v[{m.LACC}:{m.LACC + 3}], temporaries v[{m.tmp0}:{m.tmp1 - 1}], "
                   f"scales v[{m.SC}:{m.SC + 1}], K / V / ones addresses v[{m.KA}:{m.end - 1}]")


# =====================================================================================================================
# the "pv" form of the e4m3 kernel (round 5; rsa_attn_fp8_kernel.hip, HYB instances): one block = one 64-key tile of one wave
#     S_nxt^T (two 32-key halves) = K(tile+1) . Q^T + MB     16 x v_mfma_f32_32x32x16 on the 2-BYTE K rows (A = one ds_read_b128 per
#                                                            k-step from the 16 KiB K tile, image of rsa_attn_kernel.hip) and the
#                                                            2-byte Q fragments (32 registers; Q carries sm_scale log2e 8)
#     P codes, row sum, O^T += V8^T . P, mx                  exactly the e4m3 block above (code map form)
# Rings of THREE slots (K 3 x 16 KiB at LDS 0, V 3 x 8 KiB behind it): K(tile+1) sits in slot (tile + 1) % 3, V(tile) in
# tile % 3, S_cur is SA on even tiles -> six variants, T = tile % 6.  The V read addresses carry the V ring's base (49 152 is
# beyond what the 16-bit offset field could add to a K address with slot and d-tile offsets on top).
# The LDS operand registers are a pool of eight 4-register slots (QK^T fragments take one, the 8-register operands of the row
# sum and of P . V two, aligned): a read may re-target a slot once the MFMA AFTER its last consumer has been issued (the rule
# of the e4m3 block's ring); QK^T fragments are read six MFMAs ahead (a 2-byte MFMA is half as long as an e4m3 one), the rest three.
# =====================================================================================================================
class Map8H:
    def __init__(self, D8=128):
        self.D8, self.KS, self.DT = D8, D8 // 16, D8 // 32
        self.NPK, self.NPV = D8 // 32, D8 // 64          # LDS-DMA pieces per wave: K tile (64 rows x 2 D8 bytes), V tile (D8 x 64 bytes)
        r = 0
        self.O = r; r += 16 * self.DT
        self.Q = r; r += 4 * self.KS
        self.SA = r; r += 32
        self.SB = r; r += 32
        self.MB = r; r += 16
        self.LACC = r; r += 4
        self.tmp0 = r
        self.OP = r; r += 4 * NSLOT8H
        self.T0 = r; r += 1
        self.T1 = r; r += 1
        self.tmp1 = r
        r = (r + 1) & ~1
        self.SC = r; r += 2
        self.VA = r; r += 2          # V read addresses [chunk], V ring base included (an even-aligned pair)
        self.KB = r; r += 1          # K read address of k-step 0 (row r of slot 0); k-step ks = this ^ (ks << 5) (the tile's XOR
                                     # swizzle), built in T0 / T1 just before the reads; 32-key half and ring slot are immediates
        r = (r + 1) & ~1
        self.ONES = r; r += 8        # A operand of the row-sum product (e4m3 1.0 or 0 in all 32 bytes: a constant of the lane)
        r = (r + 3) & ~3
        self.DK = r; r += self.NPK   # dma form: LDS-DMA lane offsets of the wave's K pieces of tile + 3 (rows clamped: per tile)
        r = (r + 1) & ~1
        self.DV = r; r += self.NPV   # ... of its V pieces (a second one = the first + 4 096: constants of the lane)
        self.end = r


NSLOT8H = 6      # 4-register operand slots (256 registers per wave at two waves per SIMD: the block pins 212 of them at head dim 128)


DMA8H_GAPS = {128: [1, 4, 7, 10, 13, 16],     # dma form: K pieces 0..3, V pieces 0, 1 behind these MFMAs of the 21
              64: [1, 4, 7]}                  # head dim 64: K pieces 0, 1, V piece 0 of the 11


def gen_block8h(T6, dt, dma=False, D8=128):
    """dma: the block also issues the wave's six LDS-DMA pieces -- K(tile + 3) into ring slot T6 % 3 (= K(tile)'s), V(tile + 2) into
    (T6 + 2) % 3 -- one per MFMA shadow (see gen_block8).  Scalar operands: %[kb16] = the head's K rows, %[vsrc] = first byte of the
    wave's first V piece, %[ldsw] = LDS address of the wave's first piece in slot 0 of the K ring."""
    m = Map8H(D8)
    KTILE, VTILE = 128 * D8, 64 * D8          # bytes of a K tile (64 keys x 2 D8: 16 / 8 KiB) and of a V tile (D8 x 64: 8 / 4 KiB)
    mf = MFMA16[dt]
    SC_, SN = (m.SA, m.SB) if T6 % 2 == 0 else (m.SB, m.SA)
    kslot, vslot = (T6 + 1) % 3, T6 % 3
    s = Stream(COST32)
    lines = s.lines
    ops = []      # (kind, x, y, reads [(address register, offset)], slots)
    for ks in range(m.KS):       # the two halves' chains alternate: no MFMA waits for the one just before it
        kreg = m.KB if ks == 0 else (m.T0 if ks % 2 == 0 else m.T1)
        for sub in range(2):
            ops.append(("qk", sub, ks, [(kreg, kslot * KTILE + sub * (KTILE // 2))], 1))
    n_qk = len(ops)
    ops.append(("rs", 0, 0, [], 0))
    for d in range(m.DT):
        off = vslot * VTILE + d * 2048
        ops.append(("pv", d, 0, [(m.VA, off), (m.VA + 1, off)], 2))
    n = len(ops)
    slot_of, consumer = {}, [None] * NSLOT8H     # consumer[s] = index of the op that reads slot s (None: free)
    state = dict(issued=-1)

    def read(j, cur):
        need = ops[j][4]
        if need == 0:
            return
        for s0 in range(0, NSLOT8H, need):
            # (cur - 2: the MFMA AFTER the slot's last consumer has been issued, the rule of the e4m3 block's ring)
            if all(consumer[s0 + u] is None or consumer[s0 + u] <= cur - 2 for u in range(need)):
                break
        else:
            raise AssertionError(("no free operand slot", T6, j, cur, consumer))
        for u in range(need):
            consumer[s0 + u] = j
        slot_of[j] = s0
        b = m.OP + 4 * s0
        kind, sub, ks = ops[j][0], ops[j][1], ops[j][2]
        if kind == "qk" and sub == 0 and ks > 0:
            assert state["issued"] < n_qk, "T0 / T1 belong to the row maximum from P . V 0 on"
            lines.append(f"v_xor_b32 {vr(ops[j][3][0][0])}, {hex(ks << 5)}, {vr(m.KB)}")
        s.read(j, operand_reads(b, ops[j][3]))

    # vector work: the code-map conversions of S_cur in place (as gen_block8), then the row maximum of S_nxt
    s.work, s.maxw = codemap_work(SC_), row_max1(m.T0, m.T1, SN, 16, 2)
    nxt = 0           # next op whose operand read has not been issued

    def top_up(cur):
        """issue the reads of the next ops while an operand slot is free (`cur` = the op about to issue)"""
        nonlocal nxt
        while nxt < n:
            try:
                read(nxt, cur)
            except AssertionError:
                break
            nxt += 1

    lines.append("s_setprio 2")
    top_up(0)
    s.emit_work(48, False)
    for i, (kind, x, y, _, _) in enumerate(ops):
        if kind != "qk" and s.work:   # the row sum and P . V read the whole packed P
            s.emit_work(0, False, force_all=True)
        assert i < nxt, ("operand never read", T6, i)
        if ops[i][4]:
            s.wait_for(i)
        b = m.OP + 4 * slot_of.get(i, slot_of.get(i - 1, 0))
        if kind == "qk":
            c = vr(m.MB, 16) if y == 0 else vr(SN + 16 * x, 16)
            lines.append(f"{mf} {vr(SN + 16 * x, 16)}, {vr(b, 4)}, {vr(m.Q + 4 * y, 4)}, {c}")
        elif kind == "rs":
            lines.append("s_nop 1")
            lines.append(f"v_mfma_f32_16x16x128_f8f6f4 {vr(m.LACC, 4)}, {vr(m.ONES, 8)}, {vr(SC_, 8)}, {vr(m.LACC, 4)}")
        else:
            lines.append(f"v_mfma_scale_f32_32x32x64_f8f6f4 {vr(m.O + 16 * x, 16)}, {vr(b, 8)}, {vr(SC_, 8)}, {vr(m.O + 16 * x, 16)}, "
                         f"{vr(m.SC)}, {vr(m.SC + 1)} op_sel:[1,1,0] op_sel_hi:[0,0,0]")
        state["issued"] = i
        top_up(i + 1)
        if dma and i in DMA8H_GAPS[D8]:
            j = DMA8H_GAPS[D8].index(i)
            if j < m.NPK:
                dst, vo, src = (T6 % 3) * KTILE + j * 4096, m.DK + j, "%[kb16]"
            else:
                dst, vo, src = 3 * KTILE + ((T6 + 2) % 3) * VTILE + (j - m.NPK) * 4096, m.DV + j - m.NPK, "%[vsrc]"
            lines += lds_dma(vo, src, m0=("%[ldsw]", dst))
        # row max of S_nxt: two MFMAs behind the last QK^T MFMA
        s.emit_work(10 ** 6 if i == n - 1 else (20 if kind == "qk" else 48), i >= n_qk + 1)
    assert not s.work and not s.maxw and nxt == n
    lines.append("s_setprio 0")
    return lines


def main8h(out):
    for D8 in (128, 64):
        tag = "" if D8 == 128 else "64"
        for dt in ("bf16", "f16"):
            for dma in (False, True):
                for T6 in range(6):
                    out.append(macro(f"RSA_K5F8H{tag}_BLOCK{'D' if dma else ''}_{dt.upper()}_T{T6}", gen_block8h(T6, dt, dma, D8)))
        m = Map8H(D8)
        ins = [pin("", m.Q + 16 * i, 16, f"qv[{i}]") for i in range(m.KS // 4)]     # Q fragments of four k-steps per 16-register value
        ins += [pin("", m.MB, 16, "mblk"), pin("", m.SC, 1, "sca"), pin("", m.SC + 1, 1, "scb"), pin("", m.VA, 2, "vah"),
                pin("", m.KB, 1, "kah"), pin("", m.ONES, 8, "onesv")]
        out.append(ops_macro(f"RSA_K5F8H{tag}_OPS", outs8(m), ins))
        insd = ins + [pin("", m.DK, m.NPK, "dk"), pin("", m.DV, m.NPV, "dv"), '[kb16] "s"(kb16)', '[vsrc] "s"(vsrc)', '[ldsw] "s"(ldsw)']
        out.append(ops_macro(f"RSA_K5F8H{tag}_OPSD", outs8(m), insd))
        out.append(f"#define RSA_K5F8H{tag}_CLOBBER " + clobbers("v", range(m.tmp0, m.tmp1)))
        out.append(f"// pv form, head dim {D8}: O v[0:{m.Q - 1}], Q v[{m.Q}:{m.SA - 1}], SA v[{m.SA}:{m.SB - 1}], SB v[{m.SB}:{m.MB - 1}], reference block "
                   f"v[{m.MB}:{m.LACC - 1}], l v[{m.LACC}:{m.LACC + 3}], temporaries v[{m.tmp0}:{m.tmp1 - 1}], scales v[{m.SC}:{m.SC + 1}], "
                   f"V / K addresses v[{m.VA}:{m.KB}], ones v[{m.ONES}:{m.ONES + 7}], DMA lane offsets v[{m.DK}:{m.end - 1}]")

if __name__ == "__main__":
    main()
