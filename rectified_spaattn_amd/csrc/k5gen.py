"""Shared core of K5's instruction-stream generators (gen_k5_block.py -> rsa_attn_block.h, gen_k5_block64.py -> rsa_attn_block64.h).

What every hand-placed stream is made of, once: register names, the stream with its counted lgkmcnt waits, the dealing of vector
work into MFMA shadows by issue cost, the row-maximum chain, the code-map conversion order, the LDS-DMA piece, and the printing
of macros and pinned operands.  What is specific to a kernel -- its register map, operand order, ring rule, gaps, work lists and
its COST table -- stays in its generator.  Changing anything here changes BOTH headers (csrc/Makefile lists this file as a
prerequisite of both); tests/test_k5_streams_cpu.py re-checks every wait of both on the CPU.
"""

MFMA16 = dict(bf16="v_mfma_f32_32x32x16_bf16", f16="v_mfma_f32_32x32x16_f16")
CVT_PK = dict(bf16="v_cvt_pk_bf16_f32", f16="v_cvt_pk_f16_f32")


def _regs(prefix):
    return lambda a, n=1: f"{prefix}{a}" if n == 1 else f"{prefix}[{a}:{a + n - 1}]"


vr, ar, sr = _regs("v"), _regs("a"), _regs("s")      # arch VGPRs, accumulator VGPRs, SGPRs: one register or a range of n


class Stream:
    """The instruction lines of one asm statement and the bookkeeping of its LDS reads.  LDS reads return in issue order, so the
    wait in front of an MFMA counts the reads issued AFTER the one it needs: they may still fly."""

    def __init__(self, cost=None):
        self.lines = []
        self.cost = cost             # issue cycles per kind of work item (emit_work)
        self.work, self.maxw = [], []
        self._reads = []             # issue order of the LDS reads: (tag, count)

    def in_flight(self, tag, count):
        """`count` reads of operand `tag` that were issued in front of this statement."""
        self._reads.append((tag, count))

    def read(self, tag, texts):
        self.lines += texts
        self.in_flight(tag, len(texts))

    def wait_for(self, tag):
        idx = [i for i, (t, _) in enumerate(self._reads) if t == tag][-1]
        self.lines.append(f"s_waitcnt lgkmcnt({sum(c for _, c in self._reads[idx + 1:])})")

    def emit_work(self, cycles, allow_max, force_all=False):
        """Deal (kind, text) items into one MFMA shadow until their issue costs fill `cycles` (force_all: until the queue is
        empty): the work queue first, then -- where the shadow may read S_nxt -- the row-maximum queue."""
        used = 0
        while used < cycles or force_all:
            queue = self.work or (allow_max and self.maxw)
            if not queue:
                break
            k, t = queue.pop(0)
            self.lines.append(t)
            used += self.cost[k]


def row_max(T, S, mx, pairs=8, chains=2, nop=1):
    """mx[h] = row maximum of the score tile at S[h] (2 * pairs registers) with the temporaries T[h] = (t0, t1); several tiles
    (the two row halves of the 64-row kernel) go instruction by instruction in turn.  chains = 2: two v_max3 chains per tile,
    merged by a v_max; 1: one chain.  Returns (chain, tail) as (kind, text) items: the tail is the exchange between the lane
    halves -- v_permlane32_swap wants wait states behind the VALU write of its operands and in front of a reader of its results."""
    H = range(len(S))
    t = [[vr(T[h][0]), vr(T[h][1])] for h in H]
    chain = []
    for c in range(chains):
        chain += [("max", f"v_max_f32 {t[h][c]}, {vr(S[h] + 2 * c)}, {vr(S[h] + 2 * c + 1)}") for h in H]
    for i in range(chains, pairs):
        chain += [("max", f"v_max3_f32 {t[h][i % chains]}, {t[h][i % chains]}, {vr(S[h] + 2 * i)}, {vr(S[h] + 2 * i + 1)}") for h in H]
    if chains == 2:
        chain += [("max", f"v_max_f32 {t[h][0]}, {t[h][0]}, {t[h][1]}") for h in H]
    chain += [("mov", f"v_mov_b32 {t[h][1]}, {t[h][0]}") for h in H]
    tail = ([("nop", f"s_nop {nop}")] + [("swap", f"v_permlane32_swap_b32 {t[h][0]}, {t[h][1]}") for h in H]
            + [("nop", f"s_nop {nop}")] + [("max", f"v_max_f32 {mx[h]}, {t[h][0]}, {t[h][1]}") for h in H])
    return chain, tail


def row_max1(t0, t1, S, pairs, chains):
    """The one-tile form of the 32-row kernels: the whole of it as one queue, the result in %[mx]."""
    chain, tail = row_max([(t0, t1)], [S], ["%[mx]"], pairs, chains)
    return chain + tail


def codemap_work(S):
    """Code-map form of the e4m3 kernels: the accumulator holds 8 log2(P) + 56, the e4m3 CODE of P up to rounding: one
    v_cvt_pk_u8_f32 per score (round to nearest even, saturating at 0: tools/probes/cvt_pk_u8_probe.hip), no exponential, no
    fp8 conversion.  Word j = register j of S[0]; registers 0..7 are all sources of words 0 and 1, so those two go first (word 1
    starts once word 0 has read register 1), the rest in interleaved pairs (no back-to-back dependent conversions)."""
    def byte(j, e):
        sub, w4 = divmod(j, 4)
        return ("cvt8", f"v_cvt_pk_u8_f32 {vr(S + j)}, {vr(S + 16 * sub + 4 * w4 + e)}, {e}, {vr(S + j)}")
    work = [byte(0, 0), byte(0, 1), byte(1, 0), byte(0, 2), byte(1, 1), byte(0, 3), byte(1, 2), byte(1, 3)]
    for j in (2, 4, 6):
        for e in range(4):
            work += [byte(j, e), byte(j + 1, e)]
    return work


def lds_dma(lane_offsets, src, m0=None):
    """One LDS-DMA piece (1 KiB): rows from `src` + the lane offset register, to the LDS address in M0 (m0 = (base, offset): set
    here) + the instruction offset."""
    lines = []
    if m0 is not None:
        lines += [f"s_add_u32 m0, {m0[0]}, {m0[1]}", "s_nop 0"]      # (M0 write -> LDS-DMA: one wait state)
    return lines + [f"global_load_lds_dwordx4 {vr(lane_offsets)}, {src}"]


def macro(name, lines):
    """`#define NAME \\` + the lines as one C string literal per instruction, and the blank line behind it."""
    return f"#define {name} \\\n" + " \\\n".join(f'    "{l}\\n\\t"' for l in lines) + "\n"


def pin(mod, a, n, expr):
    """An asm operand pinned to v[a : a + n - 1] through a physical-register constraint (mod: "+", "=" or "" for an input)."""
    return f'"{mod}{{{vr(a, n)}}}"({expr})'


def ops_macro(name, *lists):
    """`#define NAME : outputs : inputs`: the operand lists of an asm statement"""
    return (f"#define {name} : " + " : ".join(", ".join(l) for l in lists)).rstrip()


def clobbers(prefix, regs):
    return ", ".join(f'"{prefix}{r}"' for r in regs)
