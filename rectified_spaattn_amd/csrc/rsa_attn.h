// Shared declarations of the K5 attention kernels (rsa_attn_kernel64.hip, rsa_attn_kernel.hip: bf16 / fp16;
// rsa_attn_fp8_kernel.hip: e4m3) and their host sides (rsa_attn.hip): argument structs, the walk plan, aligned starts.
#pragma once
#include <string.h>

#include <type_traits>

#include "rsa_common.h"
#include "rsa_walk_order.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename Tag>
struct Elem;
template <>
struct Elem<bf16_tag> {
    static __device__ __forceinline__ f32x16 mfma(s16x8 a, s16x8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                       c, 0, 0, 0);
    }
    static __device__ __forceinline__ unsigned short from_f32(float f) {
        return __builtin_bit_cast(unsigned short, (__bf16)f);
    }
    static __device__ __forceinline__ s16x8 cvt8(const float* f) {
        bf16x8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (__bf16)f[i];
        return __builtin_bit_cast(s16x8, r);
    }
};
template <>
struct Elem<fp16_tag> {
    static __device__ __forceinline__ f32x16 mfma(s16x8 a, s16x8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c,
                                                      0, 0, 0);
    }
    static __device__ __forceinline__ unsigned short from_f32(float f) {
        return __builtin_bit_cast(unsigned short, (_Float16)f);
    }
    static __device__ __forceinline__ s16x8 cvt8(const float* f) {
        f16x8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (_Float16)f[i];
        return __builtin_bit_cast(s16x8, r);
    }
};

enum { MODE_SPARSE = 0, MODE_DENSE = 1 };

// What every K5 kernel needs to plan its walk and to store: the output, the kept lists, the shape and the launch's work
// mapping (filled by rsa_plan_walk, rsa_attn.hip).  AttnArgs below and Attn8Args (rsa_attn_fp8_kernel.hip) add their operands.
struct WalkArgs {
    unsigned short* out;
    long osb, osh, oss;
    const int32_t* cols;    // [BH, NBv, NB_total]
    const int32_t* counts;  // [BH, NBv]
    const float* R;         // [BH, NBv] or null
    const float* comp;      // [BH, NBv, D] or null
    float* tpart;           // split-KV partials of the text query blocks (rsa_part_row), or null
    float* tail_part;       // ... of the tail pieces (below)
    unsigned* gsync;        // start-alignment counters of this launch (below), or null
    int mode, H, Sq, Sk;
    int NBv, NQB, NB_total;  // sparse: q blocks < NBv use lists; NQB = total q blocks
    int kv_valid, kv_text_valid, q_text_end;  // sparse mode (q_text_end = NBv * block + q_text_valid)
    int q_split, kv_split;                    // dense mode
    int causal;                               // dense mode: rsa_seg_hi
    int n_heavy_pad, NBp, BH;                 // work mapping (rsa_walk_map)
    int tsplit, tper;                         // workgroups per text block, key blocks per workgroup
    int heavy_last;                           // the (split) text-row pieces are the LAST workgroups of the grid
    // Tail split: sparse workgroups [0, tail_first) walk their whole list; the tail_n x tail_p workgroups behind them are the
    // pieces of the tail_n sparse blocks tail_first .. (piece i = block tail_first + i / tail_p, part i % tail_p of its list),
    // partials to tail_part; the text pieces follow.  tail_n = 0: no split
    int tail_first, tail_n, tail_p;
    int gsync_gen;                            // aligned starts: workgroups an XCD holds at a time (a generation)
    int gsync_ratio;                          // ... walks that keep 1 / gsync_ratio of the keys or more are not held (default 2)
    int k5_static;                            // 64-row kernel, bf16: the steady state keeps the softmax reference it is entered with (checked, redone if it overflowed)
    // Walk order of the sparse units (rsa_walk_order.h): u16 [BH, NBp], rank -> unit, written by the walk_order kernels (rsa_attn.hip) in
    // front of this launch into the end of the caller's tpart; null = the eighth map (every kernel but the 64-row kernel's plain sparse
    // calls; no room; tuning key k5_walk_order = 0)
    const unsigned short* order;
};

struct AttnArgs : WalkArgs {
    const unsigned short *q, *k, *v;
    long qsb, qsh, qss, ksb, ksh, kss, vsb, vsh, vss;
    float qk_scale;
    int rows256;                              // 64-row kernel, dense calls: NQB / NBv count 256-row tiles (four waves per workgroup, one K/V ring)
    int blk;                                  // tokens per block: 128 (the 64-row kernel), or 64 (sparse calls through the _ex entry points: the 32-row kernel)
    int txt0;                                 // blk 64: first text query row (NBv * 64); text units of 128 rows from there
    // Per-row key ranges of a sparse call (rsa_block_sparse_ranged_fwd; the RANGED instantiations of the 64-row kernel): query
    // row r of batch item b sees the keys [row_lo[b * range_sb + r], row_hi[b * range_sb + r]) of its kept blocks, clamped into
    // [0, kv_valid].  row_hi NULL = no ranges (every other kernel and call); row_lo NULL = 0; range_sb 0 = one array for the batch.
    // LAST members: every field above keeps the kernarg offset the kernels without ranges read it at.
    const int32_t* row_lo;
    const int32_t* row_hi;
    long range_sb;
    // Grouped-query K/V heads (rsa_block_sparse_gqa_fwd; the GQA instantiations): query head h reads K/V head h / kv_group and
    // walks the lists of list head h / list_group (H / list_group list heads per batch item).  gqa: 0 = none (1 / 1: every other
    // call, whose kernels read none of the three), RSA_GQA_HEAD = each query head a walk of its own, RSA_GQA_PAIR = two query
    // heads of one K/V head and one list per workgroup (BH then counts head PAIRS).  Behind the ranges for the same reason.
    int kv_group, list_group, gqa;
};
enum { RSA_GQA_NONE = 0, RSA_GQA_HEAD = 1, RSA_GQA_PAIR = 2 };

// The kernel's own arguments, read in place: the argument struct must be the kernel's ONLY parameter (it then sits at offset 0
// of the kernarg segment).  The 64-row and 32-row kernels take their arguments this way, not through the by-value parameter: once
// the walk plan is the shared functions below, every use of that parameter is a plain field read and hipcc loads the whole
// struct at the head of the kernel; the fields the epilogue needs then stay live across the walk (scalar registers spilled at
// head dim 128).  Through the pointer each field is loaded where it is used, as at every use of a by-value parameter hipcc
// does not take apart.
template <typename A>
__device__ __forceinline__ const A& rsa_kernargs() {
    return *static_cast<const A*>((const void*)__builtin_amdgcn_kernarg_segment_ptr());
}

// ---------------------------------------------------------------------------------------------------------------------
// The walk plan of a workgroup, shared by the three K5 kernels (rsa_attn_kernel64.hip, rsa_attn_kernel.hip,
// rsa_attn_fp8_kernel.hip).  Out-parameters, not returned structs: after inlining the values are the callers' own scalars.
//
// Work mapping: grid index -> (batch * head, unit, piece); returns what the workgroup walks (WALK_NONE = padding workgroup).
// A head's sparse units (query blocks; n_units = NBv, or the (NBv + 1) >> 1 PAIRS of 64-token blocks) are padded to NBp, a
// multiple of 8: workgroup v of them goes to XCD
// v & 7, which takes the (v & 7)-th contiguous eighth of the head's units.  The dense text-row blocks (unit = NBv + text block)
// come FIRST when each is one long walk over every key block (no split-KV buffer: the longest work first), and LAST when they
// are split into tsplit pieces shorter than a sparse walk (heavy_last; tsp = the piece): with aligned starts the launch advances
// in generations of 8 x 64 workgroups, and the short pieces then fill the slots the last, partial generation leaves idle instead
// of adding a generation of their own.  Tail split (tail_n > 0; sparse units first): the units from index tail_first on -- the
// last, partial generation -- are walked by tail_p workgroups each, which together fill the slots that generation would leave
// idle; tail >= 0 is such a piece's index (else -1) and tsp its part of the kept list.
// With an order table (WalkArgs::order; the 64-row kernel's plain sparse calls) the whole walks are dealt in RUNS instead: the
// workgroups an XCD holds together walk consecutive units of ONE head in the table's order; the pieces of a split tail stay the
// units of the map above (rsa_walk_order.h: the arithmetic of both maps lives there, in plain C++).
template <bool ORDERED = false>
__device__ __forceinline__ int rsa_walk_map(const WalkArgs& a, int work, int n_units, int& bh, int& unit, int& tsp, int& tail) {
    return rsa_walk_map_t<ORDERED>(a, work, n_units, bh, unit, tsp, tail);
}

// Sparse walk of visual block rowi (= bh * NBv + block): its kept list, or part tsp of it for a tail piece (tail >= 0)
__device__ __forceinline__ void rsa_walk_list(const WalkArgs& a, long rowi, int tail, int tsp, const int32_t*& list, int& n_items) {
    list = a.cols + rowi * a.NB_total;
    n_items = a.counts[rowi];
    if (tail >= 0) {
        const int per = (n_items + a.tail_p - 1) / a.tail_p, first = tsp * per;
        const int left = n_items - first;
        list += first;
        n_items = left < 0 ? 0 : (left < per ? left : per);
    }
}
// Walk of a text block over the key blocks (of blk tokens) of the valid text keys, or slice tsp of them (split-KV)
__device__ __forceinline__ void rsa_walk_text(const WalkArgs& a, int blk, int tsp, int& first_blk, int& n_items) {
    n_items = (a.kv_text_valid + blk - 1) / blk;
    if (a.tsplit > 1) {
        first_blk = tsp * a.tper;
        n_items = n_items - first_blk < a.tper ? n_items - first_blk : a.tper;
        if (n_items < 0) n_items = 0;
    }
}

// Dense mode: one or two (query rows, key rows) segments -- rows below q_split see keys [0, kv_split), the others
// [kv_split, Sk) (attn.py:107-120).  causal = bottom-right aligned inside a segment: key j of a segment visible to its row i iff
// j <= i + (keys - rows) (flash-attn's convention; equal to the top-left form of the reference's "torch" / "vanilla" modes,
// attn.py:101-106 / :129-133, whenever a segment has as many keys as rows -- the only case the Python side lets through.  The
// reference's "flash" mode never passes `causal` on, attn.py:107-116, and neither does attn.py here).
// One past the last key row `row` may see:
__device__ __forceinline__ int rsa_seg_hi(const WalkArgs& a, int row) {
    const bool s1 = row >= a.q_split;
    const int lo = s1 ? a.kv_split : 0, hi = s1 ? a.Sk : a.kv_split;
    if (!a.causal) return hi;
    const int rows = s1 ? a.Sq - a.q_split : a.q_split, rin = row - (s1 ? a.q_split : 0);
    const int lim = lo + rin + 1 + ((hi - lo) - rows);
    return lim < lo ? lo : (lim < hi ? lim : hi);
}
// the key range [lo, hi) of query row grow (rows past the sequence: the last row's)
__device__ __forceinline__ void rsa_dense_row(const WalkArgs& a, int grow, int& lo, int& hi) {
    lo = grow < a.q_split ? 0 : a.kv_split;
    hi = rsa_seg_hi(a, grow < a.Sq ? grow : a.Sq - 1);
}
// ... and of the tile of `rows` query rows from row0: the extremes of its rows' ranges and the key blocks it walks
__device__ __forceinline__ void rsa_dense_tile(const WalkArgs& a, int row0, int rows, int& lo_max, int& hi_min, int& hi_max,
                                               int& first_blk, int& n_items) {
    const int row1 = row0 + rows;
    int lo_min;
    const int rlast = (row1 <= a.Sq ? row1 : a.Sq) - 1;   // last real row of the tile
    if (row1 <= a.q_split) { lo_min = 0; lo_max = 0; }
    else if (row0 >= a.q_split) { lo_min = lo_max = a.kv_split; }
    else { lo_min = 0; lo_max = a.kv_split; }
    // rsa_seg_hi grows with the row inside a segment: extremes of the tile sit at its first / last row of each segment
    hi_min = rsa_seg_hi(a, row0);
    hi_max = rsa_seg_hi(a, rlast);
    if (row0 < a.q_split && rlast >= a.q_split) {   // the tile straddles the two segments
        const int h0 = rsa_seg_hi(a, a.q_split - 1), h1 = rsa_seg_hi(a, a.q_split);
        hi_min = hi_min < h1 ? hi_min : h1;
        hi_max = hi_max > h0 ? hi_max : h0;
    }
    first_blk = lo_min / RSA_BLOCK;
    n_items = (hi_max + RSA_BLOCK - 1) / RSA_BLOCK - first_blk;
    if (hi_max <= lo_min) n_items = 0;
}

// the partial row a walk stores to: piece `tail` of tail_part, or piece tsp of text block `unit` in tpart (tsplit pieces per block)
__device__ __forceinline__ float* rsa_part_of(const WalkArgs& a, int bh, int unit, int tsp, int tail, int row, int D) {
    return tail >= 0 ? a.tail_part + rsa_part_row(tail, row, D)
                     : a.tpart + rsa_part_row(((long)bh * (a.NQB - a.NBv) + (unit - a.NBv)) * a.tsplit + tsp, row, D);
}

// ---------------------------------------------------------------------------------------------------------------------
// The fragment layer: what knows how the operands and the accumulator of a 32 x 32 MFMA lie across the lanes, once for the K5
// kernels.  Lane (r = lane & 31, hh = lane >> 5) owns query row r; register 4 g + i of an O^T tile of 32 d (d tile dt) is
// d = 32 dt + 8 g + 4 hh + i: four consecutive d per register quad.
//
// Scaled 2-byte Q fragment of one k-step (B operand of v_mfma_f32_32x32x16: the lane's k = 16 ks + 8 hh .. + 7, qp points at
// them): q * scale rounded to the input type (scale = sm_scale * log2(e), times PMap's unit in the pv form); zeros for a row
// past the sequence (!ok)
template <typename Tag>
__device__ __forceinline__ s16x8 rsa_q_frag(const unsigned short* qp, bool ok, float scale) {
    uint4 raw = make_uint4(0, 0, 0, 0);
    if (ok) raw = *reinterpret_cast<const uint4*>(qp);
    const unsigned w4[4] = {raw.x, raw.y, raw.z, raw.w};
    float f[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = rsa_to_f32<Tag>((unsigned short)(w4[e] & 0xFFFF)) * scale;
        f[2 * e + 1] = rsa_to_f32<Tag>((unsigned short)(w4[e] >> 16)) * scale;
    }
    return Elem<Tag>::cvt8(f);
}

// Split-KV partial of a row (pp = rsa_part_of: rows are 8-byte aligned): d tile dt of the unnormalised O, then the running
// maximum (log2 domain) and the row sum behind the row's D values, from lane half 0
__device__ __forceinline__ void rsa_part_tile(float* pp, int dt, int hh, const f32x16& o) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; i += 2)
            *reinterpret_cast<float2*>(pp + 32 * dt + 8 * g + 4 * hh + i) = make_float2(o[4 * g + i], o[4 * g + i + 1]);
}
__device__ __forceinline__ void rsa_part_ml(float* pp, int D, int hh, float m, float l) {
    if (hh == 0) *reinterpret_cast<float2*>(pp + D) = make_float2(m, l);
}

// The compensation values the lane adds to its row, cv[dt][g] = cp[32 dt + 8 g + 4 hh .. + 3], or zeros (cp null: a row that
// is not rectified).  ALL loads are issued here, back to back, one wait: loaded per (dt, g) inside the store loop each load's
// latency (L2 / HBM: 1-2 k cycles) is exposed in turn -- 30 k of a 64-row wave's 535 k cycles with nothing else on the SIMD to
// cover it (stamps: profiles/r04_k5_w64.md)
template <int DT>
__device__ __forceinline__ void rsa_comp_row(float4 (&cv)[DT][4], const float* cp, int hh) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) cv[dt][g] = make_float4(0, 0, 0, 0);
    if (cp) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) cv[dt][g] = *reinterpret_cast<const float4*>(cp + 32 * dt + 8 * g + 4 * hh);
    }
}

// The rectified store of d tile dt of a row (op = the row's first output element): O * sc + comp, one fma rounded to fp32, THEN
// the conversion to the storage type (what the oracle does).  Left alone, hipcc folds fma + conversion into v_fma_mixlo_f16
// (one rounding, straight to fp16) in one store form and not in the other; the empty asm keeps the fp32 value, so both store
// forms write the same bytes (tests/test_gpu_store_forms.py).
// WIDE (needs 16-byte aligned output rows): lane (r, 0) holds d = 8g .. 8g+3 and lane (r, 1) d = 8g+4 .. 8g+7 of the tile; one
// v_permlane32_swap per packed register pair regroups two g's so that each lane owns 8 consecutive d: 2 stores of 16 B per lane
// and tile instead of 4 of 8 B (the store tail of a row-per-lane epilogue is issue-bound).
template <typename Tag, bool WIDE>
__device__ __forceinline__ void rsa_out_tile(unsigned short* op, int dt, int hh, const f32x16& o, float sc, const float4 (&cv)[4]) {
    uint2 pk[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float c[4] = {cv[g].x, cv[g].y, cv[g].z, cv[g].w};
        unsigned short w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float rr = __builtin_fmaf(o[4 * g + i], sc, c[i]);
            asm volatile("" : "+v"(rr));
            w[i] = Elem<Tag>::from_f32(rr);
        }
        pk[g].x = (unsigned)w[0] | ((unsigned)w[1] << 16);
        pk[g].y = (unsigned)w[2] | ((unsigned)w[3] << 16);
    }
    if constexpr (WIDE) {
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            // X' = [X.lower, Y.lower], Y' = [X.upper, Y.upper]  (X = pk[2 gp], Y = pk[2 gp + 1])
            const auto sx = __builtin_amdgcn_permlane32_swap(pk[2 * gp].x, pk[2 * gp + 1].x, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(pk[2 * gp].y, pk[2 * gp + 1].y, false, false);
            uint4 w4;
            w4.x = sx[0]; w4.y = sy[0]; w4.z = sx[1]; w4.w = sy[1];
            *reinterpret_cast<uint4*>(op + 32 * dt + 8 * (2 * gp + hh)) = w4;
        }
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<uint2*>(op + 32 * dt + 8 * g + 4 * hh) = pk[g];
    }
}

// Host plan of a launch (rsa_attn.hip): text split, text pieces first or last, padding, tail split and the grid size, from the
// shape and the policy of the kernel family that asks.
struct WalkPolicy {
    int blk;                   // tokens per block; 64: the sparse units are pairs of query blocks
    int short_grid_text_cap;   // most pieces per text block on grids of fewer than 8 generations (longer grids, shard invariance: 16)
    bool tail_split;           // the kernel can store a tail piece's partial ...
    bool tail_beside_text;     // ... and a split tail pays beside text pieces placed last (else only in launches without text rows)
};
// *nblocks = workgroups to launch (0: nothing to do).  rsa_combine_walk: the passes behind the kernel, tail pieces then text pieces.
int rsa_plan_walk(WalkArgs& a, int BH, int D, const WalkPolicy& pol, size_t tpart_bytes, long* nblocks);
int rsa_combine_walk(const WalkArgs& a, int D, int blk, int dtype, hipStream_t s);
int rsa_launch_bsfwd(const AttnArgs& a, dim3 grid, size_t lds_bytes, int D, int dtype, hipStream_t s);     // rsa_attn_kernel.hip
int rsa_launch_bsfwd64(const AttnArgs& a, dim3 grid, size_t lds_bytes, int D, int dtype, hipStream_t s);   // rsa_attn_kernel64.hip
// ... its grouped-query instantiations (a.gqa != RSA_GQA_NONE; wide / lds_bytes as rsa_launch_bsfwd64 worked them out): rsa_attn_kernel64_gqa.hip, _gqa_pair.hip
int rsa_launch_bsfwd64_gqa(const AttnArgs& a, bool wide, dim3 grid, size_t lds_bytes, int D, int dtype, hipStream_t s);
int rsa_launch_bsfwd64_gqa_pair(const AttnArgs& a, bool wide, dim3 grid, size_t lds_bytes, int D, int dtype, hipStream_t s);
int rsa_check_out(const rsa_out4& o);
void rsa_set_fp8_variant(int v);      // rsa_attn_fp8_kernel.hip; tuning key "fp8_variant"
void rsa_set_fp8_smooth_k(int v);     // rsa_fp8.hip; tuning key "fp8_smooth_k"

// ---------------------------------------------------------------------------------------------------------------------
// Aligned starts of the sparse walks (all K5 kernels; host side: rsa_gsync_slot in rsa_attn.hip).
// Workgroup b runs on XCD b & 7 and is the (b >> 3)-th workgroup that XCD receives; the XCD holds `gen` of them at a time
// (its 32 CUs x the kernel's workgroups per CU, asked of the runtime by the launcher: 64 for the kernels at head dim 128),
// so "generation" g = (b >> 3) / gen can only be resident once generation g - 1 has left.  Every workgroup announces itself in the counter of (g, XCD) when it starts and, in front of its first
// staging instruction, waits until its whole generation has: the 64 walks of an XCD then start their ascending key lists
// TOGETHER and meet in the XCD's L2 (4 MiB = the K, V of 64 key blocks of ONE head) instead of each finding the other 63 at unrelated
// positions (HunyuanVideo R2, 10 % of the keys kept at random: L2 hit rate 15 % -> 41 %, 116 -> 79 GB over the fabric:
// profiles/r04_k5_gsync.md).  How often they meet then depends on WHICH 64 walks a generation holds: with the order table
// (rsa_walk_order.h) they are one head's, neighbours by mean kept key block -- 41.5 % -> 62.9 % hits, 79.3 -> 50.1 GB at the same
// shape, for about 3 % of the launch's time: the fabric was not what bounded it (profiles/k5_walk_order.md).  Advisory only -- the results do not depend on it: a
// bounded wait, switched off for the rest of the launch by the first workgroup that runs into the bound (word 0), so
// kernels of other processes sharing the device cannot stall this one.  Walks that keep half of the keys or more are not held
// back (round 4 drew that line at a fifth; measured at the reference scripts' operating points in round 5 --
// profiles/r05_k5_gsync_ratio.txt -- walks of 20 % of the keys gain 2.6 % from the wait, walks of 25 % on Wan2.1's 40 heads 8 %).
// ... nor are the walks of a head whose K, V mostly fit the L2 anyway (fewer than 256 key blocks = 16 MB: Wan2.2-TI2V's 214 blocks,
// 24.8 % kept, lost 2 % to the wait; measured with the guard above at 1/2, profiles/r05_k5_gsync_ratio.txt)
constexpr int RSA_GSYNC_MIN_BLOCKS = 256;
constexpr unsigned RSA_GSYNC_MAXG = 4096;    // generations with a counter (x 8 XCDs x 64 workgroups: 2 M workgroups)
constexpr int RSA_GSYNC_RING = 8;            // launches in flight with counters of their own
constexpr size_t RSA_GSYNC_SLOT_WORDS = 8 + 8 * (size_t)RSA_GSYNC_MAXG;
struct GsyncTicket { unsigned* cnt; unsigned expect; };

__device__ __forceinline__ GsyncTicket rsa_gsync_announce(unsigned* gsync, int gen) {
    GsyncTicket tk{nullptr, 0u};
    if (gsync) {
        const unsigned xcd = blockIdx.x & 7, n = blockIdx.x >> 3, g = n / (unsigned)gen;
        if (g < RSA_GSYNC_MAXG) {
            tk.cnt = gsync + 8 + g * 8 + xcd;
            const unsigned nx = (gridDim.x - xcd + 7) >> 3, left = nx - (unsigned)gen * g;
            tk.expect = left < (unsigned)gen ? left : (unsigned)gen;
            if (threadIdx.x == 0) __hip_atomic_fetch_add(tk.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return tk;
}

// (every thread of the workgroup calls it: ends in a workgroup barrier)
__device__ __forceinline__ void rsa_gsync_wait(unsigned* gsync, GsyncTicket tk, int n_items, int nb_total, int ratio = 2) {
    if (!tk.cnt) return;
    if (threadIdx.x == 0 && ratio * n_items < nb_total && nb_total >= RSA_GSYNC_MIN_BLOCKS &&
        __hip_atomic_load(gsync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        const int bound = 32 + 3 * n_items;      // x (s_sleep 32 + one L2 round trip) ~ 2 us; a kept block takes ~3.4 us
        int it = 0;
        while (__hip_atomic_load(tk.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < tk.expect) {
            __builtin_amdgcn_s_sleep(32);
            if (++it > bound) { __hip_atomic_store(gsync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
        }
    }
    __syncthreads();
}
// host: the counters of one launch (cleared in stream order in front of it) or null.  which: 1 = the 64-row kernel (on by
// default), 2 = the 32-row kernel (64-token blocks) and the e4m3 kernels (off by default: with two waves per SIMD they gain
// nothing from it and lose the wait, profiles/r04_k5_gsync.md) -- bits of the tuning key "k5_gsync"; wg_per_cu = what the runtime says fits
// (hipOccupancyMaxActiveBlocksPerMultiprocessor); *gen = workgroups per XCD generation
unsigned* rsa_gsync_slot(int which, unsigned grid, int wg_per_cu, hipStream_t s, int* gen);
int rsa_k5_static();      // tuning key "k5_static" (default 1): rsa_attn_kernel64.hip, optimistic static reference
int rsa_gsync_ratio();    // tuning key "k5_gsync_ratio" (default 2: walks keeping half of the keys or more are not held)
int rsa_wg_per_cu(const void* kernel, int block, size_t lds_bytes);   // cached hipOccupancyMaxActiveBlocksPerMultiprocessor; 0 = unknown
// launch `kernel` with the launch's alignment counters filled into its argument struct (sparse lists only: dense walks share their keys anyway)
#define RSA_LAUNCH_GSYNC(which, kernel, args, MODE_IS_SPARSE, grid, block, lds_bytes, stream) \
    do { \
        auto kfn_ = kernel; \
        auto aa_ = args; \
        aa_.gsync = nullptr; aa_.gsync_gen = 64; aa_.gsync_ratio = rsa_gsync_ratio(); aa_.k5_static = rsa_k5_static(); \
        if (MODE_IS_SPARSE) \
            aa_.gsync = rsa_gsync_slot(which, (grid).x, rsa_wg_per_cu(reinterpret_cast<const void*>(kfn_), block, lds_bytes), stream, \
                                       &aa_.gsync_gen); \
        kfn_<<<grid, block, lds_bytes, stream>>>(aa_); \
    } while (0)

// byte offset of 16-byte chunk `ch` of row `row` inside a [64][D] 2-byte tile.  The XOR keeps both the
// ds_read_b128 row reads (K as MFMA A operand) and the ds_read_b64_tr_b16 transposing reads (V^T as A
// operand) bank-conflict free for D = 128 (256-byte rows).
template <int D>
__device__ __forceinline__ int tile_off(int row, int ch) {
    if constexpr (D == 128) {
        return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
    } else {
        return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
    }
}

