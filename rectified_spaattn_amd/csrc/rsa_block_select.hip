// Block selection per list head on the device: the top-k budget (include/rsa.h: rsa_block_select), the
// pooled-key cache (rsa_pool_keys, rsa_block_select_pooled; section 5.13) and the top-p budget (rsa_block_select_p,
// rsa_block_select_pooled_p; section 5.15).  The only selection source.  All kernels are plain HIP C++ for wave64:
//
//   block_select_pool_kernel   one workgroup per (b, list head, query block) and per (b, K/V head, key block): the fp32 mean of
//                              the block's rows per channel.  q and k are read exactly once, 16 bytes per lane and load.  The
//                              query side adds the means of the list head's query heads in ascending order (H / Hl of them).
//   pool_keys_kernel           W workgroups per (b, K/V head) stride over the key blocks [start / block, ceil(len / block)) and
//                              write sel_pool_mean of each, read directly or through a block table, into the fp32 cache
//   block_score_kernel         `splits` workgroups per list row: each writes its slice of the row's ordered keys to the workspace
//                              (a lane group computes a whole score: nothing is summed across workgroups)
//   pool_key_bounds_kernel     pool_keys_kernel's min/max twin: per key block and channel the minimum and the maximum of the keys, into
//                              the fp32 bounds cache [.., NK, 2, D] (rsa_pool_key_bounds; section 5.19)
//   block_score_kernel<BOUND>  block_score_kernel over that cache: t = sum_d max(q_d mn_d, q_d mx_d), the upper bound of q . k
//                              over every key the block could hold (rsa_block_select_bound); the select kernels rank its keys LOADED
//   block_select[_p]_kernel    one 256-thread workgroup per list row (b, list head, query block): top-k; top-p capped at top_k
//
// The two select kernels are sel_row_body<L, LOADED, BUDGET>: the pooled scores of the visible key blocks into LDS as
// order-preserving 32-bit keys (computed, or LOADED from block_score_kernel's workspace), one decision (take_all, cut, T, need_eq),
// and the list contract of rsa_block_mask.hip (bitmask, ascending cols, counts) in 64-block ballot steps, ties to the lower block
// index by ballot / prefix popcount.  The decision is the one place where the budgets differ.  Top-k: the key T of the n_k-th best
// unforced block by a radix select over LDS histograms (8 bits a pass, sel_radix<false>).  Top-p: a block weighs
// u = floor(exp2((t - t_max) c) 2^18 + 0.5), an integer, recomputed from its key wherever it is needed: t_max by an integer maximum
// over the keys, the row's total and its forced mass by integer sums, the cut by the same radix with hist[digit] += u
// (sel_radix<true>), need_eq = ceil(rest / u_T); where the cap top_k binds, (T, need_eq) come from the counting radix instead.
//
// exp2 is __builtin_amdgcn_exp2f (v_exp_f32), the function of the attention kernels: exact at integer arguments.  Every fp32 sum has
// a fixed order; histograms and weights are unsigned integer sums (at most 8192 weights of at most 2^18): two calls, the same bytes.
#include "rsa_common.h"
#include "rsa_rows.h"

#include <math.h>
#include <type_traits>

#define SEL_NT 256
#define SEL_MAX_NK 8192
#define SEL_MAX_STEPS (SEL_MAX_NK / 64)
#define SEL_MAX_SPLITS 256      // score workgroups per list row of the pooled selection, at most
#define SELP_ONE 262144u        // 2^18: the weight of the row's best block

__device__ __forceinline__ int sel_key_limit(const int32_t* __restrict__ kv_len, int b, int kv_valid, int Sk) {
    return kv_len ? min(max(kv_len[b], 0), Sk) : kv_valid;
}

// fp32 -> u32 with the order of the floats (-0 counts as +0); and back.
__device__ __forceinline__ unsigned sel_key(float x) {
    unsigned u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// Exclusive prefix sums of cnt[0 .. n) in place (n <= SEL_MAX_STEPS) by one wave; returns the total (in every lane).
__device__ __forceinline__ int sel_wave_scan(int* cnt, int n, int lane) {
    int run = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        const int c = s < n ? cnt[s] : 0;
        int inc = c;
        for (int m = 1; m < 64; m <<= 1) {
            const int o = __shfl_up(inc, m, 64);
            if (lane >= m) inc += o;
        }
        if (s < n) cnt[s] = run + inc - c;
        run += __shfl(inc, 63, 64);
    }
    return run;
}

// The kernels that ask for a batch item's query rows are instantiated over the row source (rsa_rows.h; DESIGN.md sections 5.17, 5.18),
// their last argument: RowsPadded for the entries without row counts (no size: those kernels keep their arguments and their code),
// RowsCounted for the ragged entries and, over the scan's sanitised counts, for the packed ones, whose pool kernel alone also
// needs each item's first row of q [T, H, D]: RowsAt.
// Visible blocks of list row (b, i): a prefix [0, nvis) of the row.  Sq: the batch item's row count (Rows::count); SHORT (Rows::SHORT):
// a query block without a row sees nothing.
template <bool SHORT = false>
__device__ __forceinline__ int sel_visible(int len, int Sq, int blk, int NK, int i, int causal) {
    const long r0 = (long)i * blk, r1 = min(r0 + blk, (long)Sq) - 1, off = (long)len - Sq;
    if (SHORT && r0 >= Sq) return 0;
    int nvis = min(NK, (len + blk - 1) / blk);
    if (causal) nvis = r1 + off < 0 ? 0 : (int)min((long)nvis, (r1 + off) / blk + 1);
    return nvis;
}

// ---- pooling ---------------------------------------------------------------------------------------------------------------------
// The element loaders: what a lane reads for its 8 channels of a row, and how it adds them.  bf16 / fp16: 16 bytes.  e4m3_tag (the
// one-byte K cache of DESIGN.md section 5.14, rsa_pool_keys_kv8): 8 bytes of codes, added as float(code); the head's scale
// multiplies the finished mean once.  Everything below the loaders exists once.
struct e4m3_tag {};
template <typename Tag>
struct SelElem {
    using type = unsigned short;
    using vec = uint4;
};
template <>
struct SelElem<e4m3_tag> {
    using type = unsigned char;
    using vec = uint2;
};

template <typename Tag>
__device__ __forceinline__ void sel_add8(float (&a)[8], const typename SelElem<Tag>::vec v) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[2 * i] += rsa_to_f32<Tag>((unsigned short)(w[i] & 0xFFFFu));
        a[2 * i + 1] += rsa_to_f32<Tag>((unsigned short)(w[i] >> 16));
    }
}
template <>
__device__ __forceinline__ void sel_add8<e4m3_tag>(float (&a)[8], const uint2 v) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const unsigned w[2] = {v.x, v.y};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        a[4 * i] += lo[0];
        a[4 * i + 1] += lo[1];
        a[4 * i + 2] += hi[0];
        a[4 * i + 3] += hi[1];
    }
}

// Sum over `rows` rows (>= 1, uniform over the workgroup) of D channels: thread t < D returns channel t's sum.  Thread t reads the
// 16-byte chunk t % (D / 8) of rows t / (D / 8), + 2048 / D, ...; the partials meet over xor strides D / 8 .. 32 inside the wave
// and as (w0 + w1) + (w2 + w3) through LDS.
template <typename Tag>
__device__ __forceinline__ float sel_pool_block(const typename SelElem<Tag>::type* __restrict__ base, long stride_s, int rows,
                                                int D, float (*red)[128]) {
    using vec = typename SelElem<Tag>::vec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = D >> 3, RP = SEL_NT / C;
    const int c = tid % C;
    const typename SelElem<Tag>::type* p = base + c * 8;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int r = tid / C;
    for (; r + 3 * RP < rows; r += 4 * RP) {
        vec v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const vec*>(p + (long)(r + u * RP) * stride_s);
#pragma unroll
        for (int u = 0; u < 4; ++u) sel_add8<Tag>(a, v[u]);
    }
    for (; r < rows; r += RP) sel_add8<Tag>(a, *reinterpret_cast<const vec*>(p + (long)r * stride_s));
    for (int m = C; m < 64; m <<= 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += __shfl_xor(a[e], m, 64);
    }
    __syncthreads();   // (red may still be read from the previous head)
    if (lane < C) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = a[e];
    }
    __syncthreads();
    return tid < D ? (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]) : 0.f;
}

// The value of a key block in the selection: the fp32 sum of its `rows` (>= 1) keys below the limit, divided once by their count.
template <typename Tag>
__device__ __forceinline__ float sel_pool_mean(const typename SelElem<Tag>::type* __restrict__ base, long stride_s, int rows,
                                               int D, float (*red)[128]) {
    return sel_pool_block<Tag>(base, stride_s, rows, D, red) / (float)rows;
}

template <typename Tag, typename Rows, typename At>
__global__ __launch_bounds__(SEL_NT) void block_select_pool_kernel(rsa_tensor4 q, rsa_tensor4 k, int H, int Hkv, int Hl, int Sq,
                                                                   int Sk, int D, int blk, int NQ, int NK, long q_jobs,
                                                                   const int32_t* __restrict__ kv_len, int kv_valid,
                                                                   float* __restrict__ kbar, float* __restrict__ qsum, Rows src, At at) {
    __shared__ float red[4][128];
    const int tid = threadIdx.x;
    long job = blockIdx.x;
    if (job < q_jobs) {
        const int i = (int)(job % NQ);
        const long bh = job / NQ;
        const int hl = (int)(bh % Hl), gl = H / Hl;
        const long b = bh / Hl;
        const long r0 = (long)i * blk;
        // the block's rows below the batch item's count (uniform over the workgroup); a short item: none, in a block of padding --
        // the block's value is then 0, q is not read and cnt is not used
        const int rows = (int)min((long)blk, (long)src.count((int)b, Sq) - r0);
        const float cnt = (float)rows;
        float tot = 0.f;
        // the list head's query heads, ascending: each head's own mean, then the sum
        for (int u = 0; (!Rows::SHORT || rows > 0) && u < gl; ++u) {
            const unsigned short* base = static_cast<const unsigned short*>(q.ptr) + b * q.stride_b +
                                         (long)(hl * gl + u) * q.stride_h + r0 * q.stride_s;
            base += at.first(b) * q.stride_s;       // (0 where q has a batch dimension)
            tot += sel_pool_block<Tag>(base, q.stride_s, rows, D, red) / cnt;
        }
        if (tid < D) qsum[job * D + tid] = tot;
        return;
    }
    job -= q_jobs;
    const int j = (int)(job % NK);
    const long bh = job / NK;
    const int hk = (int)(bh % Hkv);
    const long b = bh / Hkv;
    const int len = sel_key_limit(kv_len, (int)b, kv_valid, Sk);
    const int rows = min(blk, len - j * blk);       // keys of block j below the limit (uniform over the workgroup)
    float mean = 0.f;
    if (rows > 0) {
        const unsigned short* base = static_cast<const unsigned short*>(k.ptr) + b * k.stride_b + (long)hk * k.stride_h +
                                     (long)j * blk * k.stride_s;
        mean = sel_pool_mean<Tag>(base, k.stride_s, rows, D, red);
    }
    if (tid < D) kbar[job * D + tid] = mean;
}

// The pooled-key cache: workgroup w of the W of (b, K/V head) writes the blocks start / blk + w, + W, ... below ceil(len / blk) and
// nothing else.  Both limits are uniform over the workgroup, so every barrier of sel_pool_block is met by all of it.  With a table
// the page of a block is read for written blocks only, and an entry outside [0, num_pages) gives zeros: no address is formed
// from it.  Tag = e4m3_tag: k holds codes (strides in bytes) and the mean of the codes is multiplied once by k_scale[hk]; the
// 2-byte forms never read k_scale.
template <typename Tag>
__global__ __launch_bounds__(SEL_NT) void pool_keys_kernel(rsa_tensor4 k, int Hkv, int Sk, int D, int blk, int NK, int W,
                                                           const int32_t* __restrict__ kv_len, int kv_valid,
                                                           const int32_t* __restrict__ start_dev, int start_host,
                                                           const int32_t* __restrict__ table, long table_stride_b,
                                                           int num_pages, float* __restrict__ out,
                                                           const float* __restrict__ k_scale) {
    using KT = typename SelElem<Tag>::type;
    __shared__ float red[4][128];
    const int tid = threadIdx.x;
    const int w = (int)(blockIdx.x % (unsigned)W);
    const long bh = blockIdx.x / (unsigned)W;
    const int hk = (int)(bh % Hkv);
    const long b = bh / Hkv;
    const int len = sel_key_limit(kv_len, (int)b, kv_valid, Sk);
    const int st = sel_key_limit(start_dev, (int)b, start_host, Sk);
    if (st > len) return;
    const int j_hi = min(NK, (len + blk - 1) / blk);
    for (int j = st / blk + w; j < j_hi; j += W) {
        const int rows = min(blk, len - j * blk);       // >= 1 below j_hi
        const KT* base;
        bool have = true;
        if (table) {
            const int page = table[b * table_stride_b + j];
            have = page >= 0 && page < num_pages;
            base = static_cast<const KT*>(k.ptr) + (long)(have ? page : 0) * k.stride_b + (long)hk * k.stride_h;
        } else {
            base = static_cast<const KT*>(k.ptr) + b * k.stride_b + (long)hk * k.stride_h + (long)j * blk * k.stride_s;
        }
        float mean = have ? sel_pool_mean<Tag>(base, k.stride_s, rows, D, red) : 0.f;
        if constexpr (std::is_same<Tag, e4m3_tag>::value) mean *= k_scale[hk];
        if (tid < D) out[(bh * NK + j) * D + tid] = mean;
    }
}

// ---- the bounds cache -----------------------------------------------------------------------------------------
// What a lane reads for its 8 channels of a row, as floats (e4m3: float(code)); sel_add8's loads and conversions.
template <typename Tag>
__device__ __forceinline__ void sel_unpack8(float (&x)[8], const typename SelElem<Tag>::vec v) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        x[2 * i] = rsa_to_f32<Tag>((unsigned short)(w[i] & 0xFFFFu));
        x[2 * i + 1] = rsa_to_f32<Tag>((unsigned short)(w[i] >> 16));
    }
}
template <>
__device__ __forceinline__ void sel_unpack8<e4m3_tag>(float (&x)[8], const uint2 v) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const unsigned w[2] = {v.x, v.y};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        x[4 * i] = lo[0];
        x[4 * i + 1] = lo[1];
        x[4 * i + 2] = hi[0];
        x[4 * i + 3] = hi[1];
    }
}
template <typename Tag>
__device__ __forceinline__ void sel_minmax8(float (&mn)[8], float (&mx)[8], const typename SelElem<Tag>::vec v) {
    float x[8];
    sel_unpack8<Tag>(x, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        mn[e] = fminf(mn[e], x[e]);
        mx[e] = fmaxf(mx[e], x[e]);
    }
}

// The min/max twin of sel_pool_block: per channel the minimum and the maximum over `rows` rows (>= 1, uniform over the workgroup);
// thread t < D returns channel t's pair (x: min, y: max).  The same loads, row striding and xor strides; a thread without a row
// holds (+inf, -inf), which no minimum or maximum keeps.  min and max are exact and order-free: any split of the rows gives the
// same values.
template <typename Tag>
__device__ __forceinline__ float2 sel_bounds_block(const typename SelElem<Tag>::type* __restrict__ base, long stride_s, int rows,
                                                   int D, float (*redn)[128], float (*redx)[128]) {
    using vec = typename SelElem<Tag>::vec;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = D >> 3, RP = SEL_NT / C;
    const int c = tid % C;
    const typename SelElem<Tag>::type* p = base + c * 8;
    float mn[8], mx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) mn[e] = INFINITY, mx[e] = -INFINITY;
    int r = tid / C;
    for (; r + 3 * RP < rows; r += 4 * RP) {
        vec v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const vec*>(p + (long)(r + u * RP) * stride_s);
#pragma unroll
        for (int u = 0; u < 4; ++u) sel_minmax8<Tag>(mn, mx, v[u]);
    }
    for (; r < rows; r += RP) sel_minmax8<Tag>(mn, mx, *reinterpret_cast<const vec*>(p + (long)r * stride_s));
    for (int m = C; m < 64; m <<= 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mn[e] = fminf(mn[e], __shfl_xor(mn[e], m, 64));
            mx[e] = fmaxf(mx[e], __shfl_xor(mx[e], m, 64));
        }
    }
    __syncthreads();   // (the reductions may still be read from the previous block)
    if (lane < C) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            redn[wave][lane * 8 + e] = mn[e];
            redx[wave][lane * 8 + e] = mx[e];
        }
    }
    __syncthreads();
    if (tid >= D) return make_float2(0.f, 0.f);
    return make_float2(fminf(fminf(redn[0][tid], redn[1][tid]), fminf(redn[2][tid], redn[3][tid])),
                       fmaxf(fmaxf(redx[0][tid], redx[1][tid]), fmaxf(redx[2][tid], redx[3][tid])));
}

// The bounds cache: pool_keys_kernel over sel_bounds_block.  out fp32 [B, Hkv, NK, 2, D]: the minima, then the maxima of a block.
// The written set, the table rule (an entry outside [0, num_pages): zeros, min and max alike) and the limits are pool_keys_kernel's.
// Tag = e4m3_tag: min and max over float(code), each multiplied once by k_scale[hk] (> 0: the order is kept).
template <typename Tag>
__global__ __launch_bounds__(SEL_NT) void pool_key_bounds_kernel(rsa_tensor4 k, int Hkv, int Sk, int D, int blk, int NK, int W,
                                                                 const int32_t* __restrict__ kv_len, int kv_valid,
                                                                 const int32_t* __restrict__ start_dev, int start_host,
                                                                 const int32_t* __restrict__ table, long table_stride_b,
                                                                 int num_pages, float* __restrict__ out,
                                                                 const float* __restrict__ k_scale) {
    using KT = typename SelElem<Tag>::type;
    __shared__ float redn[4][128], redx[4][128];
    const int tid = threadIdx.x;
    const int w = (int)(blockIdx.x % (unsigned)W);
    const long bh = blockIdx.x / (unsigned)W;
    const int hk = (int)(bh % Hkv);
    const long b = bh / Hkv;
    const int len = sel_key_limit(kv_len, (int)b, kv_valid, Sk);
    const int st = sel_key_limit(start_dev, (int)b, start_host, Sk);
    if (st > len) return;
    const int j_hi = min(NK, (len + blk - 1) / blk);
    for (int j = st / blk + w; j < j_hi; j += W) {
        const int rows = min(blk, len - j * blk);       // >= 1 below j_hi
        const KT* base;
        bool have = true;
        if (table) {
            const int page = table[b * table_stride_b + j];
            have = page >= 0 && page < num_pages;
            base = static_cast<const KT*>(k.ptr) + (long)(have ? page : 0) * k.stride_b + (long)hk * k.stride_h;
        } else {
            base = static_cast<const KT*>(k.ptr) + b * k.stride_b + (long)hk * k.stride_h + (long)j * blk * k.stride_s;
        }
        float2 mm = have ? sel_bounds_block<Tag>(base, k.stride_s, rows, D, redn, redx) : make_float2(0.f, 0.f);
        if constexpr (std::is_same<Tag, e4m3_tag>::value) {
            const float sc = k_scale[hk];
            mm.x *= sc, mm.y *= sc;
        }
        if (tid < D) {
            float* o = out + (bh * NK + j) * 2 * D + tid;
            o[0] = mm.x;
            o[D] = mm.y;
        }
    }
}

// ---- scores ----------------------------------------------------------------------------------------------------------------------
// Scores of the key blocks [lo, hi) of one list row as ordered keys into dst[j], by one workgroup.  L = D / 4 lanes share one
// pooled key row (a float4 each); a wave scores 64 / L key blocks per step.  kb: the pooled rows of (b, K/V head); qrow: the row's
// pooled query.
template <int L>
__device__ __forceinline__ void sel_score_blocks(const float* __restrict__ kb, const float* __restrict__ qrow, int lo, int hi,
                                                 unsigned* dst) {
    constexpr int D = 4 * L, RW = 64 / L, U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane % L, sub = lane / L;
    const float4 qv = *reinterpret_cast<const float4*>(qrow + cl * 4);
    kb += cl * 4;
    for (int j0 = lo + wave * RW; j0 < hi; j0 += 4 * RW * U) {
        float4 kv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 4 * RW + sub;
            kv[u] = j < hi ? *reinterpret_cast<const float4*>(kb + (long)j * D) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 4 * RW + sub;
            float p = fmaf(qv.w, kv[u].w, fmaf(qv.z, kv[u].z, fmaf(qv.y, kv[u].y, qv.x * kv[u].x)));
#pragma unroll
            for (int m = 1; m < L; m <<= 1) p += __shfl_xor(p, m, 64);
            if (cl == 0 && j < hi) dst[j] = sel_key(p);
        }
    }
}

// The bound scores of the key blocks [lo, hi) of one list row: sel_score_blocks over the bounds cache.  kb:
// the (min, max) row pairs of (b, K/V head), 2 D floats a block.  t = sum over d of max(q_d mn_d, q_d mx_d): per lane four terms,
// each the larger of two separately rounded fp32 products, added as ((x + y) + z) + w; the lanes meet over the same xor strides.
template <int L>
__device__ __forceinline__ void sel_bound_score_blocks(const float* __restrict__ kb, const float* __restrict__ qrow, int lo, int hi,
                                                       unsigned* dst) {
    constexpr int D = 4 * L, RW = 64 / L, U = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane % L, sub = lane / L;
    const float4 qv = *reinterpret_cast<const float4*>(qrow + cl * 4);
    kb += cl * 4;
    for (int j0 = lo + wave * RW; j0 < hi; j0 += 4 * RW * U) {
        float4 mn[U], mx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 4 * RW + sub;
            mn[u] = j < hi ? *reinterpret_cast<const float4*>(kb + (long)j * 2 * D) : make_float4(0.f, 0.f, 0.f, 0.f);
            mx[u] = j < hi ? *reinterpret_cast<const float4*>(kb + (long)j * 2 * D + D) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * 4 * RW + sub;
            float p = ((fmaxf(qv.x * mn[u].x, qv.x * mx[u].x) + fmaxf(qv.y * mn[u].y, qv.y * mx[u].y)) +
                       fmaxf(qv.z * mn[u].z, qv.z * mx[u].z)) + fmaxf(qv.w * mn[u].w, qv.w * mx[u].w);
#pragma unroll
            for (int m = 1; m < L; m <<= 1) p += __shfl_xor(p, m, 64);
            if (cl == 0 && j < hi) dst[j] = sel_key(p);
        }
    }
}

// The score pass of the pooled selection spread over `splits` workgroups per list row: workgroup (row, part) writes the keys of
// its slice of the visible blocks to wkeys[row, :].  BOUND: kbar is the bounds cache kbounds [B, Hkv, NK, 2, D] and the scores are
// the bound selection's, at every `splits`.
template <int L, bool BOUND, typename Rows>
__global__ __launch_bounds__(SEL_NT) void block_score_kernel(const float* __restrict__ kbar, const float* __restrict__ qsum, int Hkv,
                                                             int Hl, int Sq, int Sk, int blk, int NQ, int NK, int splits,
                                                             const int32_t* __restrict__ kv_len, int kv_valid, int causal,
                                                             unsigned* __restrict__ wkeys, Rows src) {
    constexpr int D = 4 * L;
    const int part = (int)(blockIdx.x % (unsigned)splits);
    const long row = blockIdx.x / (unsigned)splits;
    const int i = (int)(row % NQ);
    const long bh = row / NQ;
    const int hl = (int)(bh % Hl);
    const long b = bh / Hl;
    const int hk = hl / (Hl / Hkv);
    const int nvis = sel_visible<Rows::SHORT>(sel_key_limit(kv_len, (int)b, kv_valid, Sk), src.count((int)b, Sq), blk, NK, i, causal);
    const int chunk = (NK + splits - 1) / splits;
    const int lo = part * chunk, hi = min(lo + chunk, nvis);
    if constexpr (BOUND) sel_bound_score_blocks<L>(kbar + ((b * Hkv + hk) * NK) * 2 * D, qsum + row * D, lo, hi, wkeys + row * NK);
    else sel_score_blocks<L>(kbar + ((b * Hkv + hk) * NK) * D, qsum + row * D, lo, hi, wkeys + row * NK);
}

// ---- select ----------------------------------------------------------------------------------------------------------------------
// The rows the select kernels are launched over.
struct sel_rows {
    const float* kbar;
    const float* qsum;
    const unsigned* wkeys;      // NULL: the select workgroup computes its scores
    int Hkv, Hl, Sq, Sk, blk, NQ, NK;
    const int32_t* kv_len;
    int kv_valid, causal, top_k, keep_first, keep_local;
    uint32_t* bitmask;
    int32_t* cols;
    int32_t* counts;
    float* scores;
};

struct SelForced {      // the forced blocks of a row: [0, kf) and [flo, fhi]
    int kf, flo, fhi;
    __device__ __forceinline__ bool operator()(int j) const { return j < kf || (j >= flo && j <= fhi); }
};

// The weight of the block with ordered key `key` in a row whose best visible score is tmax.  A NaN (non-finite scores) weighs 0.
__device__ __forceinline__ unsigned selp_weight(unsigned key, float tmax, float c) {
    const float a = (sel_unkey(key) - tmax) * c;
    const float x = __builtin_amdgcn_exp2f(a) * (float)SELP_ONE + 0.5f;
    return x >= 1.f ? (unsigned)fminf(x, (float)SELP_ONE) : 0u;
}

// Sums of a and of b over the workgroup, in every thread (red: 8 words).
__device__ __forceinline__ uint2 selp_sum2(unsigned a, unsigned b, unsigned* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m, 64);
        b += __shfl_xor(b, m, 64);
    }
    __syncthreads();    // (red may still be read from the previous sum)
    if (lane == 0) {
        red[2 * wave] = a;
        red[2 * wave + 1] = b;
    }
    __syncthreads();
    return make_uint2(red[0] + red[2] + red[4] + red[6], red[1] + red[3] + red[5] + red[7]);
}

// The radix select over the unforced visible keys, 8 bits a pass, on weights (MASS) or on counts (every block weighs 1): the key T
// at which the running sum over the ranking first reaches rem (0 < rem <= the sum over all of them), and what of rem is left for
// the blocks that tie at T.
template <bool MASS>
__device__ __forceinline__ void sel_radix(const unsigned* keys, int nvis, SelForced forced, float tmax, float c, unsigned rem,
                                          unsigned* hist, unsigned* wsum, unsigned* pick, unsigned& T, unsigned& left) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        const unsigned himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int j = tid; j < nvis; j += SEL_NT) {
            const unsigned key = keys[j];
            if (!forced(j) && (key & himask) == prefix) {
                const unsigned u = MASS ? selp_weight(key, tmax, c) : 1u;
                if (u) atomicAdd(&hist[(key >> shift) & 255u], u);
            }
        }
        __syncthreads();
        // thread t owns digit 255 - t: its inclusive prefix over t sums the keys with that digit or a higher one
        const unsigned h = hist[255 - tid];
        unsigned inc = h;
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned o = __shfl_up(inc, m, 64);
            if (lane >= m) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        for (int w = 0; w < wave; ++w) inc += wsum[w];
        if (inc - h < rem && rem <= inc) {      // exactly one thread: the digit in which the sum reaches rem
            pick[0] = prefix | ((unsigned)(255 - tid) << shift);
            pick[1] = rem - (inc - h);
        }
        __syncthreads();
        prefix = pick[0];
        rem = pick[1];
    }
    T = prefix;
    left = rem;
}

// One list row by one workgroup.  LOADED = 0: the scores are computed here (r.kbar, r.qsum); LOADED = 1: their keys are loaded from
// r.wkeys (block_score_kernel).  BUDGET = false: top-k (p16, c and mass are not read); true: top-p capped at top_k.
template <int L, int LOADED, bool BUDGET, bool SHORT>
__device__ __forceinline__ void sel_row_body(const sel_rows& r, int p16, float c, float* __restrict__ mass,
                                             const int32_t* __restrict__ q_len) {
    extern __shared__ unsigned keys[];              // [NK]: the scores of the visible blocks as ordered keys
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[4];
    __shared__ unsigned pick[2];
    __shared__ int step_eq[SEL_MAX_STEPS], step_kept[SEL_MAX_STEPS];
    __shared__ unsigned long long step_mask[SEL_MAX_STEPS];
    constexpr int D = 4 * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = r.blk, NK = r.NK;
    const long row = blockIdx.x;
    const int i = (int)(row % r.NQ);
    const long bh = row / r.NQ;
    const int hl = (int)(bh % r.Hl);
    const long b = bh / r.Hl;
    const int hk = hl / (r.Hl / r.Hkv);
    const int len = sel_key_limit(r.kv_len, (int)b, r.kv_valid, r.Sk);
    const int Sq = SHORT ? RowsCounted{q_len}.count((int)b, r.Sq) : r.Sq;      // the batch item's rows: r1 and off count from them

    // 1. visible blocks: a prefix [0, nvis) of the row; forced blocks: [0, kf) and [flo, fhi] within it
    const long r0 = (long)i * blk, r1 = min(r0 + blk, (long)Sq) - 1, off = (long)len - Sq;
    const int nvis = sel_visible<SHORT>(len, Sq, blk, NK, i, r.causal);
    SelForced forced = {min(r.keep_first, nvis), 1, 0};
    if (r.keep_local >= 1 && nvis > 0) {
        const long jd_lo = max(r0 + off, 0L) / blk, jd_hi = min(max(r1 + off, 0L), (long)len - 1) / blk;
        const long ext = min(r.keep_local - 1, SEL_MAX_NK);
        forced.flo = (int)max(jd_lo - ext, 0L);
        forced.fhi = (int)min(r.causal ? jd_hi : jd_hi + ext, (long)nvis - 1);
    }
    const int nf = forced.kf + max(0, forced.fhi - max(forced.flo, forced.kf) + 1);

    // 2. scores of the visible blocks
    if (LOADED) {
        const unsigned* wr = r.wkeys + row * NK;
        for (int j = tid; j < nvis; j += SEL_NT) keys[j] = wr[j];
    } else {
        sel_score_blocks<L>(r.kbar + ((b * r.Hkv + hk) * NK) * D, r.qsum + row * D, 0, nvis, keys);
    }
    __syncthreads();
    if (r.scores) {
        float* sr = r.scores + row * NK;
        for (int j = tid; j < NK; j += SEL_NT) sr[j] = j < nvis ? sel_unkey(keys[j]) : -INFINITY;
    }

    // 3. the decision (uniform over the workgroup): every unforced visible block (take_all), or with `cut` those above key T and,
    // of those that tie at T, the need_eq lowest; neither: the forced blocks alone.  n_k: what top_k leaves for unforced blocks.
    const int nunf = nvis - nf, n_k = max(r.top_k - nf, 0);
    bool take_all = false, cut;
    unsigned T = 0u, left;
    int need_eq = 0;
    if constexpr (!BUDGET) {
        take_all = n_k >= nunf;
        cut = !take_all && n_k > 0;
        if (cut) {      // the key of the n_k-th best unforced visible block
            sel_radix<false>(keys, nvis, forced, 0.f, 0.f, (unsigned)n_k, hist, wsum, pick, T, left);
            need_eq = (int)left;
        }
    } else {
        // t_max over the visible blocks, on the keys; then the row's total weight and the weight of its forced blocks
        __shared__ unsigned red[8];
        unsigned kmax = 0u;
        for (int j = tid; j < nvis; j += SEL_NT) kmax = max(kmax, keys[j]);
        for (int m = 32; m >= 1; m >>= 1) kmax = max(kmax, __shfl_xor(kmax, m, 64));
        if (lane == 0) red[wave] = kmax;
        __syncthreads();
        const float tmax = sel_unkey(max(max(red[0], red[1]), max(red[2], red[3])));
        unsigned part = 0u, fpart = 0u;
        for (int j = tid; j < nvis; j += SEL_NT) {
            const unsigned u = selp_weight(keys[j], tmax, c);
            part += u;
            if (forced(j)) fpart += u;
        }
        const uint2 sums = selp_sum2(part, fpart, red);
        const unsigned total = sums.x, fmass = sums.y;
        const unsigned target = (unsigned)(((unsigned long long)total * (unsigned)p16 + 65535ull) >> 16);      // <= total
        cut = fmass < target && n_k > 0;
        if (cut) {      // (target <= total: the unforced blocks hold target - fmass, so the sum reaches it)
            sel_radix<true>(keys, nvis, forced, tmax, c, target - fmass, hist, wsum, pick, T, left);
            const unsigned uT = selp_weight(T, tmax, c);        // > 0: its digit held weight in every pass
            need_eq = (int)((left + uT - 1u) / uT);
            if (n_k < nunf) {       // the cap may bind: n_p = #{key > T} + need_eq against n_k
                unsigned above = 0u;
                for (int j = tid; j < nvis; j += SEL_NT) above += (!forced(j) && keys[j] > T) ? 1u : 0u;
                const unsigned n_p = selp_sum2(above, 0u, red).x + (unsigned)need_eq;
                if (n_p > (unsigned)n_k) {
                    sel_radix<false>(keys, nvis, forced, tmax, c, (unsigned)n_k, hist, wsum, pick, T, left);
                    need_eq = (int)left;
                }
            }
        }
        if (mass) {     // float(sum of the kept weights) / float(total); a row that sees nothing: 0
            unsigned kpart = 0u;
            if (cut)
                for (int j = tid; j < nvis; j += SEL_NT) kpart += (!forced(j) && keys[j] > T) ? selp_weight(keys[j], tmax, c) : 0u;
            const unsigned kmass = fmass + selp_sum2(kpart, 0u, red).x + (cut ? (unsigned)need_eq * selp_weight(T, tmax, c) : 0u);
            if (tid == 0) mass[row] = total ? (float)kmass / (float)total : 0.f;
        }
    }

    // 4. the lists, in 64-block ballot steps: wave w takes steps w, w + 4, ...
    const int nsteps = (NK + 63) >> 6, NW = (NK + 31) >> 5;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int s = wave; s < nsteps; s += 4) {
        const int j = s * 64 + lane;
        const bool eq = cut && j < nvis && !forced(j) && keys[j] == T;
        const unsigned long long m = __ballot(eq);
        if (lane == 0) step_eq[s] = __popcll(m);
    }
    __syncthreads();
    if (wave == 0) sel_wave_scan(step_eq, nsteps, lane);
    __syncthreads();
    uint32_t* wr = r.bitmask + row * NW;
    for (int s = wave; s < nsteps; s += 4) {
        const int j = s * 64 + lane;
        const bool vis = j < nvis, f = vis && forced(j);
        const unsigned key = vis ? keys[j] : 0u;
        const bool eq = cut && vis && !f && key == T;
        const unsigned long long me = __ballot(eq);
        const bool kept = f || (vis && (take_all || (cut && key > T))) || (eq && step_eq[s] + __popcll(me & below) < need_eq);
        const unsigned long long m = __ballot(kept);
        if (lane < 2 && 2 * s + lane < NW) wr[2 * s + lane] = lane ? (unsigned)(m >> 32) : (unsigned)m;
        if (lane == 0) {
            step_mask[s] = m;
            step_kept[s] = __popcll(m);
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int total = sel_wave_scan(step_kept, nsteps, lane);
        if (lane == 0) r.counts[row] = total;
    }
    __syncthreads();
    int32_t* cr = r.cols + row * NK;
    for (int s = wave; s < nsteps; s += 4) {
        const unsigned long long m = step_mask[s];
        if ((m >> lane) & 1ull) cr[step_kept[s] + __popcll(m & below)] = s * 64 + lane;
    }
}

template <int L, int LOADED, typename Rows>
__global__ __launch_bounds__(SEL_NT) void block_select_kernel(const sel_rows r, Rows src) {
    sel_row_body<L, LOADED, false, Rows::SHORT>(r, 0, 0.f, nullptr, src.counts());
}

template <int L, int LOADED, typename Rows>
__global__ __launch_bounds__(SEL_NT) void block_select_p_kernel(const sel_rows r, int p16, float c, float* __restrict__ mass, Rows src) {
    sel_row_body<L, LOADED, true, Rows::SHORT>(r, p16, c, mass, src.counts());
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The budget of the top-p selection: p16 = round(top_p * 65536) in [0, 65536], c = float(score_scale * log2(e)) finite and > 0,
// mass NULL or fp32 [B * Hl * NQ].
struct sel_top_p {
    int p16;
    float c;
    float* mass;
};

// The one place that maps the head dimension to L = D / 4 lanes per pooled row: f(std::integral_constant<int, L>).
template <typename F>
static void sel_with_lanes(int D, F f) {
    switch (D) {
        case 16: f(std::integral_constant<int, 4>()); break;
        case 32: f(std::integral_constant<int, 8>()); break;
        case 64: f(std::integral_constant<int, 16>()); break;
        default: f(std::integral_constant<int, 32>()); break;
    }
}

// The one place that maps a call's row counts to the row source its kernels run over: f(RowsCounted) with q_len (the ragged
// entries' counts, or the scan's for the packed ones), f(RowsPadded) without.
template <typename F>
static void sel_with_rows(const int32_t* q_len, F f) {
    if (q_len) f(RowsCounted{q_len});
    else f(RowsPadded{});
}

// The select kernel over `rows` list rows: LOADED from r.wkeys, the top-p kernel with a budget.
static int sel_launch_select(int D, long rows, const sel_rows& r, const sel_top_p* p, const int32_t* q_len, hipStream_t s) {
    const dim3 grid((unsigned)rows);
    const size_t lds = (size_t)r.NK * sizeof(unsigned);
    sel_with_lanes(D, [&](auto lanes) {
        sel_with_rows(q_len, [&](auto src) {
            constexpr int L = decltype(lanes)::value;
            using R = decltype(src);
            auto* top_p = r.wkeys ? block_select_p_kernel<L, 1, R> : block_select_p_kernel<L, 0, R>;
            auto* top_k = r.wkeys ? block_select_kernel<L, 1, R> : block_select_kernel<L, 0, R>;
            if (p) top_p<<<grid, SEL_NT, lds, s>>>(r, p->p16, p->c, p->mass, src);
            else top_k<<<grid, SEL_NT, lds, s>>>(r, src);
        });
    });
    return rsa_launch_status();
}

// The pool kernel over the query jobs of r's rows and k_jobs key jobs behind them (none: k and kbar are not touched).  row_start: the
// packed entry, q [T, H, D] behind stride_h and stride_s, item b from row row_start[b].
static int sel_launch_pool(int dtype, int H, int D, rsa_tensor4 q, rsa_tensor4 k, long q_jobs, long k_jobs, const sel_rows& r,
                           float* kbar, float* qsum, const int32_t* q_len, hipStream_t s, const int32_t* row_start = nullptr) {
    const dim3 grid((unsigned)(q_jobs + k_jobs));
    auto launch = [&](auto src, auto at) {
        using R = decltype(src);
        using A = decltype(at);
        auto* kernel = dtype == RSA_BF16 ? block_select_pool_kernel<bf16_tag, R, A> : block_select_pool_kernel<fp16_tag, R, A>;
        kernel<<<grid, SEL_NT, 0, s>>>(q, k, H, r.Hkv, r.Hl, r.Sq, r.Sk, D, r.blk, r.NQ, r.NK, q_jobs, r.kv_len, r.kv_valid, kbar, qsum,
                                       src, at);
    };
    if (row_start) launch(RowsCounted{q_len}, RowsAt{row_start});
    else sel_with_rows(q_len, [&](auto src) { launch(src, RowsPadded{}); });
    return rsa_launch_status();
}

// The workspace of the plain selection (the pooled queries and keys) or of the pooled one (the pooled queries, the ordered keys).
static int sel_sizes(bool pooled, int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    if (!bytes || B <= 0 || Hkv <= 0 || Hl <= 0 || NQ <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (D != 16 && D != 32 && D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (NK > SEL_MAX_NK) return RSA_ERR_UNSUPPORTED;     // K5's key-block limit
    const size_t q_jobs = (size_t)B * Hl * NQ, k_jobs = (size_t)B * Hkv * NK;     // one workgroup per job; pooled: per row and split
    if ((pooled ? q_jobs * SEL_MAX_SPLITS : q_jobs + k_jobs) > 0x7FFFFFFFull) return RSA_ERR_UNSUPPORTED;
    *bytes = pooled ? q_jobs * ((size_t)D * sizeof(float) + (size_t)NK * sizeof(unsigned)) : (q_jobs + k_jobs) * (size_t)D * sizeof(float);
    return RSA_OK;
}

// What rsa_block_select[_p] and rsa_block_select_pooled[_p] check alike, in the order that decides the status of a call that is
// wrong in two ways (the caller's own checks before it and behind it all return RSA_ERR_BAD_ARG).  cap: the keys the K side can
// hold, Sk or NK * block.
static int sel_check(bool pooled, int B, int H, int D, int dtype, rsa_tensor4 q, const sel_rows& r, const int32_t* q_len, long cap,
                     size_t* need) {
    if (B <= 0 || H <= 0 || r.Hkv <= 0 || r.Hl <= 0 || r.Sq <= 0) return RSA_ERR_BAD_ARG;
    if (H % r.Hkv || (r.Hl != r.Hkv && r.Hl != H)) return RSA_ERR_BAD_ARG;
    if (r.blk != 64 && r.blk != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 16 && D != 32 && D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (r.NQ != (int)(((long)r.Sq + r.blk - 1) / r.blk) || r.NK != (int)((cap + r.blk - 1) / r.blk)) return RSA_ERR_BAD_ARG;
    const int st = sel_sizes(pooled, B, r.Hkv, r.Hl, D, r.NQ, r.NK, need);
    if (st != RSA_OK) return st;
    if (r.top_k < 0 || r.keep_first < 0 || r.keep_local < 0) return RSA_ERR_BAD_ARG;
    if (!r.kv_len && (r.kv_valid < 0 || r.kv_valid > cap)) return RSA_ERR_BAD_ARG;
    if (!r.bitmask || !r.cols || !r.counts) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(q) != RSA_OK || q.stride_b < 0 || q.stride_h < 0 || q.stride_s < 0) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(r.bitmask) | reinterpret_cast<uintptr_t>(r.cols) | reinterpret_cast<uintptr_t>(r.counts) |
         reinterpret_cast<uintptr_t>(r.scores) | reinterpret_cast<uintptr_t>(r.kv_len) | reinterpret_cast<uintptr_t>(q_len)) & 3)
        return RSA_ERR_BAD_ARG;
    return RSA_OK;
}

static bool selp_budget_ok(const sel_top_p& p) {
    return p.p16 >= 0 && p.p16 <= 65536 && isfinite(p.c) && p.c > 0.f && !(reinterpret_cast<uintptr_t>(p.mass) & 3);
}

// The body of rsa_block_select and rsa_block_select_p (top_p NULL: top-k).  r: the call's arguments; kbar, qsum are set here.
static int sel_run(int B, int H, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, void* ws, size_t ws_bytes, sel_rows r,
                   const sel_top_p* top_p, const int32_t* q_len, void* stream) {
    if ((top_p && !selp_budget_ok(*top_p)) || r.Sk <= 0) return RSA_ERR_BAD_ARG;
    size_t need = 0;
    const int st = sel_check(false, B, H, D, dtype, q, r, q_len, r.Sk, &need);
    if (st != RSA_OK) return st;
    if (!ws || rsa_check_tensor(k) != RSA_OK || k.stride_b < 0 || k.stride_h < 0 || k.stride_s < 0) return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return RSA_ERR_BAD_ARG;
    if (ws_bytes < need) return RSA_ERR_WORKSPACE;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const long q_jobs = (long)B * r.Hl * r.NQ, k_jobs = (long)B * r.Hkv * r.NK;
    float* qsum = static_cast<float*>(ws);              // [B, Hl, NQ, D]
    float* kbar = qsum + q_jobs * D;                    // [B, Hkv, NK, D]
    r.kbar = kbar, r.qsum = qsum;
    const int rc = sel_launch_pool(dtype, H, D, q, k, q_jobs, k_jobs, r, kbar, qsum, q_len, s);
    return rc != RSA_OK ? rc : sel_launch_select(D, q_jobs, r, top_p, q_len, s);
}

extern "C" int rsa_block_select_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return sel_sizes(false, B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_p_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return sel_sizes(false, B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                                int keep_first, int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                                int32_t* counts, float* scores, void* stream) {
    return sel_run(B, H, D, dtype, q, k, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK, kv_len_dev, kv_valid,
                   causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores}, nullptr, nullptr, stream);
}

extern "C" int rsa_block_select_p(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                  rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                                  int keep_first, int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                                  int32_t* counts, float* scores, int p16, float c, float* mass, void* stream) {
    const sel_top_p p = {p16, c, mass};
    return sel_run(B, H, D, dtype, q, k, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK, kv_len_dev, kv_valid,
                   causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores}, &p, nullptr, stream);
}

// ---- the pooled-key cache ----------------------------------------------------------------------------------
// Both entries: kv8 = k holds e4m3 codes (no dtype; head dims 64 / 128; 8-byte loads) and k_scale is there.  bounds: the entries of
// the bounds cache (section 5.19), whose out holds 2 D floats a block: the same checks and grid, pool_key_bounds_kernel.
static int sel_pool_keys_run(bool kv8, bool bounds, int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k,
                             const int32_t* block_table, int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev,
                             int kv_valid, const int32_t* start_dev, int start, int workgroups_per_head, float* out,
                             const float* k_scale, void* stream) {
    if (B <= 0 || Hkv <= 0 || Sk <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (!kv8 && dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (kv8 ? (D != 64 && D != 128) : (D != 16 && D != 32 && D != 64 && D != 128)) return RSA_ERR_UNSUPPORTED;
    if (NK != (int)(((long)Sk + block - 1) / block)) return RSA_ERR_BAD_ARG;
    if (NK > SEL_MAX_NK) return RSA_ERR_UNSUPPORTED;
    if (!kv_len_dev && (kv_valid < 0 || kv_valid > Sk)) return RSA_ERR_BAD_ARG;
    if (!start_dev && (start < 0 || start > Sk)) return RSA_ERR_BAD_ARG;
    if (workgroups_per_head < 0) return RSA_ERR_BAD_ARG;
    if (!out || !k.ptr) return RSA_ERR_BAD_ARG;
    if (kv8) {      // (strides in bytes: 8 of them per lane and load)
        if (!k_scale || (reinterpret_cast<uintptr_t>(k_scale) & 3)) return RSA_ERR_BAD_ARG;
        if ((reinterpret_cast<uintptr_t>(k.ptr) & 7) || (k.stride_b % 8) || (k.stride_h % 8) || (k.stride_s % 8)) return RSA_ERR_BAD_ARG;
    } else if (rsa_check_tensor(k) != RSA_OK) {
        return RSA_ERR_BAD_ARG;
    }
    if (k.stride_b < 0 || k.stride_h < 0 || k.stride_s < 0) return RSA_ERR_BAD_ARG;
    if (block_table && (num_pages <= 0 || table_stride_b < 0)) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(kv_len_dev) | reinterpret_cast<uintptr_t>(start_dev)) & 3)
        return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(out) & 15) return RSA_ERR_BAD_ARG;       // (the selection reads the cache 16 bytes a lane)
    int W = workgroups_per_head;
    if (W == 0) {   // the exact count with two host limits; every block with start 0; else the two an append of <= block keys touches
        if (!kv_len_dev && !start_dev) W = start > kv_valid ? 1 : max(1, (kv_valid + block - 1) / block - start / block);
        else W = (!start_dev && start == 0) ? NK : 2;
    }
    W = min(W, NK);
    if ((size_t)B * Hkv * W > 0x7FFFFFFFull) return RSA_ERR_UNSUPPORTED;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((size_t)B * Hkv * W));
    auto* kernel = kv8 ? pool_keys_kernel<e4m3_tag> : dtype == RSA_BF16 ? pool_keys_kernel<bf16_tag> : pool_keys_kernel<fp16_tag>;
    if (bounds)
        kernel = kv8 ? pool_key_bounds_kernel<e4m3_tag>
                     : dtype == RSA_BF16 ? pool_key_bounds_kernel<bf16_tag> : pool_key_bounds_kernel<fp16_tag>;
    kernel<<<grid, SEL_NT, 0, s>>>(k, Hkv, Sk, D, block, NK, W, kv_len_dev, kv_valid, start_dev, start, block_table,
                                   (long)table_stride_b, num_pages, out, k_scale);     // (k_scale: NULL unless kv8)
    return rsa_launch_status();
}

extern "C" int rsa_pool_keys(int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                             int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid,
                             const int32_t* start_dev, int start, int workgroups_per_head, float* out, void* stream) {
    return sel_pool_keys_run(false, false, B, Hkv, Sk, D, dtype, block, NK, k, block_table, table_stride_b, num_pages, kv_len_dev, kv_valid,
                             start_dev, start, workgroups_per_head, out, nullptr, stream);
}

// The cache from an e4m3 K: per block the fp32 sum of float(code) in sel_pool_block's order, divided once
// by the count, multiplied once by k_scale[hk] (DEVICE fp32 [Hkv]).
extern "C" int rsa_pool_keys_kv8(int B, int Hkv, int Sk, int D, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                                 int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid,
                                 const int32_t* start_dev, int start, int workgroups_per_head, float* out, const float* k_scale,
                                 void* stream) {
    return sel_pool_keys_run(true, false, B, Hkv, Sk, D, 0, block, NK, k, block_table, table_stride_b, num_pages, kv_len_dev, kv_valid,
                             start_dev, start, workgroups_per_head, out, k_scale, stream);
}

// The bounds cache: rsa_pool_keys' and rsa_pool_keys_kv8's argument lists; out fp32 [B, Hkv, NK, 2, D].
extern "C" int rsa_pool_key_bounds(int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k,
                                   const int32_t* block_table, int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev,
                                   int kv_valid, const int32_t* start_dev, int start, int workgroups_per_head, float* out,
                                   void* stream) {
    return sel_pool_keys_run(false, true, B, Hkv, Sk, D, dtype, block, NK, k, block_table, table_stride_b, num_pages, kv_len_dev,
                             kv_valid, start_dev, start, workgroups_per_head, out, nullptr, stream);
}

extern "C" int rsa_pool_key_bounds_kv8(int B, int Hkv, int Sk, int D, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                                       int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid,
                                       const int32_t* start_dev, int start, int workgroups_per_head, float* out,
                                       const float* k_scale, void* stream) {
    return sel_pool_keys_run(true, true, B, Hkv, Sk, D, 0, block, NK, k, block_table, table_stride_b, num_pages, kv_len_dev, kv_valid,
                             start_dev, start, workgroups_per_head, out, k_scale, stream);
}

// The library's choice of score_splits, a function of the shapes alone (measured: profiles/pooled_select_perf.txt).
// One pass of sel_score_blocks' loop per score workgroup (4096 / D key blocks: 32 at D = 128), which is the best or within the
// baseline's spread of the best at both measured row counts (8 rows x 1024 blocks: 32 splits; 64 rows x 256 blocks: 8); at most 64
// splits and about 1024 workgroups, and none where the list rows alone give two workgroups per compute unit (not measured there).
// The bound selection (section 5.19) takes the same choice: at both row counts it is the best split count measured for it too
// (profiles/select_bound_perf.txt).
static int sel_default_splits(size_t rows, int NK, int D) {
    if (rows >= 512) return 1;
    const int pass = 4096 / D;
    const int by_blocks = (NK + pass - 1) / pass, by_rows = (int)((1024 + rows - 1) / rows);
    return max(1, min(min(by_blocks, by_rows), 64));
}

// The packed entry's batch: T rows of q, cu_seqlens_q and the scratch of 2 (B + 1) int32 the scan writes.
struct SelPacked {
    int T;
    const int32_t* cu;
    int32_t* items;
};

// The body of rsa_block_select_pooled and rsa_block_select_pooled_p (top_p NULL: top-k).  r: the call's arguments; Sk, kbar, qsum
// and wkeys are set here.  pk: the packed entry (r.Sq = M; q_len is then set here, to the scan's row counts).  bound: pooled_k is the
// bounds cache (section 5.19) -- the score pass is then block_score_kernel<L, true> at every split count, one included, and the select
// kernels run LOADED: they gain no form of their own.
static int sel_pooled_run(int B, int H, int D, int dtype, rsa_tensor4 q, const float* pooled_k, int score_splits, void* ws,
                          size_t ws_bytes, sel_rows r, const sel_top_p* top_p, const int32_t* q_len, void* stream,
                          const SelPacked* pk = nullptr, bool bound = false) {
    if ((top_p && !selp_budget_ok(*top_p)) || r.NK <= 0) return RSA_ERR_BAD_ARG;
    if (pk) {
        if (pk->T <= 0 || r.Sq <= 0 || r.Sq > pk->T || !pk->cu || !pk->items || B >= 0x7FFFFFFF) return RSA_ERR_BAD_ARG;
        if ((reinterpret_cast<uintptr_t>(pk->cu) | reinterpret_cast<uintptr_t>(pk->items)) & 3) return RSA_ERR_BAD_ARG;
        q.stride_b = 0;
        q_len = pk->items + B + 1;
    }
    size_t need = 0;
    const int st = sel_check(true, B, H, D, dtype, q, r, q_len, (long)r.NK * r.blk, &need);
    if (st != RSA_OK) return st;
    if (score_splits < 0 || score_splits > SEL_MAX_SPLITS || !ws || !pooled_k) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(pooled_k)) & 15) return RSA_ERR_BAD_ARG;
    if (ws_bytes < need) return RSA_ERR_WORKSPACE;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const long q_jobs = (long)B * r.Hl * r.NQ;
    const int splits = min(score_splits ? score_splits : sel_default_splits((size_t)q_jobs, r.NK, D), r.NK);
    float* qsum = static_cast<float*>(ws);                              // [B, Hl, NQ, D]
    unsigned* wkeys = reinterpret_cast<unsigned*>(qsum + q_jobs * D);   // [B, Hl, NQ, NK]
    r.Sk = r.NK * r.blk;        // the capacity of the cache
    r.kbar = pooled_k, r.qsum = qsum, r.wkeys = (bound || splits > 1) ? wkeys : nullptr;
    if (pk) pk_scan_launch(pk->cu, B, pk->T, r.Sq, r.blk, 0, 0, pk->items, pk->items + B + 1, nullptr, s);
    int rc = sel_launch_pool(dtype, H, D, q, q, q_jobs, 0, r, nullptr, qsum, q_len, s, pk ? pk->items : nullptr);    // the pooled queries
    if (rc != RSA_OK) return rc;
    if (bound || splits > 1) {
        const dim3 grid((unsigned)(q_jobs * splits));
        sel_with_lanes(D, [&](auto lanes) {
            sel_with_rows(q_len, [&](auto src) {
                constexpr int L = decltype(lanes)::value;
                using R = decltype(src);
                auto* kernel = bound ? block_score_kernel<L, true, R> : block_score_kernel<L, false, R>;
                kernel<<<grid, SEL_NT, 0, s>>>(pooled_k, qsum, r.Hkv, r.Hl, r.Sq, r.Sk, r.blk, r.NQ, r.NK, splits, r.kv_len, r.kv_valid,
                                               r.causal, wkeys, src);
            });
        });
        rc = rsa_launch_status();
        if (rc != RSA_OK) return rc;
    }
    return sel_launch_select(D, q_jobs, r, top_p, q_len, s);
}

extern "C" int rsa_block_select_pooled_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return sel_sizes(true, B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_pooled_p_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return sel_sizes(true, B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_pooled(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK,
                                       rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal,
                                       int top_k, int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes,
                                       uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, void* stream) {
    return sel_pooled_run(B, H, D, dtype, q, pooled_k, score_splits, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, 0, block, NQ,
                          NK, kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores}, nullptr,
                          nullptr, stream);
}

extern "C" int rsa_block_select_pooled_p(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK,
                                         rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid,
                                         int causal, int top_k, int keep_first, int keep_local, int score_splits, void* ws,
                                         size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                                         int p16, float c, float* mass, void* stream) {
    const sel_top_p p = {p16, c, mass};
    return sel_pooled_run(B, H, D, dtype, q, pooled_k, score_splits, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, 0, block, NQ,
                          NK, kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores}, &p,
                          nullptr, stream);
}

// ---- ragged selection: a row count per batch item.  The _p entries' argument lists with q_len_dev, DEVICE
// int32 [B] (clamped into [0, Sq] on the device; NULL: the existing entry's call), in front of the stream; p16 = -1: plain top-k
// (c and mass are then not read).
extern "C" int rsa_block_select_ragged(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                       rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                                       int keep_first, int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                                       int32_t* counts, float* scores, int p16, float c, float* mass, const int32_t* q_len_dev,
                                       void* stream) {
    const sel_top_p p = {p16, c, mass};
    return sel_run(B, H, D, dtype, q, k, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK, kv_len_dev, kv_valid,
                   causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores}, p16 == -1 ? nullptr : &p, q_len_dev,
                   stream);
}

extern "C" int rsa_block_select_pooled_ragged(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK,
                                              rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid,
                                              int causal, int top_k, int keep_first, int keep_local, int score_splits, void* ws,
                                              size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                                              int p16, float c, float* mass, const int32_t* q_len_dev, void* stream) {
    const sel_top_p p = {p16, c, mass};
    return sel_pooled_run(B, H, D, dtype, q, pooled_k, score_splits, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, 0, block, NQ,
                          NK, kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores},
                          p16 == -1 ? nullptr : &p, q_len_dev, stream);
}

// ---- packed selection: q [T, H, D] with cu_seqlens_q.  rsa_block_select_pooled_ragged's argument list with
// T in front, M = max_q_len where Sq stood (NQ = ceil(M / block)), and cu_seqlens_q_dev, DEVICE int32 [B + 1], with item_ws, DEVICE
// int32 [2 (B + 1)] scratch, where q_len_dev stood.  One launch more than the ragged entry: the scan.
extern "C" int rsa_block_select_pooled_packed(int T, int B, int H, int Hkv, int Hl, int max_q_len, int D, int dtype, int block, int NQ,
                                              int NK, rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid,
                                              int causal, int top_k, int keep_first, int keep_local, int score_splits, void* ws,
                                              size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                                              int p16, float c, float* mass, const int32_t* cu_seqlens_q_dev, int32_t* item_ws,
                                              void* stream) {
    const sel_top_p p = {p16, c, mass};
    const SelPacked pk = {T, cu_seqlens_q_dev, item_ws};
    return sel_pooled_run(B, H, D, dtype, q, pooled_k, score_splits, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, max_q_len, 0,
                          block, NQ, NK, kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores},
                          p16 == -1 ? nullptr : &p, nullptr, stream, &pk);
}

// ---- bound selection: the selection from the bounds cache.  rsa_block_select_pooled_ragged's and
// rsa_block_select_pooled_packed's argument lists and statuses; pooled_k is the bounds cache, fp32 [B, Hkv, NK, 2, D].  p16 = -1:
// plain top-k; q_len_dev NULL: every item has Sq rows.
extern "C" int rsa_block_select_bound_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return sel_sizes(true, B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_bound(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                                      const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                                      int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask,
                                      int32_t* cols, int32_t* counts, float* scores, int p16, float c, float* mass,
                                      const int32_t* q_len_dev, void* stream) {
    const sel_top_p p = {p16, c, mass};
    return sel_pooled_run(B, H, D, dtype, q, pooled_k, score_splits, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, Sq, 0, block, NQ,
                          NK, kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores},
                          p16 == -1 ? nullptr : &p, q_len_dev, stream, nullptr, true);
}

extern "C" int rsa_block_select_bound_packed(int T, int B, int H, int Hkv, int Hl, int max_q_len, int D, int dtype, int block, int NQ,
                                             int NK, rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid,
                                             int causal, int top_k, int keep_first, int keep_local, int score_splits, void* ws,
                                             size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                                             int p16, float c, float* mass, const int32_t* cu_seqlens_q_dev, int32_t* item_ws,
                                             void* stream) {
    const sel_top_p p = {p16, c, mass};
    const SelPacked pk = {T, cu_seqlens_q_dev, item_ws};
    return sel_pooled_run(B, H, D, dtype, q, pooled_k, score_splits, ws, ws_bytes, {nullptr, nullptr, nullptr, Hkv, Hl, max_q_len, 0,
                          block, NQ, NK, kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols, counts, scores},
                          p16 == -1 ? nullptr : &p, nullptr, stream, &pk, true);
}
