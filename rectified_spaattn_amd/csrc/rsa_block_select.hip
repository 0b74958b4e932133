// Top-k block selection per list head on the device (include/rsa.h: rsa_block_select_bytes, rsa_block_select; DESIGN.md
// section 5.11).  Two kernels, both plain HIP C++ for wave64:
//
//   block_select_pool_kernel   one workgroup per (b, list head, query block) and per (b, K/V head, key block): the fp32 mean of
//                              the block's rows per channel.  q and k are read exactly once, 16 bytes per lane and load.  The
//                              query side adds the means of the list head's query heads in ascending order (H / Hl of them).
//   block_select_kernel        one 256-thread workgroup per list row (b, list head, query block): the pooled scores of the
//                              visible key blocks into LDS as order-preserving 32-bit keys, the k-th best by a radix select over
//                              LDS histograms (8 bits a pass), ties to the lower block index by ballot / prefix popcount, and the
//                              list contract of rsa_block_mask.hip (bitmask, ascending cols, counts) in 64-block ballot steps.
//
// The pooled-key cache (rsa_pool_keys, rsa_block_select_pooled_bytes, rsa_block_select_pooled) runs the
// same device code: sel_pool_mean, sel_score_blocks and the select body below exist once.
//
//   pool_keys_kernel           W workgroups per (b, K/V head) stride over the key blocks [start / block, ceil(len / block)) and
//                              write sel_pool_mean of each, read directly or through a block table, into the fp32 cache
//   block_score_kernel         `splits` workgroups per list row: each writes its slice of the row's ordered keys to the workspace
//                              (a lane group computes a whole score: nothing is summed across workgroups)
//   block_select_kernel<L, 1>  the select body over keys loaded from that workspace instead of computed
//
// Every sum has a fixed order (no floating-point atomics; the histograms count integers): two calls give the same bytes.
//
// The score-and-select device functions live in rsa_block_select.h, which the top-p selection (rsa_block_select_p.hip, DESIGN.md
// section 5.15) includes too; the host bodies sel_run / sel_pooled_run serve both and hand the select launch to it with a budget.
#include "rsa_block_select.h"

#include <type_traits>

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

template <typename Tag>
__global__ __launch_bounds__(SEL_NT) void block_select_pool_kernel(rsa_tensor4 q, rsa_tensor4 k, int H, int Hkv, int Hl, int Sq,
                                                                   int Sk, int D, int blk, int NQ, int NK, long q_jobs,
                                                                   const int32_t* __restrict__ kv_len, int kv_valid,
                                                                   float* __restrict__ kbar, float* __restrict__ qsum) {
    __shared__ float red[4][128];
    const int tid = threadIdx.x;
    long job = blockIdx.x;
    if (job < q_jobs) {
        const int i = (int)(job % NQ);
        const long bh = job / NQ;
        const int hl = (int)(bh % Hl), gl = H / Hl;
        const long b = bh / Hl;
        const long r0 = (long)i * blk;
        const int rows = (int)min((long)blk, (long)Sq - r0);
        const float cnt = (float)rows;
        float tot = 0.f;
        for (int u = 0; u < gl; ++u) {      // the list head's query heads, ascending: each head's own mean, then the sum
            const unsigned short* base = static_cast<const unsigned short*>(q.ptr) + b * q.stride_b +
                                         (long)(hl * gl + u) * q.stride_h + r0 * q.stride_s;
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

// ---- score and select ------------------------------------------------------------------------------------------------------------
// The score pass of the pooled selection spread over `splits` workgroups per list row: workgroup (row, part) writes the keys of
// its slice of the visible blocks to wkeys[row, :].
template <int L>
__global__ __launch_bounds__(SEL_NT) void block_score_kernel(const float* __restrict__ kbar, const float* __restrict__ qsum, int Hkv,
                                                             int Hl, int Sq, int Sk, int blk, int NQ, int NK, int splits,
                                                             const int32_t* __restrict__ kv_len, int kv_valid, int causal,
                                                             unsigned* __restrict__ wkeys) {
    constexpr int D = 4 * L;
    const int part = (int)(blockIdx.x % (unsigned)splits);
    const long row = blockIdx.x / (unsigned)splits;
    const int i = (int)(row % NQ);
    const long bh = row / NQ;
    const int hl = (int)(bh % Hl);
    const long b = bh / Hl;
    const int hk = hl / (Hl / Hkv);
    const int nvis = sel_visible(sel_key_limit(kv_len, (int)b, kv_valid, Sk), Sq, blk, NK, i, causal);
    const int chunk = (NK + splits - 1) / splits;
    const int lo = part * chunk, hi = min(lo + chunk, nvis);
    sel_score_blocks<L>(kbar + ((b * Hkv + hk) * NK) * D, qsum + row * D, lo, hi, wkeys + row * NK);
}

// LOADED = 0: the scores are computed here (kbar, qsum); LOADED = 1: their keys are loaded from wkeys [rows, NK] (block_score_kernel).
template <int L, int LOADED>
__global__ __launch_bounds__(SEL_NT) void block_select_kernel(const float* __restrict__ kbar, const float* __restrict__ qsum,
                                                              const unsigned* __restrict__ wkeys,
                                                              int Hkv, int Hl, int Sq, int Sk, int blk, int NQ, int NK,
                                                              const int32_t* __restrict__ kv_len, int kv_valid, int causal,
                                                              int top_k, int keep_first, int keep_local,
                                                              uint32_t* __restrict__ bitmask, int32_t* __restrict__ cols,
                                                              int32_t* __restrict__ counts, float* __restrict__ scores) {
    extern __shared__ unsigned keys[];              // [NK]: the scores of the visible blocks as ordered keys
    __shared__ int hist[256];
    __shared__ int wsum[4];
    __shared__ unsigned pick[2];
    __shared__ int step_eq[SEL_MAX_STEPS], step_kept[SEL_MAX_STEPS];
    __shared__ unsigned long long step_mask[SEL_MAX_STEPS];
    constexpr int D = 4 * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row = blockIdx.x;
    const int i = (int)(row % NQ);
    const long bh = row / NQ;
    const int hl = (int)(bh % Hl);
    const long b = bh / Hl;
    const int hk = hl / (Hl / Hkv);
    const int len = sel_key_limit(kv_len, (int)b, kv_valid, Sk);

    // visible blocks: a prefix [0, nvis) of the row; forced blocks: [0, kf) and [flo, fhi] within it
    const long r0 = (long)i * blk, r1 = min(r0 + blk, (long)Sq) - 1, off = (long)len - Sq;
    const int nvis = sel_visible(len, Sq, blk, NK, i, causal);
    const int kf = min(keep_first, nvis);
    int flo = 1, fhi = 0;
    if (keep_local >= 1 && nvis > 0) {
        const long jd_lo = max(r0 + off, 0L) / blk, jd_hi = min(max(r1 + off, 0L), (long)len - 1) / blk;
        const long ext = min(keep_local - 1, SEL_MAX_NK);
        flo = (int)max(jd_lo - ext, 0L);
        fhi = (int)min(causal ? jd_hi : jd_hi + ext, (long)nvis - 1);
    }
    const int nf = kf + max(0, fhi - max(flo, kf) + 1);
    auto forced = [&](int j) { return j < kf || (j >= flo && j <= fhi); };

    // scores of the visible blocks
    if (LOADED) {
        const unsigned* wr = wkeys + row * NK;
        for (int j = tid; j < nvis; j += SEL_NT) keys[j] = wr[j];
    } else {
        sel_score_blocks<L>(kbar + ((b * Hkv + hk) * NK) * D, qsum + row * D, 0, nvis, keys);
    }
    __syncthreads();
    if (scores) {
        float* sr = scores + row * NK;
        for (int j = tid; j < NK; j += SEL_NT) sr[j] = j < nvis ? sel_unkey(keys[j]) : -INFINITY;
    }

    // the key of the need-th best unforced visible block
    const int nunf = nvis - nf, need = max(top_k - nf, 0);
    const bool take_all = need >= nunf;
    const bool radix = !take_all && need > 0;
    unsigned T = 0u;
    int need_eq = 0;
    if (radix) {    // (uniform over the workgroup)
        unsigned prefix = 0u;
        int rem = need;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const unsigned himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
            for (int j = tid; j < nvis; j += SEL_NT) {
                const unsigned key = keys[j];
                if (!forced(j) && (key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            // thread t owns digit 255 - t: its inclusive prefix over t counts the keys with that digit or a higher one
            const int h = hist[255 - tid];
            int inc = h;
            for (int m = 1; m < 64; m <<= 1) {
                const int o = __shfl_up(inc, m, 64);
                if (lane >= m) inc += o;
            }
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            for (int w = 0; w < wave; ++w) inc += wsum[w];
            if (inc - h < rem && rem <= inc) {      // exactly one thread: the digit that holds the rem-th best
                pick[0] = prefix | ((unsigned)(255 - tid) << shift);
                pick[1] = (unsigned)(rem - (inc - h));
            }
            __syncthreads();
            prefix = pick[0];
            rem = (int)pick[1];
        }
        T = prefix;
        need_eq = rem;      // of the blocks that tie at T, the need_eq lowest are kept
    }

    // the lists, in 64-block ballot steps: wave w takes steps w, w + 4, ...
    const int nsteps = (NK + 63) >> 6, NW = (NK + 31) >> 5;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int s = wave; s < nsteps; s += 4) {
        const int j = s * 64 + lane;
        const bool eq = radix && j < nvis && !forced(j) && keys[j] == T;
        const unsigned long long m = __ballot(eq);
        if (lane == 0) step_eq[s] = __popcll(m);
    }
    __syncthreads();
    if (wave == 0) sel_wave_scan(step_eq, nsteps, lane);
    __syncthreads();
    uint32_t* wr = bitmask + row * NW;
    for (int s = wave; s < nsteps; s += 4) {
        const int j = s * 64 + lane;
        const bool vis = j < nvis, f = vis && forced(j);
        const unsigned key = vis ? keys[j] : 0u;
        const bool eq = radix && vis && !f && key == T;
        const unsigned long long me = __ballot(eq);
        const bool kept = f || (vis && (take_all || (radix && key > T))) || (eq && step_eq[s] + __popcll(me & below) < need_eq);
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
        if (lane == 0) counts[row] = total;
    }
    __syncthreads();
    int32_t* cr = cols + row * NK;
    for (int s = wave; s < nsteps; s += 4) {
        const unsigned long long m = step_mask[s];
        if ((m >> lane) & 1ull) cr[step_kept[s] + __popcll(m & below)] = s * 64 + lane;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static int sel_check_sizes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    if (B <= 0 || Hkv <= 0 || Hl <= 0 || NQ <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (D != 16 && D != 32 && D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (NK > SEL_MAX_NK) return RSA_ERR_UNSUPPORTED;     // K5's key-block limit
    const size_t q_jobs = (size_t)B * Hl * NQ, k_jobs = (size_t)B * Hkv * NK;
    if (q_jobs + k_jobs > 0x7FFFFFFFull) return RSA_ERR_UNSUPPORTED;     // one workgroup each
    if (bytes) *bytes = (q_jobs + k_jobs) * (size_t)D * sizeof(float);
    return RSA_OK;
}

extern "C" int rsa_block_select_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    if (!bytes) return RSA_ERR_BAD_ARG;
    return sel_check_sizes(B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                                int keep_first, int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                                int32_t* counts, float* scores, void* stream) {
    return sel_run(B, H, Hkv, Hl, Sq, Sk, D, dtype, block, NQ, NK, q, k, kv_len_dev, kv_valid, causal, top_k, keep_first, keep_local,
                   ws, ws_bytes, bitmask, cols, counts, scores, nullptr, stream);
}

int sel_run(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q, rsa_tensor4 k,
            const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first, int keep_local, void* ws,
            size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, const sel_top_p* top_p,
            void* stream) {
    if (B <= 0 || H <= 0 || Hkv <= 0 || Hl <= 0 || Sq <= 0 || Sk <= 0) return RSA_ERR_BAD_ARG;
    if (H % Hkv || (Hl != Hkv && Hl != H)) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 16 && D != 32 && D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (NQ != (int)(((long)Sq + block - 1) / block) || NK != (int)(((long)Sk + block - 1) / block)) return RSA_ERR_BAD_ARG;
    size_t need = 0;
    const int st = sel_check_sizes(B, Hkv, Hl, D, NQ, NK, &need);
    if (st != RSA_OK) return st;
    if (top_k < 0 || keep_first < 0 || keep_local < 0) return RSA_ERR_BAD_ARG;
    if (!kv_len_dev && (kv_valid < 0 || kv_valid > Sk)) return RSA_ERR_BAD_ARG;
    if (!ws || !bitmask || !cols || !counts) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(q) != RSA_OK || rsa_check_tensor(k) != RSA_OK) return RSA_ERR_BAD_ARG;
    if (q.stride_b < 0 || q.stride_h < 0 || q.stride_s < 0 || k.stride_b < 0 || k.stride_h < 0 || k.stride_s < 0)
        return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(bitmask) | reinterpret_cast<uintptr_t>(cols) | reinterpret_cast<uintptr_t>(counts) |
         reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(kv_len_dev)) & 3)
        return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return RSA_ERR_BAD_ARG;
    if (ws_bytes < need) return RSA_ERR_WORKSPACE;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const long q_jobs = (long)B * Hl * NQ, k_jobs = (long)B * Hkv * NK;
    float* qsum = static_cast<float*>(ws);              // [B, Hl, NQ, D]
    float* kbar = qsum + q_jobs * D;                    // [B, Hkv, NK, D]
    const dim3 pool_grid((unsigned)(q_jobs + k_jobs));
    if (dtype == RSA_BF16)
        block_select_pool_kernel<bf16_tag><<<pool_grid, SEL_NT, 0, s>>>(q, k, H, Hkv, Hl, Sq, Sk, D, block, NQ, NK, q_jobs,
                                                                        kv_len_dev, kv_valid, kbar, qsum);
    else
        block_select_pool_kernel<fp16_tag><<<pool_grid, SEL_NT, 0, s>>>(q, k, H, Hkv, Hl, Sq, Sk, D, block, NQ, NK, q_jobs,
                                                                        kv_len_dev, kv_valid, kbar, qsum);
    int rc = rsa_launch_status();
    if (rc != RSA_OK) return rc;
    if (top_p)
        return sel_launch_top_p(D, q_jobs, {kbar, qsum, nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK, kv_len_dev, kv_valid, causal != 0,
                                            top_k, keep_first, keep_local, bitmask, cols, counts, scores}, *top_p, s);
    const dim3 grid((unsigned)q_jobs);
    const size_t lds = (size_t)NK * sizeof(unsigned);
#define SEL_LAUNCH(LANES)                                                                                                       \
    block_select_kernel<LANES, 0><<<grid, SEL_NT, lds, s>>>(kbar, qsum, nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK, kv_len_dev,    \
                                                            kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask,     \
                                                            cols, counts, scores)
    switch (D) {
        case 16: SEL_LAUNCH(4); break;
        case 32: SEL_LAUNCH(8); break;
        case 64: SEL_LAUNCH(16); break;
        default: SEL_LAUNCH(32); break;
    }
#undef SEL_LAUNCH
    return rsa_launch_status();
}

// ---- the pooled-key cache ----------------------------------------------------------------------------------
// Both entries: kv8 = k holds e4m3 codes (no dtype; head dims 64 / 128; 8-byte loads) and k_scale is there.
static int sel_pool_keys_run(bool kv8, int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k,
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
    if (kv8)
        pool_keys_kernel<e4m3_tag><<<grid, SEL_NT, 0, s>>>(k, Hkv, Sk, D, block, NK, W, kv_len_dev, kv_valid, start_dev, start,
                                                           block_table, (long)table_stride_b, num_pages, out, k_scale);
    else if (dtype == RSA_BF16)
        pool_keys_kernel<bf16_tag><<<grid, SEL_NT, 0, s>>>(k, Hkv, Sk, D, block, NK, W, kv_len_dev, kv_valid, start_dev, start,
                                                           block_table, (long)table_stride_b, num_pages, out, nullptr);
    else
        pool_keys_kernel<fp16_tag><<<grid, SEL_NT, 0, s>>>(k, Hkv, Sk, D, block, NK, W, kv_len_dev, kv_valid, start_dev, start,
                                                           block_table, (long)table_stride_b, num_pages, out, nullptr);
    return rsa_launch_status();
}

extern "C" int rsa_pool_keys(int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                             int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid,
                             const int32_t* start_dev, int start, int workgroups_per_head, float* out, void* stream) {
    return sel_pool_keys_run(false, B, Hkv, Sk, D, dtype, block, NK, k, block_table, table_stride_b, num_pages, kv_len_dev, kv_valid,
                             start_dev, start, workgroups_per_head, out, nullptr, stream);
}

// The cache from an e4m3 K: per block the fp32 sum of float(code) in sel_pool_block's order, divided once
// by the count, multiplied once by k_scale[hk] (DEVICE fp32 [Hkv]).
extern "C" int rsa_pool_keys_kv8(int B, int Hkv, int Sk, int D, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                                 int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid,
                                 const int32_t* start_dev, int start, int workgroups_per_head, float* out, const float* k_scale,
                                 void* stream) {
    return sel_pool_keys_run(true, B, Hkv, Sk, D, 0, block, NK, k, block_table, table_stride_b, num_pages, kv_len_dev, kv_valid,
                             start_dev, start, workgroups_per_head, out, k_scale, stream);
}

static int sel_pooled_check_sizes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    if (B <= 0 || Hkv <= 0 || Hl <= 0 || NQ <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (D != 16 && D != 32 && D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (NK > SEL_MAX_NK) return RSA_ERR_UNSUPPORTED;
    const size_t q_jobs = (size_t)B * Hl * NQ;
    if (q_jobs * SEL_MAX_SPLITS > 0x7FFFFFFFull) return RSA_ERR_UNSUPPORTED;    // one workgroup per row and split
    if (bytes) *bytes = q_jobs * ((size_t)D * sizeof(float) + (size_t)NK * sizeof(unsigned));   // the pooled queries, the keys
    return RSA_OK;
}

// The library's choice of score_splits, a function of the shapes alone (measured: profiles/pooled_select_perf.txt).
// One pass of sel_score_blocks' loop per score workgroup (4096 / D key blocks: 32 at D = 128), which is the best or within the
// baseline's spread of the best at both measured row counts (8 rows x 1024 blocks: 32 splits; 64 rows x 256 blocks: 8); at most 64
// splits and about 1024 workgroups, and none where the list rows alone give two workgroups per compute unit (not measured there).
static int sel_default_splits(size_t rows, int NK, int D) {
    if (rows >= 512) return 1;
    const int pass = 4096 / D;
    const int by_blocks = (NK + pass - 1) / pass, by_rows = (int)((1024 + rows - 1) / rows);
    return max(1, min(min(by_blocks, by_rows), 64));
}

extern "C" int rsa_block_select_pooled_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    if (!bytes) return RSA_ERR_BAD_ARG;
    return sel_pooled_check_sizes(B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_pooled(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK,
                                       rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal,
                                       int top_k, int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes,
                                       uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, void* stream) {
    return sel_pooled_run(B, H, Hkv, Hl, Sq, D, dtype, block, NQ, NK, q, pooled_k, kv_len_dev, kv_valid, causal, top_k, keep_first,
                          keep_local, score_splits, ws, ws_bytes, bitmask, cols, counts, scores, nullptr, stream);
}

int sel_pooled_run(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                   const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first,
                   int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                   int32_t* counts, float* scores, const sel_top_p* top_p, void* stream) {
    if (B <= 0 || H <= 0 || Hkv <= 0 || Hl <= 0 || Sq <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (H % Hkv || (Hl != Hkv && Hl != H)) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 16 && D != 32 && D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (NQ != (int)(((long)Sq + block - 1) / block)) return RSA_ERR_BAD_ARG;
    size_t need = 0;
    const int st = sel_pooled_check_sizes(B, Hkv, Hl, D, NQ, NK, &need);
    if (st != RSA_OK) return st;
    const int Sk = NK * block;      // the capacity of the cache
    if (top_k < 0 || keep_first < 0 || keep_local < 0) return RSA_ERR_BAD_ARG;
    if (score_splits < 0 || score_splits > SEL_MAX_SPLITS) return RSA_ERR_BAD_ARG;
    if (!kv_len_dev && (kv_valid < 0 || kv_valid > Sk)) return RSA_ERR_BAD_ARG;
    if (!ws || !pooled_k || !bitmask || !cols || !counts) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(q) != RSA_OK) return RSA_ERR_BAD_ARG;
    if (q.stride_b < 0 || q.stride_h < 0 || q.stride_s < 0) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(bitmask) | reinterpret_cast<uintptr_t>(cols) | reinterpret_cast<uintptr_t>(counts) |
         reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(kv_len_dev)) & 3)
        return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(pooled_k)) & 15) return RSA_ERR_BAD_ARG;
    if (ws_bytes < need) return RSA_ERR_WORKSPACE;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const long q_jobs = (long)B * Hl * NQ;
    const int splits = min(score_splits ? score_splits : sel_default_splits((size_t)q_jobs, NK, D), NK);
    float* qsum = static_cast<float*>(ws);                              // [B, Hl, NQ, D]
    unsigned* wkeys = reinterpret_cast<unsigned*>(qsum + q_jobs * D);   // [B, Hl, NQ, NK]
    // the pooled queries: the query jobs of the pool kernel alone (no key job in the grid: k and kbar are not touched)
    if (dtype == RSA_BF16)
        block_select_pool_kernel<bf16_tag><<<dim3((unsigned)q_jobs), SEL_NT, 0, s>>>(q, q, H, Hkv, Hl, Sq, Sk, D, block, NQ, NK, q_jobs,
                                                                                     kv_len_dev, kv_valid, nullptr, qsum);
    else
        block_select_pool_kernel<fp16_tag><<<dim3((unsigned)q_jobs), SEL_NT, 0, s>>>(q, q, H, Hkv, Hl, Sq, Sk, D, block, NQ, NK, q_jobs,
                                                                                     kv_len_dev, kv_valid, nullptr, qsum);
    int rc = rsa_launch_status();
    if (rc != RSA_OK) return rc;
    const dim3 grid((unsigned)q_jobs), sgrid((unsigned)(q_jobs * splits));
    const size_t lds = (size_t)NK * sizeof(unsigned);
#define SEL_LAUNCH(LANES)                                                                                                       \
    if (splits > 1) {                                                                                                           \
        block_score_kernel<LANES><<<sgrid, SEL_NT, 0, s>>>(pooled_k, qsum, Hkv, Hl, Sq, Sk, block, NQ, NK, splits, kv_len_dev,  \
                                                           kv_valid, causal != 0, wkeys);                                       \
        rc = rsa_launch_status();                                                                                               \
        if (rc != RSA_OK) return rc;                                                                                            \
    }                                                                                                                           \
    if (top_p)                                                                                                                  \
        return sel_launch_top_p(D, q_jobs, {pooled_k, qsum, splits > 1 ? wkeys : nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK,       \
                                            kv_len_dev, kv_valid, causal != 0, top_k, keep_first, keep_local, bitmask, cols,    \
                                            counts, scores}, *top_p, s);                                                        \
    if (splits > 1) {                                                                                                           \
        block_select_kernel<LANES, 1><<<grid, SEL_NT, lds, s>>>(pooled_k, qsum, wkeys, Hkv, Hl, Sq, Sk, block, NQ, NK,          \
                                                                kv_len_dev, kv_valid, causal != 0, top_k, keep_first,           \
                                                                keep_local, bitmask, cols, counts, scores);                     \
    } else {                                                                                                                    \
        block_select_kernel<LANES, 0><<<grid, SEL_NT, lds, s>>>(pooled_k, qsum, nullptr, Hkv, Hl, Sq, Sk, block, NQ, NK,        \
                                                                kv_len_dev, kv_valid, causal != 0, top_k, keep_first,           \
                                                                keep_local, bitmask, cols, counts, scores);                     \
    }
    switch (D) {
        case 16: SEL_LAUNCH(4); break;
        case 32: SEL_LAUNCH(8); break;
        case 64: SEL_LAUNCH(16); break;
        default: SEL_LAUNCH(32); break;
    }
#undef SEL_LAUNCH
    return rsa_launch_status();
}
