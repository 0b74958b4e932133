// What the two selection units share (rsa_block_select.hip: the top-k selection, DESIGN.md sections 5.11 and 5.13;
// rsa_block_select_p.hip: the top-p selection, section 5.15): the ordered score keys, the visible prefix of a list row, the score
// arithmetic, and the one host body that checks the arguments and launches the pooling and score kernels for both.
#pragma once
#include "rsa_common.h"

#include <math.h>

#define SEL_NT 256
#define SEL_MAX_NK 8192
#define SEL_MAX_STEPS (SEL_MAX_NK / 64)
#define SEL_MAX_SPLITS 256      // score workgroups per list row of the pooled selection, at most

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

// Visible blocks of list row (b, i): a prefix [0, nvis) of the row.
__device__ __forceinline__ int sel_visible(int len, int Sq, int blk, int NK, int i, int causal) {
    const long r0 = (long)i * blk, r1 = min(r0 + blk, (long)Sq) - 1, off = (long)len - Sq;
    int nvis = min(NK, (len + blk - 1) / blk);
    if (causal) nvis = r1 + off < 0 ? 0 : (int)min((long)nvis, (r1 + off) / blk + 1);
    return nvis;
}

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

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The budget of the top-p selection: p16 = round(top_p * 65536) in [0, 65536], c = float(score_scale * log2(e)) finite and > 0,
// mass NULL or fp32 [B * Hl * NQ].
struct sel_top_p {
    int p16;
    float c;
    float* mass;
};

// The bodies of rsa_block_select and rsa_block_select_pooled (rsa_block_select.hip): every check, the pooling and score launches,
// and the select launch -- block_select_kernel with top_p NULL, else sel_launch_top_p (rsa_block_select_p.hip).
int sel_run(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q, rsa_tensor4 k,
            const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first, int keep_local, void* ws,
            size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, const sel_top_p* top_p,
            void* stream);
int sel_pooled_run(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                   const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first,
                   int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                   int32_t* counts, float* scores, const sel_top_p* top_p, void* stream);

// The rows block_select_kernel and block_select_p_kernel are launched over, in the kernels' parameter order.
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
int sel_launch_top_p(int D, long rows, const sel_rows& r, const sel_top_p& p, hipStream_t s);
