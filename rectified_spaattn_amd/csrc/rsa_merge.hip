// N-way merge of attention partials (rsa_merge_partials): partial i is a 2-byte out_i and an fp32 log-sum-exp
// lse_i in natural log -- what the decode and extend entries return --, an optional sink is one more partial of one logit per head
// whose out is zero.  One launch, no workspace, no host read; every pointer and stride travels by value in the kernel arguments.
//
//   merge_kernel<Tag, N, D, V>   one lane owns V channels of one row (V = 8: one 16-byte load per partial and one 16-byte store;
//                                V = 4: the 8-byte form for pointers or strides that are only 8-byte / 4-element aligned), D / V lanes
//                                share a row and each reads the row's N log-sum-exps.  N is a template parameter: the N row loads and
//                                the N lse loads of a lane are all issued before the first use.  A bounded grid walks the rows with a
//                                grid stride.  Per row, fp32, the partials in ascending order and the sink last:
//                                    m*  = max over the live entries of lse_i                 (live: lse_i > -inf)
//                                    w_i = exp2((lse_i - m*) * log2 e)                        one subtraction, one multiplication, v_exp_f32
//                                    acc = fmaf(w_i, out_i[c], acc), l = l + w_i              a partial that is not live is skipped
//                                    out[c] = acc / l (IEEE), one conversion;  lse = m* + ln 2 * log2 l    (no live entry: 0, -inf)
//                                Both forms run this arithmetic per element and give the same bytes.
//
// The result may alias one partial exactly: a lane loads every element it needs before it stores, and no other lane touches them; a
// row's lanes lie in one wave (D / V divides 64), so an lse that is read by all of them and stored by one is read first as well.
// NaNs are honoured and nothing is contracted (the Makefile): the skip tests and the division are the contract.
#include "rsa_common.h"

#define MERGE_NT 256
#define MERGE_MAX_GRID 2048     // workgroups at most (256 CUs x 8): rows beyond one pass are walked with a grid stride
#define MERGE_MAX_N 8

template <typename Tag>
__device__ __forceinline__ unsigned short merge_from_f32(float f);
template <>
__device__ __forceinline__ unsigned short merge_from_f32<bf16_tag>(float f) {
    return __builtin_bit_cast(unsigned short, (__bf16)f);
}
template <>
__device__ __forceinline__ unsigned short merge_from_f32<fp16_tag>(float f) {
    return __builtin_bit_cast(unsigned short, (_Float16)f);
}

// Off: the type of a stride and of an element offset -- unsigned where every view of the call spans fewer than 2^32 elements (the
// strides then fit the scalar registers at N = 8 and an offset is three 32-bit multiply-adds), long otherwise.
template <int N, typename Off>
struct MergeArgs {
    const unsigned short* o[N];     // the partials' outs, element strides (b, h, s)
    Off osb[N], osh[N], oss[N];
    const float* l[N];              // their log-sum-exps
    Off lsb[N], lsh[N], lss[N];
    const float* sink;              // [H] or null
    unsigned short* out;
    Off rsb, rsh, rss;
    float* lse;                     // or null
    Off esb, esh, ess;
    int H, S;
    int rows;                       // B * H * S
};

template <int V>
struct MergeVec;
template <>
struct MergeVec<8> {
    using T = uint4;
    static __device__ __forceinline__ void words(const uint4& v, unsigned* w) { w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    static __device__ __forceinline__ uint4 make(const unsigned* w) { return make_uint4(w[0], w[1], w[2], w[3]); }
};
template <>
struct MergeVec<4> {
    using T = uint2;
    static __device__ __forceinline__ void words(const uint2& v, unsigned* w) { w[0] = v.x; w[1] = v.y; }
    static __device__ __forceinline__ uint2 make(const unsigned* w) { return make_uint2(w[0], w[1]); }
};

template <typename Tag, int N, int D, int V, typename Off>
__global__ __launch_bounds__(MERGE_NT) void merge_kernel(const MergeArgs<N, Off> a) {
    using Vec = typename MergeVec<V>::T;
    constexpr int LPR = D / V;                  // lanes per row: 8, 16 or 32 -- a row never straddles a wave
    constexpr int RPB = MERGE_NT / LPR;         // rows per workgroup and pass
    constexpr float LOG2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;
    const int c = (int)(threadIdx.x % LPR) * V;
    const int step = (int)gridDim.x * RPB;      // (at most 2048 * 32 rows a pass)
    for (long row = (long)blockIdx.x * RPB + threadIdx.x / LPR; row < a.rows; row += step) {
        const unsigned r = (unsigned)row;
        const unsigned bh = r / (unsigned)a.S;
        const unsigned bq = bh / (unsigned)a.H;
        const Off s = r - bh * (unsigned)a.S, b = bq, h = bh - bq * (unsigned)a.H;
        Vec x[N];
        float ls[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {           // every load of the lane, before the first use
            x[i] = *reinterpret_cast<const Vec*>(a.o[i] + b * a.osb[i] + h * a.osh[i] + s * a.oss[i] + c);
            ls[i] = a.l[i][b * a.lsb[i] + h * a.lsh[i] + s * a.lss[i]];
        }
        const float sk = a.sink ? a.sink[h] : -INFINITY;
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (ls[i] > -INFINITY) m = fmaxf(m, ls[i]);
        if (sk > -INFINITY) m = fmaxf(m, sk);
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        float lt = 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (!(ls[i] > -INFINITY)) continue;         // not live (a NaN log-sum-exp among them): skipped, never multiplied
            const float w = __builtin_amdgcn_exp2f((ls[i] - m) * LOG2E);
            unsigned xw[V / 2];
            MergeVec<V>::words(x[i], xw);
#pragma unroll
            for (int e = 0; e < V; ++e)
                acc[e] = __builtin_fmaf(w, rsa_to_f32<Tag>((unsigned short)(xw[e / 2] >> (16 * (e & 1)))), acc[e]);
            lt = lt + w;
        }
        if (sk > -INFINITY) lt = lt + __builtin_amdgcn_exp2f((sk - m) * LOG2E);      // the sink: into l, not into acc
        const bool any = m > -INFINITY;
        unsigned ow[V / 2];
#pragma unroll
        for (int e = 0; e < V; e += 2) {
            const float lo = any ? acc[e] / lt : 0.f, hi = any ? acc[e + 1] / lt : 0.f;
            ow[e / 2] = (unsigned)merge_from_f32<Tag>(lo) | ((unsigned)merge_from_f32<Tag>(hi) << 16);
        }
        *reinterpret_cast<Vec*>(a.out + b * a.rsb + h * a.rsh + s * a.rss + c) = MergeVec<V>::make(ow);
        if (a.lse && c == 0) {
            const float t = LN2 * __builtin_amdgcn_logf(lt);
            a.lse[b * a.esb + h * a.esh + s * a.ess] = any ? m + t : -INFINITY;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct MergeSpan {      // the bytes a strided view touches: [lo, hi)
    uintptr_t lo, hi;
};
static MergeSpan merge_span(const void* p, int64_t sb, int64_t sh, int64_t ss, long B, long H, long S, long inner, int elem) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    if (B <= 0 || H <= 0 || S <= 0) return {lo, lo};
    return {lo, lo + (uintptr_t)((B - 1) * sb + (H - 1) * sh + (S - 1) * ss + inner) * (uintptr_t)elem};
}
static bool merge_meet(const MergeSpan& x, const MergeSpan& y) { return x.lo < y.hi && y.lo < x.hi; }

struct MergeCall {      // what the entry hands on once every check has passed
    int dtype, D, H, S, rows;
    bool wide;              // 16 bytes a lane (every pointer 16-byte aligned, every stride a multiple of 8), else 8
    const rsa_tensor4* outs;
    const float* const* lses;
    const int64_t* ls;
    const float* sink;
    rsa_out4 out;
    float* lse_out;
    int64_t esb, esh, ess;
    hipStream_t s;
};

template <typename Tag, int N, int D, typename Off>
static void merge_launch(const MergeCall& c, const MergeArgs<N, Off>& a) {
    const int lpr = D / (c.wide ? 8 : 4), rpb = MERGE_NT / lpr;
    const long need = ((long)a.rows + rpb - 1) / rpb;
    const int grid = (int)(need < MERGE_MAX_GRID ? need : MERGE_MAX_GRID);
    if (c.wide) merge_kernel<Tag, N, D, 8, Off><<<grid, MERGE_NT, 0, c.s>>>(a);
    else merge_kernel<Tag, N, D, 4, Off><<<grid, MERGE_NT, 0, c.s>>>(a);
}

template <int N, typename Off>
static void merge_with(const MergeCall& c) {
    MergeArgs<N, Off> a;
    for (int i = 0; i < N; ++i) {
        a.o[i] = static_cast<const unsigned short*>(c.outs[i].ptr);
        a.osb[i] = (Off)c.outs[i].stride_b, a.osh[i] = (Off)c.outs[i].stride_h, a.oss[i] = (Off)c.outs[i].stride_s;
        a.l[i] = c.lses[i];
        a.lsb[i] = (Off)c.ls[3 * i], a.lsh[i] = (Off)c.ls[3 * i + 1], a.lss[i] = (Off)c.ls[3 * i + 2];
    }
    a.sink = c.sink;
    a.out = static_cast<unsigned short*>(c.out.ptr);
    a.rsb = (Off)c.out.stride_b, a.rsh = (Off)c.out.stride_h, a.rss = (Off)c.out.stride_s;
    a.lse = c.lse_out;
    a.esb = (Off)c.esb, a.esh = (Off)c.esh, a.ess = (Off)c.ess;
    a.H = c.H, a.S = c.S, a.rows = c.rows;
    if (c.dtype == RSA_BF16) {
        if (c.D == 128) merge_launch<bf16_tag, N, 128, Off>(c, a);
        else merge_launch<bf16_tag, N, 64, Off>(c, a);
    } else {
        if (c.D == 128) merge_launch<fp16_tag, N, 128, Off>(c, a);
        else merge_launch<fp16_tag, N, 64, Off>(c, a);
    }
}

extern "C" int rsa_merge_partials(int N, int B, int H, int S, int D, int dtype, const rsa_tensor4* outs, const float* const* lses,
                                  const int64_t* lse_strides, const float* sink, rsa_out4 out, float* lse_out, int64_t lse_out_stride_b,
                                  int64_t lse_out_stride_h, int64_t lse_out_stride_s, void* stream) {
    if (N < 1 || N > MERGE_MAX_N || B < 0 || H < 0 || S < 0) return RSA_ERR_BAD_ARG;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if ((long)B * H > 0x7fffffffL || (long)B * H * S > 0x7fffffffL) return RSA_ERR_UNSUPPORTED;     // the row index is 32-bit
    if (!outs || !lses || !lse_strides || !out.ptr) return RSA_ERR_BAD_ARG;
    auto aligned = [](const void* p, int64_t sb, int64_t sh, int64_t ss, unsigned bytes, int elems) {
        return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0 && sb % elems == 0 && sh % elems == 0 && ss % elems == 0;
    };
    bool wide = aligned(out.ptr, out.stride_b, out.stride_h, out.stride_s, 16, 8);
    if (!aligned(out.ptr, out.stride_b, out.stride_h, out.stride_s, 8, 4)) return RSA_ERR_BAD_ARG;
    // a result row is written once: its strides are positive where the axis has more than one entry
    if ((B > 1 && out.stride_b <= 0) || (H > 1 && out.stride_h <= 0) || (S > 1 && out.stride_s <= 0)) return RSA_ERR_BAD_ARG;
    if (out.stride_b < 0 || out.stride_h < 0 || out.stride_s < 0) return RSA_ERR_BAD_ARG;
    if (lse_out) {
        if (reinterpret_cast<uintptr_t>(lse_out) & 3) return RSA_ERR_BAD_ARG;
        if ((B > 1 && lse_out_stride_b <= 0) || (H > 1 && lse_out_stride_h <= 0) || (S > 1 && lse_out_stride_s <= 0)) return RSA_ERR_BAD_ARG;
        if (lse_out_stride_b < 0 || lse_out_stride_h < 0 || lse_out_stride_s < 0) return RSA_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(sink) & 3) return RSA_ERR_BAD_ARG;
    const MergeSpan ro = merge_span(out.ptr, out.stride_b, out.stride_h, out.stride_s, B, H, S, D, 2);
    const MergeSpan rl = merge_span(lse_out, lse_out_stride_b, lse_out_stride_h, lse_out_stride_s, B, H, S, 1, 4);
    if (lse_out && merge_meet(ro, rl)) return RSA_ERR_BAD_ARG;
    // 32-bit element offsets where every view spans fewer than 2^32 elements
    bool small = (ro.hi - ro.lo) / 2 < (1ul << 32) && (rl.hi - rl.lo) / 4 < (1ul << 32);
    if (sink && (merge_meet(ro, {reinterpret_cast<uintptr_t>(sink), reinterpret_cast<uintptr_t>(sink) + 4 * (uintptr_t)H}) ||
                 (lse_out && merge_meet(rl, {reinterpret_cast<uintptr_t>(sink), reinterpret_cast<uintptr_t>(sink) + 4 * (uintptr_t)H}))))
        return RSA_ERR_BAD_ARG;
    for (int i = 0; i < N; ++i) {
        const rsa_tensor4& t = outs[i];
        const int64_t* ls = lse_strides + 3 * i;
        if (!t.ptr || !lses[i] || (reinterpret_cast<uintptr_t>(lses[i]) & 3)) return RSA_ERR_BAD_ARG;
        if (t.stride_b < 0 || t.stride_h < 0 || t.stride_s < 0 || ls[0] < 0 || ls[1] < 0 || ls[2] < 0) return RSA_ERR_BAD_ARG;
        if (!aligned(t.ptr, t.stride_b, t.stride_h, t.stride_s, 8, 4)) return RSA_ERR_BAD_ARG;
        wide = wide && aligned(t.ptr, t.stride_b, t.stride_h, t.stride_s, 16, 8);
        // the result meets a partial only as that partial: the same pointer and the same strides
        const MergeSpan po = merge_span(t.ptr, t.stride_b, t.stride_h, t.stride_s, B, H, S, D, 2);
        const MergeSpan pl = merge_span(lses[i], ls[0], ls[1], ls[2], B, H, S, 1, 4);
        small = small && (po.hi - po.lo) / 2 < (1ul << 32) && (pl.hi - pl.lo) / 4 < (1ul << 32);
        const bool same_o = t.ptr == out.ptr && t.stride_b == out.stride_b && t.stride_h == out.stride_h && t.stride_s == out.stride_s;
        const bool same_l = lse_out && lses[i] == lse_out && ls[0] == lse_out_stride_b && ls[1] == lse_out_stride_h && ls[2] == lse_out_stride_s;
        if ((merge_meet(ro, po) && !same_o) || merge_meet(ro, pl)) return RSA_ERR_BAD_ARG;
        if (lse_out && ((merge_meet(rl, pl) && !same_l) || merge_meet(rl, po))) return RSA_ERR_BAD_ARG;
    }
    const int rows = B * H * S;
    if (rows == 0) return RSA_OK;
    const MergeCall c = {dtype, D, H, S, rows, wide, outs, lses, lse_strides, sink, out, lse_out, lse_out_stride_b, lse_out_stride_h,
                         lse_out_stride_s, static_cast<hipStream_t>(stream)};
#define MERGE_CASE(n)                                \
    case n:                                          \
        if (small) merge_with<n, unsigned>(c);       \
        else merge_with<n, long>(c);                 \
        break;
    switch (N) {
        MERGE_CASE(1) MERGE_CASE(2) MERGE_CASE(3) MERGE_CASE(4) MERGE_CASE(5) MERGE_CASE(6) MERGE_CASE(7) MERGE_CASE(8)
    }
#undef MERGE_CASE
    return rsa_launch_status();
}
