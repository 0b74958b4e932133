// The writer of the MXFP4 K/V cache (include/rsa.h: rsa_kv4_append): new K / V rows of the query's 2-byte
// type become OCP e2m1 codes, two to a byte (element 2 i in the low nibble of byte i), with one e8m0 scale byte per 32 channels of
// a row, and land in a contiguous or paged cache.  One kernel, plain HIP C++, one memory-bound pass:
//
//   kv4_append_kernel   one lane per 32-channel group of a new row: 64 bytes in (four 16-byte loads), 16 bytes of codes out (one
//                       16-byte store) and one scale byte.  The group is the lane's own, so its maximum needs no LDS and no lane
//                       exchange.  blockIdx.y picks K or V.  Token t < n_new[b] of batch item b goes to position start[b] + t; a
//                       position at or beyond the capacity, or (paged) one whose table entry lies outside [0, num_pages), is
//                       dropped: no address is formed from an unchecked index.  The call writes the D / 2 + D / 32 bytes of each
//                       placed row and no other byte.
//
// Byte contract per group (tests/kv4_ref.py is the expression; the instruction serves it):
//   a     = the largest |x_d| of the group, a NaN element left out (taken on the 15 magnitude bits of the 2-byte inputs, whose
//           order is the values' order);
//   e     = clamp(exponent_field(a as fp32) - 127 - 2, -13, 13): zero, a subnormal and everything below 2^-11 give -13, +-Inf and
//           everything from 2^15 on give 13; the scale byte is e + 127;
//   code  = x_d * 2^-e rounded to nearest even onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6, the sign of x_d kept (-0 and
//           a negative that rounds to zero are 0x8); a NaN element is code 0x0 (e2m1 has no NaN: a documented limit).
// v_cvt_scalef32_pk_fp4_{bf16,f16} does the division by 2^e, the rounding and the saturation of a pair of elements in one
// instruction; what it is not asked to decide is done in integer code in front of it: a NaN element is cleared to +0 in the packed
// input word, and the exponent comes from the integer maximum.
#include "rsa_kv_append.h"

#define KV4_E_MIN (-13)
#define KV4_E_MAX 13

struct Kv4Own {
    unsigned char* scales[2];           // [B, Hkv, Sk, D / 32] or page pools [P, Hkv, blk, D / 32]: beside the codes, which are dst
    long esb[2], esh[2], ess[2];
    static constexpr int ELEMS = 32, ALIGN = 16;    // one lane: a 32-channel group of a row, a 16-byte store of codes
};

// The type's layout: the magnitude bits of Inf, and the shared exponent of a group whose largest magnitude is m (15 bits, not a
// NaN).  The exponent field of m as an fp32 is the bf16 field itself, and the fp16 field + 112 for a normal fp16; an fp16 subnormal
// lies below 2^-14, where the clamp gives KV4_E_MIN as it does for the field 0.
template <typename Tag>
struct Kv4Elem;
template <>
struct Kv4Elem<bf16_tag> {
    static constexpr unsigned INF = 0x7F80u;
    static __device__ __forceinline__ int exponent(unsigned m) { return (int)(m >> 7) - 127 - 2; }
    static __device__ __forceinline__ unsigned cvt(unsigned old, unsigned pair, float scale, int sel) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 x = __builtin_bit_cast(bf16x2, pair);
        switch (sel) {
            case 0: return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, x, scale, 0);
            case 1: return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, x, scale, 1);
            case 2: return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, x, scale, 2);
            default: return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, x, scale, 3);
        }
    }
};
template <>
struct Kv4Elem<fp16_tag> {
    static constexpr unsigned INF = 0x7C00u;
    static __device__ __forceinline__ int exponent(unsigned m) { return (int)(m >> 10) - 15 - 2; }
    static __device__ __forceinline__ unsigned cvt(unsigned old, unsigned pair, float scale, int sel) {
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        const f16x2 x = __builtin_bit_cast(f16x2, pair);
        switch (sel) {
            case 0: return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, x, scale, 0);
            case 1: return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, x, scale, 1);
            case 2: return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, x, scale, 2);
            default: return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, x, scale, 3);
        }
    }
};

// One packed input word: its NaN halves cleared to +0, and the group maximum taken over what is left.
template <typename Tag>
__device__ __forceinline__ unsigned kv4_clean(unsigned w, unsigned& amax) {
    const unsigned lo = w & 0x7FFFu, hi = (w >> 16) & 0x7FFFu;
    if (lo > Kv4Elem<Tag>::INF) w &= 0xFFFF0000u;
    else amax = max(amax, lo);
    if (hi > Kv4Elem<Tag>::INF) w &= 0x0000FFFFu;
    else amax = max(amax, hi);
    return w;
}

template <typename Tag>
__global__ __launch_bounds__(KV_NT) void kv4_append_kernel(const KvAppendArgs<Kv4Own> a) {
    KvPlace at;
    if (!kv_place<false>(a, (long)blockIdx.x * KV_NT + threadIdx.x, at)) return;
    const uint4* sp = reinterpret_cast<const uint4*>(KV_SEL(src) + at.b * KV_SEL(ssb) + (long)at.hk * KV_SEL(ssh) +
                                                     at.srow * KV_SEL(sss) + 32 * at.c);
    uint4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = sp[i];
    unsigned amax = 0;
    unsigned p[16];                     // the group's 16 pairs, NaN halves cleared
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        p[4 * i] = kv4_clean<Tag>(x[i].x, amax);
        p[4 * i + 1] = kv4_clean<Tag>(x[i].y, amax);
        p[4 * i + 2] = kv4_clean<Tag>(x[i].z, amax);
        p[4 * i + 3] = kv4_clean<Tag>(x[i].w, amax);
    }
    const int e = min(max(Kv4Elem<Tag>::exponent(amax), KV4_E_MIN), KV4_E_MAX);
    const unsigned sbyte = (unsigned)(e + 127);
    const float scale = __uint_as_float(sbyte << 23);
    unsigned o[4] = {0u, 0u, 0u, 0u};   // pair j is byte j & 3 of word j >> 2
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j >> 2] = Kv4Elem<Tag>::cvt(o[j >> 2], p[j], scale, j & 3);
    *reinterpret_cast<uint4*>(KV_SEL(dst) + at.item * KV_SEL(dsb) + (long)at.hk * KV_SEL(dsh) + at.row * KV_SEL(dss) + 16 * at.c) =
        make_uint4(o[0], o[1], o[2], o[3]);
    KV_SEL(x.scales)[at.item * KV_SEL(x.esb) + (long)at.hk * KV_SEL(x.esh) + at.row * KV_SEL(x.ess) + at.c] = (unsigned char)sbyte;
}

extern "C" int rsa_kv4_append(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                              rsa_out4 k_codes, rsa_out4 k_scales, rsa_out4 v_codes, rsa_out4 v_scales, const int32_t* block_table,
                              int64_t table_stride_b, int num_pages, const int32_t* start_dev, int start, const int32_t* n_new_dev,
                              int n_new, void* stream) {
    const rsa_out4 scales[2] = {k_scales, v_scales};
    bool own_ok = true;
    for (int w = 0; w < 2; ++w)
        own_ok = own_ok && scales[w].ptr && scales[w].stride_b >= 0 && scales[w].stride_h >= 0 && scales[w].stride_s >= 0;
    KvAppendArgs<Kv4Own> a;
    dim3 grid;
    const int st = kv_append_door(B, Hkv, T, Sk, D, dtype, block, {k_new, v_new}, {k_codes, v_codes}, block_table, table_stride_b,
                                  num_pages, start_dev, start, n_new_dev, n_new, own_ok, 0, false, a, grid);
    if (st != RSA_OK) return st;
    for (int w = 0; w < 2; ++w) {
        a.x.scales[w] = static_cast<unsigned char*>(scales[w].ptr);
        a.x.esb[w] = scales[w].stride_b; a.x.esh[w] = scales[w].stride_h; a.x.ess[w] = scales[w].stride_s;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == RSA_BF16) kv4_append_kernel<bf16_tag><<<grid, KV_NT, 0, s>>>(a);
    else kv4_append_kernel<fp16_tag><<<grid, KV_NT, 0, s>>>(a);
    return rsa_launch_status();
}
