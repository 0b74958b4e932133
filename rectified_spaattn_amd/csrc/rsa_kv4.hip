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
#include "rsa_common.h"

#include <type_traits>

#define KV4_NT 256
#define KV4_E_MIN (-13)
#define KV4_E_MAX 13

struct Kv4Args {
    const unsigned short* src[2];       // k_new, v_new [B, Hkv, T, D]: strides in elements
    long ssb[2], ssh[2], sss[2];
    unsigned char* codes[2];            // [B, Hkv, Sk, D / 2] or page pools [P, Hkv, blk, D / 2]: strides in bytes
    long csb[2], csh[2], css[2];
    unsigned char* scales[2];           // [B, Hkv, Sk, D / 32] or page pools [P, Hkv, blk, D / 32]
    long esb[2], esh[2], ess[2];
    const int32_t* table;               // [B, >= Sk / blk] or null: contiguous caches
    long tsb;
    int num_pages;
    const int32_t *start_dev, *n_new_dev;       // device values (clamped here) or null: the host values
    int start, n_new;
    int Hkv, T, Sk, blk, G;             // G = D / 32 lanes per row
    long lanes;                         // B * Hkv * T * G
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
__global__ __launch_bounds__(KV4_NT) void kv4_append_kernel(const Kv4Args a) {
    const long g = (long)blockIdx.x * KV4_NT + threadIdx.x;
    if (g >= a.lanes) return;
    const int w = blockIdx.y;           // 0: K, 1: V
    const int c = (int)(g % a.G);
    const int t = (int)((g / a.G) % a.T);
    const int hk = (int)((g / ((long)a.G * a.T)) % a.Hkv);
    const long b = g / ((long)a.G * a.T * a.Hkv);
    const int n = a.n_new_dev ? min(max(a.n_new_dev[b], 0), a.T) : a.n_new;
    if (t >= n) return;
    const int st = a.start_dev ? min(max(a.start_dev[b], 0), a.Sk) : a.start;
    const long pos = (long)st + t;
    if (pos >= a.Sk) return;            // beyond the capacity: dropped
    long row = pos, item = b;
    if (a.table) {
        const int page = a.table[b * a.tsb + pos / a.blk];
        if (page < 0 || page >= a.num_pages) return;        // no page: dropped
        item = page;
        row = pos % a.blk;
    }
#define KV4_SEL(f) (w ? a.f[1] : a.f[0])      // (uniform selects: the argument arrays are never indexed by a register)
    const uint4* sp = reinterpret_cast<const uint4*>(KV4_SEL(src) + b * KV4_SEL(ssb) + (long)hk * KV4_SEL(ssh) +
                                                     (long)t * KV4_SEL(sss) + 32 * c);
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
    *reinterpret_cast<uint4*>(KV4_SEL(codes) + item * KV4_SEL(csb) + (long)hk * KV4_SEL(csh) + row * KV4_SEL(css) + 16 * c) =
        make_uint4(o[0], o[1], o[2], o[3]);
    KV4_SEL(scales)[item * KV4_SEL(esb) + (long)hk * KV4_SEL(esh) + row * KV4_SEL(ess) + c] = (unsigned char)sbyte;
#undef KV4_SEL
}

extern "C" int rsa_kv4_append(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                              rsa_out4 k_codes, rsa_out4 k_scales, rsa_out4 v_codes, rsa_out4 v_scales, const int32_t* block_table,
                              int64_t table_stride_b, int num_pages, const int32_t* start_dev, int start, const int32_t* n_new_dev,
                              int n_new, void* stream) {
    if (B <= 0 || Hkv <= 0 || T <= 0 || Sk <= 0) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (!start_dev && (start < 0 || start > Sk)) return RSA_ERR_BAD_ARG;
    if (!n_new_dev && (n_new < 0 || n_new > T)) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(k_new) != RSA_OK || rsa_check_tensor(v_new) != RSA_OK) return RSA_ERR_BAD_ARG;
    const rsa_tensor4 src[2] = {k_new, v_new};
    const rsa_out4 codes[2] = {k_codes, v_codes}, scales[2] = {k_scales, v_scales};
    for (int w = 0; w < 2; ++w) {
        if (src[w].stride_b < 0 || src[w].stride_h < 0 || src[w].stride_s < 0) return RSA_ERR_BAD_ARG;
        if (!codes[w].ptr || (reinterpret_cast<uintptr_t>(codes[w].ptr) & 15)) return RSA_ERR_BAD_ARG;     // 16-byte stores
        if (codes[w].stride_b < 0 || codes[w].stride_h < 0 || codes[w].stride_s < 0) return RSA_ERR_BAD_ARG;
        if ((codes[w].stride_b % 16) || (codes[w].stride_h % 16) || (codes[w].stride_s % 16)) return RSA_ERR_BAD_ARG;
        if (!scales[w].ptr || scales[w].stride_b < 0 || scales[w].stride_h < 0 || scales[w].stride_s < 0) return RSA_ERR_BAD_ARG;
    }
    if (block_table && (num_pages <= 0 || table_stride_b < 0 || Sk % block)) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(start_dev) | reinterpret_cast<uintptr_t>(n_new_dev)) & 3)
        return RSA_ERR_BAD_ARG;
    const long lanes = (long)B * Hkv * T * (D / 32);
    const long groups = (lanes + KV4_NT - 1) / KV4_NT;
    if (groups > 0x7FFFFFFFl) return RSA_ERR_UNSUPPORTED;

    Kv4Args a;
    for (int w = 0; w < 2; ++w) {
        a.src[w] = static_cast<const unsigned short*>(src[w].ptr);
        a.ssb[w] = src[w].stride_b; a.ssh[w] = src[w].stride_h; a.sss[w] = src[w].stride_s;
        a.codes[w] = static_cast<unsigned char*>(codes[w].ptr);
        a.csb[w] = codes[w].stride_b; a.csh[w] = codes[w].stride_h; a.css[w] = codes[w].stride_s;
        a.scales[w] = static_cast<unsigned char*>(scales[w].ptr);
        a.esb[w] = scales[w].stride_b; a.esh[w] = scales[w].stride_h; a.ess[w] = scales[w].stride_s;
    }
    a.table = block_table;
    a.tsb = table_stride_b;
    a.num_pages = num_pages;
    a.start_dev = start_dev;
    a.n_new_dev = n_new_dev;
    a.start = start;
    a.n_new = n_new;
    a.Hkv = Hkv; a.T = T; a.Sk = Sk; a.blk = block; a.G = D / 32;
    a.lanes = lanes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)groups, 2);
    if (dtype == RSA_BF16) kv4_append_kernel<bf16_tag><<<grid, KV4_NT, 0, s>>>(a);
    else kv4_append_kernel<fp16_tag><<<grid, KV4_NT, 0, s>>>(a);
    return rsa_launch_status();
}
