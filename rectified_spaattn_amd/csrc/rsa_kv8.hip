// The writer of the e4m3 K/V cache (include/rsa.h: rsa_kv8_append): new K / V rows of the query's 2-byte
// type become one-byte e4m3 codes under one static fp32 scale per K/V head and land in a contiguous or paged cache.  One kernel,
// plain HIP C++, a memory-bound copy:
//
//   kv8_append_kernel   one lane per 8 elements of a new row: a 16-byte load, eight divisions, an 8-byte store.  blockIdx.y picks
//                       K or V.  Token t < n_new[b] of batch item b goes to position start[b] + t; a position at or beyond the
//                       capacity, or (paged) one whose table entry lies outside [0, num_pages), is dropped: no address is formed
//                       from an unchecked index.  The call writes the D bytes of each placed row and no other byte.
//
// Byte contract per element: y = x / scale[hk] as ONE IEEE fp32 division (this file is compiled with -ffp-contract=off), y clamped
// to [-448, 448], then v_cvt_pk_fp8_f32: round to nearest even, subnormals kept (rsa_fp8_emit.h); a NaN quotient becomes the
// NaN code with the sign bit of its input.  That is (x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn) bit for bit.
// The scales are not checked: a scale that is zero, negative, infinite or NaN garbles the rows of its head and nothing else,
// since no address depends on a scale.
//
// The packed form (rsa_kv8_append_packed) is an instantiation of its own, PK: k_new / v_new are [T, Hkv, D]
// with cu_seqlens, and token t < n_b of item b is row s_b + t of them (rsa_rows.h: s the sanitised starts, n_b = s_{b+1} - s_b).
// One lane per 8 elements of a row of [0, T): the row's item by pk_find over row_start, which pk_scan_kernel wrote; a row of no
// item places nothing.
#include "rsa_common.h"
#include "rsa_rows.h"

#include <type_traits>

#define KV8_NT 256

struct Kv8Args {
    const unsigned short* src[2];       // k_new, v_new [B, Hkv, T, D]: strides in elements
    long ssb[2], ssh[2], sss[2];
    unsigned char* dst[2];              // the caches [B, Hkv, Sk, D] or page pools [P, Hkv, blk, D]: strides in bytes
    long dsb[2], dsh[2], dss[2];
    const float* scale[2];              // [Hkv] each
    const int32_t* table;               // [B, >= Sk / blk] or null: contiguous caches
    long tsb;
    int num_pages;
    const int32_t *start_dev, *n_new_dev;       // device values (clamped here) or null: the host values
    int start, n_new;
    int Hkv, T, Sk, blk, CH;            // CH = D / 8 lanes per row
    long lanes;                         // B * Hkv * T * CH
};

template <typename Tag>
__device__ __forceinline__ unsigned kv8_quant4(unsigned w0, unsigned w1, float s) {
    const unsigned short e[4] = {(unsigned short)(w0 & 0xFFFFu), (unsigned short)(w0 >> 16), (unsigned short)(w1 & 0xFFFFu),
                                 (unsigned short)(w1 >> 16)};
    float y[4];
    unsigned nan = 0;       // the NaN codes of the quotients that are NaN, each with the sign of its input (bit 15 of both types)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float d = __fdiv_rn(rsa_to_f32<Tag>(e[i]), s);
        y[i] = fminf(fmaxf(d, -448.f), 448.f);      // (fminf / fmaxf drop a NaN: its code is put in below)
        if (d != d) nan |= (0x7Fu | ((unsigned)(e[i] >> 15) << 7)) << (8 * i);
    }
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], r, true);
    // A NaN keeps its sign, as on torch's CPU path (NaN / s is the operand quieted): the division sequence of the device does not
    // promise that, so the code is formed from the input's sign bit.  A NaN code has all seven low bits set: or-ing it in is enough
    // once the sign bit of the clamped stand-in (+-448 or 0) is cleared.
    const unsigned lanes = ((nan >> 6) & 0x01010101u) * 0xFFu;      // 0xFF in every byte that holds a NaN code
    return ((unsigned)r & ~lanes) | nan;
}

// The packed kernel's arguments: the padded kernel's (T = the rows of k_new, lanes = T * Hkv * CH, ssb unused) and the items.
struct Kv8Packed : Kv8Args {
    const int32_t* row_start;           // DEVICE [B + 1], written by pk_scan_kernel
    int B, steps;
};

template <typename Tag, bool PK = false>
__global__ __launch_bounds__(KV8_NT) void kv8_append_kernel(typename std::conditional<PK, Kv8Packed, Kv8Args>::type a) {
    const long g = (long)blockIdx.x * KV8_NT + threadIdx.x;
    if (g >= a.lanes) return;
    const int w = blockIdx.y;           // 0: K, 1: V
    const int c = (int)(g % a.CH);
    int t = (int)((g / a.CH) % a.T);
    int hk = (int)((g / ((long)a.CH * a.T)) % a.Hkv);
    long b = g / ((long)a.CH * a.T * a.Hkv);
    long srow = t;                      // the token's row in k_new / v_new (behind b * ssb)
    if constexpr (PK) {                 // lanes run (row, head, piece): the row's item, and its index in it
        hk = (int)((g / a.CH) % a.Hkv);
        srow = g / ((long)a.CH * a.Hkv);
        b = pk_find(a.row_start, a.B, a.steps, (int)srow);
        t = (int)srow - a.row_start[b];
        if (t < 0 || t >= a.row_start[b + 1] - a.row_start[b]) return;     // a row of no item
    }
    const int n = PK ? a.T : (a.n_new_dev ? min(max(a.n_new_dev[b], 0), a.T) : a.n_new);
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
#define KV8_SEL(f) (w ? a.f[1] : a.f[0])      // (uniform selects: the argument arrays are never indexed by a register)
    const uint4 x = *reinterpret_cast<const uint4*>(KV8_SEL(src) + (PK ? 0 : b * KV8_SEL(ssb)) + (long)hk * KV8_SEL(ssh) +
                                                    srow * KV8_SEL(sss) + 8 * c);
    const float s = KV8_SEL(scale)[hk];
    uint2 o;
    o.x = kv8_quant4<Tag>(x.x, x.y, s);
    o.y = kv8_quant4<Tag>(x.z, x.w, s);
    *reinterpret_cast<uint2*>(KV8_SEL(dst) + item * KV8_SEL(dsb) + (long)hk * KV8_SEL(dsh) + row * KV8_SEL(dss) + 8 * c) = o;
#undef KV8_SEL
}

// Both entries.  cu: the packed entry's cu_seqlens (then T = the rows of k_new / v_new, n_new is not read and item_ws, DEVICE
// int32 [B + 1], takes the scan's row_start); null: the padded entry.
static int kv8_run(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                   rsa_out4 k_cache, rsa_out4 v_cache, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                   const int32_t* start_dev, int start, const int32_t* n_new_dev, int n_new, const float* k_scale,
                   const float* v_scale, const int32_t* cu, int32_t* item_ws, bool packed, void* stream) {
    if (packed && (!cu || !item_ws || ((reinterpret_cast<uintptr_t>(cu) | reinterpret_cast<uintptr_t>(item_ws)) & 3) || B >= 0x7FFFFFFF))
        return RSA_ERR_BAD_ARG;
    if (B <= 0 || Hkv <= 0 || T <= 0 || Sk <= 0) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (!start_dev && (start < 0 || start > Sk)) return RSA_ERR_BAD_ARG;
    if (!n_new_dev && (n_new < 0 || n_new > T)) return RSA_ERR_BAD_ARG;
    if (!k_scale || !v_scale) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(k_new) != RSA_OK || rsa_check_tensor(v_new) != RSA_OK) return RSA_ERR_BAD_ARG;
    const rsa_tensor4 src[2] = {k_new, v_new};
    const rsa_out4 dst[2] = {k_cache, v_cache};
    for (int w = 0; w < 2; ++w) {
        if (src[w].stride_b < 0 || src[w].stride_h < 0 || src[w].stride_s < 0) return RSA_ERR_BAD_ARG;
        if (!dst[w].ptr || (reinterpret_cast<uintptr_t>(dst[w].ptr) & 7)) return RSA_ERR_BAD_ARG;      // 8-byte stores
        if (dst[w].stride_b < 0 || dst[w].stride_h < 0 || dst[w].stride_s < 0) return RSA_ERR_BAD_ARG;
        if ((dst[w].stride_b % 8) || (dst[w].stride_h % 8) || (dst[w].stride_s % 8)) return RSA_ERR_BAD_ARG;
    }
    if (block_table && (num_pages <= 0 || table_stride_b < 0 || Sk % block)) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(start_dev) | reinterpret_cast<uintptr_t>(n_new_dev) |
         reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale)) & 3)
        return RSA_ERR_BAD_ARG;
    const long lanes = (packed ? 1L : (long)B) * Hkv * T * (D / 8);
    const long groups = (lanes + KV8_NT - 1) / KV8_NT;
    if (groups > 0x7FFFFFFFl) return RSA_ERR_UNSUPPORTED;

    Kv8Packed a;
    for (int w = 0; w < 2; ++w) {
        a.src[w] = static_cast<const unsigned short*>(src[w].ptr);
        a.ssb[w] = src[w].stride_b; a.ssh[w] = src[w].stride_h; a.sss[w] = src[w].stride_s;
        a.dst[w] = static_cast<unsigned char*>(dst[w].ptr);
        a.dsb[w] = dst[w].stride_b; a.dsh[w] = dst[w].stride_h; a.dss[w] = dst[w].stride_s;
    }
    a.scale[0] = k_scale;
    a.scale[1] = v_scale;
    a.table = block_table;
    a.tsb = table_stride_b;
    a.num_pages = num_pages;
    a.start_dev = start_dev;
    a.n_new_dev = n_new_dev;
    a.start = start;
    a.n_new = n_new;
    a.Hkv = Hkv; a.T = T; a.Sk = Sk; a.blk = block; a.CH = D / 8;
    a.lanes = lanes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)groups, 2);
    if (packed) {
        a.row_start = item_ws;
        a.B = B;
        a.steps = pk_steps(B);
        pk_scan_launch(cu, B, T, T, block, 0, 0, item_ws, nullptr, nullptr, s);
        if (dtype == RSA_BF16) kv8_append_kernel<bf16_tag, true><<<grid, KV8_NT, 0, s>>>(a);
        else kv8_append_kernel<fp16_tag, true><<<grid, KV8_NT, 0, s>>>(a);
        return rsa_launch_status();
    }
    const Kv8Args& a0 = a;
    if (dtype == RSA_BF16) kv8_append_kernel<bf16_tag><<<grid, KV8_NT, 0, s>>>(a0);
    else kv8_append_kernel<fp16_tag><<<grid, KV8_NT, 0, s>>>(a0);
    return rsa_launch_status();
}

extern "C" int rsa_kv8_append(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                              rsa_out4 k_cache, rsa_out4 v_cache, const int32_t* block_table, int64_t table_stride_b,
                              int num_pages, const int32_t* start_dev, int start, const int32_t* n_new_dev, int n_new,
                              const float* k_scale, const float* v_scale, void* stream) {
    return kv8_run(B, Hkv, T, Sk, D, dtype, block, k_new, v_new, k_cache, v_cache, block_table, table_stride_b, num_pages, start_dev,
                   start, n_new_dev, n_new, k_scale, v_scale, nullptr, nullptr, false, stream);
}

// The packed form: k_new / v_new [T, Hkv, D] read through stride_h and stride_s (a row of the packed tensor; stride_b is not read),
// cu_seqlens_dev DEVICE int32 [B + 1] where n_new stood, item_ws DEVICE int32 [B + 1] scratch.  Two launches.
extern "C" int rsa_kv8_append_packed(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                                     rsa_out4 k_cache, rsa_out4 v_cache, const int32_t* block_table, int64_t table_stride_b,
                                     int num_pages, const int32_t* start_dev, int start, const int32_t* cu_seqlens_dev,
                                     int32_t* item_ws, const float* k_scale, const float* v_scale, void* stream) {
    k_new.stride_b = 0, v_new.stride_b = 0;
    return kv8_run(B, Hkv, T, Sk, D, dtype, block, k_new, v_new, k_cache, v_cache, block_table, table_stride_b, num_pages, start_dev,
                   start, nullptr, T, k_scale, v_scale, cu_seqlens_dev, item_ws, true, stream);
}
