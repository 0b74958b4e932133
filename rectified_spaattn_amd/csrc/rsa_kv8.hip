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
#include "rsa_kv_append.h"
#include "rsa_rows.h"

#include <type_traits>

struct Kv8Own {
    const float* scale[2];              // [Hkv] each
    static constexpr int ELEMS = 8, ALIGN = 8;      // one lane: 8 elements of a row, an 8-byte store
};

// The packed kernel's arguments: the padded kernel's (T = the rows of k_new, lanes = T * Hkv * CH, ssb unused) and the items.
struct Kv8Packed : KvAppendArgs<Kv8Own> {
    const int32_t* row_start;           // DEVICE [B + 1], written by pk_scan_kernel
    int B, steps;
    __device__ __forceinline__ int item_of(int row) const { return pk_find(row_start, B, steps, row); }
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

template <typename Tag, bool PK = false>
__global__ __launch_bounds__(KV_NT) void kv8_append_kernel(
    typename std::conditional<PK, Kv8Packed, KvAppendArgs<Kv8Own>>::type a) {
    KvPlace at;
    if (!kv_place<PK>(a, (long)blockIdx.x * KV_NT + threadIdx.x, at)) return;
    const uint4 x = *reinterpret_cast<const uint4*>(KV_SEL(src) + (PK ? 0 : at.b * KV_SEL(ssb)) + (long)at.hk * KV_SEL(ssh) +
                                                    at.srow * KV_SEL(sss) + 8 * at.c);
    const float s = KV_SEL(x.scale)[at.hk];
    uint2 o;
    o.x = kv8_quant4<Tag>(x.x, x.y, s);
    o.y = kv8_quant4<Tag>(x.z, x.w, s);
    *reinterpret_cast<uint2*>(KV_SEL(dst) + at.item * KV_SEL(dsb) + (long)at.hk * KV_SEL(dsh) + at.row * KV_SEL(dss) + 8 * at.c) = o;
}

// Both entries.  cu: the packed entry's cu_seqlens (then T = the rows of k_new / v_new, n_new is not read and item_ws, DEVICE
// int32 [B + 1], takes the scan's row_start); null: the padded entry.
static int kv8_run(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                   rsa_out4 k_cache, rsa_out4 v_cache, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                   const int32_t* start_dev, int start, const int32_t* n_new_dev, int n_new, const float* k_scale,
                   const float* v_scale, const int32_t* cu, int32_t* item_ws, bool packed, void* stream) {
    if (packed && (!cu || !item_ws || ((reinterpret_cast<uintptr_t>(cu) | reinterpret_cast<uintptr_t>(item_ws)) & 3) || B >= 0x7FFFFFFF))
        return RSA_ERR_BAD_ARG;
    Kv8Packed a;
    dim3 grid;
    const int st = kv_append_door(B, Hkv, T, Sk, D, dtype, block, {k_new, v_new}, {k_cache, v_cache}, block_table, table_stride_b,
                                  num_pages, start_dev, start, n_new_dev, n_new, k_scale && v_scale,
                                  reinterpret_cast<uintptr_t>(k_scale) | reinterpret_cast<uintptr_t>(v_scale), packed, a, grid);
    if (st != RSA_OK) return st;
    a.x.scale[0] = k_scale;
    a.x.scale[1] = v_scale;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (packed) {
        a.row_start = item_ws;
        a.B = B;
        a.steps = pk_steps(B);
        pk_scan_launch(cu, B, T, T, block, 0, 0, item_ws, nullptr, nullptr, s);
        if (dtype == RSA_BF16) kv8_append_kernel<bf16_tag, true><<<grid, KV_NT, 0, s>>>(a);
        else kv8_append_kernel<fp16_tag, true><<<grid, KV_NT, 0, s>>>(a);
        return rsa_launch_status();
    }
    const KvAppendArgs<Kv8Own>& a0 = a;
    if (dtype == RSA_BF16) kv8_append_kernel<bf16_tag><<<grid, KV_NT, 0, s>>>(a0);
    else kv8_append_kernel<fp16_tag><<<grid, KV_NT, 0, s>>>(a0);
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
