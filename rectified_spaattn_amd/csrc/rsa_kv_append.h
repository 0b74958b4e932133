// What the writers of the K/V caches share (rsa_kv8.hip: e4m3; rsa_kv4.hip: MXFP4, section 5.23): the
// kernel arguments, the rule that takes a token of k_new / v_new to its row of a live cache, and the host door in front of a launch.
// A unit keeps its byte contract, its quantising body, the kernel shell around kv_place and its extern "C" entries.
//
//   KvAppendArgs<X>  the arguments of a writer kernel.  X is the unit's own part and sits between the destination's strides and
//                    `table`, where each unit's own members stood, so every member keeps its kernarg offset.  X also names
//                    ELEMS, the elements of a row that one lane converts, and ALIGN, the bytes of the store they leave by.
//   kv_place         lane g -> (w, c, b, hk, srow, item, row), or false: the lane places nothing.  Token t < n_new[b] of batch item
//                    b goes to position start[b] + t; a position at or beyond the capacity, or (paged) one whose table entry lies
//                    outside [0, num_pages), is dropped: no address is formed from an unchecked index.
//   kv_append_door   the refusals both entries make, in their order, and the fill of what the arguments share.
#pragma once
#include "rsa_common.h"

#define KV_NT 256
// K's or V's member f, for a kernel shell: it names the shell's arguments `a` and its KvPlace `at`, and nothing else may use it.
#define KV_SEL(f) (at.w ? a.f[1] : a.f[0])       // (uniform selects: the argument arrays are never indexed by a register)

template <typename X>
struct KvAppendArgs {
    const unsigned short* src[2];       // k_new, v_new [B, Hkv, T, D]: strides in elements
    long ssb[2], ssh[2], sss[2];
    unsigned char* dst[2];              // the caches [B, Hkv, Sk, row bytes] or page pools [P, Hkv, blk, row bytes]: strides in bytes
    long dsb[2], dsh[2], dss[2];
    X x;
    const int32_t* table;               // [B, >= Sk / blk] or null: contiguous caches
    long tsb;
    int num_pages;
    const int32_t *start_dev, *n_new_dev;       // device values (clamped here) or null: the host values
    int start, n_new;
    int Hkv, T, Sk, blk, CH;            // CH = D / X::ELEMS lanes per row
    long lanes;                         // B * Hkv * T * CH
};

struct KvPlace {
    int w, c, hk;                       // 0: K, 1: V; the lane's piece of the row; the K/V head
    long b, srow;                       // the batch item; the token's row in k_new / v_new (behind b * ssb)
    long item, row;                     // the cache's batch item or page, and the row in it
};

template <bool PK, typename A>
__device__ __forceinline__ bool kv_place(const A& a, long g, KvPlace& at) {
    if (g >= a.lanes) return false;
    const int w = blockIdx.y;
    const int c = (int)(g % a.CH);
    int t = (int)((g / a.CH) % a.T);
    int hk = (int)((g / ((long)a.CH * a.T)) % a.Hkv);
    long b = g / ((long)a.CH * a.T * a.Hkv);
    long srow = t;
    if constexpr (PK) {                 // A adds row_start [B + 1] and item_of(row) over it (rsa_kv8.hip: Kv8Packed).
                                        // Lanes run (row, head, piece): the row's item, and its index in it
        hk = (int)((g / a.CH) % a.Hkv);
        srow = g / ((long)a.CH * a.Hkv);
        b = a.item_of((int)srow);
        t = (int)srow - a.row_start[b];
        if (t < 0 || t >= a.row_start[b + 1] - a.row_start[b]) return false;    // a row of no item
    }
    const int n = PK ? a.T : (a.n_new_dev ? min(max(a.n_new_dev[b], 0), a.T) : a.n_new);
    if (t >= n) return false;
    const int st = a.start_dev ? min(max(a.start_dev[b], 0), a.Sk) : a.start;
    const long pos = (long)st + t;
    if (pos >= a.Sk) return false;      // beyond the capacity: dropped
    long row = pos, item = b;
    if (a.table) {
        const int page = a.table[b * a.tsb + pos / a.blk];
        if (page < 0 || page >= a.num_pages) return false;      // no page: dropped
        item = page;
        row = pos % a.blk;
    }
    at = {w, c, hk, b, srow, item, row};
    return true;
}

// own_ok: the unit's own refusals (all RSA_ERR_BAD_ARG, like their neighbours here); own_ptrs: its device pointers that are read as
// 4-byte words, or-ed.  packed: T = the rows of k_new and the lanes run over them alone.  On RSA_OK `a` holds everything but a.x.
template <typename X>
static int kv_append_door(int B, int Hkv, int T, int Sk, int D, int dtype, int block, const rsa_tensor4 (&src)[2],
                          const rsa_out4 (&dst)[2], const int32_t* block_table, int64_t table_stride_b, int num_pages,
                          const int32_t* start_dev, int start, const int32_t* n_new_dev, int n_new, bool own_ok, uintptr_t own_ptrs,
                          bool packed, KvAppendArgs<X>& a, dim3& grid) {
    if (B <= 0 || Hkv <= 0 || T <= 0 || Sk <= 0) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (!start_dev && (start < 0 || start > Sk)) return RSA_ERR_BAD_ARG;
    if (!n_new_dev && (n_new < 0 || n_new > T)) return RSA_ERR_BAD_ARG;
    if (!own_ok) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(src[0]) != RSA_OK || rsa_check_tensor(src[1]) != RSA_OK) return RSA_ERR_BAD_ARG;
    for (int w = 0; w < 2; ++w) {
        if (src[w].stride_b < 0 || src[w].stride_h < 0 || src[w].stride_s < 0) return RSA_ERR_BAD_ARG;
        if (!dst[w].ptr || (reinterpret_cast<uintptr_t>(dst[w].ptr) % X::ALIGN)) return RSA_ERR_BAD_ARG;       // the lane's store
        if (dst[w].stride_b < 0 || dst[w].stride_h < 0 || dst[w].stride_s < 0) return RSA_ERR_BAD_ARG;
        if ((dst[w].stride_b % X::ALIGN) || (dst[w].stride_h % X::ALIGN) || (dst[w].stride_s % X::ALIGN)) return RSA_ERR_BAD_ARG;
    }
    if (block_table && (num_pages <= 0 || table_stride_b < 0 || Sk % block)) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(block_table) | reinterpret_cast<uintptr_t>(start_dev) | reinterpret_cast<uintptr_t>(n_new_dev) |
         own_ptrs) & 3)
        return RSA_ERR_BAD_ARG;
    const long lanes = (packed ? 1L : (long)B) * Hkv * T * (D / X::ELEMS);
    const long groups = (lanes + KV_NT - 1) / KV_NT;
    if (groups > 0x7FFFFFFFl) return RSA_ERR_UNSUPPORTED;

    for (int w = 0; w < 2; ++w) {
        a.src[w] = static_cast<const unsigned short*>(src[w].ptr);
        a.ssb[w] = src[w].stride_b; a.ssh[w] = src[w].stride_h; a.sss[w] = src[w].stride_s;
        a.dst[w] = static_cast<unsigned char*>(dst[w].ptr);
        a.dsb[w] = dst[w].stride_b; a.dsh[w] = dst[w].stride_h; a.dss[w] = dst[w].stride_s;
    }
    a.table = block_table;
    a.tsb = table_stride_b;
    a.num_pages = num_pages;
    a.start_dev = start_dev;
    a.n_new_dev = n_new_dev;
    a.start = start;
    a.n_new = n_new;
    a.Hkv = Hkv; a.T = T; a.Sk = Sk; a.blk = block; a.CH = D / X::ELEMS;
    a.lanes = lanes;
    grid = dim3((unsigned)groups, 2);
    return RSA_OK;
}
