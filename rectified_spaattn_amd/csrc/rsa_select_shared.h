// What the selection unit (rsa_block_select.hip) shares with a score pass in a unit of its own (rsa_select_antidiag.hip; DESIGN.md
// section 5.22): the ordered keys the select kernels rank, the visible prefix of a list row, and the two host calls through which
// such a pass has its arguments checked and its keys ranked.
#pragma once
#include "rsa_common.h"

#define SEL_NT 256
#define SEL_MAX_NK 8192

// fp32 -> u32 with the order of the floats (-0 counts as +0).
__device__ __forceinline__ unsigned sel_key(float x) {
    unsigned u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

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

// A selection over padded rows whose scores come from elsewhere: rsa_block_select_ragged's arguments without k, the workspace and
// the row counts.  p16 = -1: plain top-k.
struct sel_ext_call {
    int B, H, Hkv, Hl, Sq, Sk, D, dtype, blk, NQ, NK;
    rsa_tensor4 q;
    const int32_t* kv_len;
    int kv_valid, causal, top_k, keep_first, keep_local;
    uint32_t* bitmask;
    int32_t* cols;
    int32_t* counts;
    float* scores;
    int p16;
    float c;
    float* mass;
};
// The budget check and sel_check of rsa_block_select, with their statuses, in their order.
int sel_ext_check(const sel_ext_call& e);
// The select kernels over the call's B Hl NQ list rows, LOADED from wkeys [B, Hl, NQ, NK].
int sel_ext_select(const sel_ext_call& e, const unsigned* wkeys, void* stream);
