// Caller-supplied block masks <-> the kept lists K5 walks (include/rsa.h: rsa_block_mask_to_lists, rsa_lists_to_block_mask).
//
// The list contract is K3's (rsa_stats.hip, the end of select_mask_kernel): per (bh, query block) row
//     bitmask [row][NW]  bit j % 32 of word j / 32 = block j kept, NW = ceil(NK / 32), bits >= NK zero
//     cols    [row][NK]  the kept block indices in ascending order; only the first counts[row] entries are written
//     counts  [row]
// with NK the row's length (NB_total of a layout).  At 64-token blocks K5 forms the union of query blocks 2i and 2i + 1 itself
// from cols / counts (rsa_attn_kernel.hip), so the same three buffers serve both block sizes.
#include "rsa_common.h"

// One wave per mask row, the row in 64-byte steps: lane l reads byte b0 + l (coalesced 1-byte loads, sixteen steps issued
// before the first is used), a ballot turns the 64 bytes into the bits K3's writer produces for the same step -- the two bitmask
// words of the step are parked in lanes 2u and 2u + 1 and the 32 words of sixteen steps leave in one store instruction, the
// ascending list entries go to the running offset plus the prefix popcount of the lanes below.  The mask row needs no alignment:
// a row of the HunyuanVideo 720p mask is 902 bytes long.
__global__ __launch_bounds__(256) void block_mask_to_lists_kernel(const uint8_t* __restrict__ mask, long sb, long sh, long sq,
                                                                  int H, int NQ, int NK, long rows, uint32_t* __restrict__ bitmask,
                                                                  int32_t* __restrict__ cols, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long bh = row / NQ;
    const int q = (int)(row % NQ);
    const uint8_t* src = mask + (bh / H) * sb + (bh % H) * sh + (long)q * sq;
    const int NW = (NK + 31) >> 5;
    int32_t* cr = cols + row * NK;
    uint32_t* wr = bitmask + row * NW;
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr int U = 16;   // 64-byte steps in flight per lane
    int off = 0;
    for (int c0 = 0; c0 < NK; c0 += 64 * U) {
        uint8_t v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = c0 + 64 * u + lane;
            v[u] = j < NK ? src[j] : (uint8_t)0;
        }
        unsigned wd = 0u;   // bitmask word (c0 >> 5) + lane, lanes 0 .. 2U - 1
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b0 = c0 + 64 * u;
            if (b0 < NK) {   // (uniform over the wave)
                const bool f = v[u] != 0;
                const unsigned long long m = __ballot(f);
                if (f) cr[off + __popcll(m & below)] = b0 + lane;
                off += __popcll(m);
                wd = lane == 2 * u ? (unsigned)m : (lane == 2 * u + 1 ? (unsigned)(m >> 32) : wd);
            }
        }
        const int wi = (c0 >> 5) + lane;   // (the words of steps past NK lie at or beyond NW)
        if (lane < 2 * U && wi < NW) wr[wi] = wd;
    }
    if (lane == 0) counts[row] = off;
}

// The inverse: one wave per row, lane l writes bytes l, l + 64, ... of the dense [B, H, NQ, NK] 0/1 mask from the bitmask words.
__global__ __launch_bounds__(256) void lists_to_block_mask_kernel(const uint32_t* __restrict__ bitmask, int NK, long rows,
                                                                  uint8_t* __restrict__ mask) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int NW = (NK + 31) >> 5;
    const uint32_t* wr = bitmask + row * NW;
    uint8_t* dst = mask + row * NK;
    for (int j = lane; j < NK; j += 64) dst[j] = (uint8_t)((wr[j >> 5] >> (j & 31)) & 1u);
}

static int check_rows(int B, int H, int NQ, int NK, long* rows) {
    if (B <= 0 || H <= 0 || NQ <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (NK > 8192) return RSA_ERR_UNSUPPORTED;   // K5's key-block limit (its kept list lives in LDS as u16)
    *rows = (long)B * H * NQ;
    if ((*rows + 3) / 4 > 0x7FFFFFFFL) return RSA_ERR_UNSUPPORTED;
    return RSA_OK;
}

extern "C" int rsa_block_mask_to_lists(int B, int H, int NQ, int NK, const uint8_t* mask, int64_t mask_stride_b,
                                       int64_t mask_stride_h, int64_t mask_stride_q, uint32_t* bitmask, int32_t* cols,
                                       int32_t* counts, void* stream) {
    long rows = 0;
    const int st = check_rows(B, H, NQ, NK, &rows);
    if (st != RSA_OK) return st;
    if (!mask || !bitmask || !cols || !counts) return RSA_ERR_BAD_ARG;
    if (mask_stride_b < 0 || mask_stride_h < 0 || mask_stride_q < 0) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(bitmask) | reinterpret_cast<uintptr_t>(cols) | reinterpret_cast<uintptr_t>(counts)) & 3)
        return RSA_ERR_BAD_ARG;
    block_mask_to_lists_kernel<<<dim3((unsigned)((rows + 3) / 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        mask, mask_stride_b, mask_stride_h, mask_stride_q, H, NQ, NK, rows, bitmask, cols, counts);
    return rsa_launch_status();
}

extern "C" int rsa_lists_to_block_mask(int B, int H, int NQ, int NK, const uint32_t* bitmask, uint8_t* mask, void* stream) {
    long rows = 0;
    const int st = check_rows(B, H, NQ, NK, &rows);
    if (st != RSA_OK) return st;
    if (!bitmask || !mask || (reinterpret_cast<uintptr_t>(bitmask) & 3)) return RSA_ERR_BAD_ARG;
    lists_to_block_mask_kernel<<<dim3((unsigned)((rows + 3) / 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(bitmask, NK, rows,
                                                                                                             mask);
    return rsa_launch_status();
}
