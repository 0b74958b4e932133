// Where a batch item's query rows come from, and how many there are (DESIGN.md sections 5.16 - 5.18): the row sources that the
// decode / extend kernels (rsa_decode.hip) and the selection kernels (rsa_block_select.hip) are instantiated over, and what the
// three packed calls (rsa_block_sparse_extend_packed, rsa_block_select_pooled_packed, rsa_kv8_append_packed) share.
//
//   RowsPadded       q [B, H, Sq, D]: every item has Sq rows.  It has no size: a kernel over it carries no argument for it.
//   RowsCounted      the same q with q_len, DEVICE int32 [B]: item b has q_len[b] rows, clamped into [0, Sq].
//   RowsPacked       q [T, H, D] holds the items back to back: item b is rows [row_start[b], row_start[b + 1]) of it, at most Sq
//                    (= M) of them.  piece_start, B and steps take a row group or a row of q to its item (pk_find).
//   RowsAt           first(b) alone, = row_start[b], for the packed selection's pool kernel: the scan has written the clamped counts
//                    by then, so it takes them as RowsCounted with RowsAt beside it, and the other kernels are RowsCounted's.
//   They have        count(b, Sq)   the item's rows (b: an int or a long, as the caller holds it; RowsPacked: its kernels in
//                                   rsa_decode.hip take the difference of row_start themselves);
//                    first(b)       the item's first row in q: 0 where q has a batch dimension;
//                    SHORT          whether count can fall below Sq at all (a group, a block or a row can then be padding);
//                    BATCHED        whether q has a batch dimension (item b at b * stride_b) or is packed (at row first(b)).
//   WithRows<A, R>   the kernel arguments A with the source behind them; every member of A keeps its offset.
//
// The packed batch (section 5.18): cu_seqlens_q, DEVICE int32 [B + 1], says where each item starts.
//
//   pk_scan_kernel   ONE workgroup.  s_b = the running maximum of clamp(cu[b], 0, T), n_b = min(s_{b+1} - s_b, M): whatever cu holds,
//                    0 <= s_0 <= .. <= s_B <= T and the items' rows [s_b, s_b + n_b) are disjoint ranges of [0, T).  It writes
//                    row_start [B + 1] = s, and where asked n_rows [B] = n and piece_start [B + 1], the exclusive prefix sums of
//                    pk_pieces(n_b).  Thread i owns `per` consecutive entries; the running maximum and the sums cross threads by
//                    two scans through LDS.  Every loop bound is a host value.
//   pk_find          the largest b in [0, B) with start[b] <= x, by `steps` = ceil(log2 B) halvings of [0, B - 1]: every index it
//                    forms lies in [0, B - 1] whatever the array holds.
//
// No address is formed from a value of cu: the kernels behind the scan read row_start / n_rows / piece_start only.
#pragma once
#include "rsa_common.h"

#define PK_NT 256

struct PkScan {
    int B, T, M;            // items, rows of q (the token budget), rows of an item at most
    int blk, qg, cpb;       // the row groups of the extend call (piece_start only): rows of a query block, of a group, groups per
                            // full query block
    int per;                // entries per thread: ceil((B + 1) / PK_NT)
};

// Row groups of an item of n rows: cpb per full query block and ceil(rem / qg) for the rows behind them.
__host__ __device__ __forceinline__ int pk_pieces(int n, int blk, int qg, int cpb) {
    const int qb = n / blk;
    return qb * cpb + (n - qb * blk + qg - 1) / qg;
}

static inline int pk_steps(int B) {
    int steps = 0;
    while ((1L << steps) < B) ++steps;
    return steps;
}

__device__ __forceinline__ int pk_find(const int32_t* start, int B, int steps, int x) {
    int lo = 0, hi = B - 1;
    for (int it = 0; it < steps; ++it) {
        const int mid = (lo + hi + 1) >> 1;         // in [lo, hi]: within [0, B - 1]
        const int v = start[mid];
        if (lo < hi) {
            if (v <= x) lo = mid;
            else hi = mid - 1;
        }
    }
    return lo;
}

struct RowsPadded {
    int none[0];                // (an empty struct would still take 4 bytes as a kernel argument; this takes none)
    static constexpr bool SHORT = false, BATCHED = true;
    template <typename I> __device__ __forceinline__ int count(I, int Sq) const { return Sq; }
    __device__ __forceinline__ const int32_t* counts() const { return nullptr; }
    template <typename I> __device__ __forceinline__ long first(I) const { return 0; }
};

struct RowsCounted {
    const int32_t* q_len;       // DEVICE [B]
    static constexpr bool SHORT = true, BATCHED = true;
    template <typename I> __device__ __forceinline__ int count(I b, int Sq) const { return min(max(q_len[b], 0), Sq); }
    __device__ __forceinline__ const int32_t* counts() const { return q_len; }
    template <typename I> __device__ __forceinline__ long first(I) const { return 0; }
};

struct RowsAt {
    const int32_t* row_start;   // DEVICE [B + 1], written by pk_scan_kernel
    template <typename I> __device__ __forceinline__ long first(I b) const { return row_start[b]; }
};

struct RowsPacked {
    const int32_t *row_start, *piece_start;     // DEVICE [B + 1] each, written by pk_scan_kernel: sanitised, ascending
    int B, steps;                               // items; halvings of the search (pk_steps)
    static constexpr bool SHORT = true, BATCHED = false;
    template <typename I> __device__ __forceinline__ long first(I b) const { return row_start[b]; }
    __device__ __forceinline__ int item_of_row(int t) const { return pk_find(row_start, B, steps, t); }     // the item of row t of q
};

template <typename A, typename R>
struct WithRows : A {
    [[no_unique_address]] R src;
};

// (a template so that every translation unit that launches it carries its own copy)
template <int UNUSED>
__global__ __launch_bounds__(PK_NT) void pk_scan_kernel(const int32_t* __restrict__ cu, PkScan s, int32_t* __restrict__ row_start,
                                                        int32_t* __restrict__ n_rows, int32_t* __restrict__ piece_start) {
    __shared__ int red[PK_NT];
    const int tid = threadIdx.x, j0 = tid * s.per;
    auto at = [&](int j) { return min(max(cu[j], 0), s.T); };       // (j <= B asked of the caller)
    int mx = 0;
    for (int e = 0; e < s.per; ++e)
        if (j0 + e <= s.B) mx = max(mx, at(j0 + e));
    red[tid] = mx;
    __syncthreads();
    for (int d = 1; d < PK_NT; d <<= 1) {
        const int o = tid >= d ? red[tid - d] : 0;
        __syncthreads();
        red[tid] = max(red[tid], o);
        __syncthreads();
    }
    const int before = tid ? red[tid - 1] : 0;      // the running maximum in front of this thread's entries
    __syncthreads();
    int run = before, sum = 0;
    for (int e = 0; e < s.per; ++e) {
        const int j = j0 + e;
        if (j > s.B) break;
        run = max(run, at(j));
        row_start[j] = run;
        if (j < s.B) {
            const int n = min(max(run, at(j + 1)) - run, s.M);
            if (n_rows) n_rows[j] = n;
            sum += pk_pieces(n, s.blk, s.qg, s.cpb);
        }
    }
    if (!piece_start) return;       // (uniform)
    red[tid] = sum;
    __syncthreads();
    for (int d = 1; d < PK_NT; d <<= 1) {
        const int o = tid >= d ? red[tid - d] : 0;
        __syncthreads();
        red[tid] += o;
        __syncthreads();
    }
    run = before;
    sum = tid ? red[tid - 1] : 0;
    for (int e = 0; e < s.per; ++e) {
        const int j = j0 + e;
        if (j > s.B) break;
        run = max(run, at(j));
        piece_start[j] = sum;       // (entry B: the total, from the thread that owns it)
        if (j < s.B) sum += pk_pieces(min(max(run, at(j + 1)) - run, s.M), s.blk, s.qg, s.cpb);
    }
}

// The scan's launch.  n_rows / piece_start may be null (not written); blk, qg, cpb are read for piece_start only.
static inline void pk_scan_launch(const int32_t* cu, int B, int T, int M, int blk, int qg, int cpb, int32_t* row_start,
                                  int32_t* n_rows, int32_t* piece_start, hipStream_t s) {
    const PkScan a = {B, T, M, blk, qg > 0 ? qg : 1, cpb, (int)(((long)B + 1 + PK_NT - 1) / PK_NT)};
    pk_scan_kernel<0><<<dim3(1), PK_NT, 0, s>>>(cu, a, row_start, n_rows, piece_start);
}

// Bytes of n int32 values at the head of a workspace, rounded so that what follows stays 16-byte aligned.
static inline size_t pk_head_bytes(long n) { return ((size_t)n * sizeof(int32_t) + 15) & ~(size_t)15; }
