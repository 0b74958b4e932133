// K5 host side: the plan of a launch (rsa_plan_walk: every K5 kernel's), the combine passes behind it, argument checks and
// launches of the 2-byte block-sparse attention kernels (rsa_attn_kernel64.hip, rsa_attn_kernel.hip).
// rsa_block_sparse_fwd, rsa_dense_fwd and rsa_rectified_attention of include/rsa.h live here.
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include "rsa_attn.h"

// =====================================================================================================
// host side
// =====================================================================================================
static int g_k5_tsplit = 1;     // 1 = split-KV for the text query blocks when the partial buffer is given
extern int g_rsa_k3_prefix;
extern int g_rsa_k3_long;
extern int g_rsa_k4_split;
extern int g_rsa_k2_dma;
static int g_k5_tail_split = 1; // the last, partial generation's walks split over its idle slots (rsa_attn.h::rsa_walk_map)
static int g_k5_text_last = 1;  // split text-row pieces at the end of the grid (rsa_attn.h::rsa_walk_map)
static int g_shard_invariant = 0; // rsa_set_shard_invariant: nothing about a row's arithmetic may depend on the size of the launch
static int g_k5_gsync_ratio = 2; // aligned starts: walks that keep 1 / ratio of the keys or more are not held back
int rsa_gsync_ratio() { return g_k5_gsync_ratio; }
static int g_k5_rows256 = 1;    // dense calls at head dim 128: 256-row tiles (0 = 128-row tiles, the sparse calls' form)
static int g_k5_static = 1;     // 64-row kernel, bf16: optimistic static softmax reference in the steady-state loop (0 = online body only)
int rsa_k5_static() { return g_k5_static; }
static int g_k5_gqa_pair = 0;   // grouped-query calls: 1 = two query heads of one K/V head and one list share a workgroup's K/V ring where they can (rsa_gqa_form)
static int g_k5_walk_order = 1; // 64-row kernel, plain sparse calls: runs of one head's walks per XCD generation, in the order of the walk_order kernels (0 = the eighth map, no order kernels)
static int g_k5_order_overlap = 50; // ... a head whose adjacent kept lists share this percentage of their entries or more keeps its units in index order
static int g_k5_gsync = 1;      // aligned starts of the sparse walks (rsa_attn.h): bit 0 = in the 64-row kernel, bit 1 = in the 32-row (64-token blocks) and e4m3 kernels

// Tuning / diagnostics hook (not part of the data path).  The switches are process-global, so the hook only works in a
// process that opted in with the environment variable RSA_TUNING=1 (the A/B tools and the variant tests); a production
// host cannot have its kernels changed under it by another library user.
extern "C" int rsa_set_tuning(const char* key, int value) {
    static const bool enabled = [] { const char* e = getenv("RSA_TUNING"); return e && e[0] == '1'; }();
    if (!key) return RSA_ERR_BAD_ARG;
    if (!enabled) return RSA_ERR_UNSUPPORTED;
    if (strcmp(key, "k3_prefix") == 0) { g_rsa_k3_prefix = value; return RSA_OK; }
    if (strcmp(key, "k3_long") == 0) { g_rsa_k3_long = value; return RSA_OK; }
    if (strcmp(key, "k4_split") == 0) { g_rsa_k4_split = value; return RSA_OK; }
    if (strcmp(key, "k2_dma") == 0) { g_rsa_k2_dma = value; return RSA_OK; }
    if (strcmp(key, "k5_static") == 0) { g_k5_static = value; return RSA_OK; }
    if (strcmp(key, "k5_rows256") == 0) { g_k5_rows256 = value; return RSA_OK; }
    if (strcmp(key, "k5_tsplit") == 0) { g_k5_tsplit = value; return RSA_OK; }
    if (strcmp(key, "k5_gsync") == 0) { g_k5_gsync = value; return RSA_OK; }
    if (strcmp(key, "k5_gsync_ratio") == 0) { g_k5_gsync_ratio = value; return RSA_OK; }
    if (strcmp(key, "k5_text_last") == 0) { g_k5_text_last = value; return RSA_OK; }
    if (strcmp(key, "k5_tail_split") == 0) { g_k5_tail_split = value; return RSA_OK; }
    if (strcmp(key, "k5_walk_order") == 0) { g_k5_walk_order = value; return RSA_OK; }
    if (strcmp(key, "k5_order_overlap") == 0) { g_k5_order_overlap = value; return RSA_OK; }
    if (strcmp(key, "k5_gqa_pair") == 0) { g_k5_gqa_pair = value; return RSA_OK; }
    if (strcmp(key, "fp8_variant") == 0) { rsa_set_fp8_variant(value); return RSA_OK; }
    if (strcmp(key, "fp8_smooth_k") == 0) { rsa_set_fp8_smooth_k(value); return RSA_OK; }
    return RSA_ERR_BAD_ARG;
}

// Merge of the split-KV partials of the text query blocks (K5 wrote, per part, unnormalised O, the running maximum m in
// the log2 domain and the row sum l): one wave per query row, lanes over the head dim.  Rows beyond the valid text rows
// are written as zeros (as the 1-workgroup form does).
template <typename Tag>
__global__ __launch_bounds__(256) void text_combine_kernel(const float* __restrict__ tpart, unsigned short* out,
                                                           long osb, long osh, long oss, int D, int H, int txt0, int ntq,
                                                           int tsplit, int q_text_end, int Sq, long rows_total) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows_total) return;
    const long bhq = row / RSA_BLOCK;
    const int r = (int)(row % RSA_BLOCK);
    const long bh = bhq / ntq;
    const int tq = (int)(bhq % ntq);
    const int grow = txt0 + tq * RSA_BLOCK + r;   // (txt0 = NBv * block: the text rows, in units of 128)
    if (grow >= Sq) return;
    const float* base = tpart + rsa_part_row(bhq * tsplit, r, D);
    const long pstride = rsa_part_row(1, 0, D);
    // (round 6: every load of the row issued up front -- (m, l) of all pieces, then the pieces' values eight at a time -- instead of
    // one dependent round trip per piece; the sums run in the same order, piece 0 first: same bytes)
    constexpr int MAXP = RSA_TEXT_SPLIT;
    float mv[MAXP], lv[MAXP];
#pragma unroll
    for (int s = 0; s < MAXP; ++s) {
        const int sc = s < tsplit ? s : 0;
        const float2 ml = *reinterpret_cast<const float2*>(base + sc * pstride + D);
        mv[s] = s < tsplit ? ml.x : -INFINITY;
        lv[s] = ml.y;
    }
    float M = -INFINITY;
#pragma unroll
    for (int s = 0; s < MAXP; ++s) M = fmaxf(M, mv[s]);
    float L = 0.0f;
    float acc[2] = {0.0f, 0.0f};
#pragma unroll
    for (int s0 = 0; s0 < MAXP; s0 += 8) {
        if (s0 >= tsplit) break;
        float x[8][2];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int sc = s0 + u < tsplit ? s0 + u : 0;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int d = lane + 64 * e;
                x[u][e] = d < D ? base[sc * pstride + d] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u < tsplit) {
                const float wgt = (mv[s0 + u] == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(mv[s0 + u] - M);
                L += lv[s0 + u] * wgt;
                acc[0] += x[u][0] * wgt;
                acc[1] += x[u][1] * wgt;
            }
        }
    }
    const float inv = (grow < q_text_end && L > 0.0f) ? 1.0f / L : 0.0f;
    unsigned short* op = out + (bh / H) * osb + (bh % H) * osh + (long)grow * oss;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int d = lane + 64 * e;
        if (d < D) op[d] = Elem<Tag>::from_f32(acc[e] * inv);
    }
}

extern "C" int rsa_set_shard_invariant(int on) {
    const int prev = g_shard_invariant;
    g_shard_invariant = on != 0;
    return prev;
}

// Tail split (rsa_attn.h::rsa_walk_map): merge the tail_p partials of every tail block, then what the
// kernel's own epilogue does -- normalise, rectify (O . R / l + comp as one fma rounded to fp32), convert, store.  One wave per
// query row, lane = d and d + 64.
template <typename Tag>
__global__ __launch_bounds__(256) void tail_combine_kernel(const float* __restrict__ part, unsigned short* out, long osb, long osh,
                                                           long oss, int H, int NBv, int NBp, int tail_first, int tail_n, int tail_p,
                                                           const float* __restrict__ R, const float* __restrict__ comp, int Sq) {
    constexpr int D = 128;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)tail_n * RSA_BLOCK) return;
    const int t = (int)(row / RSA_BLOCK), r = (int)(row % RSA_BLOCK);
    const int v = tail_first + t, bh = v / NBp;
    const int qblk = rsa_walk_unit(v % NBp, NBp);     // (a tail piece's unit is the eighth map's, with and without an order table: rsa_walk_order.h)
    const int grow = qblk * RSA_BLOCK + r;
    if (qblk >= NBv || grow >= Sq) return;
    const float* base = part + rsa_part_row((long)t * tail_p, r, D);
    const long pstride = rsa_part_row(1, 0, D);
    float M = -INFINITY;
    for (int p = 0; p < tail_p; ++p) M = fmaxf(M, base[p * pstride + D]);
    float L = 0.0f, acc[2] = {0.0f, 0.0f};
    for (int p = 0; p < tail_p; ++p) {
        const float m = base[p * pstride + D], l = base[p * pstride + D + 1];
        const float wgt = (m == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(m - M);
        L += l * wgt;
        acc[0] += base[p * pstride + lane] * wgt;
        acc[1] += base[p * pstride + lane + 64] * wgt;
    }
    const long rowi = (long)bh * NBv + qblk;
    const float sc = (L > 0.0f ? 1.0f / L : 0.0f) * (R ? R[rowi] : 1.0f);
    unsigned short* op = out + (long)(bh / H) * osb + (long)(bh % H) * osh + (long)grow * oss;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int d = lane + 64 * e;
        float x = __builtin_fmaf(acc[e], sc, comp ? comp[rowi * D + d] : 0.0f);
        asm volatile("" : "+v"(x));     // (fma, THEN the conversion: as the kernel's epilogue)
        op[d] = Elem<Tag>::from_f32(x);
    }
}

// The passes behind a K5 kernel: the tail pieces' merge, then the text pieces' (blk: tokens per block, the text rows start at NBv * blk)
int rsa_combine_walk(const WalkArgs& a, int D, int blk, int dtype, hipStream_t s) {
    if (a.tail_n > 0) {
        const dim3 grid((unsigned)(((long)a.tail_n * RSA_BLOCK + 3) / 4));
        if (dtype == RSA_BF16)
            tail_combine_kernel<bf16_tag><<<grid, 256, 0, s>>>(a.tail_part, a.out, a.osb, a.osh, a.oss, a.H, a.NBv, a.NBp, a.tail_first,
                                                             a.tail_n, a.tail_p, a.R, a.comp, a.Sq);
        else
            tail_combine_kernel<fp16_tag><<<grid, 256, 0, s>>>(a.tail_part, a.out, a.osb, a.osh, a.oss, a.H, a.NBv, a.NBp, a.tail_first,
                                                             a.tail_n, a.tail_p, a.R, a.comp, a.Sq);
        const int st = rsa_launch_status();
        if (st != RSA_OK) return st;
    }
    const int ntq = a.NQB - a.NBv;
    const long rows = (long)a.BH * ntq * RSA_BLOCK;
    if (a.tsplit <= 1 || rows <= 0) return RSA_OK;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (dtype == RSA_BF16)
        text_combine_kernel<bf16_tag><<<grid, 256, 0, s>>>(a.tpart, a.out, a.osb, a.osh, a.oss, D, a.H, a.NBv * blk, ntq, a.tsplit,
                                                         a.q_text_end, a.Sq, rows);
    else
        text_combine_kernel<fp16_tag><<<grid, 256, 0, s>>>(a.tpart, a.out, a.osb, a.osh, a.oss, D, a.H, a.NBv * blk, ntq, a.tsplit,
                                                         a.q_text_end, a.Sq, rows);
    return rsa_launch_status();
}

// Aligned starts (rsa_attn.h): the counters are a ring of slots in a __device__ array of the code object (no allocation, nothing
// to free), one slot per launch, cleared in stream order in front of it; a slot shared by two launches in flight (more than
// RING of them, on different streams) costs alignment, never correctness.  Grids of more than two generations only.
__device__ unsigned g_rsa_gsync[RSA_GSYNC_RING][RSA_GSYNC_SLOT_WORDS];
unsigned* rsa_gsync_slot(int which, unsigned grid, int wg_per_cu, hipStream_t s, int* gen) {
    static std::atomic<unsigned*> base[64];
    static std::atomic<unsigned> ticket{0};
    *gen = 32 * (wg_per_cu > 0 ? wg_per_cu : 2);     // 32 CUs per XCD
    if (!(g_k5_gsync & which) || wg_per_cu <= 0 || grid <= 16u * (unsigned)*gen) return nullptr;   // two generations or fewer: nothing to align
    const unsigned gens = ((grid + 7) / 8 + *gen - 1) / *gen;
    int dev = -1;
    if (gens > RSA_GSYNC_MAXG || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    unsigned* b = base[dev].load();
    if (!b) {
        // the generation arithmetic is the full chip's: 8 XCDs x 32 CUs, workgroup b on XCD b & 7 (a partitioned device -- CPX,
        // fewer CUs -- holds fewer workgroups than a generation expects: every first wait would run into its bound)
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus != 256) {
            base[dev].store(reinterpret_cast<unsigned*>(1));
            return nullptr;
        }
        if (hipGetSymbolAddress(reinterpret_cast<void**>(&b), HIP_SYMBOL(g_rsa_gsync)) != hipSuccess) return nullptr;
        base[dev].store(b);
    }
    if (b == reinterpret_cast<unsigned*>(1)) return nullptr;     // (not a full MI355X: see above)
    unsigned* slot = b + (size_t)(ticket.fetch_add(1) % RSA_GSYNC_RING) * RSA_GSYNC_SLOT_WORDS;
    return hipMemsetAsync(slot, 0, (8 + 8 * (size_t)gens) * sizeof(unsigned), s) == hipSuccess ? slot : nullptr;
}
int rsa_wg_per_cu(const void* kernel, int block, size_t lds_bytes) {
    struct Entry { const void* k; size_t lds; int dev, n; };
    static Entry cache[64];
    static std::atomic<int> used{0};
    static std::mutex mu;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const int nu = used.load(std::memory_order_acquire);
    for (int i = 0; i < nu; ++i)
        if (cache[i].k == kernel && cache[i].lds == lds_bytes && cache[i].dev == dev) return cache[i].n;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, lds_bytes) != hipSuccess) n = 0;
    std::lock_guard<std::mutex> lk(mu);
    const int at = used.load();
    if (at < 64) { cache[at] = Entry{kernel, lds_bytes, dev, n}; used.store(at + 1, std::memory_order_release); }
    return n;
}

int rsa_plan_walk(WalkArgs& a, int BH, int D, const WalkPolicy& pol, size_t tpart_bytes, long* nblocks) {
    *nblocks = 0;
    const int blk = pol.blk;
    const int ntq = a.NQB - a.NBv;
    if (a.tpart && tpart_bytes == 0) return RSA_ERR_WORKSPACE;   // capacity not declared (rsa_buffers.tpart_bytes, 0.5.0)
    const size_t piece_bytes = (size_t)rsa_part_row(1, 0, D) * sizeof(float);
    a.BH = BH;
    a.order = nullptr;                       // (launch_attn: the order table of the 64-row kernel's plain sparse calls)
    a.NBp = ((blk == 64 ? (a.NBv + 1) >> 1 : a.NBv) + 7) & ~7;   // (blk 64: pairs of query blocks)
    // split-KV for the dense text rows: without it one workgroup walks every key block of a text query block (902 at the
    // HunyuanVideo shape = 10 kept lists) -- hidden among 21 600 sparse blocks on one GPU, the critical path when the
    // heads are sharded over 8
    const int n_txt_items = (a.kv_text_valid + blk - 1) / blk;
    a.tsplit = 1; a.tper = n_txt_items;
    if (a.mode == MODE_SPARSE && ntq > 0 && a.tpart && g_k5_tsplit && n_txt_items >= 32) {
        const int sp = n_txt_items / 16;
        // 16 pieces per text block; with the 2-byte kernels 32 (RSA_TEXT_SPLIT, what tpart is sized for) on grids of fewer than 8
        // generations, where the pieces of 0.6 of a sparse walk's life would be the last to finish behind a split tail (and the
        // combine pass that doubles with them is still small)
        int cap = ((long)BH * a.NBp < 8 * 512 && !g_shard_invariant) ? pol.short_grid_text_cap : 16;
        const size_t room = tpart_bytes / ((size_t)BH * (size_t)ntq * piece_bytes);   // what the caller's buffer holds
        if ((size_t)cap > room) cap = (int)room;
        a.tsplit = sp > cap ? cap : sp;
        if (a.tsplit < 2) a.tsplit = 1;
        a.tper = (n_txt_items + a.tsplit - 1) / a.tsplit;
    }
    const int n_heavy = ntq > 0 ? BH * ntq * a.tsplit : 0;
    a.heavy_last = a.tsplit > 1 && g_k5_text_last;
    a.n_heavy_pad = (n_heavy + 7) & ~7;
    const long n_sparse = (long)BH * a.NBp;
    *nblocks = (long)a.n_heavy_pad + n_sparse;
    // Tail split (sparse lists): 512 workgroups run at a time (2 per CU), each for about as long as the others, so a launch costs
    // ceil(workgroups / 512) lives; when the last generation of sparse blocks is less than half full, its blocks' walks are
    // split over the idle slots (tail_p pieces each, partials behind the text region of tpart, which always starts RSA_TEXT_SPLIT
    // pieces per text block in) and merged by a combine pass.  Which blocks are split depends on the grid: a sharded and an
    // unsharded run then agree on those blocks within rounding, not byte for byte (tuning key k5_tail_split = 0 keeps every
    // walk whole).  The pieces AND the text-row pieces behind them must fit the 512 slots together: otherwise whatever starts
    // late (0.6 of a life for a text piece) ends the launch as late as the unsplit tail did (measured: 3 heads of the headline
    // shape, 456 pieces + 96 text pieces: 1.92 ms against 1.88 unsplit).
    // (e4m3 kernel, tail_beside_text = false: with its shorter lives and two waves per SIMD the split measured +1.6 % on Wan2.2-TI2V
    // and -2.3 % at 3 heads of the HunyuanVideo shape, where the text pieces end the launch either way: profiles/r04_k5_tail_split.txt)
    a.tail_first = a.tail_n = a.tail_p = 0; a.tail_part = nullptr;
    if (pol.tail_split && a.mode == MODE_SPARSE && a.tpart && (n_heavy == 0 || (pol.tail_beside_text && a.heavy_last)) && g_k5_tail_split &&
        !g_shard_invariant) {
        const long full = n_sparse / 512, T = n_sparse % 512;
        const long room = 512 - a.n_heavy_pad;
        const long P = T > 0 ? (room / T < 4 ? room / T : 4) : 0;      // T x P <= 512 = RSA_TAIL_PIECES
        const size_t text_pieces = (size_t)BH * (size_t)ntq * RSA_TEXT_SPLIT;
        if (full >= 1 && T > 0 && P >= 2 && (text_pieces + (size_t)(T * P)) * piece_bytes <= tpart_bytes) {
            a.tail_first = (int)(full * 512); a.tail_n = (int)T; a.tail_p = (int)P;
            a.tail_part = a.tpart + rsa_part_row((long)text_pieces, 0, D);
            *nblocks = (long)a.tail_first + (long)a.tail_n * a.tail_p + a.n_heavy_pad;
        }
    }
    if (*nblocks <= 0) { *nblocks = 0; return RSA_OK; }
    if (*nblocks > 0x7FFFFFFF) return RSA_ERR_UNSUPPORTED;
    if (a.NB_total > 8192) return RSA_ERR_UNSUPPORTED;  // kept list lives in LDS, 16 KiB (u16) / 32 KiB (e4m3 entries) max
    return RSA_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// Walk order of the sparse units (rsa_walk_order.h): order[bh][rank] = unit, u16 [BH, NBp], built by two small kernels.
// Key of a unit = the mean of its kept block indices in 1/64 block (19 bits; an empty list sorts last), ties to the lower unit
// index.  Walks with nearby means stay nearby for their whole lives (a walk's position at step j is an order statistic of its
// list), so the runs of `gen` consecutive ranks that an XCD holds together meet in its L2 far more often than `gen` walks taken in
// index order do (profiles/k5_walk_order.md).  Where adjacent query blocks keep nearly the same lists, index order IS the better
// order (neighbours share their keys, sorting by mean pulls them apart): a head whose mean adjacent overlap,
// |list_i & list_i+1| / |list_i| over its units with a non-empty list, is thr_pct per cent or more keeps index order.
//
// Pass 1, walk_order_unit_kernel: one WAVE per unit over the whole device.  Unit i's key and its overlap with unit i + 1 (list
// i + 1 as a bitmap in the wave's own 1 KiB of LDS, list i tested against it) -> ukey / uovl [BH, NBp].
// Pass 2, walk_order_sort_kernel: one workgroup per head.  Sums the overlaps in a fixed order, then sorts (key << 13 | unit) -- or
// the unit indices alone, for a head that keeps index order -- in LDS, NBv <= 8192.  The units of a split tail (the eighth map's units
// behind work index n_whole, which stay what they are) are left out of the sort and written at their own ranks.
constexpr int ORD_NT = 1024, ORD_BM_WORDS = 8192 / 32, ORD_UNIT_NT = 256;
constexpr unsigned ORD_KEY_EMPTY = 0x7FFFEu;     // (below the all-ones word that marks a pad or a tail unit in the sort)
__device__ __forceinline__ int ord_wave_sum(int x) {      // sum over the 64 lanes, in a scalar
    x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);     // quad_perm [1,0,3,2]
    x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);     // quad_perm [2,3,0,1]
    x += __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xF, false);    // row_ror:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false);    // row_ror:8
    return __builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16) + __builtin_amdgcn_readlane(x, 32) +
           __builtin_amdgcn_readlane(x, 48);
}
// a wave's bitmap is its own: its LDS traffic only has to be complete and in order inside the wave (no workgroup barrier)
__device__ __forceinline__ void ord_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__global__ __launch_bounds__(ORD_UNIT_NT) void walk_order_unit_kernel(const int32_t* __restrict__ cols, const int32_t* __restrict__ counts,
                                                                      unsigned* __restrict__ ukey, float* __restrict__ uovl, int BH,
                                                                      int NBv, int NBp, int NB_total) {
    __shared__ unsigned ord_bm[ORD_UNIT_NT / 64][ORD_BM_WORDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * (ORD_UNIT_NT / 64) + wv;      // wave = (bh, unit)
    if (w >= (long)BH * NBv) return;
    const int bh = (int)(w / NBv), i = (int)(w % NBv);
    unsigned* bm = ord_bm[wv];
    const long row = (long)bh * NBv + i;
    const bool has_next = i + 1 < NBv;
    const int32_t* la = cols + row * NB_total;
    const int32_t* lb = la + (has_next ? NB_total : 0);
    // (the first 128 entries of both lists are in flight together with the counts: entries past a count are read -- a row has NB_total
    // slots -- and not used)
    const int a0 = lane < NB_total ? la[lane] : -1, a1 = lane + 64 < NB_total ? la[lane + 64] : -1;
    const int b0 = lane < NB_total ? lb[lane] : -1, b1 = lane + 64 < NB_total ? lb[lane + 64] : -1;
    int na = counts[row], nb = has_next ? counts[row + 1] : 0;
    na = na < 0 ? 0 : (na < NB_total ? na : NB_total);
    nb = nb < 0 ? 0 : (nb < NB_total ? nb : NB_total);
    for (int x = lane; x < ORD_BM_WORDS; x += 64) bm[x] = 0u;
    ord_wave_sync();
    for (int x = lane; x < nb; x += 64) {
        const int e = x < 64 ? b0 : (x < 128 ? b1 : lb[x]);
        if ((unsigned)e < (unsigned)NB_total) atomicOr(&bm[e >> 5], 1u << (e & 31));
    }
    ord_wave_sync();
    int sum = 0, hit = 0;
    for (int x = lane; x < na; x += 64) {
        const int e = x < 64 ? a0 : (x < 128 ? a1 : la[x]);
        if ((unsigned)e < (unsigned)NB_total) {
            sum += e;
            hit += (int)((bm[e >> 5] >> (e & 31)) & 1u);
        }
    }
    sum = ord_wave_sum(sum);
    hit = ord_wave_sum(hit);
    if (lane == 0) {
        const unsigned key = na > 0 ? ((unsigned)sum << 6) / (unsigned)na : ORD_KEY_EMPTY;     // (sum < 2^25: at most 8192 distinct blocks < 8192)
        ukey[(long)bh * NBp + i] = (key << 13) | (unsigned)i;
        uovl[(long)bh * NBp + i] = (has_next && na > 0) ? (float)hit / (float)na : -1.0f;      // -1: no pair
    }
}
__global__ __launch_bounds__(ORD_NT) void walk_order_sort_kernel(const unsigned* __restrict__ ukey, const float* __restrict__ uovl,
                                                                 unsigned short* __restrict__ order, int NBv, int NBp, int P2,
                                                                 int n_whole, int thr_pct) {
    extern __shared__ unsigned ord_keys[];                // [P2]: P2 = the power of two >= NBv
    __shared__ float ord_ov[ORD_NT / 64];
    __shared__ int ord_np[ORD_NT / 64];
    __shared__ int ord_identity;
    const int bh = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    // ranks [0, r0) are whole walks; the ranks from r0 on are the head's share of a split tail
    const long left = (long)n_whole - (long)bh * NBp;
    const int r0 = left < 0 ? 0 : (left < NBp ? (int)left : NBp);
    const unsigned key_t = t < NBv ? ukey[(long)bh * NBp + t] : 0u;      // (in flight with the overlaps: not behind the decision they lead to)
    float ov = 0.0f;
    int np = 0;
    for (int i = t; i < NBv; i += ORD_NT) {
        const float o = uovl[(long)bh * NBp + i];
        if (o >= 0.0f) { ov += o; ++np; }
    }
    for (int m = 1; m < 64; m <<= 1) { ov += __shfl_xor(ov, m, 64); np += __shfl_xor(np, m, 64); }
    if (lane == 0) { ord_ov[wv] = ov; ord_np[wv] = np; }
    __syncthreads();
    if (t == 0) {
        float so = 0.0f;
        int sp = 0;
        for (int w = 0; w < ORD_NT / 64; ++w) { so += ord_ov[w]; sp += ord_np[w]; }
        ord_identity = so * 100.0f >= (float)thr_pct * (float)sp;
    }
    __syncthreads();
    const bool identity = ord_identity != 0;
    for (int i = t; i < P2; i += ORD_NT) {
        unsigned key = 0xFFFFFFFFu;                        // pads, and the units of the tail: behind every whole walk
        if (i < NBv && rsa_walk_unit_inv(i, NBp) < r0) key = identity ? (unsigned)i : (i == t ? key_t : ukey[(long)bh * NBp + i]);
        ord_keys[i] = key;
    }
    __syncthreads();
    // bitonic sort, ascending.  A step with j < 64 pairs keys of one wave: those steps run on registers (key i sits in lane i & 63
    // of the wave that owns index i), only the steps with j >= 64 go through LDS and a workgroup barrier.
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j >= 64; j >>= 1) {
            for (int i = t; i < P2; i += ORD_NT) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned ka = ord_keys[i], kb = ord_keys[x];
                    if ((ka > kb) == ((i & k) == 0)) { ord_keys[i] = kb; ord_keys[x] = ka; }
                }
            }
            __syncthreads();
        }
        for (int i0 = 0; i0 < P2; i0 += ORD_NT) {          // (uniform trip count: every lane of a wave takes part in the shuffles)
            const int i = i0 + t;
            unsigned key = i < P2 ? ord_keys[i] : 0xFFFFFFFFu;
            for (int j = k >> 1 < 32 ? k >> 1 : 32; j > 0; j >>= 1) {
                const unsigned other = (unsigned)__shfl_xor((int)key, j, 64);
                const bool low = (i & j) == 0, up = (i & k) == 0;       // this lane keeps the smaller key iff low == up
                const unsigned mn = key < other ? key : other, mx = key < other ? other : key;
                key = (low == up) ? mn : mx;
            }
            if (i < P2) ord_keys[i] = key;
        }
        __syncthreads();
    }
    unsigned short* o = order + (long)bh * NBp;
    for (int r = t; r < NBp; r += ORD_NT) {
        int u;
        if (r < r0) u = (r < P2 && ord_keys[r] != 0xFFFFFFFFu) ? (int)(ord_keys[r] & 0x1FFFu) : RSA_ORDER_PAD;
        else u = rsa_walk_unit(r, NBp);                    // (the tail piece's unit; never read through the table)
        o[r] = (unsigned short)(u < NBv ? u : RSA_ORDER_PAD);
    }
}

static int launch_attn(AttnArgs& a, int BH, int D, int dtype, size_t tpart_bytes, hipStream_t s) {
    // 128-token blocks and dense calls run the 64-row kernel; 64-token blocks the 32-row kernel, whose 64-key tiles are one block
    const bool w64 = a.blk == RSA_BLOCK;
    long nblocks;
    WalkPolicy pol;
    pol.blk = a.blk;
    pol.short_grid_text_cap = RSA_TEXT_SPLIT;
    // (only the 64-row kernel stores a tail piece, and only at head dim 128; a piece's partial holds 128 rows, a head pair has 256)
    pol.tail_split = w64 && D == 128 && a.gqa != RSA_GQA_PAIR;
    pol.tail_beside_text = true;
    int st = rsa_plan_walk(a, BH, D, pol, tpart_bytes, &nblocks);
    if (st != RSA_OK || nblocks == 0) return st;
    // The order table of the sparse units (rsa_walk_order.h), for the plain sparse calls of the 64-row kernel whose sparse units start
    // at work index 0: built on this stream in front of the kernel, in what the caller's tpart has left behind the text pieces' and the
    // tail pieces' regions (the caller's own buffer, ordered by the caller's stream: never a slot another launch could recycle):
    // the table, then the per-unit keys and overlaps of its first pass.  No tpart or no room: the eighth map.
    if (g_k5_walk_order && w64 && a.mode == MODE_SPARSE && a.gqa == RSA_GQA_NONE && !a.row_hi && a.tpart && a.NBv > 0 &&
        a.NBv <= 8192 && (a.heavy_last || a.n_heavy_pad == 0)) {
        const int ntq = a.NQB - a.NBv;
        const size_t piece_bytes = (size_t)rsa_part_row(1, 0, D) * sizeof(float);
        const size_t used = ((size_t)BH * (size_t)(ntq > 0 ? ntq : 0) * RSA_TEXT_SPLIT + (size_t)a.tail_n * (size_t)a.tail_p) * piece_bytes;
        const size_t n_ent = (size_t)BH * (size_t)a.NBp;         // (NBp is a multiple of 8: the three arrays stay 4-byte aligned)
        const size_t need = n_ent * (sizeof(unsigned short) + sizeof(unsigned) + sizeof(float));
        if (used <= tpart_bytes && need <= tpart_bytes - used) {
            char* base = reinterpret_cast<char*>(a.tpart) + used;
            unsigned short* order = reinterpret_cast<unsigned short*>(base);
            unsigned* ukey = reinterpret_cast<unsigned*>(base + n_ent * sizeof(unsigned short));
            float* uovl = reinterpret_cast<float*>(ukey + n_ent);
            int P2 = 1;
            while (P2 < a.NBv) P2 <<= 1;
            const long waves = (long)BH * a.NBv, per_wg = ORD_UNIT_NT / 64;
            walk_order_unit_kernel<<<dim3((unsigned)((waves + per_wg - 1) / per_wg)), ORD_UNIT_NT, 0, s>>>(a.cols, a.counts, ukey, uovl, BH, a.NBv,
                                                                                                        a.NBp, a.NB_total);
            walk_order_sort_kernel<<<dim3((unsigned)BH), ORD_NT, (size_t)P2 * sizeof(unsigned), s>>>(
                ukey, uovl, order, a.NBv, a.NBp, P2, a.tail_n > 0 ? a.tail_first : (int)n_ent, g_k5_order_overlap);
            if ((st = rsa_launch_status()) != RSA_OK) return st;
            a.order = order;
        }
    }
    const size_t lds_bytes = (size_t)4 * 64 * D * 2 + (((size_t)a.NB_total * 2 + 15) & ~(size_t)15);
    st = w64 ? rsa_launch_bsfwd64(a, dim3((unsigned)nblocks), lds_bytes, D, dtype, s)
             : rsa_launch_bsfwd(a, dim3((unsigned)nblocks), lds_bytes, D, dtype, s);
    return st != RSA_OK ? st : rsa_combine_walk(a, D, a.blk, dtype, s);
}

static void fill_qkv(AttnArgs& a, const rsa_tensor4& q, const rsa_tensor4& k, const rsa_tensor4& v,
                     const rsa_out4& out) {
    a.q = static_cast<const unsigned short*>(q.ptr); a.qsb = q.stride_b; a.qsh = q.stride_h; a.qss = q.stride_s;
    a.k = static_cast<const unsigned short*>(k.ptr); a.ksb = k.stride_b; a.ksh = k.stride_h; a.kss = k.stride_s;
    a.v = static_cast<const unsigned short*>(v.ptr); a.vsb = v.stride_b; a.vsh = v.stride_h; a.vss = v.stride_s;
    a.out = static_cast<unsigned short*>(out.ptr); a.osb = out.stride_b; a.osh = out.stride_h; a.oss = out.stride_s;
    a.row_lo = nullptr; a.row_hi = nullptr; a.range_sb = 0;     // no per-row key ranges (rsa_block_sparse_ranged_fwd sets them)
    a.kv_group = 1; a.list_group = 1; a.gqa = RSA_GQA_NONE;     // every head its own K/V head and lists (rsa_block_sparse_gqa_fwd sets them)
}

int rsa_check_out(const rsa_out4& o) {
    if (!o.ptr || (reinterpret_cast<uintptr_t>(o.ptr) & 7)) return RSA_ERR_BAD_ARG;
    if ((o.stride_b % 4) || (o.stride_h % 4) || (o.stride_s % 4)) return RSA_ERR_BAD_ARG;  // 8-byte stores
    return RSA_OK;
}

static int block_sparse_fwd_b(const rsa_layout* l, int blk, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                              const rsa_buffers* buf, rsa_out4 out, void* stream) {
    int st = rsa_check_layout_b(l, blk);
    if (st != RSA_OK) return st;
    if ((st = rsa_check_tensor(q)) || (st = rsa_check_tensor(k)) || (st = rsa_check_tensor(v)) ||
        (st = rsa_check_out(out)))
        return st;
    if (!buf || (l->NBv > 0 && (!buf->cols || !buf->counts))) return RSA_ERR_BAD_ARG;
    if ((buf->R == nullptr) != (buf->comp == nullptr)) return RSA_ERR_BAD_ARG;
    AttnArgs a;
    fill_qkv(a, q, k, v, out);
    a.cols = buf->cols; a.counts = buf->counts; a.R = buf->R; a.comp = buf->comp;
    a.tpart = buf->tpart;
    a.mode = MODE_SPARSE; a.H = l->H; a.Sq = l->S; a.Sk = l->S;
    a.NBv = l->NBv; a.NQB = l->NB_total; a.NB_total = l->NB_total;
    a.blk = blk; a.txt0 = l->NBv * blk;
    if (blk == 64) a.NQB = l->NBv + (l->NB_total - l->NBv + 1) / 2;   // text rows in 128-row units
    a.kv_valid = l->kv_valid; a.kv_text_valid = l->kv_text_valid;
    a.q_text_end = l->NBv * blk + l->q_text_valid;
    a.q_split = 0; a.kv_split = 0; a.causal = 0; a.rows256 = 0;
    a.qk_scale = (float)((1.0 / sqrt((double)l->D)) * 1.44269504);  // sm_scale * 1.44269504 (hunyuan :145)
    return launch_attn(a, l->B * l->H, l->D, l->dtype, buf->tpart_bytes, static_cast<hipStream_t>(stream));
}
extern "C" int rsa_block_sparse_fwd(const rsa_layout* l, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                    const rsa_buffers* buf, rsa_out4 out, void* stream) {
    return block_sparse_fwd_b(l, RSA_BLOCK, q, k, v, buf, out, stream);
}
extern "C" int rsa_block_sparse_fwd_ex(const rsa_layout_ex* lx, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                       const rsa_buffers* buf, rsa_out4 out, void* stream) {
    return rsa_layout_ex_ok(lx) ? block_sparse_fwd_b(&lx->base, lx->block, q, k, v, buf, out, stream) : RSA_ERR_BAD_ARG;
}

// Plain block-sparse attention over caller-supplied lists (rsa_block_mask_to_lists): the sparse walk of the rectified call with
// no R / comp (the epilogue stores acc / l), the caller's scale, Sq query rows in NQ blocks and no text rows (NQB = NBv = NQ, so
// nothing is written past row Sq), Sk key rows of which those >= kv_valid are masked.
// (the checks and the arguments rsa_block_sparse_plain_fwd and rsa_block_sparse_ranged_fwd share)
static int plain_args(AttnArgs& a, int B, int H, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, int kv_valid,
                      double sm_scale, const rsa_tensor4& q, const rsa_tensor4& k, const rsa_tensor4& v, const int32_t* cols,
                      const int32_t* counts, float* tpart, size_t tpart_bytes, const rsa_out4& out) {
    if (block != 64 && block != RSA_BLOCK) return RSA_ERR_UNSUPPORTED;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0) return RSA_ERR_BAD_ARG;
    if (NQ != (Sq + block - 1) / block || NK <= 0 || NK > (Sk + block - 1) / block) return RSA_ERR_BAD_ARG;
    if (NK > 8192) return RSA_ERR_UNSUPPORTED;
    if (kv_valid <= 0 || kv_valid > Sk) return RSA_ERR_BAD_ARG;   // (a key row is clamped into [0, kv_valid) before it is staged)
    if (!std::isfinite(sm_scale)) return RSA_ERR_BAD_ARG;       // (any sign: the online softmax needs none)
    if (!cols || !counts) return RSA_ERR_BAD_ARG;
    if (tpart && tpart_bytes == 0) return RSA_ERR_WORKSPACE;
    int st;
    if ((st = rsa_check_tensor(q)) || (st = rsa_check_tensor(k)) || (st = rsa_check_tensor(v)) || (st = rsa_check_out(out)))
        return st;
    fill_qkv(a, q, k, v, out);
    a.cols = cols; a.counts = counts; a.R = nullptr; a.comp = nullptr;
    a.tpart = tpart;
    a.mode = MODE_SPARSE; a.H = H; a.Sq = Sq; a.Sk = Sk;
    a.NBv = NQ; a.NQB = NQ; a.NB_total = NK;
    a.blk = block; a.txt0 = NQ * block;
    a.kv_valid = kv_valid; a.kv_text_valid = 0; a.q_text_end = 0;
    a.q_split = 0; a.kv_split = 0; a.causal = 0; a.rows256 = 0;
    a.qk_scale = (float)(sm_scale * 1.44269504);   // (as the reference kernel's launcher: hunyuan :145)
    return RSA_OK;
}
extern "C" int rsa_block_sparse_plain_fwd(int B, int H, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, int kv_valid,
                                          double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const int32_t* cols,
                                          const int32_t* counts, float* tpart, size_t tpart_bytes, rsa_out4 out, void* stream) {
    AttnArgs a;
    const int st = plain_args(a, B, H, Sq, Sk, D, dtype, block, NQ, NK, kv_valid, sm_scale, q, k, v, cols, counts, tpart, tpart_bytes, out);
    if (st != RSA_OK) return st;
    return launch_attn(a, B * H, D, dtype, tpart ? tpart_bytes : 0, static_cast<hipStream_t>(stream));
}

// ... with a key range per query row (rsa.h): the same walk through the RANGED instantiations of the 64-row kernel.  128-token
// blocks only: the 32-row kernel, which walks 64-token blocks, masks against ONE scalar key limit per launch, not a range per row.
extern "C" int rsa_block_sparse_ranged_fwd(int B, int H, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, int kv_valid,
                                           double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const int32_t* cols,
                                           const int32_t* counts, const int32_t* row_lo, const int32_t* row_hi,
                                           int64_t range_stride_b, float* tpart, size_t tpart_bytes, rsa_out4 out, void* stream) {
    if (block != RSA_BLOCK) return RSA_ERR_UNSUPPORTED;
    if (!row_hi || range_stride_b < 0) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(row_lo) | reinterpret_cast<uintptr_t>(row_hi)) & 3) return RSA_ERR_BAD_ARG;
    AttnArgs a;
    const int st = plain_args(a, B, H, Sq, Sk, D, dtype, block, NQ, NK, kv_valid, sm_scale, q, k, v, cols, counts, tpart, tpart_bytes, out);
    if (st != RSA_OK) return st;
    a.row_lo = row_lo; a.row_hi = row_hi; a.range_sb = (long)range_stride_b;
    return launch_attn(a, B * H, D, dtype, tpart ? tpart_bytes : 0, static_cast<hipStream_t>(stream));
}

// ... with grouped-query K/V heads (rsa.h): k / v hold Hkv heads, the lists Hl per batch item.  Form (b), a head pair per workgroup,
// where two neighbouring query heads share both their K/V head and their list row and the kernel is the 64-row one; else form (a),
// the MHA launch with two divisions in its address arithmetic.  Hkv = Hl = H is the MHA call itself: the kernels of the two
// entries above.
static int rsa_gqa_form(int H, int Hkv, int Hl, int block, int pair_enabled) {
    if (Hkv == H && Hl == H) return RSA_GQA_NONE;
    const bool pair = pair_enabled && block == RSA_BLOCK && (H / Hkv) % 2 == 0 && (H / Hl) % 2 == 0;
    return pair ? RSA_GQA_PAIR : RSA_GQA_HEAD;
}
extern "C" int rsa_block_sparse_gqa_fwd(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                        int kv_valid, double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                        const int32_t* cols, const int32_t* counts, const int32_t* row_lo, const int32_t* row_hi,
                                        int64_t range_stride_b, float* tpart, size_t tpart_bytes, rsa_out4 out, void* stream) {
    if (H <= 0 || Hkv <= 0 || Hl <= 0 || H % Hkv || H % Hl) return RSA_ERR_BAD_ARG;
    if (row_hi && block == 64) return RSA_ERR_UNSUPPORTED;     // (the 32-row kernel has no per-row range)
    if ((!row_hi && row_lo) || range_stride_b < 0) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(row_lo) | reinterpret_cast<uintptr_t>(row_hi)) & 3) return RSA_ERR_BAD_ARG;
    AttnArgs a;
    const int st = plain_args(a, B, H, Sq, Sk, D, dtype, block, NQ, NK, kv_valid, sm_scale, q, k, v, cols, counts, tpart, tpart_bytes, out);
    if (st != RSA_OK) return st;
    a.row_lo = row_lo; a.row_hi = row_hi; a.range_sb = row_hi ? (long)range_stride_b : 0;
    a.kv_group = H / Hkv; a.list_group = H / Hl;
    a.gqa = rsa_gqa_form(H, Hkv, Hl, block, g_k5_gqa_pair);
    // a head pair per workgroup: the walk plan counts pairs (rsa_walk_map itself is the MHA call's)
    const int BH = a.gqa == RSA_GQA_PAIR ? B * (H / 2) : B * H;
    return launch_attn(a, BH, D, dtype, tpart ? tpart_bytes : 0, static_cast<hipStream_t>(stream));
}

static int dense_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                     int q_split, int kv_split, int causal, rsa_out4 out, void* stream) {
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0) return RSA_ERR_BAD_ARG;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (q_split < 0 || q_split > Sq || kv_split < 0 || kv_split > Sk) return RSA_ERR_BAD_ARG;
    int st;
    if ((st = rsa_check_tensor(q)) || (st = rsa_check_tensor(k)) || (st = rsa_check_tensor(v)) ||
        (st = rsa_check_out(out)))
        return st;
    AttnArgs a;
    fill_qkv(a, q, k, v, out);
    a.cols = nullptr; a.counts = nullptr; a.R = nullptr; a.comp = nullptr;
    a.tpart = nullptr;
    a.tsplit = 1; a.tper = 0;
    a.mode = MODE_DENSE; a.H = H; a.Sq = Sq; a.Sk = Sk;
    a.blk = RSA_BLOCK; a.txt0 = 0;
    // 256-row tiles once there are at least two of them (a shorter call keeps 128-row tiles)
    a.rows256 = (g_k5_rows256 && Sq > 256) ? 1 : 0;
    const int rw = a.rows256 ? 2 * RSA_BLOCK : RSA_BLOCK;
    a.NQB = (Sq + rw - 1) / rw; a.NBv = a.NQB; a.NB_total = (Sk + RSA_BLOCK - 1) / RSA_BLOCK;
    a.kv_valid = Sk; a.kv_text_valid = Sk; a.q_text_end = 0;
    a.q_split = q_split; a.kv_split = kv_split; a.causal = causal;
    a.qk_scale = (float)((1.0 / sqrt((double)D)) * 1.44269504);
    return launch_attn(a, B * H, D, dtype, 0, static_cast<hipStream_t>(stream));
}

extern "C" int rsa_dense_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k,
                             rsa_tensor4 v, int q_split, int kv_split, rsa_out4 out, void* stream) {
    return dense_fwd(B, H, Sq, Sk, D, dtype, q, k, v, q_split, kv_split, 0, out, stream);
}

extern "C" int rsa_dense_causal_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k,
                                    rsa_tensor4 v, int q_split, int kv_split, rsa_out4 out, void* stream) {
    return dense_fwd(B, H, Sq, Sk, D, dtype, q, k, v, q_split, kv_split, 1, out, stream);
}

extern "C" int rsa_rectified_attention(const rsa_layout* l, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                       const uint8_t* neighbor, int top_k, float p_remain, void* workspace,
                                       size_t workspace_bytes, rsa_out4 out, void* stream) {
    rsa_buffers buf;
    int st = rsa_carve_workspace(l, workspace, workspace_bytes, &buf);
    if (st != RSA_OK) return st;
    if ((st = rsa_pool_stats(l, q, k, v, &buf, stream))) return st;
    if ((st = rsa_pooled_scores(l, k, &buf, stream))) return st;
    if ((st = rsa_select_mask(l, neighbor, top_k, p_remain, &buf, stream))) return st;
    if ((st = rsa_compensation(l, &buf, stream))) return st;
    return rsa_block_sparse_fwd(l, q, k, v, &buf, out, stream);
}

extern "C" int rsa_rectified_attention_ex(const rsa_layout_ex* lx, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                          const uint8_t* neighbor, int top_k, float p_remain, void* workspace,
                                          size_t workspace_bytes, rsa_out4 out, void* stream) {
    if (!rsa_layout_ex_ok(lx)) return RSA_ERR_BAD_ARG;
    if (lx->block == RSA_BLOCK)
        return rsa_rectified_attention(&lx->base, q, k, v, neighbor, top_k, p_remain, workspace, workspace_bytes, out, stream);
    rsa_buffers buf;
    int st = rsa_carve_workspace_ex(lx, workspace, workspace_bytes, &buf);
    if (st != RSA_OK) return st;
    if ((st = rsa_pool_stats_ex(lx, q, k, v, &buf, stream))) return st;
    if ((st = rsa_pooled_scores_ex(lx, k, &buf, stream))) return st;
    if ((st = rsa_select_mask_ex(lx, neighbor, top_k, p_remain, &buf, stream))) return st;
    if ((st = rsa_compensation_ex(lx, &buf, stream))) return st;
    return rsa_block_sparse_fwd_ex(lx, q, k, v, &buf, out, stream);
}
