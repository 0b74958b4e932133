// Top-p block selection per list row on the device (include/rsa.h: rsa_block_select_p, rsa_block_select_pooled_p; DESIGN.md
// section 5.15): the budget of a row is the shortest prefix of its ranking whose softmax mass reaches top_p, capped at top_k.
// Pooling, the scores and the score pass of the pooled form are rsa_block_select.hip's kernels, launched by its host bodies
// (sel_run, sel_pooled_run); this unit holds the select kernel and the four entries.
//
//   block_select_p_kernel   one 256-thread workgroup per list row.  The ordered keys of the visible blocks in LDS, as in
//                           block_select_kernel.  A block weighs u = floor(exp2((t - t_max) c) 2^18 + 0.5), an integer, recomputed
//                           from its key wherever it is needed: t_max by an integer maximum over the keys, the row's total and its
//                           forced mass by integer sums, the cut by the radix select of block_select_kernel with hist[digit] += u
//                           in place of += 1.  The threshold key T and the count of blocks tied at T that are still needed,
//                           ceil(rest / u_T), then go to block_select_kernel's tie rule and list writer; where the cap top_k
//                           binds, (T, count) come from the counting radix instead.
//
// exp2 is __builtin_amdgcn_exp2f (v_exp_f32), the function of the attention kernels: exact at integer arguments.  Every sum is an
// unsigned integer sum (at most 8192 weights of at most 2^18): no order, two calls give the same bytes.
#include "rsa_block_select.h"

#define SELP_ONE 262144u    // 2^18: the weight of the row's best block

struct SelForced {      // the forced blocks of a row: [0, kf) and [flo, fhi]
    int kf, flo, fhi;
    __device__ __forceinline__ bool operator()(int j) const { return j < kf || (j >= flo && j <= fhi); }
};

// The weight of the block with ordered key `key` in a row whose best visible score is tmax.  A NaN (non-finite scores) weighs 0.
__device__ __forceinline__ unsigned selp_weight(unsigned key, float tmax, float c) {
    const float a = (sel_unkey(key) - tmax) * c;
    const float x = __builtin_amdgcn_exp2f(a) * (float)SELP_ONE + 0.5f;
    return x >= 1.f ? (unsigned)fminf(x, (float)SELP_ONE) : 0u;
}

// Sums of a and of b over the workgroup, in every thread (red: 8 words).
__device__ __forceinline__ uint2 selp_sum2(unsigned a, unsigned b, unsigned* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m, 64);
        b += __shfl_xor(b, m, 64);
    }
    __syncthreads();    // (red may still be read from the previous sum)
    if (lane == 0) {
        red[2 * wave] = a;
        red[2 * wave + 1] = b;
    }
    __syncthreads();
    return make_uint2(red[0] + red[2] + red[4] + red[6], red[1] + red[3] + red[5] + red[7]);
}

// block_select_kernel's radix select over the unforced visible keys, 8 bits a pass, on weights (MASS) or on counts: the key T at
// which the running sum over the ranking first reaches rem (0 < rem <= the sum over all of them), and what of rem is left for the
// blocks that tie at T.
template <bool MASS>
__device__ __forceinline__ void selp_radix(const unsigned* keys, int nvis, SelForced forced, float tmax, float c, unsigned rem,
                                           unsigned* hist, unsigned* wsum, unsigned* pick, unsigned& T, unsigned& left) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0u;
        __syncthreads();
        const unsigned himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int j = tid; j < nvis; j += SEL_NT) {
            const unsigned key = keys[j];
            if (!forced(j) && (key & himask) == prefix) {
                const unsigned u = MASS ? selp_weight(key, tmax, c) : 1u;
                if (u) atomicAdd(&hist[(key >> shift) & 255u], u);
            }
        }
        __syncthreads();
        // thread t owns digit 255 - t: its inclusive prefix over t sums the keys with that digit or a higher one
        const unsigned h = hist[255 - tid];
        unsigned inc = h;
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned o = __shfl_up(inc, m, 64);
            if (lane >= m) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        for (int w = 0; w < wave; ++w) inc += wsum[w];
        if (inc - h < rem && rem <= inc) {      // exactly one thread: the digit in which the sum reaches rem
            pick[0] = prefix | ((unsigned)(255 - tid) << shift);
            pick[1] = rem - (inc - h);
        }
        __syncthreads();
        prefix = pick[0];
        rem = pick[1];
    }
    T = prefix;
    left = rem;
}

// LOADED = 0: the scores are computed here (r.kbar, r.qsum); LOADED = 1: their keys are loaded from r.wkeys (block_score_kernel).
template <int L, int LOADED>
__global__ __launch_bounds__(SEL_NT) void block_select_p_kernel(const sel_rows r, int p16, float c, float* __restrict__ mass) {
    extern __shared__ unsigned keys[];              // [NK]: the scores of the visible blocks as ordered keys
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[4], red[8];
    __shared__ unsigned pick[2];
    __shared__ int step_eq[SEL_MAX_STEPS], step_kept[SEL_MAX_STEPS];
    __shared__ unsigned long long step_mask[SEL_MAX_STEPS];
    constexpr int D = 4 * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = r.blk, NK = r.NK, Sq = r.Sq;
    const long row = blockIdx.x;
    const int i = (int)(row % r.NQ);
    const long bh = row / r.NQ;
    const int hl = (int)(bh % r.Hl);
    const long b = bh / r.Hl;
    const int hk = hl / (r.Hl / r.Hkv);
    const int len = sel_key_limit(r.kv_len, (int)b, r.kv_valid, r.Sk);

    // visible blocks: a prefix [0, nvis) of the row; forced blocks: [0, kf) and [flo, fhi] within it (block_select_kernel's)
    const long r0 = (long)i * blk, r1 = min(r0 + blk, (long)Sq) - 1, off = (long)len - Sq;
    const int nvis = sel_visible(len, Sq, blk, NK, i, r.causal);
    SelForced forced = {min(r.keep_first, nvis), 1, 0};
    if (r.keep_local >= 1 && nvis > 0) {
        const long jd_lo = max(r0 + off, 0L) / blk, jd_hi = min(max(r1 + off, 0L), (long)len - 1) / blk;
        const long ext = min(r.keep_local - 1, SEL_MAX_NK);
        forced.flo = (int)max(jd_lo - ext, 0L);
        forced.fhi = (int)min(r.causal ? jd_hi : jd_hi + ext, (long)nvis - 1);
    }
    const int nf = forced.kf + max(0, forced.fhi - max(forced.flo, forced.kf) + 1);

    // scores of the visible blocks
    if (LOADED) {
        const unsigned* wr = r.wkeys + row * NK;
        for (int j = tid; j < nvis; j += SEL_NT) keys[j] = wr[j];
    } else {
        sel_score_blocks<L>(r.kbar + ((b * r.Hkv + hk) * NK) * D, r.qsum + row * D, 0, nvis, keys);
    }
    __syncthreads();
    if (r.scores) {
        float* sr = r.scores + row * NK;
        for (int j = tid; j < NK; j += SEL_NT) sr[j] = j < nvis ? sel_unkey(keys[j]) : -INFINITY;
    }

    // t_max over the visible blocks, on the keys; then the row's total weight and the weight of its forced blocks
    unsigned kmax = 0u;
    for (int j = tid; j < nvis; j += SEL_NT) kmax = max(kmax, keys[j]);
    for (int m = 32; m >= 1; m >>= 1) kmax = max(kmax, __shfl_xor(kmax, m, 64));
    if (lane == 0) red[wave] = kmax;
    __syncthreads();
    const float tmax = sel_unkey(max(max(red[0], red[1]), max(red[2], red[3])));
    unsigned part = 0u, fpart = 0u;
    for (int j = tid; j < nvis; j += SEL_NT) {
        const unsigned u = selp_weight(keys[j], tmax, c);
        part += u;
        if (forced(j)) fpart += u;
    }
    const uint2 sums = selp_sum2(part, fpart, red);
    const unsigned total = sums.x, fmass = sums.y;
    const unsigned target = (unsigned)(((unsigned long long)total * (unsigned)p16 + 65535ull) >> 16);      // <= total

    // (T, need_eq): the unforced blocks above key T are kept, and of those that tie at T the need_eq lowest
    const int nunf = nvis - nf, n_k = max(r.top_k - nf, 0);
    const bool cut = fmass < target && n_k > 0;     // else the forced blocks alone (uniform over the workgroup)
    unsigned T = 0u;
    int need_eq = 0;
    if (cut) {      // (target <= total: the unforced blocks hold target - fmass, so the sum reaches it)
        unsigned left;
        selp_radix<true>(keys, nvis, forced, tmax, c, target - fmass, hist, wsum, pick, T, left);
        const unsigned uT = selp_weight(T, tmax, c);        // > 0: its digit held weight in every pass
        need_eq = (int)((left + uT - 1u) / uT);
        if (n_k < nunf) {       // the cap may bind: n_p = #{key > T} + need_eq against n_k
            unsigned above = 0u;
            for (int j = tid; j < nvis; j += SEL_NT) above += (!forced(j) && keys[j] > T) ? 1u : 0u;
            const unsigned n_p = selp_sum2(above, 0u, red).x + (unsigned)need_eq;
            if (n_p > (unsigned)n_k) {
                selp_radix<false>(keys, nvis, forced, tmax, c, (unsigned)n_k, hist, wsum, pick, T, left);
                need_eq = (int)left;
            }
        }
    }
    if (mass) {     // float(sum of the kept weights) / float(total); a row that sees nothing: 0
        unsigned kpart = 0u;
        if (cut)
            for (int j = tid; j < nvis; j += SEL_NT) kpart += (!forced(j) && keys[j] > T) ? selp_weight(keys[j], tmax, c) : 0u;
        const unsigned kmass = fmass + selp_sum2(kpart, 0u, red).x + (cut ? (unsigned)need_eq * selp_weight(T, tmax, c) : 0u);
        if (tid == 0) mass[row] = total ? (float)kmass / (float)total : 0.f;
    }

    // the lists, in 64-block ballot steps: wave w takes steps w, w + 4, ... (block_select_kernel's writer)
    const int nsteps = (NK + 63) >> 6, NW = (NK + 31) >> 5;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int s = wave; s < nsteps; s += 4) {
        const int j = s * 64 + lane;
        const bool eq = cut && j < nvis && !forced(j) && keys[j] == T;
        const unsigned long long m = __ballot(eq);
        if (lane == 0) step_eq[s] = __popcll(m);
    }
    __syncthreads();
    if (wave == 0) sel_wave_scan(step_eq, nsteps, lane);
    __syncthreads();
    uint32_t* wr = r.bitmask + row * NW;
    for (int s = wave; s < nsteps; s += 4) {
        const int j = s * 64 + lane;
        const bool vis = j < nvis, f = vis && forced(j);
        const unsigned key = vis ? keys[j] : 0u;
        const bool eq = cut && vis && !f && key == T;
        const unsigned long long me = __ballot(eq);
        const bool kept = f || (cut && vis && key > T) || (eq && step_eq[s] + __popcll(me & below) < need_eq);
        const unsigned long long m = __ballot(kept);
        if (lane < 2 && 2 * s + lane < NW) wr[2 * s + lane] = lane ? (unsigned)(m >> 32) : (unsigned)m;
        if (lane == 0) {
            step_mask[s] = m;
            step_kept[s] = __popcll(m);
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int kept_total = sel_wave_scan(step_kept, nsteps, lane);
        if (lane == 0) r.counts[row] = kept_total;
    }
    __syncthreads();
    int32_t* cr = r.cols + row * NK;
    for (int s = wave; s < nsteps; s += 4) {
        const unsigned long long m = step_mask[s];
        if ((m >> lane) & 1ull) cr[step_kept[s] + __popcll(m & below)] = s * 64 + lane;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int sel_launch_top_p(int D, long rows, const sel_rows& r, const sel_top_p& p, hipStream_t s) {
    const dim3 grid((unsigned)rows);
    const size_t lds = (size_t)r.NK * sizeof(unsigned);
#define SELP_LAUNCH(LANES)                                                                           \
    if (r.wkeys) block_select_p_kernel<LANES, 1><<<grid, SEL_NT, lds, s>>>(r, p.p16, p.c, p.mass);   \
    else block_select_p_kernel<LANES, 0><<<grid, SEL_NT, lds, s>>>(r, p.p16, p.c, p.mass)
    switch (D) {
        case 16: SELP_LAUNCH(4); break;
        case 32: SELP_LAUNCH(8); break;
        case 64: SELP_LAUNCH(16); break;
        default: SELP_LAUNCH(32); break;
    }
#undef SELP_LAUNCH
    return rsa_launch_status();
}

static bool selp_budget_ok(const sel_top_p& p) {
    return p.p16 >= 0 && p.p16 <= 65536 && isfinite(p.c) && p.c > 0.f && !(reinterpret_cast<uintptr_t>(p.mass) & 3);
}

extern "C" int rsa_block_select_p_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return rsa_block_select_bytes(B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_p(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                  rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                                  int keep_first, int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                                  int32_t* counts, float* scores, int p16, float c, float* mass, void* stream) {
    const sel_top_p p = {p16, c, mass};
    if (!selp_budget_ok(p)) return RSA_ERR_BAD_ARG;
    return sel_run(B, H, Hkv, Hl, Sq, Sk, D, dtype, block, NQ, NK, q, k, kv_len_dev, kv_valid, causal, top_k, keep_first, keep_local,
                   ws, ws_bytes, bitmask, cols, counts, scores, &p, stream);
}

extern "C" int rsa_block_select_pooled_p_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes) {
    return rsa_block_select_pooled_bytes(B, Hkv, Hl, D, NQ, NK, bytes);
}

extern "C" int rsa_block_select_pooled_p(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK,
                                         rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid,
                                         int causal, int top_k, int keep_first, int keep_local, int score_splits, void* ws,
                                         size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                                         int p16, float c, float* mass, void* stream) {
    const sel_top_p p = {p16, c, mass};
    if (!selp_budget_ok(p)) return RSA_ERR_BAD_ARG;
    return sel_pooled_run(B, H, Hkv, Hl, Sq, D, dtype, block, NQ, NK, q, pooled_k, kv_len_dev, kv_valid, causal, top_k, keep_first,
                          keep_local, score_splits, ws, ws_bytes, bitmask, cols, counts, scores, &p, stream);
}
