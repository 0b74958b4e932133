// Block selection by the observed attention mass of the last query rows (include/rsa.h: rsa_block_select_observed; DESIGN.md section
// 5.24): the score pass in front of the select kernels of rsa_block_select.hip, a translation unit of its own.  It reaches that unit
// through rsa_select_shared.h alone: sel_key and sel_visible on the device, sel_ext_check and sel_ext_select on the host.  The select
// kernels rank the keys this pass writes LOADED and gain no form of their own.
//
// W <= 64 observation rows of every query head meet every key they see once: one pass over K, four launches.
//
//   observed_score_kernel<Tag, D, BLK>   one 4-wave workgroup per (b, K/V head, pass of four query heads, key split).  A wave owns one
//       query head and keeps its W rows -- up to four 16-row tiles, rows >= W zero -- as the A operands of
//       v_mfma_f32_16x16x32_{bf16,f16} for the whole walk, loaded once, straight from q_obs.  A key block [BLK][D] moves through LDS
//       (16-byte chunks, chunk ci of key n at ci ^ (n & 7) against bank conflicts), is shared by the four waves (one K/V head's keys
//       are read once for four heads), is zero-filled at keys >= len_b on the load, is found through the block table once per block
//       and is prefetched into registers under the products of the block before it.  Per block, row tile and row the wave reduces the
//       BLK logits to a pair (m, l): m the maximum of the raw dot products over the row's visible keys, l = sum of
//       exp2((a - m) c2), c2 = sm_scale log2(e) -- the scale meets the difference, which is rounded where it is small.  Lane-local
//       over the BLK / 16 column groups, then over the 16 column lanes by xor shuffles (1, 2, 4, 8).  OB_LOWEST, finite, stands in
//       for the maximum of a row that saw nothing in the block (l = 0).  Masking runs only in blocks that touch len_b or the causal
//       edge.  The pair goes to the workspace as fp32, stats [B, H, NK, W, 2].  Key splits walk the blocks sp, sp + splits, ..: they
//       write disjoint blocks, so the split count cannot change a byte.
//   observed_rows_kernel   one 1024-thread workgroup per (b, h); thread (jl, r) = tid / W, tid % W, JL = 1024 / W lanes jl.  Per row r
//       the online combine (M, L) <- (max(M, m), L exp2((M - M') c2) + l exp2((m - M') c2)) over jb = jl, jl + JL, .. ascending, then
//       over the JL lanes by a halving tree through LDS; the pair goes to rowstat [B, H, W, 2].
//   observed_mass_kernel   one 1024-thread workgroup per (b, hl, chunk of JL key blocks); thread (jl, r) takes block jb = chunk JL + jl:
//       v[r] = sum over the list head's query heads h, ascending, of l exp2((m - M) c2) / L (a row with L = 0 saw nothing and adds
//       nothing), P = sum over ascending r of v[r] by one thread through LDS, and the ordered key of ln(max(P, 2^-126)) into wkeys
//       [B, Hl, 1, NK].
//   the shared select launch ranks wkeys.
//
// Every sum has one fixed order, nothing is added atomically: two calls give the same bytes.
#include "rsa_select_shared.h"

#include <math.h>
#include <type_traits>

typedef float ob_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ob_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ob_f16x8 __attribute__((ext_vector_type(8)));

#define OB_LOWEST (-3.0e38f)    // the maximum of a row that has seen nothing: finite, so that no inf - inf is formed
#define OB_MAX_W 64             // observation rows: four 16-row MFMA tiles
#define OB_MAX_SPLITS 256
#define OB_MASS_NT 1024
#define OB_FILL 512             // score workgroups from which the default asks for no further key split

template <typename Tag>
__device__ __forceinline__ ob_f32x4 ob_mfma(const uint4 a, const uint4 b, const ob_f32x4 c) {
    if constexpr (std::is_same<Tag, bf16_tag>::value)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ob_bf16x8, a), __builtin_bit_cast(ob_bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ob_f16x8, a), __builtin_bit_cast(ob_f16x8, b), c, 0, 0, 0);
}

struct ob_args {
    rsa_tensor4 q, k;
    int H, Hkv, Hl, W, Sk, blk, NK;
    const int32_t* kv_len;
    int kv_valid, causal;
    const int32_t* table;   // NULL: k is [B, Hkv, Sk, D]; else k is the page pool and block jb of item b is page table[b tsb + jb]
    long tsb;
    int num_pages;
    float c2;               // sm_scale log2(e): the log2 domain
    int NPASS, splits;      // passes of four heads over a K/V head's group, key splits
    int chunks;             // chunks of 1024 / W key blocks of a list row: the mass kernel's workgroups per row
    float* stats;           // [B, H, NK, W, 2]
    float* rowstat;         // [B, H, W, 2]
    unsigned* wkeys;        // [B, Hl, 1, NK]
};

// The visible key blocks of an item: a prefix.  (The last live row sees every key below len_b, causal or not.)
__device__ __forceinline__ int ob_visible(const ob_args& a, int len) { return sel_visible(len, a.W, a.blk, a.NK, 0, a.causal); }

template <typename Tag, int D, int BLK>
__global__ __launch_bounds__(SEL_NT) void observed_score_kernel(const ob_args a) {
    constexpr int CPK = D / 8;                  // 16-byte chunks of a key
    constexpr int KS = D / 32;                  // MFMA steps over the head dim
    constexpr int NCG = BLK / 16;               // 16-key column groups of a block
    constexpr int NLD = BLK * CPK / SEL_NT;     // chunks a thread stages per block
    __shared__ uint4 ktile[BLK * CPK];          // [BLK][CPK], chunk ci of key n at ci ^ (n & 7)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h = lane >> 4;
    unsigned rest = blockIdx.x;
    const int sp = (int)(rest % (unsigned)a.splits);
    rest /= (unsigned)a.splits;
    const int pass = (int)(rest % (unsigned)a.NPASS);
    rest /= (unsigned)a.NPASS;
    const int hk = (int)(rest % (unsigned)a.Hkv);
    const long b = rest / (unsigned)a.Hkv;
    const int g = a.H / a.Hkv, hg = pass * 4 + wave, head = hk * g + hg;
    const bool live = hg < g;                   // a wave without a head still stages K
    const int W = a.W, len = rsa_key_limit(a.kv_len, (int)b, a.kv_valid, a.Sk);
    const long off = (long)len - W;
    const int nvis = ob_visible(a, len), nt = (W + 15) >> 4;

    // the Q operand, once for the walk: lane (c, h) holds row 16 t + c, elements 32 ks + 8 h .. + 8
    uint4 qf[4][KS];
    {
        const unsigned short* qb = static_cast<const unsigned short*>(a.q.ptr) + b * a.q.stride_b + (long)(live ? head : 0) * a.q.stride_h;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int row = 16 * t + c;
                qf[t][ks] = make_uint4(0u, 0u, 0u, 0u);
                if (live && row < W) qf[t][ks] = *reinterpret_cast<const uint4*>(qb + (long)row * a.q.stride_s + ks * 32 + 8 * h);
            }
    }

    const unsigned short* kp = static_cast<const unsigned short*>(a.k.ptr);
    uint4 pre[NLD];
    auto load_tile = [&](int jb) {      // keys at or beyond the limit, and a page outside the pool: zeros, and no address is formed
        long base;
        bool ok = true;
        if (a.table) {
            const int pg = a.table[b * a.tsb + jb];
            ok = pg >= 0 && pg < a.num_pages;
            base = (long)pg * a.k.stride_b + (long)hk * a.k.stride_h;
        } else {
            base = b * a.k.stride_b + (long)hk * a.k.stride_h + (long)jb * BLK * a.k.stride_s;
        }
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int cid = tid + n * SEL_NT, kl = cid / CPK;
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (ok && (long)jb * BLK + kl < len) pre[n] = *reinterpret_cast<const uint4*>(kp + base + (long)kl * a.k.stride_s + (cid % CPK) * 8);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int cid = tid + n * SEL_NT, kl = cid / CPK;
            ktile[kl * CPK + ((cid % CPK) ^ (kl & 7))] = pre[n];
        }
    };

    if (sp < nvis) {
        load_tile(sp);
        store_tile();
    }
    for (int jb = sp; jb < nvis; jb += a.splits) {
        __syncthreads();    // block jb is in LDS
        const int nxt = jb + a.splits;
        if (nxt < nvis) load_tile(nxt);
        if (live) {
            const long last = (long)(jb + 1) * BLK - 1;     // the block's last key
            const bool edge = last >= len || (a.causal && last > off);
            float* st = a.stats + (((b * a.H + head) * a.NK + jb) * W) * 2;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= nt) break;
                // lane (c, h): key 16 cg + c of the block, rows 16 t + 4 h + e
                ob_f32x4 acc[NCG];
#pragma unroll
                for (int cg = 0; cg < NCG; ++cg) {
                    acc[cg] = ob_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        acc[cg] = ob_mfma<Tag>(qf[t][ks], ktile[(16 * cg + c) * CPK + ((ks * 4 + h) ^ (c & 7))], acc[cg]);
                }
                if (edge) {
#pragma unroll
                    for (int cg = 0; cg < NCG; ++cg) {
                        const long key = (long)jb * BLK + 16 * cg + c;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const bool vis = key < len && (!a.causal || key <= 16 * t + 4 * h + e + off);
                            acc[cg][e] = vis ? acc[cg][e] : -INFINITY;
                        }
                    }
                }
                float m[4], l[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float mx = OB_LOWEST;
#pragma unroll
                    for (int cg = 0; cg < NCG; ++cg) mx = fmaxf(mx, acc[cg][e]);
                    for (int mk = 1; mk < 16; mk <<= 1) mx = fmaxf(mx, __shfl_xor(mx, mk, 64));
                    float s = 0.f;
#pragma unroll
                    for (int cg = 0; cg < NCG; ++cg) s += __builtin_amdgcn_exp2f((acc[cg][e] - mx) * a.c2);
                    for (int mk = 1; mk < 16; mk <<= 1) s += __shfl_xor(s, mk, 64);
                    m[e] = mx, l[e] = s;
                }
                // every column lane holds the pairs of rows 4 h + e: lane c < 4 writes row 4 h + c
                const float mw = c == 0 ? m[0] : c == 1 ? m[1] : c == 2 ? m[2] : m[3];
                const float lw = c == 0 ? l[0] : c == 1 ? l[1] : c == 2 ? l[2] : l[3];
                const int row = 16 * t + 4 * h + c;
                if (c < 4 && row < W) *reinterpret_cast<float2*>(st + 2 * row) = make_float2(mw, lw);
            }
        }
        __syncthreads();    // every wave is done with block jb
        if (nxt < nvis) store_tile();
    }
}

// (M, L) <- (M, L) + (m, l): the log-sum-exp of two key sets in the log2 domain, the scale at the difference.
__device__ __forceinline__ void ob_combine(float& M, float& L, float m, float l, float c2) {
    const float mn = fmaxf(M, m);
    L = L * __builtin_amdgcn_exp2f((M - mn) * c2) + l * __builtin_amdgcn_exp2f((m - mn) * c2);
    M = mn;
}

// The statistics (M, L) of every observation row over its visible blocks: one workgroup per (b, h), thread (jl, r).
__global__ __launch_bounds__(OB_MASS_NT) void observed_rows_kernel(const ob_args a) {
    __shared__ float pm[OB_MASS_NT], pl[OB_MASS_NT];
    const int tid = threadIdx.x, W = a.W, JL = OB_MASS_NT / W, r = tid % W, jl = tid / W;
    const bool active = jl < JL;
    const long bh = blockIdx.x, b = bh / a.H;
    const int len = rsa_key_limit(a.kv_len, (int)b, a.kv_valid, a.Sk), nvis = ob_visible(a, len);
    const float2* st = reinterpret_cast<const float2*>(a.stats) + (bh * a.NK) * W + r;      // + jb W
    float M = OB_LOWEST, L = 0.f;
    if (active)
        for (int jb = jl; jb < nvis; jb += JL) {
            const float2 s = st[(long)jb * W];
            ob_combine(M, L, s.x, s.y, a.c2);
        }
    pm[tid] = M, pl[tid] = L;
    __syncthreads();
    for (int s = OB_MASS_NT / 2; s >= 1; s >>= 1) {
        if (active && jl < s && jl + s < JL) {
            ob_combine(M, L, pm[tid + s * W], pl[tid + s * W], a.c2);
            pm[tid] = M, pl[tid] = L;
        }
        __syncthreads();
    }
    if (jl == 0) reinterpret_cast<float2*>(a.rowstat)[bh * W + r] = make_float2(M, L);
}

// The mass of JL = 1024 / W key blocks of a list row: one workgroup per (b, hl, chunk of JL blocks), thread (jl, r).
__global__ __launch_bounds__(OB_MASS_NT) void observed_mass_kernel(const ob_args a) {
    __shared__ float pv[OB_MASS_NT];
    const int tid = threadIdx.x, W = a.W, JL = OB_MASS_NT / W, r = tid % W, jl = tid / W;
    const long row = blockIdx.x / (unsigned)a.chunks;
    const int jb = (int)(blockIdx.x % (unsigned)a.chunks) * JL + jl;
    const int hl = (int)(row % a.Hl);
    const long b = row / a.Hl;
    const int g = a.H / a.Hkv, gl = a.Hl == a.Hkv ? g : 1, h0 = hl * gl;     // the list head's query heads
    const int len = rsa_key_limit(a.kv_len, (int)b, a.kv_valid, a.Sk), nvis = ob_visible(a, len);
    if (jb - jl >= nvis) return;        // (uniform: the chunk holds no visible block)
    const bool mine = jl < JL && jb < nvis;
    float v = 0.f;
    if (mine)
        for (int hh = 0; hh < gl; ++hh) {
            const long bh = b * a.H + h0 + hh;
            const float2 s = reinterpret_cast<const float2*>(a.stats)[(bh * a.NK + jb) * W + r];
            const float2 ML = reinterpret_cast<const float2*>(a.rowstat)[bh * W + r];
            if (ML.y > 0.f) v += s.y * __builtin_amdgcn_exp2f((s.x - ML.x) * a.c2) / ML.y;
        }
    pv[tid] = v;
    __syncthreads();
    if (mine && r == 0) {
        float P = 0.f;
        for (int x = 0; x < W; ++x) P += pv[tid + x];
        a.wkeys[row * a.NK + jb] = sel_key(logf(fmaxf(P, 1.1754943508222875e-38f)));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static size_t ob_keys_bytes(int B, int Hl, int NK) { return (((size_t)B * Hl * NK * sizeof(unsigned)) + 15) & ~(size_t)15; }

extern "C" int rsa_block_select_observed_bytes(int B, int H, int Hkv, int Hl, int W, int D, int block, int NQ, int NK, size_t* bytes) {
    if (!bytes || B <= 0 || H <= 0 || Hkv <= 0 || Hl <= 0 || W <= 0 || NQ <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (H % Hkv || (Hl != Hkv && Hl != H)) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if ((D != 64 && D != 128) || NK > SEL_MAX_NK) return RSA_ERR_UNSUPPORTED;
    if (W > OB_MAX_W || NQ != 1) return RSA_ERR_BAD_ARG;
    if ((size_t)B * Hkv * ((H / Hkv + 3) / 4) * OB_MAX_SPLITS > 0x7FFFFFFFull) return RSA_ERR_UNSUPPORTED;
    // wkeys [B, Hl, 1, NK], stats [B, H, NK, W, 2], rowstat [B, H, W, 2]
    *bytes = ob_keys_bytes(B, Hl, NK) + (size_t)B * H * (NK + 1) * W * 2 * sizeof(float);
    return RSA_OK;
}

template <typename Tag>
static void ob_launch_score(const ob_args& a, int D, long groups, hipStream_t s) {
    const dim3 grid((unsigned)groups);
    if (D == 64) {
        if (a.blk == 64) observed_score_kernel<Tag, 64, 64><<<grid, SEL_NT, 0, s>>>(a);
        else observed_score_kernel<Tag, 64, 128><<<grid, SEL_NT, 0, s>>>(a);
    } else {
        if (a.blk == 64) observed_score_kernel<Tag, 128, 64><<<grid, SEL_NT, 0, s>>>(a);
        else observed_score_kernel<Tag, 128, 128><<<grid, SEL_NT, 0, s>>>(a);
    }
}

extern "C" int rsa_block_select_observed(int B, int H, int Hkv, int Hl, int W, int Sk, int D, int dtype, int block, int NQ, int NK,
                                         rsa_tensor4 q, rsa_tensor4 k, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                                         const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, int top_k, int keep_first,
                                         int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                                         int32_t* counts, float* scores, int p16, float c, float* mass, void* stream) {
    const sel_ext_call e = {B, H, Hkv, Hl, W, Sk, D, dtype, block, NQ, NK, q, kv_len_dev, kv_valid, causal != 0, top_k, keep_first,
                            keep_local, bitmask, cols, counts, scores, p16, c, mass};
    int st = sel_ext_check(e);
    if (st != RSA_OK) return st;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (!isfinite(sm_scale) || !(sm_scale > 0.0)) return RSA_ERR_BAD_ARG;
    size_t need = 0;
    st = rsa_block_select_observed_bytes(B, H, Hkv, Hl, W, D, block, NQ, NK, &need);
    if (st != RSA_OK) return st;
    if (!ws || rsa_check_tensor(k) != RSA_OK || k.stride_b < 0 || k.stride_h < 0 || k.stride_s < 0) return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(block_table) & 3) || (block_table && (num_pages <= 0 || table_stride_b < 0))) return RSA_ERR_BAD_ARG;
    if (score_splits < 0 || score_splits > OB_MAX_SPLITS) return RSA_ERR_BAD_ARG;
    if (ws_bytes < need) return RSA_ERR_WORKSPACE;
    const float c2 = (float)(sm_scale * 1.4426950408889634);
    if (!(c2 > 0.f) || !isfinite(c2)) return RSA_ERR_BAD_ARG;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int g = H / Hkv, npass = (g + 3) / 4;
    const long base = (long)B * Hkv * npass;
    long splits = score_splits ? score_splits : (OB_FILL + base - 1) / base;      // the default: a function of the shapes alone
    splits = splits < 1 ? 1 : splits > OB_MAX_SPLITS ? OB_MAX_SPLITS : splits;
    if (splits > NK) splits = NK;
    unsigned* wkeys = static_cast<unsigned*>(ws);
    float* stats = reinterpret_cast<float*>(static_cast<char*>(ws) + ob_keys_bytes(B, Hl, NK));
    const int JL = OB_MASS_NT / W, chunks = (NK + JL - 1) / JL;
    const ob_args a = {q, k, H, Hkv, Hl, W, Sk, block, NK, kv_len_dev, kv_valid, causal != 0, block_table, (long)table_stride_b, num_pages,
                       c2, npass, (int)splits, chunks, stats, stats + (size_t)B * H * NK * W * 2, wkeys};
    if (dtype == RSA_BF16) ob_launch_score<bf16_tag>(a, D, base * splits, s);
    else ob_launch_score<fp16_tag>(a, D, base * splits, s);
    int rc = rsa_launch_status();
    if (rc != RSA_OK) return rc;
    observed_rows_kernel<<<dim3((unsigned)((long)B * H)), OB_MASS_NT, 0, s>>>(a);
    rc = rsa_launch_status();
    if (rc != RSA_OK) return rc;
    observed_mass_kernel<<<dim3((unsigned)((long)B * Hl * chunks)), OB_MASS_NT, 0, s>>>(a);
    rc = rsa_launch_status();
    return rc != RSA_OK ? rc : sel_ext_select(e, wkeys, stream);
}
