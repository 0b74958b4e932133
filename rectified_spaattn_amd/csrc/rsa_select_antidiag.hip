// Block selection by anti-diagonal scores (include/rsa.h: rsa_block_select_antidiag): the score pass in front
// of the select kernels of rsa_block_select.hip, a translation unit of its own.  It reaches that unit through rsa_select_shared.h:
// sel_key and sel_visible on the device, sel_ext_check and sel_ext_select on the host.  The select kernels rank the keys this pass
// writes LOADED and gain no form of their own.
//
// With s = stride, row group u = rows [u s, u s + s) and key group w = keys [w s, w s + s):
//     a[u, w] = sum over t < s of <q[u s + s - 1 - t], k[w s + t]>            (the anti-diagonals (r + c) mod s = s - 1)
// is one GEMM over reshaped views: K_r[w, t D + d] = k[w s + t, d] is K read as [Sk / s, s D], Q_r the same with the rows of each
// group reversed.  16 row groups (16 s query rows: 16 s / block query blocks of one head) are the A operand of
// v_mfma_f32_16x16x32_{bf16,f16}, 16 key groups (16 s keys) the B operand, the inner dimension is KD = s D.
//
//   antidiag_score_kernel<Tag, S, D>   one 4-wave workgroup per (b, K/V head, NWT / HW query tiles) and, per pass, HW heads of the
//       K/V head's group: a wave (a wave pair at KD = 2048, each over half the inner dimension) owns one (head, query tile) and
//       keeps its reversed Q operand in registers for both walks -- loaded once, straight from q, zero at rows >= Sq.  The K tile
//       [16][KD] moves through LDS (16-byte chunks, chunk index xor (w & 7) against bank conflicts), is shared by the waves, is
//       zero-filled at keys >= len_b on the load and is prefetched into registers under the products of the tile before it.
//       Walk 1 over the visible key tiles: a lane-local online (max, sum) per row group in the log2 domain, combined over the 16
//       column lanes at the end.  Walk 2 (K out of the L2): p = exp2(x - m) / l, summed over the rows of a query block and the key
//       groups of a key block by xor shuffles, over the heads of a list head in ascending order through LDS (and, where a group
//       has more heads than a pass, on top of the earlier passes' sum in the workspace, by the thread that wrote it), then
//       t = ln(max(P, 2^-126)) as an ordered key into wkeys [B, Hl, NQ, NK].  Group masking runs only in tiles that touch len_b or
//       the causal edge.  The row statistics never leave registers: the workspace is wkeys alone.
//
// Every sum has one fixed order, nothing is added atomically: two calls give the same bytes.
#include "rsa_select_shared.h"

#include <math.h>
#include <type_traits>

typedef float ad_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ad_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ad_f16x8 __attribute__((ext_vector_type(8)));

#define AD_LOWEST (-3.0e38f)    // the running maximum of a row that has seen nothing: finite, so that no inf - inf is formed

template <typename Tag>
__device__ __forceinline__ ad_f32x4 ad_mfma(const uint4 a, const uint4 b, const ad_f32x4 c) {
    if constexpr (std::is_same<Tag, bf16_tag>::value)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ad_bf16x8, a), __builtin_bit_cast(ad_bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(ad_f16x8, a), __builtin_bit_cast(ad_f16x8, b), c, 0, 0, 0);
}

struct ad_args {
    rsa_tensor4 q, k;
    int H, Hkv, Hl, Sq, Sk, blk, NQ, NK;
    const int32_t* kv_len;
    int kv_valid, causal;
    float c2;           // sm_scale log2(e) / s: x in the log2 domain
    int HW, NPASS, QT;  // heads of a group per pass, passes (HW NPASS = H / Hkv), workgroups per (b, K/V head)
    unsigned* wkeys;
};

// The waves that share a (head, query tile), and the tiles of a workgroup.
template <int S, int D>
struct AdShape {
    static constexpr int KD = S * D, SPLIT = KD > 1024 ? 2 : 1, NWT = 4 / SPLIT, KS = KD / 32 / SPLIT;
    static constexpr int TROWS = 16 * S;        // query rows of a query tile, keys of a key tile
    static constexpr size_t LDS = (size_t)32 * KD + 2 * 4 * 16 * sizeof(double) + (SPLIT == 2 ? NWT * 64 * sizeof(ad_f32x4) : 0);
};

template <typename Tag, int S, int D>
__global__ __launch_bounds__(SEL_NT) void antidiag_score_kernel(const ad_args a) {
    using Sh = AdShape<S, D>;
    constexpr int KD = Sh::KD, SPLIT = Sh::SPLIT, NWT = Sh::NWT, KS = Sh::KS, TROWS = Sh::TROWS;
    constexpr int CPK = D / 8;          // 16-byte chunks of a key
    constexpr int CPR = KD / 8;         // 16-byte chunks of a key group: a row of the tile
    constexpr int NLD = KD / 128;       // chunks a thread stages per tile
    extern __shared__ uint4 ad_lds[];
    uint4* ktile = ad_lds;                                          // [16][CPR], chunk ci of row w at ci ^ (w & 7)
    double* red = reinterpret_cast<double*>(ad_lds + 16 * CPR);     // [2][4][4][4]: tile parity, wave slot, query block, key block
    ad_f32x4* cx = reinterpret_cast<ad_f32x4*>(red + 2 * 4 * 16);   // [NWT][64]: the second half's partial products (SPLIT == 2)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, h = lane >> 4;
    const int p = wave / SPLIT, half = wave % SPLIT;
    const int HW = a.HW, TQ = NWT / HW, hw = p % HW, tq = p / HW;
    const int qtg = (int)(blockIdx.x % (unsigned)a.QT);
    const long bh = blockIdx.x / (unsigned)a.QT;
    const int hk = (int)(bh % a.Hkv);
    const long b = bh / a.Hkv;
    const int g = a.H / a.Hkv, G = a.blk / S, QB = 16 / G;
    const int Sq = a.Sq, len = rsa_key_limit(a.kv_len, (int)b, a.kv_valid, a.Sk);
    const long off = (long)len - Sq;
    const bool perq = a.Hl != a.Hkv;                // one list row per query head: nothing is summed over heads
    const int qt = qtg * TQ + tq, u0 = qt * 16;     // the wave's query tile and its first row group
    const long row0 = (long)qt * TROWS;

    // the key tiles the workgroup walks: up to the last key group its last live row group sees
    const long rl = min((long)(qtg + 1) * TQ * TROWS, (long)Sq) - 1;
    long kend = len;
    if (a.causal) kend = min(kend, (rl / S) * S + S + off);
    const int ntiles = kend > 0 ? (int)((kend + TROWS - 1) / TROWS) : 0;

    const unsigned short* kb = static_cast<const unsigned short*>(a.k.ptr) + b * a.k.stride_b + (long)hk * a.k.stride_h;
    uint4 pre[NLD];
    auto load_tile = [&](int kt) {      // keys at or beyond the limit: zeros, and no address is formed from them
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int cid = tid + n * SEL_NT;
            const long key = (long)kt * TROWS + cid / CPK;
            pre[n] = make_uint4(0u, 0u, 0u, 0u);
            if (key < len) pre[n] = *reinterpret_cast<const uint4*>(kb + key * a.k.stride_s + (cid % CPK) * 8);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int cid = tid + n * SEL_NT;
            const int kl = cid / CPK, w = kl / S, ci = (kl % S) * CPK + cid % CPK;
            ktile[w * CPR + (ci ^ (w & 7))] = pre[n];
        }
    };

    for (int pass = 0; pass < a.NPASS; ++pass) {
        // what walk 2 left in red for key tile kt becomes keys: by thread (wave slot, query block, key block)
        auto flush = [&](int kt) {
            if (tid >= NWT * 16) return;
            const int pp = tid >> 4, iq = (tid >> 2) & 3, jk = tid & 3;
            if (iq >= QB || jk >= QB || (!perq && pp % HW)) return;
            const int i = (qtg * TQ + pp / HW) * QB + iq, j = kt * QB + jk;
            if (i >= a.NQ || j >= sel_visible(len, Sq, a.blk, a.NK, i, a.causal)) return;
            const double* rp = red + ((kt & 1) * 4 + pp) * 16 + iq * 4 + jk;
            double P = rp[0];      // (the masses are summed in fp64: the fp32 terms' rounding is all that is left in P)
            if (!perq)
                for (int x = 1; x < HW; ++x) P += rp[x * 16];      // the pass's heads, ascending
            const long hl = perq ? (long)hk * g + pass * HW + pp % HW : hk;
            unsigned* dst = a.wkeys + ((b * a.Hl + hl) * a.NQ + i) * a.NK + j;
            if (!perq && pass > 0) P = (double)__uint_as_float(*dst) + P;   // the earlier passes' heads, written by this thread
            *dst = (perq || pass == a.NPASS - 1) ? sel_key((float)log(fmax(P, 1.1754943508222875e-38))) : __float_as_uint((float)P);
        };

        // the reversed Q operand, once for both walks: lane (c, h) holds row group c, inner elements 32 ks + 8 h .. + 8
        const int head = hk * g + pass * HW + hw;
        const unsigned short* qb = static_cast<const unsigned short*>(a.q.ptr) + b * a.q.stride_b + (long)head * a.q.stride_h;
        uint4 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int idx = (half * KS + ks) * 32 + 8 * h;
            const long row = row0 + c * S + (S - 1 - idx / D);
            qf[ks] = make_uint4(0u, 0u, 0u, 0u);
            if (row < Sq) qf[ks] = *reinterpret_cast<const uint4*>(qb + row * a.q.stride_s + idx % D);
        }

        float m[4], l[4], dl[4];        // dl: the divisor of walk 2, inf for a row group that weighs nothing
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = AD_LOWEST, l[e] = 0.f, dl[e] = INFINITY;

        for (int walk = 0; walk < 2; ++walk) {
            if (ntiles > 0) {
                load_tile(0);
                store_tile();       // (behind the barrier that ended the walk before: nobody reads the tile)
            }
            for (int kt = 0; kt < ntiles; ++kt) {
                __syncthreads();    // tile kt is in LDS; walk 2: red of tile kt - 1 is complete
                if (walk == 1 && kt > 0) flush(kt - 1);
                if (kt + 1 < ntiles) load_tile(kt + 1);
                ad_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int ci = (half * KS + ks) * 4 + h;
                    acc = ad_mfma<Tag>(qf[ks], ktile[c * CPR + (ci ^ (c & 7))], acc);
                }
                if (SPLIT == 2 && half == 1) cx[p * 64 + lane] = acc;
                __syncthreads();    // every wave is done with tile kt; cx is complete
                if (kt + 1 < ntiles) store_tile();
                if (half != 0) continue;
                if (SPLIT == 2) {
                    const ad_f32x4 o = cx[p * 64 + lane];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += o[e];
                }
                // lane (c, h): key group w = 16 kt + c, row groups u0 + 4 h + e.  The maximum is kept on the raw sums and the scale
                // meets the difference: (a - max) c2 is rounded where it is small, x = a c2 would be where it is large
                float x[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = acc[e];
                const long wl = ((long)kt * 16 + 15) * S;       // the tile's last key group starts here
                if (wl >= len || (a.causal && wl > (long)u0 * S + S - 1 + off)) {
                    const long w0 = ((long)kt * 16 + c) * S;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool vis = w0 < len && (!a.causal || w0 <= (long)(u0 + 4 * h + e) * S + S - 1 + off);
                        x[e] = vis ? x[e] : -INFINITY;
                    }
                }
                if (walk == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float mn = fmaxf(m[e], x[e]);
                        l[e] = l[e] * __builtin_amdgcn_exp2f((m[e] - mn) * a.c2) + __builtin_amdgcn_exp2f((x[e] - mn) * a.c2);
                        m[e] = mn;
                    }
                } else {
                    double v = 0.0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v += (double)(__builtin_amdgcn_exp2f((x[e] - m[e]) * a.c2) / dl[e]);
                    for (int mk = 1; mk < G; mk <<= 1) v += __shfl_xor(v, mk, 64);              // the key groups of a key block
                    for (int mk = 4; mk < G; mk <<= 1) v += __shfl_xor(v, 4 * mk, 64);          // the row groups of a query block
                    if (c % G == 0 && (4 * h) % G == 0) red[((kt & 1) * 4 + p) * 16 + (4 * h / G) * 4 + c / G] = v;
                }
            }
            if (walk == 0) {
                // the row's (max, sum) over the 16 column lanes; a row group without a row, or one that saw nothing, weighs 0
                for (int mk = 1; mk < 16; mk <<= 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float mo = __shfl_xor(m[e], mk, 64), lo = __shfl_xor(l[e], mk, 64);
                        const float mn = fmaxf(m[e], mo);
                        l[e] = l[e] * __builtin_amdgcn_exp2f((m[e] - mn) * a.c2) + lo * __builtin_amdgcn_exp2f((mo - mn) * a.c2);
                        m[e] = mn;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) dl[e] = (l[e] > 0.f && (long)(u0 + 4 * h + e) * S < Sq) ? l[e] : INFINITY;
            } else if (ntiles > 0) {
                __syncthreads();
                flush(ntiles - 1);
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static bool ad_shape_ok(int D, int stride) { return (D == 64 || D == 128) && (stride == 8 || stride == 16); }

extern "C" int rsa_block_select_antidiag_bytes(int B, int H, int Hkv, int Hl, int Sq, int D, int block, int stride, int NQ, int NK,
                                               size_t* bytes) {
    if (!bytes || B <= 0 || H <= 0 || Hkv <= 0 || Hl <= 0 || Sq <= 0 || NQ <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (H % Hkv || (Hl != Hkv && Hl != H)) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (!ad_shape_ok(D, stride) || NK > SEL_MAX_NK) return RSA_ERR_UNSUPPORTED;
    if (NQ != (int)(((long)Sq + block - 1) / block)) return RSA_ERR_BAD_ARG;
    if ((size_t)B * Hl * NQ > 0x7FFFFFFFull) return RSA_ERR_UNSUPPORTED;
    *bytes = (((size_t)B * Hl * NQ * NK * sizeof(unsigned)) + 15) & ~(size_t)15;      // wkeys [B, Hl, NQ, NK] and nothing else
    return RSA_OK;
}

template <typename Tag, int S, int D>
static int ad_launch(const ad_args& a, long groups, hipStream_t s) {
    constexpr size_t lds = AdShape<S, D>::LDS;
    if (lds > 64 * 1024) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(antidiag_score_kernel<Tag, S, D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    antidiag_score_kernel<Tag, S, D><<<dim3((unsigned)groups), SEL_NT, lds, s>>>(a);
    return rsa_launch_status();
}

extern "C" int rsa_block_select_antidiag(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int stride, int NQ,
                                         int NK, rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal,
                                         double sm_scale, int top_k, int keep_first, int keep_local, void* ws, size_t ws_bytes,
                                         uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, int p16, float c,
                                         float* mass, void* stream) {
    const sel_ext_call e = {B, H, Hkv, Hl, Sq, Sk, D, dtype, block, NQ, NK, q, kv_len_dev, kv_valid, causal != 0, top_k, keep_first,
                            keep_local, bitmask, cols, counts, scores, p16, c, mass};
    int st = sel_ext_check(e);
    if (st != RSA_OK) return st;
    if (!ad_shape_ok(D, stride)) return RSA_ERR_UNSUPPORTED;
    if (!isfinite(sm_scale) || !(sm_scale > 0.0)) return RSA_ERR_BAD_ARG;
    size_t need = 0;
    st = rsa_block_select_antidiag_bytes(B, H, Hkv, Hl, Sq, D, block, stride, NQ, NK, &need);
    if (st != RSA_OK) return st;
    if (!ws || rsa_check_tensor(k) != RSA_OK || k.stride_b < 0 || k.stride_h < 0 || k.stride_s < 0) return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return RSA_ERR_BAD_ARG;
    if (ws_bytes < need) return RSA_ERR_WORKSPACE;
    const float c2 = (float)(sm_scale * 1.4426950408889634 / stride);
    if (!(c2 > 0.f) || !isfinite(c2)) return RSA_ERR_BAD_ARG;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const int g = H / Hkv, nwt = stride * D > 1024 ? 2 : 4;
    int HW = nwt;                           // the most heads of a group a workgroup's waves can take that divide the group
    while (g % HW) HW >>= 1;
    const long tiles = ((long)Sq + 16 * stride - 1) / (16 * stride), QT = (tiles + nwt / HW - 1) / (nwt / HW);
    const long groups = (long)B * Hkv * QT;
    if (groups > 0x7FFFFFFFL) return RSA_ERR_UNSUPPORTED;
    const ad_args a = {q, k, H, Hkv, Hl, Sq, Sk, block, NQ, NK, kv_len_dev, kv_valid, causal != 0, c2, HW, g / HW, (int)QT,
                       static_cast<unsigned*>(ws)};
    int rc;
    if (dtype == RSA_BF16)
        rc = stride == 8 ? (D == 64 ? ad_launch<bf16_tag, 8, 64>(a, groups, s) : ad_launch<bf16_tag, 8, 128>(a, groups, s))
                         : (D == 64 ? ad_launch<bf16_tag, 16, 64>(a, groups, s) : ad_launch<bf16_tag, 16, 128>(a, groups, s));
    else
        rc = stride == 8 ? (D == 64 ? ad_launch<fp16_tag, 8, 64>(a, groups, s) : ad_launch<fp16_tag, 8, 128>(a, groups, s))
                         : (D == 64 ? ad_launch<fp16_tag, 16, 64>(a, groups, s) : ad_launch<fp16_tag, 16, 128>(a, groups, s));
    return rc != RSA_OK ? rc : sel_ext_select(e, static_cast<const unsigned*>(ws), stream);
}
