// Block-sparse attention BACKWARD over caller block masks: dq, dk, dv of block_sparse_attention (include/rsa.h:
// rsa_block_sparse_bwd_bytes, rsa_block_sparse_bwd).  Three kernels, plain HIP C++ for wave64, two sweeps
// over the kept tiles, no float atomics and no hand-off between workgroups: the same inputs give the same bytes.
//
//   bwd_row_kernel    one 2-wave workgroup per (b, h, query block, group of 64 rows), a wave per 32 rows.  It walks the query
//                     block's kept list (ascending) in chunks of 32 keys:  S^T[key][row] = K . Qs^T, the query row on the lane, so
//                     the running maximum and the row sum are lane-local and the two lane halves of a row meet once at the end.
//                     Writes lse2[b, h, r] = m + log2 l (log2 domain; -inf for a row that sees no key) and
//                     delta[b, h, r] = sum_d dout[r, d] * out[r, d] (fp32, fixed order) to the workspace.
//   bwd_dq_kernel     the same grid and walk.  Per chunk, the query row on the lane:
//                         S'^T  = K . Qs^T  - lse2        the row constant is the initial accumulator
//                         dP'^T = V . dO^T  - delta       likewise
//                         dS^T  = exp2(S'^T) o dP'^T      (0 where the row does not see the key), rounded to the input type
//                         dq^T[d][row] += K^T . dS^T      A = K^T by ds_read_b64_tr_b16 from the wave's own [32][D] image of the
//                                                         chunk; B = the dS^T accumulator itself (its k order: bwd_tr_frag)
//                     dq = sm_scale * sum, one conversion.
//   bwd_dkdv_kernel   one workgroup per (b, K/V head, key block), a wave per 32 keys whose K and V fragments stay in registers.  It
//                     sweeps the query heads of the K/V head's group (ascending), per head the query blocks that keep this key block
//                     (ascending: the column lists = rsa_block_mask_to_lists of the transposed mask) and their 32-row slices.  Per
//                     slice, the KEY on the lane (Qs, Q and dO of the slice as [32][D] LDS images shared by the waves):
//                         S'  = Qs . K^T - lse2,  dP' = dO . V^T - delta       the row constants as initial accumulators
//                         P   = exp2(S')  (0 where invisible), dS = P o dP'    both rounded to the input type for the next products
//                         dv^T[d][key] += dO^T . P,   dk^T[d][key] += Q^T . dS  A by ds_read_b64_tr_b16, B = the accumulators
//                     dv = sum, dk = sm_scale * sum, each stored once: no sum crosses workgroups.
//
// That is eight matrix products per kept tile (S twice in the forward orientation, S and dP again in the other) where a design with
// float atomics or an ordered hand-off for dq has five: the price of reproducible bytes without a protocol between workgroups.
//
// Numeric contract: the forward's scores -- Q * (float)(sm_scale * log2 e) rounded to the input type (rsa_q_frag), log2 domain,
// fp32 --, P and dS rounded to the input type for the products they feed, fp32 accumulation, every output element rounded once.
// Keys at or beyond the limit are never multiplied: their K and V rows are replaced by zeros on the way in (they may hold NaN),
// their P is 0 by selection, and their dk / dv rows are exact zeros; so are the rows of key blocks that no query block keeps.  A
// query row that sees no key gets a zero dq row.  Every element of dq, dk and dv is written exactly once.
#include "rsa_attn.h"

#include <math.h>

#define BWD_MAX_BLOCKS 8192
#define BWD_ROW_NT 128          // row pass and dq kernel: two waves, 32 query rows each

struct BwdArgs {
    const unsigned short *q, *k, *v, *o, *g;        // g = dout
    long qsb, qsh, qss, ksb, ksh, kss, vsb, vsh, vss, osb, osh, oss, gsb, gsh, gss;
    unsigned short *dq, *dk, *dv;
    long dqsb, dqsh, dqss, dksb, dksh, dkss, dvsb, dvsh, dvss;
    const int32_t *rcols, *rcounts;     // [B * Hl, NQ, NK] / [B * Hl, NQ]: the key blocks a query block keeps
    const int32_t *ccols, *ccounts;     // [B * Hl, NK, NQ] / [B * Hl, NK]: the query blocks that keep a key block
    const int32_t* kv_len;              // device limits (clamped here) or null: kv_valid
    int kv_valid;
    int H, Hkv, Hl, Sq, Sk, NQ, NK, NKt, blk, causal;      // NKt = ceil(Sk / blk) >= NK
    float qk_scale, sm_scale;
    float *lse, *delta;                 // [B, H, Sq] each
};

template <int D>
struct BwdImg {
    static constexpr int ROWB = 2 * D + 32;     // bytes per row of a [32][D] image: rows 0 .. 7 start 8 banks apart
    static constexpr int BYTES = 32 * ROWB;
};

__device__ __forceinline__ s16x4 bwd_tr_read(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

// 32 rows x D elements from global memory (row stride `stride` elements) into an image, by NT threads; rows >= nrows become zeros
// and are not read
template <int D, int NT>
__device__ __forceinline__ void bwd_stage(unsigned char* img, const unsigned short* gp, long stride, int nrows, int t) {
    constexpr int CPR = D / 8;
#pragma unroll
    for (int p = t; p < 32 * CPR; p += NT) {
        const int row = p / CPR, ch = p % CPR;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (row < nrows) x = *reinterpret_cast<const uint4*>(gp + (long)row * stride + 8 * ch);
        *reinterpret_cast<uint4*>(img + row * BwdImg<D>::ROWB + 16 * ch) = x;
    }
}

// Fragment of k-step ks of an image read by rows: lane (r, hh) holds row r, elements 16 ks + 8 hh .. + 7 (the A operand whose
// rows are the image's rows, or the B operand whose columns are)
template <int D>
__device__ __forceinline__ s16x8 bwd_row_frag(const unsigned char* img, int r, int hh, int ks) {
    return *reinterpret_cast<const s16x8*>(img + r * BwdImg<D>::ROWB + 32 * ks + 16 * hh);
}

// A fragment of the TRANSPOSED image, d tile dt, k-step s, for a B operand that is a 32 x 32 accumulator X taken as it lies
// (registers 8 s .. 8 s + 7 converted in order): element j of lane half hh must be image row 16 s + 8 (j >> 2) + 4 hh + (j & 3),
// column 32 dt + (lane & 31).  Lane 4 q + p of a 16-lane group addresses row (.. + q), columns 4 p .. 4 p + 3 of the group's 16
// and receives the group's column (lane & 15) of the four rows.  Every lane of the wave takes part (EXEC is all ones here).
template <int D>
__device__ __forceinline__ s16x8 bwd_tr_frag(const unsigned char* img, int lane, int dt, int s) {
    const int hh = lane >> 5, g4 = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    const unsigned char* p = img + (16 * s + 4 * hh + tq) * BwdImg<D>::ROWB + 2 * (32 * dt + 16 * (g4 & 1) + 4 * tp);
    const s16x4 lo = bwd_tr_read(p), hi = bwd_tr_read(p + 8 * BwdImg<D>::ROWB);
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__device__ __forceinline__ uint4 bwd_load16(const unsigned short* p, bool ok) {
    uint4 x = make_uint4(0, 0, 0, 0);
    if (ok) x = *reinterpret_cast<const uint4*>(p);
    return x;
}

// log2 of a positive finite x, exact at the powers of two: the exponent by integer extraction, the hardware log2 on [1, 2)
__device__ __forceinline__ float bwd_log2(float x) {
    const int e = __builtin_amdgcn_frexp_expf(x);
    const float mant = __builtin_amdgcn_frexp_mantf(x);     // [0.5, 1)
    return (float)(e - 1) + __builtin_amdgcn_logf(mant * 2.0f);
}

// the key row i of a 32 x 32 accumulator holds in lane half hh
__device__ __forceinline__ int bwd_acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// What the row pass and the dq kernel share: the wave's rows and its walk
struct BwdRows {
    int b, h, qb, r0, row, kvlen, lim, glim, count;
    bool ok;
    const int32_t* list;
};
__device__ __forceinline__ BwdRows bwd_rows(const BwdArgs& a, int wave, int r) {
    BwdRows w;
    const int gpb = a.blk / 64;                 // 64-row groups per query block
    w.qb = blockIdx.x / gpb;
    w.b = blockIdx.z;
    w.h = blockIdx.y;
    w.r0 = w.qb * a.blk + (blockIdx.x - w.qb * gpb) * 64 + 32 * wave;
    w.row = w.r0 + r;
    w.ok = w.row < a.Sq;
    w.kvlen = a.kv_len ? min(max(a.kv_len[w.b], 0), a.Sk) : a.kv_valid;
    // one past the last key the lane's row sees; glim: the same of the wave's last row (no row of the wave sees a key from there on)
    const int rl = min(w.r0 + 31, a.Sq - 1);
    w.lim = !w.ok ? 0 : (a.causal ? min(w.kvlen, max(0, w.row + w.kvlen - a.Sq + 1)) : w.kvlen);
    w.glim = a.causal ? min(w.kvlen, max(0, rl + w.kvlen - a.Sq + 1)) : w.kvlen;
    const long lrow = ((long)w.b * a.Hl + w.h / (a.H / a.Hl)) * a.NQ + w.qb;
    w.count = min(max(a.rcounts[lrow], 0), a.NK);
    w.list = a.rcols + lrow * a.NK;
    return w;
}

template <typename Tag, int D>
__global__ __launch_bounds__(BWD_ROW_NT) void bwd_row_kernel(const BwdArgs a) {
    constexpr int KS = D / 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BwdImg<D>::BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    unsigned char* const kimg = lds + wave * BwdImg<D>::BYTES;
    const BwdRows w = bwd_rows(a, wave, r);
    if (w.r0 >= a.Sq) return;                   // (wave-uniform) the whole wave lies past the last row
    const int rr = w.ok ? w.row : 0;
    const unsigned short* qp = a.q + (long)w.b * a.qsb + (long)w.h * a.qsh + (long)rr * a.qss + 8 * hh;
    s16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = rsa_q_frag<Tag>(qp + 16 * ks, w.ok, a.qk_scale);
    const unsigned short* kb = a.k + (long)w.b * a.ksb + (long)(w.h / (a.H / a.Hkv)) * a.ksh;

    float m = -INFINITY, l = 0.f;
    for (int e = 0; e < w.count; ++e) {
        const int jb = w.list[e];
        if (jb < 0 || jb >= a.NKt) continue;
        for (int c = 0; c < a.blk / 32; ++c) {
            const int j0 = jb * a.blk + 32 * c;
            if (j0 >= w.glim) break;
            bwd_stage<D, 64>(kimg, kb + (long)j0 * a.kss, a.kss, w.kvlen - j0, lane);
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) s = Elem<Tag>::mfma(bwd_row_frag<D>(kimg, r, hh, ks), qf[ks], s);
            float x[16], mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                x[i] = j0 + bwd_acc_row(i, hh) < w.lim ? s[i] : -INFINITY;
                mx = fmaxf(mx, x[i]);
            }
            const float mn = fmaxf(m, mx);
            const float mref = mn == -INFINITY ? 0.f : mn;
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) ps += __builtin_amdgcn_exp2f(x[i] - mref);
            l = l * __builtin_amdgcn_exp2f(m - mref) + ps;
            m = mn;
        }
    }
    // the two lane halves of a row hold disjoint keys: they meet here (the sum is commutative: both halves hold the same bytes)
    const float mo = __shfl_xor(m, 32, 64), lo = __shfl_xor(l, 32, 64);
    const float mt = fmaxf(m, mo);
    const float mref = mt == -INFINITY ? 0.f : mt;
    const float lt = l * __builtin_amdgcn_exp2f(m - mref) + lo * __builtin_amdgcn_exp2f(mo - mref);
    // delta: the lane's half of the channels in ascending order, then the other half's
    float dl = 0.f;
    {
        const unsigned short* op = a.o + (long)w.b * a.osb + (long)w.h * a.osh + (long)rr * a.oss + (D / 2) * hh;
        const unsigned short* gp = a.g + (long)w.b * a.gsb + (long)w.h * a.gsh + (long)rr * a.gss + (D / 2) * hh;
#pragma unroll
        for (int ch = 0; ch < D / 16; ++ch) {
            const uint4 xo = bwd_load16(op + 8 * ch, w.ok), xg = bwd_load16(gp + 8 * ch, w.ok);
            const unsigned wo[4] = {xo.x, xo.y, xo.z, xo.w}, wg[4] = {xg.x, xg.y, xg.z, xg.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dl = __builtin_fmaf(rsa_to_f32<Tag>((unsigned short)(wg[i] & 0xFFFF)), rsa_to_f32<Tag>((unsigned short)(wo[i] & 0xFFFF)), dl);
                dl = __builtin_fmaf(rsa_to_f32<Tag>((unsigned short)(wg[i] >> 16)), rsa_to_f32<Tag>((unsigned short)(wo[i] >> 16)), dl);
            }
        }
    }
    dl = dl + __shfl_xor(dl, 32, 64);
    if (w.ok && hh == 0) {
        const long idx = ((long)w.b * a.H + w.h) * a.Sq + w.row;
        a.lse[idx] = lt > 0.f ? mt + bwd_log2(lt) : -INFINITY;
        a.delta[idx] = dl;
    }
}

template <typename Tag, int D>
__global__ __launch_bounds__(BWD_ROW_NT) void bwd_dq_kernel(const BwdArgs a) {
    constexpr int KS = D / 16, DT = D / 32;
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * BwdImg<D>::BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    unsigned char* const kimg = lds + 2 * wave * BwdImg<D>::BYTES;
    unsigned char* const vimg = kimg + BwdImg<D>::BYTES;
    const BwdRows w = bwd_rows(a, wave, r);
    if (w.r0 >= a.Sq) return;                   // (wave-uniform)
    const int rr = w.ok ? w.row : 0;
    const unsigned short* qp = a.q + (long)w.b * a.qsb + (long)w.h * a.qsh + (long)rr * a.qss + 8 * hh;
    const unsigned short* gp = a.g + (long)w.b * a.gsb + (long)w.h * a.gsh + (long)rr * a.gss + 8 * hh;
    s16x8 qf[KS], gf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = rsa_q_frag<Tag>(qp + 16 * ks, w.ok, a.qk_scale);
        gf[ks] = __builtin_bit_cast(s16x8, bwd_load16(gp + 16 * ks, w.ok));
    }
    // the row constants: -lse2 and -delta (a row that sees nothing has lse2 = -inf: none of its keys passes the selection below)
    float nl = 0.f, nd = 0.f;
    if (w.ok) {
        const long idx = ((long)w.b * a.H + w.h) * a.Sq + w.row;
        const float ls = a.lse[idx];
        nl = ls > -INFINITY ? -ls : 0.f;
        nd = -a.delta[idx];
    }
    const int hk = w.h / (a.H / a.Hkv);
    const unsigned short* kb = a.k + (long)w.b * a.ksb + (long)hk * a.ksh;
    const unsigned short* vb = a.v + (long)w.b * a.vsb + (long)hk * a.vsh;
    f32x16 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;

    for (int e = 0; e < w.count; ++e) {
        const int jb = w.list[e];
        if (jb < 0 || jb >= a.NKt) continue;
        for (int c = 0; c < a.blk / 32; ++c) {
            const int j0 = jb * a.blk + 32 * c;
            if (j0 >= w.glim) break;
            bwd_stage<D, 64>(kimg, kb + (long)j0 * a.kss, a.kss, w.kvlen - j0, lane);
            bwd_stage<D, 64>(vimg, vb + (long)j0 * a.vss, a.vss, w.kvlen - j0, lane);
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = nl; dp[i] = nd; }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                s = Elem<Tag>::mfma(bwd_row_frag<D>(kimg, r, hh, ks), qf[ks], s);
                dp = Elem<Tag>::mfma(bwd_row_frag<D>(vimg, r, hh, ks), gf[ks], dp);
            }
            float ds[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = j0 + bwd_acc_row(i, hh) < w.lim ? __builtin_amdgcn_exp2f(s[i]) : 0.f;
                ds[i] = p * dp[i];
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const s16x8 dsf = Elem<Tag>::cvt8(ds + 8 * st);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) acc[dt] = Elem<Tag>::mfma(bwd_tr_frag<D>(kimg, lane, dt, st), dsf, acc[dt]);
            }
        }
    }
    if (w.ok) {
        unsigned short* op = a.dq + (long)w.b * a.dqsb + (long)w.h * a.dqsh + (long)w.row * a.dqss;
        const float4 zero[4] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) rsa_out_tile<Tag, false>(op, dt, hh, acc[dt], a.sm_scale, zero);
    }
}

template <typename Tag, int D, int BLK>
__global__ __launch_bounds__(2 * BLK) void bwd_dkdv_kernel(const BwdArgs a) {
    constexpr int NT = 2 * BLK, KS = D / 16, DT = D / 32, IMG = BwdImg<D>::BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char lds[3 * IMG + 3 * 32 * 4];
    unsigned char* const qsimg = lds;               // the slice's scaled Q, its Q and its dO
    unsigned char* const qrimg = lds + IMG;
    unsigned char* const goimg = lds + 2 * IMG;
    float* const negl = reinterpret_cast<float*>(lds + 3 * IMG);
    float* const negd = negl + 32;
    int* const rlim = reinterpret_cast<int*>(negd + 32);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int jb = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int kvlen = a.kv_len ? min(max(a.kv_len[b], 0), a.Sk) : a.kv_valid;
    const int key = jb * BLK + 32 * wave + r;
    const bool kok = key < kvlen;
    s16x8 kf[KS], vf[KS];
    {
        const int kr = kok ? key : 0;
        const unsigned short* kp = a.k + (long)b * a.ksb + (long)hk * a.ksh + (long)kr * a.kss + 8 * hh;
        const unsigned short* vp = a.v + (long)b * a.vsb + (long)hk * a.vsh + (long)kr * a.vss + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = __builtin_bit_cast(s16x8, bwd_load16(kp + 16 * ks, kok));
            vf[ks] = __builtin_bit_cast(s16x8, bwd_load16(vp + 16 * ks, kok));
        }
    }
    f32x16 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) { dk[dt][i] = 0.f; dv[dt][i] = 0.f; }

    const int gq = a.H / a.Hkv;
    const bool live = jb < a.NK && jb * BLK < kvlen;        // (uniform) the block has a list and a key below the limit
    for (int hi = 0; live && hi < gq; ++hi) {
        const int h = hk * gq + hi;
        const long crow = ((long)b * a.Hl + h / (a.H / a.Hl)) * a.NK + jb;
        const int count = min(max(a.ccounts[crow], 0), a.NQ);
        const int32_t* clist = a.ccols + crow * a.NQ;
        const unsigned short* qb_ = a.q + (long)b * a.qsb + (long)h * a.qsh;
        const unsigned short* gb_ = a.g + (long)b * a.gsb + (long)h * a.gsh;
        const long sbase = ((long)b * a.H + h) * a.Sq;
        for (int e = 0; e < count; ++e) {
            const int qb = clist[e];
            if (qb < 0 || qb >= a.NQ) continue;
            const int rend = min((qb + 1) * BLK, a.Sq);
            for (int r0 = qb * BLK; r0 < rend; r0 += 32) {
                // (uniform) causal: the slice's last row sees no key of this block
                if (a.causal && min(r0 + 31, a.Sq - 1) + kvlen - a.Sq < jb * BLK) continue;
                __syncthreads();            // the previous slice's reads are done
                constexpr int CPR = D / 8;
#pragma unroll
                for (int p = tid; p < 32 * CPR; p += NT) {
                    const int row = p / CPR, ch = p % CPR;
                    const bool ok = r0 + row < a.Sq;
                    const long rq = ok ? r0 + row : 0;
                    const unsigned short* qp = qb_ + rq * a.qss + 8 * ch;
                    const int off = row * BwdImg<D>::ROWB + 16 * ch;
                    *reinterpret_cast<uint4*>(qrimg + off) = bwd_load16(qp, ok);
                    *reinterpret_cast<s16x8*>(qsimg + off) = rsa_q_frag<Tag>(qp, ok, a.qk_scale);
                    *reinterpret_cast<uint4*>(goimg + off) = bwd_load16(gb_ + rq * a.gss + 8 * ch, ok);
                }
                if (tid < 32) {
                    const int row = r0 + tid;
                    const bool ok = row < a.Sq;
                    float ls = -INFINITY, dl = 0.f;
                    if (ok) { ls = a.lse[sbase + row]; dl = a.delta[sbase + row]; }
                    negl[tid] = ls > -INFINITY ? -ls : 0.f;
                    negd[tid] = -dl;
                    rlim[tid] = !ok ? 0 : (a.causal ? min(kvlen, max(0, row + kvlen - a.Sq + 1)) : kvlen);
                }
                __syncthreads();
                f32x16 s, dp;
                int lim[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int qr = bwd_acc_row(i, hh);
                    s[i] = negl[qr];
                    dp[i] = negd[qr];
                    lim[i] = rlim[qr];
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    s = Elem<Tag>::mfma(bwd_row_frag<D>(qsimg, r, hh, ks), kf[ks], s);
                    dp = Elem<Tag>::mfma(bwd_row_frag<D>(goimg, r, hh, ks), vf[ks], dp);
                }
                float p[16], ds[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    p[i] = key < lim[i] ? __builtin_amdgcn_exp2f(s[i]) : 0.f;
                    ds[i] = p[i] * dp[i];
                }
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const s16x8 pf = Elem<Tag>::cvt8(p + 8 * st), dsf = Elem<Tag>::cvt8(ds + 8 * st);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        dv[dt] = Elem<Tag>::mfma(bwd_tr_frag<D>(goimg, lane, dt, st), pf, dv[dt]);
                        dk[dt] = Elem<Tag>::mfma(bwd_tr_frag<D>(qrimg, lane, dt, st), dsf, dk[dt]);
                    }
                }
            }
        }
    }
    if (key < a.Sk) {
        unsigned short* kp = a.dk + (long)b * a.dksb + (long)hk * a.dksh + (long)key * a.dkss;
        unsigned short* vp = a.dv + (long)b * a.dvsb + (long)hk * a.dvsh + (long)key * a.dvss;
        const float4 zero[4] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            rsa_out_tile<Tag, false>(kp, dt, hh, dk[dt], a.sm_scale, zero);
            rsa_out_tile<Tag, false>(vp, dt, hh, dv[dt], 1.0f, zero);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static int bwd_check_shape(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int block, int NQ, int NK) {
    if (B < 0 || H < 0 || Sq < 0 || Hkv <= 0 || Hl <= 0 || Sk <= 0 || NQ < 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (H > 0 && (H % Hkv || H % Hl || (Hl != 1 && Hl != Hkv && Hl != H))) return RSA_ERR_BAD_ARG;
    if (NQ != (Sq + block - 1) / block || NK > (Sk + block - 1) / block) return RSA_ERR_BAD_ARG;
    if (NQ > BWD_MAX_BLOCKS || (Sk + block - 1) / block > BWD_MAX_BLOCKS) return RSA_ERR_UNSUPPORTED;
    if (B > 65535 || H > 65535) return RSA_ERR_UNSUPPORTED;         // grid axes
    return RSA_OK;
}

static size_t bwd_rows_bytes(int B, int H, int Sq) { return (((size_t)B * H * Sq * 4) + 15) & ~(size_t)15; }

extern "C" int rsa_block_sparse_bwd_bytes(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int block, int NQ, int NK,
                                          size_t* bytes) {
    if (!bytes) return RSA_ERR_BAD_ARG;
    const int st = bwd_check_shape(B, H, Hkv, Hl, Sq, Sk, D, block, NQ, NK);
    if (st != RSA_OK) return st;
    *bytes = 2 * bwd_rows_bytes(B, H, Sq);      // lse2, then delta
    return RSA_OK;
}

template <typename Tag, int D>
static void bwd_launch(const BwdArgs& a, int B, hipStream_t s) {
    const dim3 grid_rows(a.NQ * (a.blk / 64), a.H, B), grid_keys(a.NKt, a.Hkv, B);
    bwd_row_kernel<Tag, D><<<grid_rows, BWD_ROW_NT, 0, s>>>(a);
    bwd_dq_kernel<Tag, D><<<grid_rows, BWD_ROW_NT, 0, s>>>(a);
    if (a.blk == 128) bwd_dkdv_kernel<Tag, D, 128><<<grid_keys, 256, 0, s>>>(a);
    else bwd_dkdv_kernel<Tag, D, 64><<<grid_keys, 128, 0, s>>>(a);
}

extern "C" int rsa_block_sparse_bwd(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                                    int kv_valid, const int32_t* kv_len_dev, int causal, double sm_scale, rsa_tensor4 q,
                                    rsa_tensor4 k, rsa_tensor4 v, rsa_tensor4 out, rsa_tensor4 dout, const int32_t* row_cols,
                                    const int32_t* row_counts, const int32_t* col_cols, const int32_t* col_counts, void* ws,
                                    size_t ws_bytes, rsa_out4 dq, rsa_out4 dk, rsa_out4 dv, void* stream) {
    int st = bwd_check_shape(B, H, Hkv, Hl, Sq, Sk, D, block, NQ, NK);
    if (st != RSA_OK) return st;
    if (dtype != RSA_BF16 && dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (kv_valid < 0 || kv_valid > Sk || !(sm_scale == sm_scale)) return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(kv_len_dev) & 3) return RSA_ERR_BAD_ARG;
    const rsa_tensor4* ins[5] = {&q, &k, &v, &out, &dout};
    for (const rsa_tensor4* t : ins) {
        if ((st = rsa_check_tensor(*t)) != RSA_OK) return st;
        if (t->stride_b < 0 || t->stride_h < 0 || t->stride_s < 0) return RSA_ERR_BAD_ARG;
    }
    const rsa_out4* outs[3] = {&dq, &dk, &dv};
    for (int i = 0; i < 3; ++i) {           // a result row is written once: positive strides where an axis has more than one entry
        const rsa_out4& o = *outs[i];
        if ((st = rsa_check_out(o)) != RSA_OK) return st;
        const int heads = i == 0 ? H : Hkv, rows = i == 0 ? Sq : Sk;
        if ((B > 1 && o.stride_b <= 0) || (heads > 1 && o.stride_h <= 0) || (rows > 1 && o.stride_s <= 0)) return RSA_ERR_BAD_ARG;
        if (o.stride_b < 0 || o.stride_h < 0 || o.stride_s < 0) return RSA_ERR_BAD_ARG;
    }
    if (!row_cols || !row_counts || !col_cols || !col_counts) return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(row_cols) | reinterpret_cast<uintptr_t>(row_counts) | reinterpret_cast<uintptr_t>(col_cols) |
         reinterpret_cast<uintptr_t>(col_counts)) & 3)
        return RSA_ERR_BAD_ARG;
    const size_t rb = bwd_rows_bytes(B, H, Sq);
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15)) return RSA_ERR_BAD_ARG;
    if (ws_bytes < 2 * rb) return RSA_ERR_WORKSPACE;
    if (B == 0 || H == 0 || Sq == 0) return RSA_OK;

    BwdArgs a;
    a.q = static_cast<const unsigned short*>(q.ptr), a.qsb = q.stride_b, a.qsh = q.stride_h, a.qss = q.stride_s;
    a.k = static_cast<const unsigned short*>(k.ptr), a.ksb = k.stride_b, a.ksh = k.stride_h, a.kss = k.stride_s;
    a.v = static_cast<const unsigned short*>(v.ptr), a.vsb = v.stride_b, a.vsh = v.stride_h, a.vss = v.stride_s;
    a.o = static_cast<const unsigned short*>(out.ptr), a.osb = out.stride_b, a.osh = out.stride_h, a.oss = out.stride_s;
    a.g = static_cast<const unsigned short*>(dout.ptr), a.gsb = dout.stride_b, a.gsh = dout.stride_h, a.gss = dout.stride_s;
    a.dq = static_cast<unsigned short*>(dq.ptr), a.dqsb = dq.stride_b, a.dqsh = dq.stride_h, a.dqss = dq.stride_s;
    a.dk = static_cast<unsigned short*>(dk.ptr), a.dksb = dk.stride_b, a.dksh = dk.stride_h, a.dkss = dk.stride_s;
    a.dv = static_cast<unsigned short*>(dv.ptr), a.dvsb = dv.stride_b, a.dvsh = dv.stride_h, a.dvss = dv.stride_s;
    a.rcols = row_cols, a.rcounts = row_counts, a.ccols = col_cols, a.ccounts = col_counts;
    a.kv_len = kv_len_dev, a.kv_valid = kv_valid;
    a.H = H, a.Hkv = Hkv, a.Hl = Hl, a.Sq = Sq, a.Sk = Sk, a.NQ = NQ, a.NK = NK, a.NKt = (Sk + block - 1) / block, a.blk = block;
    a.causal = causal ? 1 : 0;
    a.qk_scale = (float)(sm_scale * 1.44269504);    // (as rsa_block_sparse_plain_fwd)
    a.sm_scale = (float)sm_scale;
    a.lse = static_cast<float*>(ws);
    a.delta = reinterpret_cast<float*>(static_cast<unsigned char*>(ws) + rb);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == RSA_BF16) {
        if (D == 128) bwd_launch<bf16_tag, 128>(a, B, s);
        else bwd_launch<bf16_tag, 64>(a, B, s);
    } else {
        if (D == 128) bwd_launch<fp16_tag, 128>(a, B, s);
        else bwd_launch<fp16_tag, 64>(a, B, s);
    }
    return rsa_launch_status();
}
