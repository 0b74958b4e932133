// K3 from a caller's block mask (include/rsa.h: rsa_select_from_mask, rsa_rectified_attention_masked and their _ex forms).
//
// The rectified call's selection pass is K1 (pool) -> K2 (pooled scores + GAPR) -> K3 (softmax, IPAR, sort, threshold, unions,
// R, w, lists) -> K4 (comp = w . vbar).  Only K3's sort and unions depend on how the kept set is chosen: here the kept set is
// the caller's mask row as it stands, so the pass reads the row and skips the sort.  Everything else is K3's: the softmax and
// IPAR in select_mask_long_kernel's order (contract C5 / C6: bit-identical probabilities), R as the contract's strided tree over
// M = kept | GAPR, w = probs outside M, and the kept lists in K3's format.
// Compiled with -ffp-contract=off, as rsa_stats.hip: every fused multiply-add of the contract is explicit.
#include "rsa_common.h"

struct MaskSelectArgs {
    const float* scores;
    const uint8_t* unrel;
    const uint8_t* mask;
    long msb, msh, msq;   // mask byte strides (b, h: 0 = broadcast); the key axis is contiguous
    float *probs, *w, *R;
    uint32_t* bitmask;
    int32_t *cols, *counts;
    int H, NBv, n_txt, NS, L, NB_total, NW;
    float scale;
    float blk;            // tokens per block: IPAR's weight of a visual block
};

// One 256-thread workgroup per (bh, visual query block) row; thread t owns the elements j = t (mod 256) in ascending j, which
// are the contract's 256 strided partial sums (as in select_mask_long_kernel).
// dynamic LDS: float xs[NS] | u8 mk[NB_total], mk bit 0 = kept (the caller's byte != 0), bit 1 = GAPR (unrel, j < NBv)
__global__ __launch_bounds__(256) void select_from_mask_kernel(MaskSelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float red[4];
    const int t = threadIdx.x;
    const long row = blockIdx.x;
    const long bh = row / a.NBv;
    const int qblk = (int)(row % a.NBv);
    float* xs = reinterpret_cast<float*>(smem);
    uint8_t* mk = smem + (((size_t)a.NS * 4 + 15) & ~(size_t)15);
    const float* sc = a.scores + row * a.NS;
    const uint8_t* mrow = a.mask + (bh / a.H) * a.msb + (bh % a.H) * a.msh + (long)qblk * a.msq;
    const uint8_t* urow = a.unrel + row * a.NBv;
    const bool has_txt = a.n_txt > 0;

    // the row's mask and GAPR bytes (read first: nothing below waits on them before the first barrier), scaled scores, row maximum
#pragma unroll 4
    for (int j = t; j < a.NB_total; j += 256) {
        const uint8_t kb = mrow[j] != 0 ? 1 : 0;
        const uint8_t ub = (j < a.NBv && urow[j] != 0) ? 2 : 0;
        mk[j] = kb | ub;
    }
    float mx = -INFINITY;
#pragma unroll 4
    for (int j = t; j < a.NS; j += 256) {
        const float x = sc[j] * a.scale;
        xs[j] = x;
        mx = fmaxf(mx, x);
    }
    mx = block_max(mx, red);
    // exp and denominator (C6)
    float part = 0.0f;
    for (int j = t; j < a.NS; j += 256) {
        const float e = rsa_exp(xs[j] - mx);
        xs[j] = e;
        part = part + e;
    }
    const float Z = block_tree_sum(part, red);
    for (int j = t; j < a.NS; j += 256) xs[j] = xs[j] / Z;
    if (has_txt) {   // IPAR: the text tokens' probabilities collapse into one entry (column NBv)
        __syncthreads();
        float pn = 0.0f, pt = 0.0f;
        for (int j = t; j < a.NBv; j += 256) pn = pn + xs[j];
        for (int u = t; u < a.n_txt; u += 256) pt = pt + xs[a.NBv + u];
        const float normal_sum = block_tree_sum(pn, red);
        const float text_sum = block_tree_sum(pt, red);
        const float denom = normal_sum * a.blk + text_sum;
        __syncthreads();
        for (int j = t; j < a.NBv; j += 256) xs[j] = (xs[j] * a.blk) / denom;
        if (t == 0) xs[a.NBv] = text_sum / denom;
    }
    __syncthreads();
    // probs, then R and w over M = kept | GAPR (j < NBv), M_NBv = kept_NBv (mk of j >= NBv carries no GAPR bit)
    float pr = 0.0f;
    for (int j = t; j < a.L; j += 256) {
        const float pj = xs[j];
        const bool mm = mk[j] != 0;
        a.probs[row * a.L + j] = pj;
        pr = pr + (mm ? pj : 0.0f);
        a.w[row * a.L + j] = mm ? 0.0f : pj;
    }
    const float Rv = block_tree_sum(pr, red);
    if (t == 0) a.R[row] = Rv;
    // bitmask words and the ascending list: wave 0 walks the row in 64-block steps, as the end of select_mask_kernel does
    if (t < 64) {
        const int lane = t;
        int off = 0;
        for (int b0 = 0; b0 < a.NB_total; b0 += 64) {
            const int j = b0 + lane;
            const bool f = j < a.NB_total && (mk[j] & 1) != 0;
            const unsigned long long m = __ballot(f);
            if (f) a.cols[row * a.NB_total + off + __popcll(m & ((1ull << lane) - 1ull))] = j;
            off += __popcll(m);
            const int wi = (b0 >> 5) + (lane >> 5);
            if ((lane & 31) == 0 && wi < a.NW) a.bitmask[row * a.NW + wi] = (unsigned)(m >> (lane & 32));
        }
        if (lane == 0) a.counts[row] = off;
    }
}

// Host-side checks, all before any launch.  The row-length refusal is select_mask_b's (rsa_stats.hip) for the same layout: its
// one-wave kernel serves every row it accepts, and its workgroup-per-row kernel refuses rows of more than 8 192 entries or key
// blocks, or more than 150 KB of LDS -- the conditions below, with the same LDS formula.
static int mask_select_check(const rsa_layout* l, int blk, const uint8_t* mask, int64_t sb, int64_t sh, int64_t sq,
                             const rsa_buffers* buf, size_t* lds) {
    int st = rsa_check_layout_b(l, blk);
    if (st != RSA_OK) return st;
    if (!mask || !buf || !buf->scores || !buf->unrel || !buf->probs || !buf->w || !buf->R || !buf->bitmask || !buf->cols ||
        !buf->counts)
        return RSA_ERR_BAD_ARG;
    if (sb < 0 || sh < 0 || sq <= 0) return RSA_ERR_BAD_ARG;
    const int L = l->NBv + (l->n_txt > 0 ? 1 : 0), NS = l->NBv + l->n_txt;
    int n2 = 64;
    while (n2 < L) n2 <<= 1;
    if (l->NBv > 0) {
        if (n2 > 8192 || l->NB_total > 8192) return RSA_ERR_UNSUPPORTED;
        const size_t k3_long = (((size_t)NS * 4 + 15) & ~(size_t)15) + (size_t)n2 * 8 + (((size_t)l->NB_total + 15) & ~(size_t)15);
        if (k3_long > 150 * 1024) return RSA_ERR_UNSUPPORTED;
    }
    *lds = (((size_t)NS * 4 + 15) & ~(size_t)15) + (((size_t)l->NB_total + 15) & ~(size_t)15);
    return RSA_OK;
}

static int select_from_mask_b(const rsa_layout* l, int blk, const uint8_t* mask, int64_t sb, int64_t sh, int64_t sq,
                              const rsa_buffers* buf, void* stream) {
    size_t lds = 0;
    const int st = mask_select_check(l, blk, mask, sb, sh, sq, buf, &lds);
    if (st != RSA_OK) return st;
    if (l->NBv == 0) return RSA_OK;
    MaskSelectArgs a;
    a.scores = buf->scores; a.unrel = buf->unrel; a.mask = mask;
    a.msb = sb; a.msh = sh; a.msq = sq;
    a.probs = buf->probs; a.w = buf->w; a.R = buf->R; a.bitmask = buf->bitmask; a.cols = buf->cols; a.counts = buf->counts;
    a.H = l->H; a.NBv = l->NBv; a.n_txt = l->n_txt; a.NS = l->NBv + l->n_txt; a.L = l->NBv + (l->n_txt > 0 ? 1 : 0);
    a.NB_total = l->NB_total; a.NW = (l->NB_total + 31) / 32;
    a.scale = (float)(1.0 / sqrt((double)l->D));  // head_dim ** -0.5 rounded to fp32, as K3
    a.blk = (float)blk;
    const long rows = (long)l->B * l->H * l->NBv;
    if (rows > 0x7FFFFFFFL) return RSA_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(select_from_mask_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
    select_from_mask_kernel<<<dim3((unsigned)rows), 256, lds, static_cast<hipStream_t>(stream)>>>(a);
    return rsa_launch_status();
}

extern "C" int rsa_select_from_mask(const rsa_layout* l, const uint8_t* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                                    int64_t mask_stride_q, const rsa_buffers* buf, void* stream) {
    return select_from_mask_b(l, RSA_BLOCK, mask, mask_stride_b, mask_stride_h, mask_stride_q, buf, stream);
}

extern "C" int rsa_select_from_mask_ex(const rsa_layout_ex* lx, const uint8_t* mask, int64_t mask_stride_b,
                                       int64_t mask_stride_h, int64_t mask_stride_q, const rsa_buffers* buf, void* stream) {
    return rsa_layout_ex_ok(lx)
               ? select_from_mask_b(&lx->base, lx->block, mask, mask_stride_b, mask_stride_h, mask_stride_q, buf, stream)
               : RSA_ERR_BAD_ARG;
}

extern "C" int rsa_rectified_attention_masked(const rsa_layout* l, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                              const uint8_t* mask, int64_t sb, int64_t sh, int64_t sq, void* workspace,
                                              size_t workspace_bytes, rsa_out4 out, void* stream) {
    rsa_buffers buf;
    size_t lds = 0;
    int st = rsa_carve_workspace(l, workspace, workspace_bytes, &buf);
    if (st != RSA_OK) return st;
    if ((st = mask_select_check(l, RSA_BLOCK, mask, sb, sh, sq, &buf, &lds))) return st;
    if ((st = rsa_pool_stats(l, q, k, v, &buf, stream))) return st;
    if ((st = rsa_pooled_scores(l, k, &buf, stream))) return st;
    if ((st = rsa_select_from_mask(l, mask, sb, sh, sq, &buf, stream))) return st;
    if ((st = rsa_compensation(l, &buf, stream))) return st;
    return rsa_block_sparse_fwd(l, q, k, v, &buf, out, stream);
}

extern "C" int rsa_rectified_attention_masked_ex(const rsa_layout_ex* lx, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                                 const uint8_t* mask, int64_t sb, int64_t sh, int64_t sq, void* workspace,
                                                 size_t workspace_bytes, rsa_out4 out, void* stream) {
    if (!rsa_layout_ex_ok(lx)) return RSA_ERR_BAD_ARG;
    if (lx->block == RSA_BLOCK)
        return rsa_rectified_attention_masked(&lx->base, q, k, v, mask, sb, sh, sq, workspace, workspace_bytes, out, stream);
    rsa_buffers buf;
    size_t lds = 0;
    int st = rsa_carve_workspace_ex(lx, workspace, workspace_bytes, &buf);
    if (st != RSA_OK) return st;
    if ((st = mask_select_check(&lx->base, lx->block, mask, sb, sh, sq, &buf, &lds))) return st;
    if ((st = rsa_pool_stats_ex(lx, q, k, v, &buf, stream))) return st;
    if ((st = rsa_pooled_scores_ex(lx, k, &buf, stream))) return st;
    if ((st = rsa_select_from_mask_ex(lx, mask, sb, sh, sq, &buf, stream))) return st;
    if ((st = rsa_compensation_ex(lx, &buf, stream))) return st;
    return rsa_block_sparse_fwd_ex(lx, q, k, v, &buf, out, stream);
}
