/*
 * rsa.h -- C-ABI of librsa_hip.so: the MI355X (gfx950) rectified block-sparse attention path.
 *
 * This is the drop-in boundary for the reference's hot path (BienLuky/Rectified-SpaAttn).  The reference has
 * no FFI of its own (it is pure Python + one Triton kernel); each entry point below names the reference
 * function (file:line under the reference root) whose work it replaces, and INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; all tensor pointers are DEVICE pointers unless marked host
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never allocates, never
 *     synchronises, never throws; returns RSA_OK or a negative rsa_status
 *   - q/k/v are [B, H, S, D] views described by element strides (stride_b, stride_h, stride_s); the head
 *     dimension is contiguous.  dtype: RSA_BF16 or RSA_FP16 (2-byte elements)
 *   - "bh" below means the flattened index b*H + h
 *   - statistics follow the fp32 numeric contract written in oracle/rsa_oracle.c (C1..C8)
 */
#ifndef RSA_H_
#define RSA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSA_BLOCK 128 /* tokens per block (block_size_M = block_size_N = 128 in every reference script) */

typedef enum rsa_status {
    RSA_OK = 0,
    RSA_ERR_BAD_ARG = -1,       /* null pointer, negative size, inconsistent layout */
    RSA_ERR_UNSUPPORTED = -2,   /* head_dim not in {64,128}, dtype unknown, row too long for the select kernel */
    RSA_ERR_WORKSPACE = -3,     /* workspace too small */
    RSA_ERR_LAUNCH = -4         /* hipGetLastError() after a launch was not hipSuccess */
} rsa_status;

typedef enum rsa_dtype { RSA_BF16 = 0, RSA_FP16 = 1 } rsa_dtype;

/* Geometry of one self-attention call.  The four reference variants differ only in these numbers
 * (hunyuan :313-332, flux :307-320, cogvideo :306-322, wan21 :297-313). */
typedef struct rsa_layout {
    int32_t B, H, D;
    int32_t S;               /* true sequence length (q and kv) */
    int32_t NB_total;        /* ceil(S / 128): the reference zero-pads up to this */
    int32_t NBv;             /* visual blocks == sparse query blocks */
    int32_t n_txt;           /* valid text tokens scored individually ("attenable"); 0 = no text tail, no IPAR */
    int32_t kv_valid;        /* kv columns >= kv_valid are masked in the sparse pass ("seqlens") */
    int32_t pool_valid;      /* K/V rows >= pool_valid count as zero when pooling (hunyuan zeroes them :307-308) */
    int32_t text_end_block;  /* text blocks [NBv, text_end_block) are kept by every query block */
    int32_t first_frame_blocks; /* wan: rows < ffb keep cols < ffb (wan21 :270-271) */
    int32_t q_text_valid;    /* text query rows [NBv*128, NBv*128+q_text_valid): dense attention */
    int32_t kv_text_valid;   /*   ... over kv [0, kv_text_valid); later rows up to S are written as 0 */
    int32_t dtype;           /* rsa_dtype */
} rsa_layout;

typedef struct rsa_tensor4 { /* a [B, H, S, D] view */
    const void* ptr;
    int64_t stride_b, stride_h, stride_s; /* in elements */
} rsa_tensor4;

typedef struct rsa_out4 {
    void* ptr;
    int64_t stride_b, stride_h, stride_s;
} rsa_out4;

/* Sizes (in elements) of the intermediate buffers for a layout; all are per call.  Fill the struct with
 * rsa_carve_workspace, or zero it first (memset) and set the members by hand: a member this header adds in a later
 * version is then NULL = "feature not used" (check rsa_version() >= 300 for this layout: 15 members; >= 310 for the
 * block-scaled rsa_fp8_operands). */
typedef struct rsa_buffers {
    float* qbar;      /* [BH, NBv, D]       block means of visual Q            */
    float* aq;        /* [BH, NBv, D]       mean |Q - qbar|                    */
    float* kbar;      /* [BH, NBv, D]                                          */
    float* ak;        /* [BH, NBv, D]                                          */
    float* vbar;      /* [BH, NB_total, D]                                     */
    float* scores;    /* [BH, NBv, NBv + n_txt]  unscaled pooled scores        */
    uint8_t* unrel;   /* [BH, NBv, NBv]     GAPR: 1 = pooled compensation NOT trustworthy */
    float* probs;     /* [BH, NBv, L]       L = NBv + (n_txt > 0): implicit full attention row */
    float* w;         /* [BH, NBv, L]       compensation weights (probs where dropped & reliable, else 0) */
    float* R;         /* [BH, NBv]          rectification factor               */
    float* comp;      /* [BH, NBv, D]       sum_j w_ij * vbar_j                 */
    uint32_t* bitmask;/* [BH, NBv, ceil(NB_total/32)]  kept blocks, bit j%32 of word j/32 */
    int32_t* cols;    /* [BH, NBv, NB_total] kept block indices ascending (first counts[] entries valid) */
    int32_t* counts;  /* [BH, NBv]                                              */
    /* split-KV partials (may be NULL: then nothing is split).  First region: the dense TEXT query blocks -- K5 splits each
     * text block's key range over up to RSA_TEXT_SPLIT workgroups and a small combine kernel merges them (NULL: one workgroup
     * walks all keys of a text block).  Second region, RSA_TAIL_PIECES more [128, D + 2] blocks behind it (since 0.4.0): the
     * walks of the LAST, partial generation of sparse query blocks, split over the workgroup slots that generation would
     * leave idle (head dim 128; merged, rectified and stored by a second combine kernel): */
    float* tpart;     /* [BH * (NB_total - NBv) * RSA_TEXT_SPLIT + RSA_TAIL_PIECES, 128, D + 2]  unnormalised O, then (m, l) per query row */
    /* (since 0.5.0; not a buffer: RSA_NUM_BUFFERS stays 15) bytes the caller allocated behind tpart.  rsa_carve_workspace
     * fills it; a host that sets tpart by hand must set it too: K5 clamps the text split and the tail split to what fits,
     * and a non-NULL tpart with tpart_bytes == 0 is refused (RSA_ERR_WORKSPACE) instead of trusted -- the formula above grew
     * in 0.4.0, and a buffer sized by an older header would otherwise be overrun. */
    size_t tpart_bytes;
} rsa_buffers;
#define RSA_NUM_BUFFERS 15
#define RSA_TEXT_SPLIT 32
#define RSA_TAIL_PIECES 512

/* Library identification: returns 10000*major + 100*minor + patch. */
int rsa_version(void);

/* ABI guard (since 0.6.0).  rsa_buffers GREW in 0.5.0 (tpart_bytes behind the 15 pointers) and carries no size member of
 * its own: a host compiled against an older header hands the library a shorter struct, and what lies behind it is read as a
 * capacity.  Call this ONCE after loading the library, with the macros of the header the host was compiled against:
 *     if (rsa_abi_check(RSA_HEADER_VERSION, sizeof(rsa_buffers), sizeof(rsa_layout)) != RSA_OK) refuse to run;
 * RSA_OK iff the library was built from a header with the same struct sizes and the same major.minor; RSA_ERR_UNSUPPORTED
 * otherwise.  (The Python host calls it when it loads the library; examples/c_host does too.) */
#define RSA_HEADER_VERSION 601
int rsa_abi_check(int header_version, size_t sizeof_rsa_buffers, size_t sizeof_rsa_layout);

/* Process-global switch (default 0).  K5 plans two things from the SIZE OF THE LAUNCH: how many pieces the dense text rows
 * are split into (32 on grids of fewer than 8 generations, else 16) and whether the walks of the last, partial generation are
 * split over its idle slots.  Both change the summation order of the rows they touch, so a head-sharded run (3 heads per
 * rank) and the unsharded one (24 heads) agree on those rows within rounding, not byte for byte.  on != 0 plans both per
 * head (16 text pieces, no tail split): every rank then produces exactly the bytes the unsharded call produces for its
 * heads, at 3-5 % of K5 on short grids.  Returns the previous value.
 * Nothing else looks at the launch: the selection pass is per (b, h) with or without the switch -- K4 picks between its two
 * forms (which differ in bits) from NBv alone -- so mask, lists, R and comp of a rank are the unsharded call's bytes always. */
int rsa_set_shard_invariant(int on);

/* Bytes needed for each rsa_buffers member, written in member order into sizes[RSA_NUM_BUFFERS], and their sum
 * (each rounded up to 256 B) into *total.  Lets a caller carve one workspace.  Replaces the ~25 temporaries
 * the reference allocates per call (hunyuan :189-262, :348-357). */
int rsa_buffer_bytes(const rsa_layout* lay, size_t sizes[RSA_NUM_BUFFERS], size_t* total);

/* Carve `ws` (>= total bytes from rsa_buffer_bytes, 256-B aligned) into an rsa_buffers. */
int rsa_carve_workspace(const rsa_layout* lay, void* ws, size_t ws_bytes, rsa_buffers* out);

/* K1 -- one HBM pass over Q (visual rows), K, V: block means and mean-absolute-deviations.
 * Replaces: Q/K pooling hunyuan :189-194 (wan21 :189-192), V pooling :356, and the |Q - qbar| / |K - kbar|
 * statistics of estimate_pr_gain, gapr_mask.py:19-23,:30. */
int rsa_pool_stats(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const rsa_buffers* buf,
                   void* stream);

/* K2 -- pooled scores qbar.kbar^T (+ one column per valid text token), and the GAPR bit.
 * Replaces: bmm hunyuan :198-205 and estimate_pr_gain gapr_mask.py:26-42. */
int rsa_pooled_scores(const rsa_layout* lay, rsa_tensor4 k, const rsa_buffers* buf, void* stream);

/* K3 -- per (b,h,q-block) row: softmax, IPAR, stable descending sort, cumulative threshold, top-k,
 * neighbour / text / first-frame union, bitmask + ascending column list, R and compensation weights.
 * neighbor: device uint8 [NBv, NBv] (row-major, nonzero = neighbour) or NULL.
 * Replaces: hunyuan :208-277 (wan21 :206-271) and the rectification masks :348-355. */
int rsa_select_mask(const rsa_layout* lay, const uint8_t* neighbor, int top_k, float p_remain,
                    const rsa_buffers* buf, void* stream);

/* K4 -- comp = w @ vbar.  Replaces torch.matmul(attn_pool_novalid, value_pool), hunyuan :357. */
int rsa_compensation(const rsa_layout* lay, const rsa_buffers* buf, void* stream);

/* K5 -- block-sparse flash attention over the kept lists with the fused rectification epilogue
 *   O = (acc / l) * R + comp   for visual query blocks, exact dense attention for text query rows,
 * written straight into `out` ([B, S, H, D] element strides: the reference's final permute+reshape,
 * hunyuan :383-387, becomes a strided store).
 * Replaces: _triton_block_sparse_attention_onehot + kernel hunyuan :15-168, the R/comp combine :365,
 * the text-row flash call :371-380 and the concat :383. */
int rsa_block_sparse_fwd(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                         const rsa_buffers* buf, rsa_out4 out, void* stream);

/* The whole operator = K1..K5 on one stream.  Replaces rectified_block_sparse_attention /
 * block_sparse_attention_combined (hunyuan :283-417, flux :282-405, cogvideo :282-407, wan21 :276-386). */
int rsa_rectified_attention(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                            const uint8_t* neighbor, int top_k, float p_remain, void* workspace,
                            size_t workspace_bytes, rsa_out4 out, void* stream);

/* Dense attention with the reference's two-segment varlen semantics (attn.py:107-120 as called from
 * hunyuan :503-524): query rows < q_split attend kv [0, kv_split); rows >= q_split attend kv [kv_split, Sk).
 * q: [B,H,Sq,D], k/v: [B,H,Sk,D]; out: [B,Sq,H,D]-strided.  With q_split = Sq, kv_split = Sk it is plain
 * softmax attention (fullattn mode "torch"/"vanilla", attn.py:101-106, :121-149, without bias). */
int rsa_dense_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                  int q_split, int kv_split, rsa_out4 out, void* stream);
/* The same with causal = True (attn.py:60-73 forwards it to flash_attn_varlen_func, :108-116): inside a segment key j
 * is visible to row i iff j <= i + (keys - rows) -- flash-attn's bottom-right alignment, which is the top-left mask of
 * the reference's "torch" / "vanilla" modes (attn.py:105, :129-133) whenever a segment has as many keys as rows. */
int rsa_dense_causal_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                         int q_split, int kv_split, rsa_out4 out, void* stream);

/* Dense attention with an arbitrary mask: fullattn's "torch" / "vanilla" modes when attn_mask depends on the query row
 * (attn.py:101-106: SDPA takes any mask broadcastable to [b, a, s, s1]; :134-147: boolean masks become -inf, float masks are
 * added to the scores).  mask: DEVICE pointer; mask_kind: RSA_MASK_BOOL (1 byte per element, 0 = not attended),
 * RSA_MASK_ADD_2BYTE (additive, in the dtype of q) or RSA_MASK_ADD_F32; mask_stride_*: ELEMENT strides of its [b, a, s, s1]
 * view, 0 for a broadcast dimension.  A query row without any attended key gives NaN when empty_rows_nan != 0 (an explicit
 * softmax over an all -inf row: the reference's "vanilla" mode) and zeros otherwise (torch's fused SDPA since 2.5: its "torch" mode).
 * The plain kernel of the family (no pipeline of the reference builds such a mask; key masks go through rsa_dense_fwd's key
 * limit): expect a fraction of rsa_dense_fwd's rate.  D = 64 or 128; out as rsa_dense_fwd. */
#define RSA_MASK_BOOL 1
#define RSA_MASK_ADD_2BYTE 2
#define RSA_MASK_ADD_F32 3
int rsa_dense_masked_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                         const void* mask, int mask_kind, int64_t mask_stride_b, int64_t mask_stride_h,
                         int64_t mask_stride_q, int64_t mask_stride_k, int empty_rows_nan, rsa_out4 out, void* stream);

/* The same kernel with DROPOUT on the attention weights (fullattn's drop_rate: attn.py:104-106 hands it to SDPA as dropout_p,
 * :148 applies torch.dropout to the softmax's output): every weight is kept with probability 1 - drop_rate and scaled by
 * 1 / (1 - drop_rate), the softmax's denominator keeps all of them.  The keep decisions are a counter-based hash of (seed, batch *
 * head, query row, key): reproducible for a seed, not torch's Philox stream (which cannot be reproduced from outside) -- what the
 * reference's semantics fix is the distribution.  mask may be NULL with mask_kind = 0; causal != 0: key j is attended by row i
 * only if j <= i (the reference's "torch" / "vanilla" triangle).  drop_rate in [0, 1].  Since 0.5.0. */
int rsa_dense_dropout_fwd(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                          const void* mask, int mask_kind, int64_t mask_stride_b, int64_t mask_stride_h,
                          int64_t mask_stride_q, int64_t mask_stride_k, int causal, int empty_rows_nan, float drop_rate,
                          uint64_t seed, rsa_out4 out, void* stream);

/* ---- 64-token blocks (since 0.6.1; the reference's block_size_M = block_size_N = 64, rectified_hunyuan_attn.py:171-222,
 * :283-389).  Every function above keeps its 128-token meaning; these take the block size beside the layout.  All rsa_layout
 * members count blocks of `block` tokens (NB_total = ceil(S / block), text rows start at NBv * block).  rsa_buffers is the same
 * struct, sized by rsa_buffer_bytes_ex.  block = 128 gives exactly the calls above; block = 64 is the 2-byte path (no fp8
 * form); anything else is RSA_ERR_UNSUPPORTED. ---- */
typedef struct rsa_layout_ex {
    rsa_layout base;
    int32_t block;           /* tokens per block: 64 or 128 */
    int32_t reserved[3];     /* zero (the _ex entry points return RSA_ERR_BAD_ARG otherwise) */
} rsa_layout_ex;
int rsa_buffer_bytes_ex(const rsa_layout_ex* lay, size_t sizes[RSA_NUM_BUFFERS], size_t* total);
int rsa_carve_workspace_ex(const rsa_layout_ex* lay, void* ws, size_t ws_bytes, rsa_buffers* out);
int rsa_pool_stats_ex(const rsa_layout_ex* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const rsa_buffers* buf,
                      void* stream);
int rsa_pooled_scores_ex(const rsa_layout_ex* lay, rsa_tensor4 k, const rsa_buffers* buf, void* stream);
int rsa_select_mask_ex(const rsa_layout_ex* lay, const uint8_t* neighbor, int top_k, float p_remain,
                       const rsa_buffers* buf, void* stream);
int rsa_compensation_ex(const rsa_layout_ex* lay, const rsa_buffers* buf, void* stream);
/* At block 64 one workgroup (4 waves) owns the query blocks 2i and 2i + 1 and walks the union of their kept lists, one 64-key
 * tile per entry; each wave pair masks the tiles its own block did not keep. */
int rsa_block_sparse_fwd_ex(const rsa_layout_ex* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                            const rsa_buffers* buf, rsa_out4 out, void* stream);
int rsa_rectified_attention_ex(const rsa_layout_ex* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                               const uint8_t* neighbor, int top_k, float p_remain, void* workspace,
                               size_t workspace_bytes, rsa_out4 out, void* stream);

/* ---- caller-supplied block masks: the reference's _triton_block_sparse_attention_onehot (rectified_hunyuan_attn.py:108-168,
 * same in the flux / cogvideo / wan21 files) over a mask of the caller's own.  Additive: no struct above changes. ----
 *
 * Dense [B, H, NQ, NK] block mask -> the kept lists of rsa_buffers, in K3's format with NBv = NQ and NB_total = NK:
 * bitmask [BH, NQ, ceil(NK/32)], cols [BH, NQ, NK] (ascending; only the first counts[] entries are written), counts [BH, NQ].
 * mask: DEVICE uint8, nonzero = kept (a torch bool tensor has these bytes); ELEMENT strides per axis, 0 for a broadcast axis,
 * the key axis contiguous.  NK <= 8192 (K5's key-block limit).  One wave per row. */
int rsa_block_mask_to_lists(int B, int H, int NQ, int NK, const uint8_t* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                            int64_t mask_stride_q, uint32_t* bitmask, int32_t* cols, int32_t* counts, void* stream);
/* The inverse: bitmask [BH, NQ, ceil(NK/32)] -> contiguous [B, H, NQ, NK] uint8 mask of 0 / 1. */
int rsa_lists_to_block_mask(int B, int H, int NQ, int NK, const uint32_t* bitmask, uint8_t* mask, void* stream);

/* Plain block-sparse attention (K5 without the rectification epilogue) over such lists:
 *   O[b, h, i] = softmax over the keys j < kv_valid of the kept blocks of row block i / block of (sm_scale q_i . k_j) applied to V
 * q [B, H, Sq, D], k / v [B, H, Sk, D] (Sq and Sk may differ; the last query and key blocks may be ragged); cols / counts as
 * rsa_block_mask_to_lists writes them, with NQ = ceil(Sq / block) rows per head and NK <= ceil(Sk / block) blocks per row (keys
 * past NK * block are never visited).  1 <= kv_valid <= Sk; sm_scale finite, of either sign.  block: 64 or 128; D: 64 or 128; dtype: RSA_BF16 / RSA_FP16.  Exactly
 * the rows < Sq of `out` (a [B, Sq, H, D]-strided view as in rsa_block_sparse_fwd) are written; a row without a visible key is 0.
 * tpart / tpart_bytes: optional partial buffer (NULL / 0: nothing is split); with >= RSA_TAIL_PIECES * 128 * (D + 2) floats, the
 * walks of a last, partial generation of workgroups are split over its idle slots (head dim 128, 128-token blocks), as in
 * rsa_block_sparse_fwd. */
int rsa_block_sparse_plain_fwd(int B, int H, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, int kv_valid,
                               double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const int32_t* cols,
                               const int32_t* counts, float* tpart, size_t tpart_bytes, rsa_out4 out, void* stream);

/* The same call with a key range per query row (found by symbol: the header version stays 6.1).  Query row r of batch item b and
 * head h sees key j iff its block is in the lists  and  lo <= j < hi  and  j < kv_valid  and  j < NK * block, with
 *     lo = row_lo[b * range_stride_b + r]  (row_lo NULL: 0),   hi = row_hi[b * range_stride_b + r],
 * DEVICE int32 arrays of Sq entries per batch item (range_stride_b = 0: one array for every batch item), clamped into
 * [0, kv_valid] on the device -- any int32 may be passed; hi <= lo is the empty range, and a row without a visible key is 0.
 * Ranges need not grow with the row.  Causal, sliding-window and chunk-causal masks at token granularity and per-batch key
 * limits that live on the device are all such ranges (block_sparse_attention(causal= / window= / row_range=) builds them).
 * The kernel drops the listed blocks no row of a query block can see before it stages anything; blocks that some rows see only
 * in part (the diagonal of a causal mask) run masked, block by block, as the last blocks of every walk do.
 * Everything rsa_block_sparse_plain_fwd refuses is refused here; besides: block != 128 is RSA_ERR_UNSUPPORTED (64-token blocks
 * run the 32-rows-per-wave kernel, which has one scalar key limit and no per-row range); row_hi NULL, a negative stride or an
 * array that is not 4-byte aligned is RSA_ERR_BAD_ARG. */
int rsa_block_sparse_ranged_fwd(int B, int H, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, int kv_valid,
                                double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const int32_t* cols,
                                const int32_t* counts, const int32_t* row_lo, const int32_t* row_hi, int64_t range_stride_b,
                                float* tpart, size_t tpart_bytes, rsa_out4 out, void* stream);

/* The same two calls with grouped-query K/V heads (GQA; Hkv = 1: MQA; found by symbol: the header version stays 6.1).  q and out
 * hold H heads, k and v Hkv, H a multiple of Hkv; query head h reads K/V head h / (H / Hkv) -- the convention of flash-attn and of
 * torch's enable_gqa, the result of repeating every K/V head H / Hkv times along the head axis, without the copies.  cols / counts
 * hold Hl list heads per batch item ([B * Hl, NQ, NK] / [B * Hl, NQ], H a multiple of Hl): head h walks list row
 * (b * Hl + h / (H / Hl)) * NQ + query block.  Hl = Hkv is one selection per K/V head (NSA- and MoBA-style), Hl = 1 one for all heads,
 * Hl = H one per query head.  row_hi NULL (then row_lo NULL too): no ranges, else as rsa_block_sparse_ranged_fwd.
 * Two forms, same softmax: (a) every query head a walk of its own -- the launch of the MHA call, byte for byte what that call gives
 * on repeated K/V and lists; (b) two query heads of one K/V head and one list row as the four waves of one workgroup on ONE K/V
 * ring, where block = 128 and H / Hkv and H / Hl are even (no tail split then).  (b) equals (a) byte for byte unless a bf16 walk's
 * optimistic softmax reference overflowed: the workgroup then redoes BOTH heads' walks through the online body.  The library takes
 * (a) unless the tuning key k5_gqa_pair is 1.  Hkv = Hl = H launches what the two entries above launch.
 * H, Hkv or Hl non-positive or not dividing H: RSA_ERR_BAD_ARG; ranges with block 64: RSA_ERR_UNSUPPORTED; row_lo without row_hi, a
 * negative stride, a misaligned range array: RSA_ERR_BAD_ARG; besides, everything rsa_block_sparse_plain_fwd refuses.  The
 * rectified calls, the selection pass and the e4m3 forms have no grouped form: they pool K per head. */
int rsa_block_sparse_gqa_fwd(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                             int kv_valid, double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                             const int32_t* cols, const int32_t* counts, const int32_t* row_lo, const int32_t* row_hi,
                             int64_t range_stride_b, float* tpart, size_t tpart_bytes, rsa_out4 out, void* stream);

/* ---- top-k block selection per list head, written straight into the list contract above (MoBA-style; found by symbol: the
 * header version stays 6.1).  q [B, H, Sq, D], k [B, Hkv, Sk, D], H a multiple of Hkv, query head h
 * belongs to K/V head h / (H / Hkv); Hl list heads per batch item, Hl = Hkv (one selection per K/V head, scored with the sum of
 * its query heads' pooled queries) or Hl = H (one per query head).  len_b = kv_len_dev[b] clamped into [0, Sk] (DEVICE int32, B
 * values, read on the device only) or, with kv_len_dev NULL, kv_valid in [0, Sk]; off_b = len_b - Sq.
 *   pooling   qbar[b, h, i] = fp32 sum of the rows < Sq of query block i / their count; kbar[b, hk, j] the same over the keys
 *             < len_b of key block j
 *   score     t[b, hl, i, j] = sum over the list head's query heads, ascending, of <qbar[b, h, i], kbar[b, hk, j]> (fp32, no scale)
 *   visible   j * block < len_b, and with causal j * block <= r1 + off_b, r0 .. r1 the rows of query block i: the blocks in which
 *             the causal attention call lets some row of the block see some key
 *   forced    the visible j < keep_first, and with keep_local >= 1 those in [jd_lo - (keep_local - 1), jd_hi] (without causal up
 *             to jd_hi + (keep_local - 1)), jd_lo = max(r0 + off_b, 0) / block, jd_hi = min(max(r1 + off_b, 0), len_b - 1) / block
 *   kept      forced and the best max(top_k - |forced|, 0) visible unforced blocks by t, the lower j first among equals:
 *             |kept| = min(max(top_k, |forced|), |visible|)
 * Output: bitmask [B * Hl, NQ, ceil(NK/32)], cols [B * Hl, NQ, NK], counts [B * Hl, NQ] exactly as rsa_block_mask_to_lists
 * writes them (row (b * Hl + hl) * NQ + i), and, unless scores is NULL, t as fp32 [B, Hl, NQ, NK] with -inf at invisible blocks.
 * NQ = ceil(Sq / block), NK = ceil(Sk / block) <= 8192; block 64 or 128; D 16, 32, 64 or 128, all native.  ws: DEVICE scratch of
 * at least rsa_block_select_bytes(...) bytes, 16-byte aligned (the pooled vectors).  Two launches, no atomics on floats: the same
 * inputs give the same bytes.  With non-finite scores which blocks win is unspecified; the lists stay well formed.
 * Non-positive sizes, Hkv not dividing H, Hl other than Hkv or H, NQ / NK not matching Sq / Sk, a negative top_k / keep_first /
 * keep_local, kv_valid outside [0, Sk], a NULL or misaligned pointer or stride: RSA_ERR_BAD_ARG; block, D, dtype or NK outside
 * the above: RSA_ERR_UNSUPPORTED; ws_bytes too small: RSA_ERR_WORKSPACE.  Every check runs before the first HIP call. */
int rsa_block_select_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes);
int rsa_block_select(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                     rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first,
                     int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                     void* stream);

/* ---- block-sparse DECODE attention: a few query rows over a (paged) K/V cache (found by symbol: the header version stays 6.1;
 * DESIGN.md section 5.12).  q [B, H, Sq, D] with Sq <= block (ONE query block), k / v [B, Hkv, Sk, D], H a multiple of Hkv, query
 * head h reads K/V head h / (H / Hkv); Hl list heads per batch item, Hl in {1, Hkv, H}; cols [B * Hl, NK] / counts [B * Hl] as
 * rsa_block_mask_to_lists or rsa_block_select write them for NQ = 1.  A unit = the H / max(Hl, Hkv) query heads that share a K/V
 * head and a list row; its Sq * H / max(Hl, Hkv) rows must not exceed 64 (four 16-row MFMA tiles: RSA_ERR_UNSUPPORTED beyond).
 * len_b = kv_len_dev[b] clamped into [0, Sk] (DEVICE int32, B values, never read on the host) or, with kv_len_dev NULL, kv_valid.
 *   visible   row r of (b, h) sees key j iff block j / block is in the list row of (b, list head of h), j < len_b,
 *             j < NK * block, and with causal j <= r + len_b - Sq (bottom-right aligned; both block sizes).  A row without a
 *             visible key is 0 and its log-sum-exp -inf.
 *   cache     keys at or beyond len_b may hold anything (NaN, Inf): they are never multiplied.  block_table NULL: k / v are the
 *             [B, Hkv, Sk, D] views.  Otherwise block_table is DEVICE int32 [B, >= NK] with row stride table_stride_b, k / v are
 *             page pools [num_pages, Hkv, block, D] (stride_b = the page stride), Sk = the logical capacity, and key j of batch
 *             item b is row j % block of page block_table[b][j / block].  The table is read only for listed blocks that hold a
 *             key below len_b; a listed block whose page lies outside [0, num_pages), like a list entry outside [0, NK),
 *             contributes no key and is not read.
 *   numerics  those of the 2-byte rsa_block_sparse_plain_fwd: Q * (float)(sm_scale * 1.44269504) rounded to the input type,
 *             log2-domain scores, P rounded to the input type for P.V, fp32 accumulation, one division and one conversion.
 *   splits    one workgroup per (unit, split); split s takes list entries [s C, (s + 1) C), C = blocks_per_split (0: the
 *             library's choice, min(8, NK): measured, profiles/decode_perf.txt).  The grid's split extent is ceil(NK / C);
 *             workgroups past a list's end leave at once.  ws holds the partials (fp32 O, m, l per unit, split and row):
 *             rsa_block_sparse_decode_bytes(...) bytes, 16-byte aligned.  A second small launch merges them in ascending s.  The
 *             result may depend on blocks_per_split through the summation order; for one value two calls give the same bytes
 *             (no atomics on floats).
 *   outputs   out [B, H, Sq, D] through any strides that are multiples of 4 elements (pointer 8-byte aligned); lse NULL or fp32
 *             [B, H, Sq] contiguous: ln sum_j exp(sm_scale q . k_j) over the visible keys, (m + log2 l) ln 2.
 * Non-positive sizes, Hkv not dividing H, Hl not in {1, Hkv, H}, NK outside 1 .. min(ceil(Sk / block), 8192), kv_valid outside
 * [0, Sk], Sq > block, a NULL or misaligned pointer, a negative stride, a table with num_pages <= 0, a negative
 * blocks_per_split: RSA_ERR_BAD_ARG; D outside {64, 128}, block outside {64, 128}, an unknown dtype, more than 64 rows per unit:
 * RSA_ERR_UNSUPPORTED; ws_bytes too small: RSA_ERR_WORKSPACE.  Every check runs before the first HIP call. */
int rsa_block_sparse_decode_bytes(int B, int H, int Hkv, int Hl, int Sq, int D, int NK, int blocks_per_split, size_t* bytes);
int rsa_block_sparse_decode(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                            const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q, rsa_tensor4 k,
                            rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b, int num_pages, const int32_t* cols,
                            const int32_t* counts, int blocks_per_split, void* ws, size_t ws_bytes, rsa_out4 out, float* lse,
                            void* stream);

/* ---- a cache of pooled keys for the selection, and the selection from it (found by symbol: the header version stays 6.1;
 * DESIGN.md section 5.13).  One decode step is rsa_pool_keys (the blocks the step touched) -> rsa_block_select_pooled ->
 * rsa_block_sparse_decode: all on the device, no host read, capturable in one graph.
 *
 * rsa_pool_keys writes out[b, hk, j, :] (fp32 [B, Hkv, NK, D] contiguous, 16-byte aligned) = the kbar of rsa_block_select above,
 * with its summation order, for exactly the blocks j with start_b / block <= j < ceil(len_b / block), and no other byte of out;
 * start_b > len_b writes nothing.  len_b = kv_len_dev[b] clamped into [0, Sk] (DEVICE int32, B values, never read on the host) or,
 * with kv_len_dev NULL, kv_valid in [0, Sk]; start_b likewise from start_dev or start.  Keys at or beyond len_b are never loaded.
 * k: [B, Hkv, Sk, D] through any strides that are multiples of 8 elements, NK = ceil(Sk / block) <= 8192; or, with block_table
 * (DEVICE int32 [B, >= NK], row stride table_stride_b), a page pool [num_pages, Hkv, block, D] (stride_b = the page stride) with
 * Sk = NK * block: block j of batch item b is page block_table[b][j].  The table is read for written blocks only; an entry
 * outside [0, num_pages) gives a block of zeros and no address is formed from it.  workgroups_per_head workgroups per (b, K/V
 * head) stride over the block range (a device limit does not size the grid); any count >= 1 gives the same bytes; 0 = the exact
 * count when both limits are host values, NK when start is the host value 0, else 2.  One launch.
 *
 * rsa_block_select_pooled is rsa_block_select with kbar read from pooled_k (fp32 [B, Hkv, NK, D] contiguous, 16-byte aligned) and
 * Sk = NK * block: on inputs both accept, and pooled_k = rsa_pool_keys of the same k and limit, it writes the same bytes (lists
 * and scores).  Only the visible prefix of pooled_k is read; the rest may hold anything.  score_splits workgroups per list row
 * compute the row's scores (1: inside the select workgroup; 0: the library's choice, a function of B * Hl * NQ, NK and D alone; at
 * most 256); every value gives the same bytes.  ws: rsa_block_select_pooled_bytes(...) bytes, 16-byte aligned.  Two launches
 * with one split, three with more.
 * Refusals as rsa_block_select's and rsa_block_sparse_decode's: non-positive sizes, Hkv not dividing H, Hl other than Hkv or H,
 * NQ / NK not matching Sq / Sk, a negative top_k / keep_first / keep_local / workgroups_per_head / score_splits (or one above
 * 256), kv_valid or start outside [0, Sk], a NULL or misaligned pointer or stride, a negative stride, a table with num_pages <= 0:
 * RSA_ERR_BAD_ARG; block, D, dtype or NK outside the above: RSA_ERR_UNSUPPORTED; ws_bytes too small: RSA_ERR_WORKSPACE.  Every
 * check runs before the first HIP call. */
int rsa_pool_keys(int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                  int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid, const int32_t* start_dev,
                  int start, int workgroups_per_head, float* out, void* stream);
int rsa_block_select_pooled_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes);
int rsa_block_select_pooled(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                            const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first,
                            int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                            int32_t* counts, float* scores, void* stream);

/* ---- the decode step over an e4m3 K/V cache with one static fp32 scale per K/V head (found by symbol: the header version stays
 * 6.1).  The cache holds OCP e4m3fn codes, one byte per element: [B, Hkv, Sk, D], or with a block_table
 * page pools [num_pages, Hkv, block, D]; its strides count bytes.  The value of a code is float(code) * scale[hk]; k_scale and
 * v_scale are DEVICE fp32 arrays of Hkv values, positive and finite.  They are not checked and no address depends on them: a
 * zero, negative, infinite or NaN scale garbles the rows of its head and nothing else.  Head dims 64 and 128 only.
 *
 * rsa_kv8_append writes new rows.  k_new / v_new: [B, Hkv, T, D] of `dtype` through any strides rsa_block_sparse_decode accepts
 * for k / v (never copied).  Token t < n_b of batch item b goes to position start_b + t; start_b = start_dev[b] clamped into
 * [0, Sk] (DEVICE int32, B values, never read on the host) or, with start_dev NULL, start in [0, Sk]; n_b likewise from n_new_dev
 * (clamped into [0, T]) or n_new.  Sk is the capacity: the caches' rows, or with a table NKt * block for a table [B, >= NKt] with
 * row stride table_stride_b.  The grid is sized from T alone.  Per element: y = x / scale[hk] as one IEEE fp32 division, clamped to
 * [-448, 448] (+-Inf saturate; a NaN becomes the NaN code with the sign bit of its input), converted round-to-nearest-even with
 * subnormals kept.  The call writes the D
 * bytes of every placed row and no other byte; a position at or beyond Sk, or one whose table entry lies outside [0, num_pages),
 * is dropped and no address is formed from it.  Two batch items that map to one page race: the caller's business.  Caches: pointer
 * and strides multiples of 8 bytes (8-byte stores).  One launch, prefill is the call with start = 0.
 *
 * rsa_block_sparse_decode_kv8 is rsa_block_sparse_decode over such a cache: its argument list with k_scale and v_scale in front of
 * the stream; dtype names q's (and out's) type; the workspace is rsa_block_sparse_decode_bytes'.  The codes become q's type in
 * registers (exact: every finite e4m3 value is a bf16 and an fp16), the MFMAs, the softmax, the splits and the merge are those of
 * the 2-byte call.  The K scale multiplies each fp32 score once behind the dot product, before masking and the maximum; the V
 * scale multiplies the merged row once, out = round((O / l) * v_scale[hk]); l and the log-sum-exp do not see v_scale.  With
 * power-of-two scales (and nothing under- or overflowing) the bytes are those of rsa_block_sparse_decode on the cache
 * code * scale.  Every rule of that call holds word for word (visible set, device kv_len, bytes beyond len_b never multiplied,
 * unvisited blocks and out-of-range entries not read).  k: pointer and strides multiples of 8 bytes; v: of 16 bytes; other views are
 * RSA_ERR_BAD_ARG, as is a NULL or misaligned scale pointer.
 *
 * rsa_pool_keys_kv8 is rsa_pool_keys from an e4m3 k (no dtype argument; pointer and strides multiples of 8 bytes): out[b, hk, j, :] =
 * (the fp32 sum of float(code) over the block's keys below len_b, in rsa_pool_keys' order, divided once by their count) multiplied
 * once by k_scale[hk].  Every other clause of rsa_pool_keys holds.  rsa_block_select_pooled reads the fp32 cache as before.
 * Refusals as the 2-byte entries'; D outside {64, 128}: RSA_ERR_UNSUPPORTED.  Every check runs before the first HIP call. */
int rsa_kv8_append(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                   rsa_out4 k_cache, rsa_out4 v_cache, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                   const int32_t* start_dev, int start, const int32_t* n_new_dev, int n_new, const float* k_scale,
                   const float* v_scale, void* stream);
int rsa_block_sparse_decode_kv8(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q, rsa_tensor4 k,
                                rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                                const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws, size_t ws_bytes,
                                rsa_out4 out, float* lse, const float* k_scale, const float* v_scale, void* stream);
int rsa_pool_keys_kv8(int B, int Hkv, int Sk, int D, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                      int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid, const int32_t* start_dev,
                      int start, int workgroups_per_head, float* out, const float* k_scale, void* stream);

/* ---- top-p block selection: a budget per list row (found by symbol: the header version stays 6.1).
 * rsa_block_select_p and rsa_block_select_pooled_p are rsa_block_select and rsa_block_select_pooled -- their argument lists,
 * pooling, scores, visible and forced sets, outputs, workspaces (the _bytes entries return their counterparts' sizes) and refusals
 * -- with p16, c and mass in front of the stream, and top_k as the cap on the kept count.  All weights are integers:
 *   weight    t_max = the maximum of t over the row's visible blocks (forced ones included, -0 as +0); a_j = (t_j - t_max) * c, one
 *             fp32 subtraction and one fp32 multiplication; u_j = (uint32) floor(exp2(a_j) * 2^18 + 0.5) <= 2^18, the product
 *             and the sum in fp32.  c = (float)(score_scale * log2(e)) is formed by the caller; exp2 is exact at integers.
 *   target    total = sum of u_j over the visible blocks; target = (total * p16 + 65535) >> 16 in 64 bits, p16 = round(top_p * 65536)
 *   kept      the forced blocks and the first min(n_p, n_k, |unforced|) visible unforced blocks by t descending, the lower j first
 *             among equals: n_p = the length of the shortest such prefix with sum(forced u) + sum(prefix u) >= target (0 when the
 *             forced blocks alone reach it), n_k = max(top_k - |forced|, 0).  p16 = 0 keeps the forced blocks alone; p16 = 65536
 *             every block of non-zero weight, up to the cap.
 *   mass      NULL, or DEVICE fp32 [B * Hl * NQ]: (float)(sum of u_j over the kept blocks) / (float)total, 0 for a row that sees
 *             nothing.
 * The same inputs give the same bytes (integer sums).  With non-finite scores which blocks win is unspecified; the lists stay well
 * formed.  p16 outside [0, 65536], a c that is not finite or not > 0, a misaligned mass: RSA_ERR_BAD_ARG.  Every check runs before
 * the first HIP call.  The select workgroup runs in place of the top-k one: the same number of launches. */
int rsa_block_select_p_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes);
int rsa_block_select_p(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                       rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first,
                       int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores,
                       int p16, float c, float* mass, void* stream);
int rsa_block_select_pooled_p_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes);
int rsa_block_select_pooled_p(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                              const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                              int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask,
                              int32_t* cols, int32_t* counts, float* scores, int p16, float c, float* mass, void* stream);

/* ---- block-sparse EXTEND attention: a chunk of any number of query rows over a (paged, e4m3) K/V cache that already holds a
 * prefix (found by symbol: the header version stays 6.1).  rsa_block_sparse_extend and
 * rsa_block_sparse_extend_kv8 are rsa_block_sparse_decode and rsa_block_sparse_decode_kv8 -- their argument lists, operand
 * strides and alignment, len_b, the cache and table rules, the numerics, the outputs and the refusals -- with the one-query-block
 * limit and the 64-row limit lifted:
 *   shape     q [B, H, Sq, D] with any Sq >= 1; NQ = ceil(Sq / block) is derived, not passed.  Query block i is rows
 *             [i block, min((i + 1) block, Sq)) of q.  cols [B * Hl, NQ, NK] / counts [B * Hl, NQ] as rsa_block_mask_to_lists,
 *             rsa_block_select and rsa_block_select_pooled write them: the list row of (b, list head hl, query block i) is
 *             (b * Hl + hl) * NQ + i.  lse NULL or fp32 [B, H, Sq].
 *   visible   row r of (b, h) sees key j iff block j / block is in list row (b, list head of h, r / block), j < len_b,
 *             j < NK * block, and with causal j <= r + len_b - Sq (bottom-right aligned, r counted in the whole call).  A row
 *             without a visible key -- every row with r + len_b - Sq < 0 among them -- is 0 and its log-sum-exp -inf.
 *   groups    the H / max(Hl, Hkv) heads x rows-of-block-i rectangle of a unit's query block is cut into row groups of gh heads x
 *             qg query rows: gh = ceil(gu / ceil(gu / 64)), qg = min(64 / gh, Sq, block) (gu = H / max(Hl, Hkv): any gu is served).
 *             One workgroup per (row group, split); a chunk of 32 keys that starts at or beyond the causal limit of the group's
 *             last row is skipped before its loads.  On shapes rsa_block_sparse_decode serves, at an equal explicit
 *             blocks_per_split, the bytes are that call's.
 *   splits    C = blocks_per_split; 0 = the library's choice, a function of the shapes alone: min(8, NK) while the launch has
 *             fewer than 256 row groups, NK (one split) from there on.  ws: rsa_block_sparse_extend_bytes(...) bytes, 16-byte
 *             aligned = groups * ceil(NK / C) * rows16 * (D + 2) * 4, groups = B * max(Hl, Hkv) * ceil(gu / gh) * (the number of
 *             qg-row pieces of the NQ query blocks), rows16 = gh * qg rounded up to 16, 32 or 64.
 * RSA_ERR_UNSUPPORTED beyond the grid: more than 2^31 - 1 row groups, or B * H * Sq * D / 1024 > 2^31 - 1 (the merge's grid);
 * block outside {64, 128} and D outside {64, 128} likewise.  Every other refusal is the decode entries', Sq > block and the row
 * limit apart.  Every check runs before the first HIP call.  Two launches. */
int rsa_block_sparse_extend_bytes(int B, int H, int Hkv, int Hl, int Sq, int D, int block, int NK, int blocks_per_split,
                                  size_t* bytes);
int rsa_block_sparse_extend(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                            const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q, rsa_tensor4 k,
                            rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b, int num_pages, const int32_t* cols,
                            const int32_t* counts, int blocks_per_split, void* ws, size_t ws_bytes, rsa_out4 out, float* lse,
                            void* stream);
int rsa_block_sparse_extend_kv8(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q, rsa_tensor4 k,
                                rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                                const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws, size_t ws_bytes,
                                rsa_out4 out, float* lse, const float* k_scale, const float* v_scale, void* stream);

/* ---- RAGGED chunks: a row count per batch item for the extend call and for the selection (found by symbol: the header version
 * stays 6.1).  q [B, H, Sq, D] holds a padded batch -- prefill chunks, second turns, decode items and draft
 * verifications side by side -- and q_len_dev, DEVICE int32 [B], in front of the stream, the rows of each item: n_b = q_len_dev[b]
 * clamped into [0, Sq] on the device, never read on the host.  q_len_dev NULL: n_b = Sq, the call and the bytes of the entry
 * without it.  len_b (kv_len_dev / kv_valid) is the length AFTER the append: it includes item b's n_b new tokens.
 *   extend    rsa_block_sparse_extend_ragged[_kv8] are rsa_block_sparse_extend[_kv8] -- argument lists, lists, workspace
 *             (rsa_block_sparse_extend_bytes, a function of the padded shapes alone), grid, row groups, splits and refusals --
 *             with n_b where Sq counts rows.  Row r < n_b of (b, h) sees key j iff block j / block is in list row (b, list head of
 *             h, r / block), j < len_b, j < NK * block, and with causal j <= r + len_b - n_b: the extend call on rows [0, n_b) of
 *             item b with len_b, and at an equal explicit blocks_per_split its bytes.  Rows r >= n_b are written: 0, log-sum-exp
 *             -inf.  q's rows at or beyond n_b are never loaded and may hold anything, NaN included.  A row group whose first row
 *             is at or beyond n_b leaves before it reads a list entry, a table entry or a K/V byte, and the merge writes its rows
 *             without reading a partial; list rows of query blocks i >= ceil(n_b / block) are never read.
 *   select    rsa_block_select_ragged and rsa_block_select_pooled_ragged are rsa_block_select_p and rsa_block_select_pooled_p
 *             (workspaces: their _bytes entries) with q_len_dev in front of the stream; p16 = -1 is the plain top-k of
 *             rsa_block_select / rsa_block_select_pooled (c and mass are then not read).  The selection contract with n_b for
 *             Sq: qbar[b, h, i] is the mean over the rows < n_b of block i, off_b = len_b - n_b, r1 = min((i + 1) block, n_b) - 1.
 *             A query block i >= ceil(n_b / block) has no row: counts 0, bitmask words 0, scores -inf, mass 0, cols unspecified
 *             (as beyond counts).  Both entries give the same bytes on shared inputs.
 * A q_len_dev that is not 4-byte aligned: RSA_ERR_BAD_ARG; every other refusal is the counterpart's.  Every check runs before the
 * first HIP call.  The same number of launches as the counterparts; capturable, and a replay follows q_len_dev's values. */
int rsa_block_sparse_extend_ragged(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                   const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                   rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                                   const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws, size_t ws_bytes,
                                   rsa_out4 out, float* lse, const int32_t* q_len_dev, void* stream);
int rsa_block_sparse_extend_ragged_kv8(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                       const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                       rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                       int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws,
                                       size_t ws_bytes, rsa_out4 out, float* lse, const float* k_scale, const float* v_scale,
                                       const int32_t* q_len_dev, void* stream);
int rsa_block_select_ragged(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK,
                            rsa_tensor4 q, rsa_tensor4 k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k,
                            int keep_first, int keep_local, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                            int32_t* counts, float* scores, int p16, float c, float* mass, const int32_t* q_len_dev, void* stream);
int rsa_block_select_pooled_ragged(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK,
                                   rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal,
                                   int top_k, int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes,
                                   uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, int p16, float c, float* mass,
                                   const int32_t* q_len_dev, void* stream);

/* ---- PACKED batches: q [T, H, D] with cu_seqlens_q for the extend call, the pooled selection and the e4m3 append (found by
 * symbol: the header version stays 6.1).  A continuous-batching step holds its tokens back to back: q is
 * [T, H, D] (T, the token budget, a host value that fixes grid and workspace), cu_seqlens_q_dev DEVICE int32 [B + 1] says where
 * each item starts, and max_q_len (M, a host int, 1 <= M <= T: flash-attn's max_seqlen_q) bounds an item's rows.  The device
 * sanitises cu_seqlens_q once per call and never forms an address from a value of it; the host never reads it:
 *     s_b = the running maximum of clamp(cu[b], 0, T),  n_b = min(s_{b+1} - s_b, M),  item b = rows [s_b, s_b + n_b).
 * Rows t < T of no item -- behind s_B, in front of s_0, an item's rows beyond M -- are never loaded (q may hold NaN there).
 * q, out (and k_new / v_new of the append) are passed as rsa_tensor4 / rsa_out4 whose stride_s is the stride of a row (a token) and
 * stride_h that of a head; stride_b is not read.  Strides as the padded entries ask (multiples of 8 elements for q, 4 for out): a
 * view of a fused projection [T, (H + 2 Hkv) D] runs without a copy.  len_b (kv_len_dev / kv_valid) is the length AFTER the append.
 *   extend    rsa_block_sparse_extend_packed[_kv8] are rsa_block_sparse_extend_ragged[_kv8] with T in front, M where Sq stood and
 *             cu_seqlens_q_dev where q_len_dev stood.  cols / counts keep the padded layout [B * Hl, NQ, NK] / [B * Hl, NQ] with
 *             NQ = ceil(M / block); list rows of query blocks i >= ceil(n_b / block) are never read.  Item b is
 *             rsa_block_sparse_extend on q[s_b : s_b + n_b] seen as [1, H, n_b, D] with its list rows and len_b (causal: j <= r +
 *             len_b - n_b), at an equal explicit blocks_per_split its bytes, and the bytes of the ragged entry on the padded
 *             copy.  out [T, H, D] and lse fp32 [T, H]: every row is written exactly once, rows of no item as 0 / -inf before a
 *             list row or a partial is looked at.  Row groups: gh as in extend, qg = min(64 / gh, block, M) -- M = 1 runs the
 *             one-row-tile kernels decode runs.  A scan launch writes the sanitised starts and the prefix sums of the items' row
 *             groups to the head of the workspace; the split kernel's grid holds QP * U * HC workgroups, QP a host bound on the
 *             row groups any sanitised cu_seqlens_q can ask for (rsa_block_sparse_extend_packed_bytes reports it in *pieces,
 *             which may be NULL): the live ones are the first, the rest leave before they read a list entry, a table entry or a
 *             K/V byte.  blocks_per_split 0: min(8, NK) while QP * U * HC < 256, else NK.  Three launches.
 *             rsa_block_sparse_extend_packed_bytes: the workspace, a function of its host arguments alone.
 *   select    rsa_block_select_pooled_packed is rsa_block_select_pooled_ragged with T in front, M where Sq stood (NQ =
 *             ceil(M / block)) and cu_seqlens_q_dev, item_ws where q_len_dev stood; item_ws: DEVICE int32 [2 (B + 1)] scratch of
 *             the call.  Workspace: rsa_block_select_pooled_p_bytes(B, ..., NQ, NK).  Results [B * Hl, NQ, ..] with the bytes of
 *             the ragged entry on the padded copy of q with q_len = n_b.  One launch more than that entry (the scan).
 *   append    rsa_kv8_append_packed is rsa_kv8_append with k_new / v_new [T, Hkv, D] and cu_seqlens_dev, item_ws where n_new_dev,
 *             n_new stood; item_ws: DEVICE int32 [B + 1] scratch.  Token t < n_b of item b is row s_b + t and goes to position
 *             start[b] + t, with n_b = s_{b+1} - s_b (M = T).  The grid is sized from T.  Placed and untouched bytes are those of
 *             the padded entry.  Two launches.
 * Refusals (RSA_ERR_BAD_ARG), all before the first HIP call: T < 1, M outside [1, T], cu_seqlens_q_dev / item_ws NULL or not
 * 4-byte aligned, and whatever the counterpart refuses.  Capturable; a replay follows cu_seqlens_q's values. */
int rsa_block_sparse_extend_packed_bytes(int T, int B, int H, int Hkv, int Hl, int max_q_len, int D, int block, int NK,
                                         int blocks_per_split, size_t* bytes, int64_t* pieces);
int rsa_block_sparse_extend_packed(int T, int B, int H, int Hkv, int Hl, int max_q_len, int Sk, int D, int dtype, int block, int NK,
                                   const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                   rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                                   const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws, size_t ws_bytes,
                                   rsa_out4 out, float* lse, const int32_t* cu_seqlens_q_dev, void* stream);
int rsa_block_sparse_extend_packed_kv8(int T, int B, int H, int Hkv, int Hl, int max_q_len, int Sk, int D, int dtype, int block,
                                       int NK, const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                       rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                       int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws,
                                       size_t ws_bytes, rsa_out4 out, float* lse, const float* k_scale, const float* v_scale,
                                       const int32_t* cu_seqlens_q_dev, void* stream);
int rsa_block_select_pooled_packed(int T, int B, int H, int Hkv, int Hl, int max_q_len, int D, int dtype, int block, int NQ, int NK,
                                   rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal,
                                   int top_k, int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes,
                                   uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, int p16, float c, float* mass,
                                   const int32_t* cu_seqlens_q_dev, int32_t* item_ws, void* stream);
int rsa_kv8_append_packed(int B, int Hkv, int T, int Sk, int D, int dtype, int block, rsa_tensor4 k_new, rsa_tensor4 v_new,
                          rsa_out4 k_cache, rsa_out4 v_cache, const int32_t* block_table, int64_t table_stride_b, int num_pages,
                          const int32_t* start_dev, int start, const int32_t* cu_seqlens_dev, int32_t* item_ws,
                          const float* k_scale, const float* v_scale, void* stream);

/* ---- block selection by per-channel key BOUNDS: a min/max cache and the selection from it (found by symbol: the header version
 * stays 6.1).  The pooled selection scores a key block by qs . mean(k); this one by the upper bound of
 * qs . k over every key the block could hold (Quest's criterion), so one aligned key among many others cannot hide:
 *     t[b, hl, i, j] = sum over d of max(qs_d * mn_d, qs_d * mx_d),
 * qs the pooled query of rsa_block_select (the sum over the list head's query heads, ascending, of each head's fp32 row mean), mn /
 * mx the per-channel minimum / maximum of the keys of block j of (b, K/V head) below len_b.  fp32 in a fixed order: per group of
 * four channels the terms -- each the larger of two separately rounded products, no fused form -- are added as ((x + y) + z) + w,
 * the D / 4 partial sums meet over xor strides 1 .. D / 8.  One decode step is rsa_pool_key_bounds (the blocks the step touched) ->
 * rsa_block_select_bound -> rsa_block_sparse_decode: all on the device, no host read, capturable in one graph.
 *
 * rsa_pool_key_bounds / rsa_pool_key_bounds_kv8 take the argument lists of rsa_pool_keys / rsa_pool_keys_kv8 and their contract
 * word for word -- the forms of k, the limits, the written set (exactly the blocks start_b / block <= j < ceil(len_b / block), no
 * other byte), the table rule, workgroups_per_head, the refusals and their order -- with out fp32 [B, Hkv, NK, 2, D] contiguous,
 * 16-byte aligned: out[b, hk, j, 0, :] the minimum and out[b, hk, j, 1, :] the maximum over the keys of block j below len_b.  A
 * table entry outside [0, num_pages) gives zeros, min and max alike.  kv8: min and max over float(code), each multiplied once by
 * k_scale[hk] (positive: the order is kept).  Keys at or beyond len_b are never loaded; keys below it are taken to be finite (a NaN
 * there gives an unspecified value and forms no address).  min and max are exact and order-free: every workgroups_per_head gives
 * the same values, two calls the same bytes.  One pass over K, one launch.
 *
 * rsa_block_select_bound takes the argument list of rsa_block_select_pooled_ragged (p16 = -1: plain top-k, c and mass are then not
 * read; q_len_dev NULL: every item has Sq rows), rsa_block_select_bound_packed that of rsa_block_select_pooled_packed; pooled_k is
 * the bounds cache, fp32 [B, Hkv, NK, 2, D] contiguous, 16-byte aligned.  Everything behind the score -- the visible prefix, the
 * forced blocks, top-k with ties to the lower block, top-p with its weights, target, cap and mass, the lists, the scores (-inf at
 * invisible blocks), the ragged and the packed rows -- is the contract and the device code of the pooled entries.  Only the
 * visible prefix of the cache is read; the rest may hold anything.  score_splits workgroups per list row (0: the library's choice;
 * at most 256) write the row's scores to the workspace at every count, one included; every value gives the same bytes.
 * ws: rsa_block_select_bound_bytes(...) bytes (= rsa_block_select_pooled_bytes), 16-byte aligned.  Three launches (the pooled
 * queries, the scores, the selection); packed: four.  Refusals: the pooled entries', with their statuses, in their order. */
int rsa_pool_key_bounds(int B, int Hkv, int Sk, int D, int dtype, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                        int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid, const int32_t* start_dev,
                        int start, int workgroups_per_head, float* out, void* stream);
int rsa_pool_key_bounds_kv8(int B, int Hkv, int Sk, int D, int block, int NK, rsa_tensor4 k, const int32_t* block_table,
                            int64_t table_stride_b, int num_pages, const int32_t* kv_len_dev, int kv_valid,
                            const int32_t* start_dev, int start, int workgroups_per_head, float* out, const float* k_scale,
                            void* stream);
int rsa_block_select_bound_bytes(int B, int Hkv, int Hl, int D, int NQ, int NK, size_t* bytes);
int rsa_block_select_bound(int B, int H, int Hkv, int Hl, int Sq, int D, int dtype, int block, int NQ, int NK, rsa_tensor4 q,
                           const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal, int top_k, int keep_first,
                           int keep_local, int score_splits, void* ws, size_t ws_bytes, uint32_t* bitmask, int32_t* cols,
                           int32_t* counts, float* scores, int p16, float c, float* mass, const int32_t* q_len_dev, void* stream);
int rsa_block_select_bound_packed(int T, int B, int H, int Hkv, int Hl, int max_q_len, int D, int dtype, int block, int NQ, int NK,
                                  rsa_tensor4 q, const float* pooled_k, const int32_t* kv_len_dev, int kv_valid, int causal,
                                  int top_k, int keep_first, int keep_local, int score_splits, void* ws, size_t ws_bytes,
                                  uint32_t* bitmask, int32_t* cols, int32_t* counts, float* scores, int p16, float c, float* mass,
                                  const int32_t* cu_seqlens_q_dev, int32_t* item_ws, void* stream);

/* ---- the MERGE of attention partials: N results over disjoint key sets -- another rank's share of the cache, a shared prefix
 * beside each item's suffix, a dense branch beside the selected blocks -- become the result over their union (found by symbol:
 * the header version stays 6.1).  Partial i is what the decode and extend entries return: out_i, 2-byte
 * (dtype, one type for all), and lse_i, fp32, the natural-log log-sum-exp of its keys.  A non-NULL sink (DEVICE fp32 [H]) is one
 * more partial whose out is zero and whose lse is sink[h] for every row of head h (attention-sink logits).
 *   shape     1 <= N <= 8.  outs: a HOST array of N rsa_tensor4, each a [B, H, S, D] view; lses: a HOST array of N DEVICE pointers;
 *             lse_strides: a HOST array of 3 N element strides, (b, h, s) of lse_0, then of lse_1, ...  The three arrays are read
 *             during the call and not kept.  The packed form [T, H, D] / [T, H] is B = 1, S = T, stride_s the row's stride,
 *             stride_h the head's.  lse_out NULL or fp32 through its three element strides.
 *   per row   in fp32, the partials in ascending index order and the sink last:
 *                 m*  = max over the live entries of lse_i     (live: lse_i > -inf; the sink is live iff sink[h] > -inf)
 *                 w_i = exp2((lse_i - m*) * log2 e)            one subtraction, one multiplication, the hardware exp2
 *                 acc = fmaf(w_i, out_i[c], acc)               a partial that is not live is SKIPPED, never multiplied
 *                 l   = l + w_i                                the sink's weight enters l and not acc
 *                 out[c] = acc / l (IEEE), one conversion;  lse = m* + ln 2 * log2 l;  no live entry: 0 and -inf
 *             The out of a partial whose lse is -inf may hold NaN: it never reaches the result.  A row with exactly one live
 *             entry returns that partial's out and lse bytes.  Two calls give the same bytes.  A +inf lse is the caller's error and
 *             garbles its own row alone; a NaN lse counts as not live.
 *   strides   D contiguous; every other stride of every out_i and of out a non-negative multiple of 4 elements, the pointers
 *             8-byte aligned (the extend entries' output contract).  Where every pointer is 16-byte aligned and every stride a
 *             multiple of 8 a lane moves 16 bytes, else 8: the same arithmetic per element, the same bytes.  The lse tensors take
 *             any non-negative element strides (pointers 4-byte aligned); a stride of out or lse_out along an axis of more than
 *             one entry is positive.
 *   alias     out may be one out_i exactly (the same pointer and the same strides: an in-place accumulate), lse_out one lse_i
 *             exactly: every element a lane needs is read before it stores.  A result whose address range meets that of a partial,
 *             of the sink or of the other result in any other way is refused.
 * One launch over a bounded grid, no workspace, no host read of device memory: capturable in a HIP graph.
 * N outside [1, 8], a negative size, a NULL outs / lses / lse_strides / out_i / lse_i / out, a pointer or stride outside the above,
 * an overlap that is not an exact alias: RSA_ERR_BAD_ARG; D outside {64, 128}, an unknown dtype, more than 2^31 - 1 rows:
 * RSA_ERR_UNSUPPORTED.  Every check runs before the first HIP call; B, H or S of 0 then returns RSA_OK without a launch. */
int rsa_merge_partials(int N, int B, int H, int S, int D, int dtype, const rsa_tensor4* outs, const float* const* lses,
                       const int64_t* lse_strides, const float* sink, rsa_out4 out, float* lse_out, int64_t lse_out_stride_b,
                       int64_t lse_out_stride_h, int64_t lse_out_stride_s, void* stream);

/* ---- block-sparse attention BACKWARD: dq, dk, dv of the plain / grouped-query forward over a caller's block mask, with a causal
 * limit and per-item key limits (found by symbol: the header version stays 6.1).  q, out, dout
 * [B, H, Sq, D], k, v [B, Hkv, Sk, D], H a multiple of Hkv, query head h reads K/V head h / (H / Hkv) and walks the lists of list
 * head h / (H / Hl), Hl in {1, Hkv, H}.  len_b = kv_len_dev[b] clamped into [0, Sk] (DEVICE int32, B values, read on the device
 * only) or, with kv_len_dev NULL, kv_valid in [0, Sk].
 *   visible   row r of (b, h) sees key j iff its query block keeps key block j / block, j < len_b, and with causal
 *             j <= r + len_b - Sq (bottom-right aligned)
 *   lists     row_cols [B * Hl, NQ, NK] / row_counts [B * Hl, NQ]: rsa_block_mask_to_lists of the mask [B, Hl, NQ, NK];
 *             col_cols [B * Hl, NK, NQ] / col_counts [B * Hl, NK]: the same call on the mask with its last two axes exchanged (the
 *             query blocks that keep a key block, ascending).  NQ = ceil(Sq / block), NK <= ceil(Sk / block): key blocks >= NK are
 *             never visited.  Entries outside their range are skipped; no address is formed from an unchecked index.
 *   numerics  scores as the forward: q * (float)(sm_scale * 1.44269504) rounded to the 2-byte type, log2 domain, fp32.  The row
 *             statistics are recomputed (lse2 = m + log2 l, delta = sum_d dout * out, fp32 [B, H, Sq] each in ws), P = exp2(S -
 *             lse2) and dS = P * (dP - delta) are rounded to the 2-byte type for the products they feed, everything is accumulated
 *             in fp32 and dq = sm_scale * sum, dk = sm_scale * sum, dv = sum are converted once.
 *   keys      at or beyond len_b are never multiplied (k / v may hold NaN there); their dk / dv rows are zeros, as are those of key
 *             blocks no query block keeps.  A query row that sees no key gets a zero dq row.  Every element of dq [B, H, Sq, D] and
 *             dk, dv [B, Hkv, Sk, D] is written exactly once.
 * Three launches (row statistics; dq; dk and dv), no float atomics and no hand-off between workgroups: the same inputs give the same
 * bytes.  ws: DEVICE scratch of at least rsa_block_sparse_bwd_bytes(...) bytes, 16-byte aligned.  Inputs: 16-byte aligned pointers,
 * non-negative strides that are multiples of 8 elements, D contiguous; results: 8-byte aligned, strides multiples of 4 and positive
 * where an axis has more than one entry.  A NULL pointer, a bad stride, Hkv or Hl not dividing H, Hl outside {1, Hkv, H}, NQ / NK
 * not matching Sq / Sk, kv_valid outside [0, Sk]: RSA_ERR_BAD_ARG; block other than 64 / 128, D other than 64 / 128, another dtype,
 * more than 8192 query or key blocks, B or H above 65535: RSA_ERR_UNSUPPORTED; ws_bytes too small: RSA_ERR_WORKSPACE.  Every check
 * runs before the first HIP call; B, H or Sq of 0: RSA_OK without a launch. */
int rsa_block_sparse_bwd_bytes(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int block, int NQ, int NK, size_t* bytes);
int rsa_block_sparse_bwd(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NQ, int NK, int kv_valid,
                         const int32_t* kv_len_dev, int causal, double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                         rsa_tensor4 out, rsa_tensor4 dout, const int32_t* row_cols, const int32_t* row_counts,
                         const int32_t* col_cols, const int32_t* col_counts, void* ws, size_t ws_bytes, rsa_out4 dq, rsa_out4 dk,
                         rsa_out4 dv, void* stream);

/* ---- rectified attention over a caller-supplied block mask (the reference's combine, hunyuan :346-357, flux :334-343,
 * cogvideo :338-347, wan21 :328-338, on a selection the caller made, reused or edited).  Additive: no struct above changes. ----
 *
 * K3 with the caller's mask in place of the sort: per (b, h, visual query block i) row it writes probs (softmax and IPAR of the
 * contract, bit-identical to what K3 writes), then with kept = mask[b, h, i, :NB_total] (nonzero = kept, nothing added: no
 * neighbour, text-block or first-frame union) and M_j = kept_j | unrel_j for j < NBv, M_NBv = kept_NBv (the text column):
 *   R = sum of probs over M (the contract's strided tree),  w_j = M_j ? 0 : probs_j,  bitmask / cols / counts of `kept`.
 * Call it after K2 and before K4.  mask: DEVICE uint8 [B|1, H|1, NBv, NB_total] with BYTE strides b / h / q (0 = broadcast for b
 * and h; the query stride is positive) and a contiguous key axis.  A NULL mask or buffer, a negative stride or a query stride of
 * 0 is RSA_ERR_BAD_ARG; a layout rsa_select_mask refuses gets the code it returns.  A visual row whose kept blocks hold no key below
 * kv_valid comes out of K5 as comp (the reference's kernel gives NaN there).  One workgroup per row. */
int rsa_select_from_mask(const rsa_layout* lay, const uint8_t* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                         int64_t mask_stride_q, const rsa_buffers* buf, void* stream);
int rsa_select_from_mask_ex(const rsa_layout_ex* lay, const uint8_t* mask, int64_t mask_stride_b, int64_t mask_stride_h,
                            int64_t mask_stride_q, const rsa_buffers* buf, void* stream);
/* The whole operator on such a mask: K1, K2, the pass above, K4, K5 on one stream, in the workspace of
 * rsa_rectified_attention (rsa_buffer_bytes / rsa_carve_workspace).  The mask arguments are checked before the first launch. */
int rsa_rectified_attention_masked(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const uint8_t* mask,
                                   int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q, void* workspace,
                                   size_t workspace_bytes, rsa_out4 out, void* stream);
int rsa_rectified_attention_masked_ex(const rsa_layout_ex* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                      const uint8_t* mask, int64_t mask_stride_b, int64_t mask_stride_h, int64_t mask_stride_q,
                                      void* workspace, size_t workspace_bytes, rsa_out4 out, void* stream);

/* Stand-alone GAPR for callers of estimate_pr_gain (gapr_mask.py:4): blocks are [BH, N, 128, D] contiguous
 * 2-byte elements, pools [BH, N, D] fp32, scores [BH, NQ, NK] fp32 -> mask [BH, NQ, NK] uint8 (1 = ~gapr_mask). */
int rsa_estimate_pr_gain(int BH, int NQ, int NK, int D, int dtype, const void* q_blocks, const void* k_blocks,
                         const float* q_pools, const float* k_pools, const float* scores, float* scratch_aq,
                         float* scratch_ak, uint8_t* mask_out, void* stream);
/* ... with blocks of `block` tokens ([BH, N, block, D]): 64 or 128 (since 0.6.1). */
int rsa_estimate_pr_gain_ex(int BH, int NQ, int NK, int D, int dtype, int block, const void* q_blocks, const void* k_blocks,
                            const float* q_pools, const float* k_pools, const float* scores, float* scratch_aq,
                            float* scratch_ak, uint8_t* mask_out, void* stream);

/* ---- host-side geometry: produces the hot path's `neighbor` input and the token permutation ---- */

/* Generalized Hilbert ("Gilbert") curve over a t x h x w cuboid (x spans w, y spans h, z spans t; linear index =
 * z*h*w + y*w + x).  axis_order: 3 chars out of "w","h","t" = major, middle, minor axis (the scripts pass "wht",
 * main_hunyuan.py:245) or NULL for the size-ordered default.  HOST pointers; linear_to_hilbert may be NULL.
 * Replaces gilbert_mapping / gilbert_xyz2d (utils/jenga_gilbert.py:12-288, :458-504). */
int rsa_gilbert_mapping(int t, int h, int w, const char* axis_order, int32_t* linear_to_hilbert,
                        int32_t* hilbert_to_linear);

/* 26-neighbourhood relation between `block_size`-token blocks along the curve: neighbor[i*NB + j] = 1 iff some
 * point of block i touches (Chebyshev distance <= 1) a point of block j; NB = ceil(t*h*w / block_size).  HOST
 * pointer, NB*NB bytes.  Replaces gilbert_block_neighbor_mapping (utils/jenga_gilbert.py:613-693). */
int rsa_gilbert_block_neighbors(int t, int h, int w, int block_size, const char* axis_order, uint8_t* neighbor);

/* ---- producers / consumers either side of the path; DEVICE pointers ---- */

/* Row gather out[b, i, :] = x[b, order[i], :] for i < S; rows are C 2-byte elements (C % 8 == 0), strides in
 * elements.  Replaces hidden_states[:, hilbert_order] and hidden_states[:, linear_to_hilbert]
 * (scripts/main_hunyuan.py:88, :183; main_wan21t2v.py:92-93, :167). */
int rsa_permute_tokens(int B, int S, int C, const void* x, int64_t x_stride_b, int64_t x_stride_s,
                       const int32_t* order, void* out, int64_t o_stride_b, int64_t o_stride_s, void* stream);

/* Fused per-head RMSNorm (if apply_norm; weight fp32 [D] or NULL) + rotary embedding (if cos/sin non-NULL: fp32
 * [S_rope, D] tables in the interleaved-pair convention of diffusers' apply_rotary_emb, applied to tokens < S_rope)
 * over a [B,H,S,D] view, written to a strided [B,H,S,D] destination (e.g. a slice of the [visual | text] concat).
 * Replaces attn.norm_q / attn.norm_k + apply_rotary_emb + torch.cat in the processors
 * (rectified_hunyuan_attn.py:452-498, rectified_flux_attn.py:443-484). */
int rsa_qk_norm_rope(int B, int H, int S, int D, int dtype, rsa_tensor4 x, const float* weight, float eps,
                     int apply_norm, const float* cos, const float* sin, int S_rope, rsa_out4 y, void* stream);

/* Same pass with torch.nn.LayerNorm over the head dim instead of RMSNorm (CogVideoX's qk_norm = "layer_norm",
 * rectified_cogvideo_attn.py:455-466): fp32 mean / biased variance, (x - mean) * rstd * weight + bias, one rounding; weight
 * and bias [D] fp32 copies or null; tokens [0, S_rope) are rotated (the visual tokens come first). */
int rsa_qk_layernorm_rope(int B, int H, int S, int D, int dtype, rsa_tensor4 x, const float* weight, const float* bias,
                          float eps, const float* cos, const float* sin, int S_rope, rsa_out4 y, void* stream);

/* The Wan producers in one pass: RMSNorm ACROSS heads (one variance per token over all H*D channels; weight [H*D] as an
 * fp32 copy, or null; skipped when apply_norm = 0) and the rotary embedding per head, x [B, S, H*D] (row stride
 * x_stride_s elements) -> y strided [B,H,S,D].  rope_kind 0: none; 1: freqs_a = complex128 [S, D/2] (Wan2.1, the rotation
 * runs in fp64 like the reference); 2: freqs_a = cos fp32 [S, D], freqs_b = sin fp32 [S, D] with per-pair values
 * duplicated (Wan2.2).  Replaces attn.norm_q / norm_k + unflatten + apply_rotary_emb in
 * rectified_wan21_attn.py:424-438 and rectified_wan22_attn.py:54-76. */
int rsa_norm_rope_heads(int B, int H, int S, int D, int dtype, const void* x, int64_t x_stride_b, int64_t x_stride_s,
                        const float* weight, float eps, int apply_norm, int rope_kind, const void* freqs_a,
                        const void* freqs_b, rsa_out4 y, void* stream);

/* ---- fp8 operands for K5 (BASELINE config "fp8 Q/K/V on CDNA4 fp8 MFMA"; the reference has no fp8 path, its P/Q
 * rounding rule "operands in the input dtype, fp32 statistics" (rectified_hunyuan_attn.py:61-62, :97) is kept) ---- */

/* e4m3 (OCP e4m3fn) images of one call's Q, K, V in the BLOCK-SCALED format, written by rsa_pool_stats_fp8 /
 * rsa_quantize_fp8 and read by rsa_block_sparse_fwd_fp8.  Per tensor and 128-row block: y = q * sm_scale*log2(e) | k - mu
 * | v in fp32, A = max |y| over the block's valid rows, scale 2^e with the smallest e such that A * 2^-e <= 448, bytes =
 * e4m3(y * 2^-e) rounded to nearest even.  mu ("smooth K", exact under softmax) = the mean of up to 8 evenly spaced full
 * 128-row blocks of K, so nothing needs a pass of its own over a tensor.  The kernel applies the scales through the fp8
 * MFMA's E8M0 block-scale operands. */
typedef struct rsa_fp8_operands {
    uint8_t* q8;      /* [BH, NB_total*128, D]     rows >= S are zero                                                       */
    uint8_t* k8;      /* [BH, NB_total*128, D]     rows >= pool_valid are zero (needs pool_valid >= kv_valid, kv_text_valid) */
    uint8_t* v8t;     /* [BH, NB_total*2, D, 64]   V^T per 64-key tile, keys in the MFMA k-slot order (rsa_fp8_emit.h)       */
    uint32_t* scales; /* [BH, NB_total] words: byte 0 / 1 / 2 = E8M0 exponent (127 + e) of the Q / K / V block, byte 3 unused;
                       * followed by the K mean mu, [BH, D] fp32                                                            */
} rsa_fp8_operands;

/* Bytes of the four members (member order) and their 256-B-rounded sum.  D = 128 or 64. */
int rsa_fp8_operand_bytes(const rsa_layout* lay, size_t sizes[4], size_t* total);
int rsa_carve_fp8_operands(const rsa_layout* lay, void* ws, size_t ws_bytes, rsa_fp8_operands* out);

/* Stand-alone producer: mu (one small launch over 8 blocks of K), then ONE pass over Q, K, V that writes the three images
 * and the block exponents. */
int rsa_quantize_fp8(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                     const rsa_fp8_operands* ops, void* stream);

/* The same fused into the mask-selection pass: K1 (rsa_pool_stats) writes the images of every block it pools in the pass
 * that pools it (Q and K visual blocks, every V block: the tensors are read from HBM once), a small launch covers the
 * text-tail blocks of Q and K.  buf gets K1's statistics as rsa_pool_stats would write them; ops is bit-identical to
 * rsa_quantize_fp8's.  With ops->q8 == ops->k8 == NULL only the V image and the V bytes of the exponent words are written (the
 * operands of rsa_block_sparse_fwd_fp8pv; since 0.5.0). */
int rsa_pool_stats_fp8(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const rsa_buffers* buf,
                       const rsa_fp8_operands* ops, void* stream);

/* K5 on v_mfma_f32_32x32x64_f8f6f4: same lists, R, comp, text rows and output layout as rsa_block_sparse_fwd;
 * lay->dtype selects the OUTPUT element type. */
int rsa_block_sparse_fwd_fp8(const rsa_layout* lay, const rsa_fp8_operands* ops, const rsa_buffers* buf,
                             rsa_out4 out, void* stream);

/* The "pv" form (since 0.5.0): Q . K^T on the 2-byte q and k themselves (v_mfma_f32_32x32x16), e4m3 only for P and V
 * (ops->v8t and the V bytes of ops->scales; q8 / k8 are not read).  The scores are then the 2-byte path's -- the e4m3 rounding of
 * Q and K is nine tenths of rsa_block_sparse_fwd_fp8's error -- while P . V still runs at the fp8 rate: 800 matrix cycles per 64
 * keys and 32 rows against 1 024 (2-byte) and 544 (e4m3) at head dim 128.  Head dims 64 and 128. */
int rsa_block_sparse_fwd_fp8pv(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, const rsa_fp8_operands* ops,
                               const rsa_buffers* buf, rsa_out4 out, void* stream);

/* The whole operator with fp8 K5: K1..K4 on the 2-byte inputs (the mask is the bf16 path's, bit for bit; K1 in its
 * rsa_pool_stats_fp8 form, which leaves the images behind), then rsa_block_sparse_fwd_fp8. */
int rsa_rectified_attention_fp8(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                const uint8_t* neighbor, int top_k, float p_remain, void* workspace,
                                size_t workspace_bytes, void* fp8_workspace, size_t fp8_workspace_bytes,
                                rsa_out4 out, void* stream);
/* ... in the pv form (head dims 64, 128): K1 writes only the V image and its exponents, K5 = rsa_block_sparse_fwd_fp8pv.  Same workspaces
 * (the Q / K images' share of fp8_workspace stays untouched). */
int rsa_rectified_attention_fp8pv(const rsa_layout* lay, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                  const uint8_t* neighbor, int top_k, float p_remain, void* workspace,
                                  size_t workspace_bytes, void* fp8_workspace, size_t fp8_workspace_bytes,
                                  rsa_out4 out, void* stream);

/* TeaCache's step-skipping statistic (scripts/main_hunyuan.py:120, main_wan21t2v.py:112): out2[0] =
 * sum |a - b|, out2[1] = sum |b| over two equal-length 2-byte tensors (n elements, 16-B aligned) in one HBM pass
 * instead of the reference's five elementwise/reduction launches; scratch: >= 2048 floats.  DEVICE pointers. */
int rsa_rel_l1(const void* a, const void* b, int64_t n, int dtype, float* out2, float* scratch, void* stream);

/* rsa_dense_fwd with e4m3 operands (block-scaled images produced inside): quantisation pass + the fp8 kernel in dense
 * mode.  workspace: >= *total of rsa_dense_fp8_bytes, 256-B aligned.  D = 128 or 64. */
int rsa_dense_fp8_bytes(int B, int H, int Sq, int Sk, int D, size_t* total);
int rsa_dense_fwd_fp8(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                      int q_split, int kv_split, void* workspace, size_t workspace_bytes, rsa_out4 out, void* stream);
/* ... with causal = True inside each segment (rsa_dense_causal_fwd's meaning: bottom-right aligned, attn.py:108-116). */
int rsa_dense_causal_fwd_fp8(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                             int q_split, int kv_split, void* workspace, size_t workspace_bytes, rsa_out4 out,
                             void* stream);
/* The "pv" form of the dense fp8 kernel (round 5; head dims 64, 128): Q . K^T on the 2-byte q and k as they are, e4m3 only for P and the
 * V image (rsa_block_sparse_fwd_fp8pv's kernel in its dense mode).  causal != 0: as rsa_dense_causal_fwd.  Same workspace. */
int rsa_dense_fwd_fp8pv(int B, int H, int Sq, int Sk, int D, int dtype, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                        int q_split, int kv_split, int causal, void* workspace, size_t workspace_bytes, rsa_out4 out, void* stream);

/* ---- multi-GPU: the exchange step at the layer boundary.  The path itself shards by (batch, head) with
 * NO collective (reference: no cross-head dependency anywhere, rectified_hunyuan_attn.py:211-277, gapr_mask.py:15-42);
 * only a consumer that is not head-sharded (the to_out GEMM of an unsharded model) needs every rank's O.  The
 * reference's only multi-GPU code is prompt-level replication (eval/video/experiments/multigpu_hunyuan.py:290-299). ---- */

/* RCCL communicator over the ranks of one node (librccl is bound at run time).  rsa_comm_unique_id: rank 0 fills
 * id128 (HOST, 128 bytes) and distributes it by any host channel; every rank then calls rsa_comm_create. */
int rsa_comm_unique_id(void* id128);
int rsa_comm_create(int world, int rank, const void* id128, void** comm);
int rsa_comm_destroy(void* comm);
/* The rank count the communicator itself reports (ncclCommCount): lets a launcher record that the collective really spans the
 * ranks it believes it does (since 0.5.0). */
int rsa_comm_count(void* comm, int* ranks);

/* All-gather of O along the head axis: local [rows][local_row_bytes] on every rank -> full [rows][world*local_row_bytes]
 * on every rank (rank r's bytes at column offset r*local_row_bytes) = ncclAllGather into `staging`
 * ([world][rows][local_row_bytes]) + one unpack kernel.  DEVICE pointers, 16-byte aligned, local_row_bytes % 16 == 0. */
int rsa_allgather_heads(void* comm, int world, const void* local, void* staging, void* full, int64_t rows,
                        int64_t local_row_bytes, void* stream);

/* The same exchange written straight into the peers: ONE copy kernel whose workgroups are dealt over the peers (all xGMI
 * links carry their slab at once; 16-byte stores into column range [rank*local_row_bytes, +local_row_bytes) of every
 * rank's full buffer), arrival signalled through IPC-shared device flags and awaited by a one-workgroup kernel on the same
 * stream: stream-ordered end to end, no host barrier, no host synchronisation.
 *   full_of_rank / state_of_rank: HOST arrays of `world` device pointers (own buffers at index rank; the others opened with
 *   rsa_ipc_open + rsa_ipc_offset).  state = the block rsa_p2p_state_alloc() returns (FINE-GRAINED device memory, zeroed: peers
 *   write its flags over xGMI while this GPU polls them, which the memory model only defines for fine-grained allocations;
 *   rsa_p2p_state_bytes() of it are used); its word 1 turns nonzero (missing rank + 1) if a wait gave up after 4 s.
 * Every rank must call this the same number of times.  A rank may overwrite a peer's full buffer as soon as that peer has
 * issued its NEXT exchange, so alternate between two full buffers and consume each on the stream that issued the exchange. */
int rsa_p2p_state_bytes(void);
int rsa_p2p_state_alloc(void** state);   /* fine-grained, zeroed, IPC-exportable; one per rank and exchange object */
int rsa_p2p_state_free(void* state);
int rsa_p2p_state_timeout(const void* state, int* missing_rank_plus_1);   /* synchronous read of the time-out word */
int rsa_allgather_heads_p2p(int world, int rank, const void* local, void* const* full_of_rank, void* const* state_of_rank,
                            int64_t rows, int64_t local_row_bytes, void* stream);
int rsa_ipc_export(const void* dev_ptr, void* handle64);                    /* 64-byte handle of a device allocation */
int rsa_ipc_open(const void* handle64, int peer_device, void** dev_ptr);    /* map a peer's allocation here */
int rsa_ipc_close(void* dev_ptr);
int rsa_ipc_offset(const void* dev_ptr, int64_t* offset);                   /* dev_ptr - base of its allocation (a handle names the allocation) */

/* Tuning / diagnostics hook, not part of the data path.  Keys: "k5_gsync" (aligned starts of the sparse walks: bit 0 the
 * 64-rows-per-wave K5 of 128-token blocks -- default --, bit 1 the other K5 kernels, 0 off; a scheduling aid, outputs are byte-identical), "k5_text_last", "k5_tail_split" (0: the
 * walks of the last partial generation stay whole -- byte-identical results whatever the grid), "k5_tsplit" (0/1: split-KV of the text query blocks),
 * "k3_prefix" (0/1: sorted-head path of K3), "fp8_variant" (0: the product = hand-placed block, P through the e4m3 code map; 1: the same arithmetic as hipcc schedules it;
 * 2: P by v_exp_f32 + round-to-nearest e4m3 -- the two forms the tests compare the product with), "fp8_smooth_k"
 * (0: the fp8 producers take mu = 0 instead of the sampled K mean, for the same comparison).  The hook
 * is inert (RSA_ERR_UNSUPPORTED) unless the process was started with the environment variable RSA_TUNING=1. */
int rsa_set_tuning(const char* key, int value);

const char* rsa_status_string(int status);
/* hipGetErrorString of the HIP error behind the most recent RSA_ERR_LAUNCH (diagnostics only). */
const char* rsa_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RSA_H_ */
