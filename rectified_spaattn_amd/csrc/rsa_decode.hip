// Block-sparse decode attention: a few query rows over a (paged) K/V cache (include/rsa.h: rsa_block_sparse_decode_bytes,
// rsa_block_sparse_decode).  Two kernels, plain HIP C++ for wave64:
//
//   decode_split_kernel   one 4-wave workgroup per (unit, split).  A unit = the query heads that share a K/V head AND a list row:
//                         its rows (head-major: row = head_in_unit * Sq + query row, at most 64) are the columns of 16x16x32 MFMA
//                         tiles.  Split s walks entries [s C, (s + 1) C) of the unit's kept list in chunks of 32 keys; chunk c of
//                         the slice goes to wave c & 3, so the four waves share the keys of every kept block.  Per chunk and wave:
//                             S^T[key][row]  = K . Q^T        A = K straight from global memory (16 B per lane), B = the scaled Q
//                             P^T            = exp2(S^T - m)  the accumulator IS the next B operand (its k order: key_of below)
//                             O^T[d][row]   += V^T . P^T      A = V^T by ds_read_b64_tr_b16 from the wave's own [32][D] LDS image
//                         A lane owns ONE query row (lane & 15) of each row tile, so the running maximum, the row sum and the
//                         rescale of O^T are lane-local; only the chunk maximum crosses lanes (two xor steps).  K and V of the next
//                         chunk are loaded into a second register set while this one is computed.  The waves' (m, l, O) meet
//                         through LDS in ascending wave order at the end and wave 0 stores the split's partial.
//   decode_merge_kernel   per row: m* = max m_s, O = sum 2^(m_s - m*) O_s / sum 2^(m_s - m*) l_s over the splits in ascending
//                         order, one division, one conversion; optionally the log-sum-exp (m* + log2 l) ln 2.  The grid's split
//                         extent comes from NK (the host never reads a list's count); the workgroups past a list's end leave at
//                         once and the merge stops at ceil(count / C).
//
// Numeric contract of the 2-byte K5 kernels: Q * (float)(sm_scale * 1.44269504) rounded to the input type (rsa_q_frag), scores
// in the log2 domain, P rounded to the input type for P.V, fp32 accumulation.  Keys at or beyond the limit are never multiplied:
// their scores are replaced by selection, their V rows are zeroed on the way into LDS, and blocks without a key below the limit
// (or with a list / table entry out of range) are not read at all.  No atomics: the same inputs give the same bytes.
//
// The cache's element.  The e4m3 cache (the _kv8 entries) is the same two kernels instantiated over Tag =
// kv8_tag<query type>.  K and V are then one-byte codes with one fp32 scale per K/V head: a lane loads 8 bytes of K where it loads
// 16 (same keys, same d range) and half as many 16-byte pieces of V, and the codes become the query's 2-byte type in registers (the
// packed scaled conversions with a unit scale: exact, every finite e4m3 value is a bf16 and an fp16).  The K scale multiplies the
// fp32 score behind the MFMA chain, the V scale the merged row once; the V image, the MFMAs, the softmax and the meet are the code
// below.
//
// The row form: the one further template parameter of both kernels, which says whose rows a workgroup serves.
//   DecodeForm         rsa_block_sparse_decode: a whole unit, at most 64 rows of one query block.  Arguments: DecArgs / DecMergeArgs.
//   ExtendForm<Rows>   the extend entries (section 5.16): any number of query rows, query blocks and heads of a unit.  A workgroup
//                      serves a ROW GROUP (DecGroups: at most 64 rows of one batch item, unit and query block): the list row is the
//                      query block's, a row's causal limit comes from its index in its item, a chunk that starts at or beyond the
//                      limit of the group's last row is skipped before its loads (byte-neutral), and partials and the merge are
//                      indexed by (row group, split).  Arguments: decode's, the row groups and the row source behind them.  Rows
//                      (rsa_rows.h) says where an item's rows are and how many:
//     RowsPadded       rsa_block_sparse_extend: q [B, H, Sq, D], every item Sq rows.  Adds no argument.
//     RowsCounted      the _ragged entries (section 5.17): n_b = q_len[b] clamped into [0, Sq] stands where Sq is a row count -- the
//                      rows of the group (qn), the group's and each row's causal limit, the merge's row test -- and nowhere else:
//                      the grid, the groups and the partials are the padded call's.  A group whose first row is at or beyond n_b
//                      leaves before it reads a list entry, a table entry or a K/V byte; the merge writes its rows (0, -inf) unread.
//     RowsPacked       the _packed entries (section 5.18): q, out are [T, H, D], item b is rows [s_b, s_b + n_b) of them, Sq holds M.
//                      A one-workgroup scan (rsa_rows.h) sanitises cu_seqlens_q into row_start and piece_start, the exclusive
//                      prefix sums of the items' row groups, at the head of the workspace.  Split workgroup (piece p, unit, hc)
//                      finds its item by a bounded binary search over piece_start -- the live groups are the launch's first
//                      workgroups by construction, and p >= piece_start[B] leaves before it reads a list entry, a table entry or a
//                      K/V byte -- and stands where the counted group stands from there on, s_b added to the row of q.  Partials
//                      are indexed by (compact group, split); the merge runs one thread group per row t of [0, T), finds the item
//                      over row_start and writes rows outside every item (0, -inf) before it looks at a list row or a partial.
// A combination that does not exist (row counts without row groups, counts beside cu_seqlens_q) has no type.  The statements that
// find a workgroup's rows stand in the kernels under `if constexpr` on the form, in the order that keeps every kernel's instruction
// stream what it was (profiles/rows_refactor_isa.md).
#include "rsa_attn.h"
#include "rsa_rows.h"

#include <math.h>

#define DEC_NT 256
#define DEC_MAX_NK 8192
#define DEC_MAX_ROWS 64
#define DEC_CHUNK 32            // keys per wave step
#define DEC_SPLIT 8             // default list entries per split: within a fifth of the best split size at every measured shape
                                // (profiles/decode_perf.txt), and the partials it costs stay below a tenth of the K/V it reads

// The extend kernels' row groups.  The gu x rows_i rectangle of (unit, query block i) is cut into groups of
// gh heads x qg query rows (gh * qg <= 64; row = head_in_group * qg + query row in group): HC head chunks, cpb query chunks per
// full query block, QC query chunks per unit over all NQ query blocks (only the last block is ragged, so chunk qc belongs to
// block qc / cpb).  Group index = ((b * U + unit) * QC + qc) * HC + hc.  Decode is the case NQ = QC = HC = 1, gh = gu, qg = Sq.
struct DecGroups {
    int NQ, QC, cpb, HC, gh, qg;
};

struct DecArgs {
    const unsigned short *q, *k, *v;
    long qsb, qsh, qss, ksb, ksh, kss, vsb, vsh, vss;
    const int32_t* table;       // [B, >= NK] page of every key block, or null: contiguous cache
    long tsb;
    int num_pages;
    const int32_t *cols, *counts;
    const int32_t* kv_len;      // device limits (clamped here) or null: kv_valid
    int kv_valid;
    int H, Hkv, Hl, U, Sq, Sk, NK, blk, causal;
    int C, nsplit, R16;         // list entries per split, splits, rows of a partial (16 x row tiles)
    float qk_scale;
    float* ws_o;                // [B * U * nsplit, R16, D] unnormalised O
    float2* ws_ml;              // [B * U * nsplit, R16] (m in the log2 domain, l)
};

struct DecArgs8 : DecArgs {
    const float *k_scale, *v_scale;     // [Hkv]: the value of a code is float(code) * scale[hk]
};

// The extend kernels' arguments: the decode kernels' (whose layout stays as it is) and the row groups behind them.
template <typename A>
struct DecExt : A {
    DecGroups g;
    int qblk;                   // rows of a query block (the merge's base struct holds no block size)
};

// The row form a kernel is instantiated over.  Args<A>: its arguments where decode takes A -- A itself, or A, the row groups and
// the row source behind them (a padded source adds nothing; Sq holds M, the rows of an item at most, in the packed call).
struct DecodeForm {
    static constexpr bool EXT = false, BATCHED = true, SHORT = false;
    template <typename A> using Args = A;
};
template <typename R>
struct ExtendForm {
    static constexpr bool EXT = true, BATCHED = R::BATCHED, SHORT = R::SHORT;
    using Rows = R;
    template <typename A> using Args = WithRows<DecExt<A>, R>;
    R rows;                     // (host: the source the launch hands to both kernels)
};

// The cache's element: the query's own 2-byte type (Tag = bf16_tag / fp16_tag), or e4m3 codes (kv8_tag<query type>).
template <typename QTag>
struct kv8_tag {};
template <typename Tag>
struct DecCache {
    using Q = Tag;
    using elem = unsigned short;
    using Args = DecArgs;
    using MergeArgs = struct DecMergeArgs;
    using kfrag = uint4;                // 8 elements of a key: one A fragment
    static constexpr bool kv8 = false;
    static constexpr int VPIECE = 8;    // elements of a 16-byte piece of V
};
template <typename QTag>
struct DecCache<kv8_tag<QTag>> {
    using Q = QTag;
    using elem = unsigned char;
    using Args = DecArgs8;
    using MergeArgs = struct DecMergeArgs8;
    using kfrag = uint2;
    static constexpr bool kv8 = true;
    static constexpr int VPIECE = 16;
};

// Four e4m3 codes -> four elements of the query's type (element i from byte i): gfx950's packed scaled conversions with a unit
// scale, v_cvt_scalef32_pk_bf16_fp8 / v_cvt_scalef32_pk_f16_fp8, one per half of the dword: two instructions per dword.  Exact
// (every finite code is a bf16 and an fp16: nothing is rounded).
template <typename QTag>
__device__ __forceinline__ uint2 dec_cvt4(unsigned w) {
    if constexpr (std::is_same<QTag, bf16_tag>::value) {
        return make_uint2(__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false)),
                          __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true)));
    } else {
        return make_uint2(__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false)),
                          __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true)));
    }
}
template <typename QTag>
__device__ __forceinline__ uint4 dec_cvt8(uint2 w) {
    const uint2 a = dec_cvt4<QTag>(w.x), b = dec_cvt4<QTag>(w.y);
    return make_uint4(a.x, a.y, b.x, b.y);
}

template <typename Tag>
struct Mfma16;
template <>
struct Mfma16<bf16_tag> {
    static __device__ __forceinline__ f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <>
struct Mfma16<fp16_tag> {
    static __device__ __forceinline__ f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

// A chunk's operands as they come from global memory: K as the A fragments of S^T (key = 16 t + (lane & 15), d = 32 ks +
// 8 (lane >> 4) ..), V as 16-byte pieces of its [32][D] row image.  key0 < 0: nothing to do (the block is not visited).
template <int D, typename Cache>
struct DecRaw {
    typename Cache::kfrag kf[2][D / 32];
    uint4 vf[32 * D / Cache::VPIECE / 64];
    const typename Cache::elem* vb;     // the V rows of the chunk's batch item or page, and the offset of its row numbers
    long roff;
    int key0;
};

__device__ __forceinline__ s16x4 dec_tr_read(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}

template <typename CTag, int D, int MT, typename Form>
__global__ __launch_bounds__(DEC_NT, MT == 1 ? 2 : 1) void decode_split_kernel(
    const typename Form::template Args<typename DecCache<CTag>::Args> a) {
    constexpr bool EXT = Form::EXT, PACKED = !Form::BATCHED, COUNTED = Form::SHORT && !PACKED;
    using Cache = DecCache<CTag>;
    using Tag = typename Cache::Q;      // the type of q, of the MFMA operands and of the output
    using KT = typename Cache::elem;
    using Raw = DecRaw<D, Cache>;
    constexpr bool KV8 = Cache::kv8;
    constexpr int VP = Cache::VPIECE;   // elements of a 16-byte piece of V
    constexpr int KS = D / 32, DT = D / 16, CH = D / VP, VL = 32 * CH / 64;
    // At head dim 128 with four row tiles Q (64 registers) and O^T (128) do not fit beside two sets of K and V: the scaled Q
    // fragments then live in LDS (one image for the four waves) and are read again in every chunk.
    constexpr bool QLDS = D == 128 && MT == 4;
    constexpr int QROW = 2 * D + 16;        // bytes per row of that image
    constexpr int VROW = 2 * D + 32;        // bytes per key row of the V image: rows 0 .. 7 start 8 banks apart (transposed reads
                                            // of a 32-lane half touch 8 rows x 32 B: conflict-free)
    // one array: the waves' V images (behind the last barrier of the walk: the O^T tiles of waves 1 .. 3), the Q image, (m, l)
    constexpr int VIMG = 4 * DEC_CHUNK * VROW, QIMG = QLDS ? 16 * MT * QROW : 0;
    static_assert(3 * 16 * D * 4 <= VIMG, "the O^T tiles of three waves fit the V images");
    __shared__ __attribute__((aligned(16))) unsigned char lds[VIMG + QIMG + 4 * 16 * MT * 8];
    unsigned char* const vimg = lds;
    unsigned char* const qimg = lds + VIMG;
    float (*const red)[16 * D] = reinterpret_cast<float (*)[16 * D]>(lds);
    float2 (*const ml)[16 * MT] = reinterpret_cast<float2 (*)[16 * MT]>(lds + VIMG + QIMG);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lh = lane >> 4;
    // the workgroup's rows: heads [h0, h0 + hn) of the unit x query rows [q0, q0 + qn) of the call, row = head * qw + query row
    // in the group; list row (b * Hl + hl) * NQ + qb.  Decode: the whole unit (the arithmetic below, spelled as it always was).
    int ext_unit = 0, ext_b = 0, qb = 0, h0 = 0, hn = 0, q0 = 0, qn = 0, qw = 1, nq = 1, nrow = a.Sq;
    int pk_row0 = 0;                        // packed: the item's first row of q
    long gid = blockIdx.x;                  // the row group: what the partials and the merge are indexed by
    if constexpr (EXT) {
        int g = blockIdx.x;
        const int hc = g % a.g.HC;
        g /= a.g.HC;
        int qc;
        if constexpr (PACKED) {
            // packed: blockIdx.x = (piece * U + unit) * HC + hc over the QP pieces the host's bound allows.  The live pieces are
            // [0, piece_start[B]): the rest leave here.  Everything below is uniform: scalar loads, scalar registers.
            ext_unit = g % a.U;
            const int piece = g / a.U;
            if (piece >= a.src.piece_start[a.src.B]) return;
            ext_b = pk_find(a.src.piece_start, a.src.B, a.src.steps, piece);
            qc = piece - a.src.piece_start[ext_b];
            pk_row0 = (int)a.src.first(ext_b);
            nrow = min(a.src.row_start[ext_b + 1] - pk_row0, a.Sq);
        } else if constexpr (COUNTED) {
            // ragged: the workgroups are dealt query chunk by query chunk, (qc, b, unit, hc).  An item's live groups are its first
            // chunks, so the live groups of a batch of short items are the launch's first workgroups, side by side on the chip; in
            // the groups' own order they sit QC * HC apart and pile up on the few compute units that stride reaches.
            ext_unit = g % a.U;
            g /= a.U;
            const int nb = gridDim.x / (a.U * a.g.QC * a.g.HC);
            ext_b = g % nb;
            qc = g / nb;
            gid = (((long)ext_b * a.U + ext_unit) * a.g.QC + qc) * a.g.HC + hc;
        } else {
            qc = g % a.g.QC;
            g /= a.g.QC;
            ext_unit = g % a.U;
            ext_b = g / a.U;
        }
        qb = qc / a.g.cpb;
        qw = a.g.qg;
        nq = a.g.NQ;
        q0 = qb * a.blk + (qc - qb * a.g.cpb) * qw;
        if constexpr (COUNTED) nrow = a.src.count(ext_b, a.Sq);     // the batch item's rows: the causal offset counts from them
        qn = min(qw, min((qb + 1) * a.blk, nrow) - q0);
        if ((COUNTED || PACKED) && qn <= 0) return;     // (uniform) a group of padding rows: the merge writes them without a partial
        h0 = hc * a.g.gh;
        hn = min(a.g.gh, a.H / a.U - h0);
    }
    const int unit = EXT ? ext_unit : blockIdx.x % a.U, b = EXT ? ext_b : blockIdx.x / a.U, split = blockIdx.y;
    const int gu = a.H / a.U, R = a.Sq * gu;
    const int hk = unit / (a.U / a.Hkv), hl = unit / (a.U / a.Hl);
    const int kvlen = a.kv_len ? min(max(a.kv_len[b], 0), a.Sk) : a.kv_valid;
    // no row of the group sees a key at or beyond glim (causal: the limit of the group's last query row): chunks from there on
    // are skipped before their loads.  Decode's last row is the call's last: its glim is kvlen.
    const int glim = EXT && a.causal ? min(kvlen, max(0, q0 + qn + kvlen - nrow)) : kvlen;
    const long lrow = EXT ? ((long)b * a.Hl + hl) * nq + qb : (long)b * a.Hl + hl;
    const long part = ((EXT ? gid : (long)blockIdx.x) * a.nsplit + split) * a.R16;
    const int count = min(max(a.counts[lrow], 0), a.NK);
    const int first = split * a.C;
    const int n_items = max(0, min(a.C, count - first));
    if (n_items == 0) return;               // (uniform) past the list's end: the merge stops at the list's count
    if (glim == 0) {                        // (uniform) no key at all: m = -inf, l = 0; the merge never reads its O
        if (tid < 16 * MT) a.ws_ml[part + tid] = make_float2(-INFINITY, 0.f);
        return;
    }
    const int32_t* list = a.cols + lrow * a.NK + first;
    const int cshift = a.blk == 128 ? 2 : 1;        // chunks per block: 4 or 2

    // the unit's rows: scaled Q fragments (B operand of S^T: column = row tile's row lane & 15) and each row's key limit
    s16x8 qf[QLDS ? 1 : MT][QLDS ? 1 : KS];
    int lim[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int rr = 16 * mt + lr;
        bool ok = rr < R;
        int hu = ok ? rr / a.Sq : 0, qrow = ok ? rr - hu * a.Sq : 0;      // (qrow: the row's index in the whole call)
        if constexpr (EXT) {
            const int hr = rr / qw, qr = rr - hr * qw;
            ok = hr < hn && qr < qn;
            hu = ok ? h0 + hr : 0;
            qrow = ok ? q0 + qr : 0;
        }
        const unsigned short* qp = a.q + (long)b * a.qsb + (long)(unit * gu + hu) * a.qsh + (long)qrow * a.qss + 8 * lh;
        if constexpr (PACKED) qp = a.q + (long)(unit * gu + hu) * a.qsh + (long)(pk_row0 + qrow) * a.qss + 8 * lh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const s16x8 f = rsa_q_frag<Tag>(qp + 32 * ks, ok, a.qk_scale);
            if constexpr (QLDS) {
                if (wave == 0) *reinterpret_cast<s16x8*>(qimg + rr * QROW + 64 * ks + 16 * lh) = f;
            } else {
                qf[mt][ks] = f;
            }
        }
        lim[mt] = !ok ? 0 : (a.causal ? min(kvlen, max(0, qrow + kvlen - nrow + 1)) : kvlen);
    }

    f32x4 o[DT][MT];
    float m[MT], l[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        m[mt] = -INFINITY;
        l[mt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    unsigned char* vst = vimg + wave * (DEC_CHUNK * VROW);
    if constexpr (QLDS) __syncthreads();
    const KT* kbase = reinterpret_cast<const KT*>(a.k) + (long)hk * a.ksh;
    const KT* vbase = reinterpret_cast<const KT*>(a.v) + (long)hk * a.vsh;
    float kscale = 1.f;
    if constexpr (KV8) kscale = a.k_scale[hk];

    for (int e0 = 0; e0 < n_items; e0 += 64) {
        // this lane's list entry: the key block and where it lives, or -1 (out of range, no key below the limit, no page).  No
        // address is formed from an unchecked index.
        int jv = -1, pv = -1;
        if (e0 + lane < n_items) {
            const int j = list[e0 + lane];
            if (j >= 0 && j < a.NK && (long)j * a.blk < glim) {
                jv = j;
                pv = j;
                if (a.table) {
                    pv = a.table[(long)b * a.tsb + j];
                    if (pv < 0 || pv >= a.num_pages) jv = -1;
                }
            }
        }
        const int nch = min(64, n_items - e0) << cshift;

        auto load_v = [&](uint4 (&vf)[VL], const Raw& r) {
#pragma unroll
            for (int i = 0; i < VL; ++i) {
                const int idx = i * 64 + lane, vr = idx / CH, ch = idx % CH;
                const long row = min(r.key0 + vr, kvlen - 1) + r.roff;
                vf[i] = *reinterpret_cast<const uint4*>(r.vb + row * a.vss + VP * ch);
            }
        };
        auto load = [&](Raw& r, int c) {
            const int entry = c >> cshift, sub = c & ((1 << cshift) - 1);
            const int j = __shfl(jv, entry, 64), pg = __shfl(pv, entry, 64);
            const int key0 = j * a.blk + sub * DEC_CHUNK;
            r.key0 = -1;
            if (j < 0 || key0 >= glim) return;          // (uniform)
            r.key0 = key0;
            // rows at or beyond the limit are read as the last row below it: in bounds, masked (K) or zeroed (V) later
            const long roff = a.table ? -(long)j * a.blk : 0;     // paged: rows count from the page's first
            const KT* kb = kbase + (a.table ? (long)pg * a.ksb : (long)b * a.ksb);
            r.vb = vbase + (a.table ? (long)pg * a.vsb : (long)b * a.vsb);
            r.roff = roff;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long row = min(key0 + 16 * t + lr, kvlen - 1) + roff;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    r.kf[t][ks] = *reinterpret_cast<const typename Cache::kfrag*>(kb + row * a.kss + 32 * ks + 8 * lh);
            }
            load_v(r.vf, r);
        };

        auto qfrag = [&](int mt, int ks, int qoff) {
            if constexpr (QLDS) return *reinterpret_cast<const s16x8*>(qimg + qoff + 16 * mt * QROW + 64 * ks);
            else return qf[mt][ks];
        };
        auto kfrag = [&](const Raw& r, int t, int ks) {
            if constexpr (KV8) return __builtin_bit_cast(s16x8, dec_cvt8<Tag>(r.kf[t][ks]));
            else return __builtin_bit_cast(s16x8, r.kf[t][ks]);
        };
        auto compute = [&](const Raw& r) {
            if (r.key0 < 0) return;                     // (uniform: the transposed reads below need every lane)
            const int key0 = r.key0;
            int qoff = lr * QROW + 16 * lh;
            if constexpr (QLDS) asm volatile("" : "+v"(qoff));      // (read in every chunk, not hoisted back into registers)
            // S^T = K . Q^T: lane (lr, lh) gets keys key0 + 16 t + 4 lh + i of query row lr of each row tile
            s16x8 pf[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                float x[8];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
                        s = Mfma16<Tag>::mfma(kfrag(r, t, ks), qfrag(mt, ks, qoff), s);
                    if constexpr (KV8) s *= kscale;         // the K scale: one fp32 multiply of the finished score
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[4 * t + i] = key0 + 16 * t + 4 * lh + i < lim[mt] ? s[i] : -INFINITY;
                }
                float mx = x[0];
#pragma unroll
                for (int e = 1; e < 8; ++e) mx = fmaxf(mx, x[e]);
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mn = fmaxf(m[mt], mx);
                const float mref = mn == -INFINITY ? 0.f : mn;
                const float alpha = __builtin_amdgcn_exp2f(m[mt] - mref);
                float ps = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    x[e] = __builtin_amdgcn_exp2f(x[e] - mref);
                    ps += x[e];
                }
                l[mt] = l[mt] * alpha + ps;     // the lane's share of the row sum: the four lanes of a row meet at the end
                m[mt] = mn;
                // element e of the fragment is key_of(lh, e) = 16 (e >> 2) + 4 lh + (e & 3): the V^T fragments below follow it
                pf[mt] = Elem<Tag>::cvt8(x);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt][mt] *= alpha;
            }
            // V image: a key at or beyond the limit becomes a zero row (0 * NaN inside an MFMA would be NaN)
#pragma unroll
            for (int i = 0; i < VL; ++i) {
                const int idx = i * 64 + lane, vr = idx / CH, ch = idx % CH;
                const uint4 x = key0 + vr < kvlen ? r.vf[i] : make_uint4(0, 0, 0, 0);
                if constexpr (KV8) {        // (the zero code is the zero element)
                    *reinterpret_cast<uint4*>(vst + vr * VROW + 32 * ch) = dec_cvt8<Tag>(make_uint2(x.x, x.y));
                    *reinterpret_cast<uint4*>(vst + vr * VROW + 32 * ch + 16) = dec_cvt8<Tag>(make_uint2(x.z, x.w));
                } else {
                    *reinterpret_cast<uint4*>(vst + vr * VROW + 16 * ch) = x;
                }
            }
            // O^T += V^T . P^T: lane 4 q + p of a 16-lane group addresses key row (4 lh + q), d = 16 dt + 4 p .. + 3, and receives
            // d = 16 dt + lr of the rows' four keys
            const unsigned char* vp = vst + (4 * lh + (lr >> 2)) * VROW + 8 * (lr & 3);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const s16x4 lo = dec_tr_read(vp + 32 * dt), hi = dec_tr_read(vp + 16 * VROW + 32 * dt);
                const s16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) o[dt][mt] = Mfma16<Tag>::mfma(vf, pf[mt], o[dt][mt]);
            }
        };

        Raw ra, rb;
        int c = wave;
        if (c < nch) load(ra, c);
        while (c < nch) {
            if (c + 4 < nch) load(rb, c + 4);
            compute(ra);
            c += 4;
            if (c >= nch) break;
            if (c + 4 < nch) load(ra, c + 4);
            compute(rb);
            c += 4;
        }
    }

    // the waves meet: one (m, l) per row and wave, then O in ascending wave order
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        l[mt] += __shfl_xor(l[mt], 16, 64);
        l[mt] += __shfl_xor(l[mt], 32, 64);
        if (lh == 0) ml[wave][16 * mt + lr] = make_float2(m[mt], l[mt]);
    }
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        float ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) ms = fmaxf(ms, ml[w][16 * mt + lr].x);
        const float mref = ms == -INFINITY ? 0.f : ms;
        float lt = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) lt += __builtin_amdgcn_exp2f(ml[w][16 * mt + lr].x - mref) * ml[w][16 * mt + lr].y;
        const float f = __builtin_amdgcn_exp2f(m[mt] - mref);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt][mt] *= f;
        m[mt] = ms;
        l[mt] = lt;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (wave > 0) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                *reinterpret_cast<f32x4*>(&red[wave - 1][lr * D + 16 * dt + 4 * lh]) = o[dt][mt];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int w = 0; w < 3; ++w) o[dt][mt] += *reinterpret_cast<const f32x4*>(&red[w][lr * D + 16 * dt + 4 * lh]);
                *reinterpret_cast<f32x4*>(a.ws_o + (part + 16 * mt + lr) * D + 16 * dt + 4 * lh) = o[dt][mt];
            }
            if (lh == 0) a.ws_ml[part + 16 * mt + lr] = make_float2(m[mt], l[mt]);
        }
        __syncthreads();
    }
}

struct DecMergeArgs {
    const float* ws_o;
    const float2* ws_ml;
    unsigned short* out;
    long osb, osh, oss;
    float* lse;                 // [B, H, Sq] or null
    const int32_t* counts;      // [B * Hl]: splits past a list's end were never written and are not read
    int Hl, NK, C;
    int H, U, Sq, nsplit, R16;
    long rows;                  // B * H * Sq
};

struct DecMergeArgs8 : DecMergeArgs {
    const float* v_scale;       // [Hkv]: multiplies the merged row once
    int Hkv;
};

// D / 4 threads per output row, four channels each; the splits in ascending order.
template <typename CTag, int D, typename Form>
__global__ __launch_bounds__(DEC_NT) void decode_merge_kernel(const typename Form::template Args<typename DecCache<CTag>::MergeArgs> a) {
    using Tag = typename DecCache<CTag>::Q;
    constexpr int TPR = D / 4;
    const long g = (long)blockIdx.x * DEC_NT + threadIdx.x;
    const long row = g / TPR;
    const int c = (int)(g % TPR);
    if (row >= a.rows) return;
    constexpr bool EXT = Form::EXT, PACKED = !Form::BATCHED, COUNTED = Form::SHORT && !PACKED;
    int qrow = (int)(row % a.Sq), h = (int)((row / a.Sq) % a.H);
    long b = row / ((long)a.Sq * a.H);
    long orow = qrow;           // the row's place in out (behind b * osb: 0 in the packed call)
    int pk_piece0 = 0;
    if constexpr (PACKED) {         // row = t * H + h over q's T rows: the item by search, the row's index in it, or no item at all
        h = (int)(row % a.H);
        orow = row / a.H;
        b = a.src.item_of_row((int)orow);
        const int s0 = a.src.row_start[b];
        qrow = (int)orow - s0;
        if (qrow < 0 || qrow >= min(a.src.row_start[b + 1] - s0, a.Sq)) {      // 0 / -inf, no list row and no partial read
            *reinterpret_cast<uint2*>(a.out + (long)h * a.osh + orow * a.oss + 4 * c) = make_uint2(0u, 0u);
            if (a.lse && c == 0) a.lse[row] = -INFINITY;
            return;
        }
        pk_piece0 = a.src.piece_start[b];
    }
    const int gu = a.H / a.U, unit = h / gu, rr = (h % gu) * a.Sq + qrow;
    long p0 = ((b * a.U + unit) * a.nsplit) * a.R16 + rr;       // decode: the unit's partials, head-major rows
    long lrow = b * a.Hl + unit / (a.U / a.Hl);
    if constexpr (EXT) {        // the row's group and its place in it (DecGroups)
        if constexpr (COUNTED) {
            if (qrow >= min(max(a.src.q_len[b], 0), a.Sq)) {    // a padding row: 0 / -inf, no list row and no partial read
                *reinterpret_cast<uint2*>(a.out + b * a.osb + (long)h * a.osh + (long)qrow * a.oss + 4 * c) = make_uint2(0u, 0u);
                if (a.lse && c == 0) a.lse[row] = -INFINITY;
                return;
            }
        }
        const int hu = h % gu, hc = hu / a.g.gh, qb = qrow / a.qblk, qi = qrow - qb * a.qblk, qcl = qi / a.g.qg;
        long grp = ((b * a.U + unit) * a.g.QC + qb * a.g.cpb + qcl) * a.g.HC + hc;
        if constexpr (PACKED) grp = ((long)(pk_piece0 + qb * a.g.cpb + qcl) * a.U + unit) * a.g.HC + hc;    // the compact group
        p0 = (grp * a.nsplit) * a.R16 + (hu - hc * a.g.gh) * a.g.qg + (qi - qcl * a.g.qg);
        lrow = lrow * a.g.NQ + qb;
    }
    const int count = min(max(a.counts[lrow], 0), a.NK);
    const int nlive = min(a.nsplit, (count + a.C - 1) / a.C);
    float vs = 1.f;
    if constexpr (DecCache<CTag>::kv8) vs = a.v_scale[h / (a.H / a.Hkv)];      // (asked for before the partials: not behind them)
    float ms = -INFINITY;
    for (int s = 0; s < nlive; ++s) {
        const float2 v = a.ws_ml[p0 + (long)s * a.R16];
        if (v.y > 0.f) ms = fmaxf(ms, v.x);
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float lt = 0.f;
    for (int s = 0; s < nlive; ++s) {
        const float2 v = a.ws_ml[p0 + (long)s * a.R16];
        if (!(v.y > 0.f)) continue;         // an empty partial: skipped, not multiplied (its O was never written)
        const float f = __builtin_amdgcn_exp2f(v.x - ms);
        const float4 x = *reinterpret_cast<const float4*>(a.ws_o + (p0 + (long)s * a.R16) * D + 4 * c);
        acc.x += f * x.x;
        acc.y += f * x.y;
        acc.z += f * x.z;
        acc.w += f * x.w;
        lt += f * v.y;
    }
    const bool any = lt > 0.f;
    float r[4] = {any ? acc.x / lt : 0.f, any ? acc.y / lt : 0.f, any ? acc.z / lt : 0.f, any ? acc.w / lt : 0.f};
    if constexpr (DecCache<CTag>::kv8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] *= vs;
    }
    uint2 pk;
    pk.x = (unsigned)Elem<Tag>::from_f32(r[0]) | ((unsigned)Elem<Tag>::from_f32(r[1]) << 16);
    pk.y = (unsigned)Elem<Tag>::from_f32(r[2]) | ((unsigned)Elem<Tag>::from_f32(r[3]) << 16);
    *reinterpret_cast<uint2*>(a.out + (PACKED ? 0 : b * a.osb) + (long)h * a.osh + orow * a.oss + 4 * c) = pk;
    if (a.lse && c == 0) a.lse[row] = any ? (ms + __builtin_amdgcn_logf(lt)) * 0.69314718055994530942f : -INFINITY;
}

// Kernarg offsets are in the instruction stream: in all four argument structs the row groups stand where DecExt has them, a
// counted or packed source directly behind them, and a padded source takes no room.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
template <typename A, typename R>
constexpr bool dec_src_behind() {
    using E = DecExt<A>;
    using W = WithRows<E, R>;
    return sizeof(W) == sizeof(E) + sizeof(R) && __builtin_offsetof(W, src) == sizeof(E) &&
           __builtin_offsetof(W, g) == __builtin_offsetof(E, g) && __builtin_offsetof(W, qblk) == __builtin_offsetof(E, qblk);
}
template <typename A>
constexpr bool dec_args_pinned() {
    return sizeof(WithRows<DecExt<A>, RowsPadded>) == sizeof(DecExt<A>) && dec_src_behind<A, RowsCounted>() && dec_src_behind<A, RowsPacked>();
}
static_assert(dec_args_pinned<DecArgs>() && dec_args_pinned<DecArgs8>() && dec_args_pinned<DecMergeArgs>() && dec_args_pinned<DecMergeArgs8>(),
              "kernarg offsets");
#pragma clang diagnostic pop

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct DecPlan {
    int U, MT, C, nsplit;
    size_t bytes;
    long groups;                // workgroups per split: units (decode) or row groups (extend)
    long pieces;                // packed: QP, the pieces (row groups per (unit, head chunk)) the grid holds
    DecGroups g;
};

#define EXT_FILL_GROUPS 256     // row groups from which a launch fills the chip (256 CUs) without splitting its lists

enum DecKind { DEC_DECODE, DEC_EXTEND, DEC_PACKED };

// A call's plan, from host values alone: units, the row groups (DecGroups), the rows of a group, the split size (0 = the library's
// choice) and the workspace.  Decode: a group is a whole unit of at most 64 rows (block is not read).  Extend: groups of gh heads x
// qg rows.  Packed: T rows of q hold B items of at most Sq = M rows each; the extend call's row groups with M for Sq (qg = min(64 /
// gh, block, M)) and QP pieces in the grid.  An item of n rows has pk_pieces(n) of them; piece j of an item starts at row (j / cpb)
// * block + (j % cpb) * qg >= j * qmax / cpb (qmax = min(M, block); cpb * qg >= qmax), so k non-empty items that hold J pieces in
// all own at least k + (J - k) * qmax / cpb <= T rows: J <= k + (T - k) * cpb / qmax, which grows with k <= min(B, T).  QP is that
// bound, capped by B * pk_pieces(M); groups = QP * U * HC, and bytes includes the head of the workspace, row_start and piece_start.
static int dec_plan(DecKind kind, int T, int B, int H, int Hkv, int Hl, int Sq, int D, int block, int NK, int blocks_per_split,
                    DecPlan* p) {
    if (kind == DEC_PACKED && (T <= 0 || Sq <= 0 || Sq > T)) return RSA_ERR_BAD_ARG;
    if (B <= 0 || H <= 0 || Hkv <= 0 || Hl <= 0 || Sq <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (H % Hkv || (Hl != 1 && Hl != Hkv && Hl != H)) return RSA_ERR_BAD_ARG;
    if (NK > DEC_MAX_NK || blocks_per_split < 0) return RSA_ERR_BAD_ARG;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    if (kind != DEC_DECODE && block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (kind == DEC_PACKED && B >= 0x7FFFFFFF) return RSA_ERR_UNSUPPORTED;
    p->U = Hl > Hkv ? Hl : Hkv;
    const int gu = H / p->U;
    DecGroups& g = p->g;
    p->pieces = 0;
    if (kind == DEC_DECODE) {
        if ((long)Sq * gu > DEC_MAX_ROWS) return RSA_ERR_UNSUPPORTED;
        g = DecGroups{1, 1, 1, 1, gu, Sq};
        p->groups = (long)B * p->U;
        if (p->groups > 0x7FFFFFFFl) return RSA_ERR_UNSUPPORTED;
    } else {
        g.HC = (gu + DEC_MAX_ROWS - 1) / DEC_MAX_ROWS;
        g.gh = (gu + g.HC - 1) / g.HC;                  // the unit's heads in HC even chunks of at most 64
        const int qmax = Sq < block ? Sq : block;       // query rows of a full query block
        g.qg = DEC_MAX_ROWS / g.gh < qmax ? DEC_MAX_ROWS / g.gh : qmax;
        g.NQ = (int)(((long)Sq + block - 1) / block);
        g.cpb = (qmax + g.qg - 1) / g.qg;
        // grid limits: the row groups are the grid's x extent, the merge runs one thread per four output channels
        if (kind == DEC_EXTEND) {
            const long qc = (long)(g.NQ - 1) * g.cpb + (Sq - (g.NQ - 1) * block + g.qg - 1) / g.qg;
            if (qc > 0x7FFFFFFFl / g.HC || (long)B * p->U > 0x7FFFFFFFl / (qc * g.HC)) return RSA_ERR_UNSUPPORTED;
            if ((long)B * H > (0x7FFFFFFFl * (long)DEC_NT) / ((long)Sq * (D / 4))) return RSA_ERR_UNSUPPORTED;
            g.QC = (int)qc;
            p->groups = (long)B * p->U * qc * g.HC;
        } else {
            g.QC = pk_pieces(Sq, block, g.qg, g.cpb);   // (of an item of M rows: the kernels do not read it)
            const long k = B < T ? B : T;
            long qp = k + ((long)T - k) * g.cpb / qmax;
            if (qp > (long)B * g.QC) qp = (long)B * g.QC;
            if (qp > 0x7FFFFFFFl / ((long)p->U * g.HC)) return RSA_ERR_UNSUPPORTED;
            if ((long)H > (0x7FFFFFFFl * (long)DEC_NT) / ((long)T * (D / 4))) return RSA_ERR_UNSUPPORTED;
            p->pieces = qp;
            p->groups = qp * p->U * g.HC;
        }
    }
    const int rows = g.gh * g.qg;
    p->MT = rows <= 16 ? 1 : (rows <= 32 ? 2 : 4);
    if (blocks_per_split > 0) {
        p->C = blocks_per_split < NK ? blocks_per_split : NK;
    } else {        // an extend launch that fills the chip with its row groups does not split its lists
        p->C = kind == DEC_DECODE || p->groups < EXT_FILL_GROUPS ? (DEC_SPLIT < NK ? DEC_SPLIT : NK) : NK;
    }
    p->nsplit = (NK + p->C - 1) / p->C;
    p->bytes = (kind == DEC_PACKED ? pk_head_bytes(2 * ((long)B + 1)) : 0) +
               (size_t)p->groups * p->nsplit * (16 * p->MT) * ((size_t)D + 2) * sizeof(float);
    return RSA_OK;
}

static int dec_plan_bytes(DecKind kind, int T, int B, int H, int Hkv, int Hl, int Sq, int D, int block, int NK, int blocks_per_split,
                          size_t* bytes, int64_t* pieces) {
    if (!bytes) return RSA_ERR_BAD_ARG;
    DecPlan p;
    const int st = dec_plan(kind, T, B, H, Hkv, Hl, Sq, D, block, NK, blocks_per_split, &p);
    if (st == RSA_OK) {
        *bytes = p.bytes;
        if (pieces) *pieces = p.pieces;
    }
    return st;
}

extern "C" int rsa_block_sparse_extend_packed_bytes(int T, int B, int H, int Hkv, int Hl, int max_q_len, int D, int block, int NK,
                                                    int blocks_per_split, size_t* bytes, int64_t* pieces) {
    return dec_plan_bytes(DEC_PACKED, T, B, H, Hkv, Hl, max_q_len, D, block, NK, blocks_per_split, bytes, pieces);
}

extern "C" int rsa_block_sparse_decode_bytes(int B, int H, int Hkv, int Hl, int Sq, int D, int NK, int blocks_per_split,
                                             size_t* bytes) {
    return dec_plan_bytes(DEC_DECODE, 0, B, H, Hkv, Hl, Sq, D, 0, NK, blocks_per_split, bytes, nullptr);
}

extern "C" int rsa_block_sparse_extend_bytes(int B, int H, int Hkv, int Hl, int Sq, int D, int block, int NK,
                                             int blocks_per_split, size_t* bytes) {
    return dec_plan_bytes(DEC_EXTEND, 0, B, H, Hkv, Hl, Sq, D, block, NK, blocks_per_split, bytes, nullptr);
}

// The one place that maps a call's cache element, query type, head dimension and row tiles to the kernels' template arguments:
// f(cache tag, std::integral_constant<int, D>, std::integral_constant<int, MT>).
template <typename F>
static void dec_with_shape(bool kv8, int dtype, int D, int MT, F f) {
    auto with_tag = [&](auto ctag) {
        auto with_d = [&](auto d) {
            if (MT == 1) f(ctag, d, std::integral_constant<int, 1>());
            else if (MT == 2) f(ctag, d, std::integral_constant<int, 2>());
            else f(ctag, d, std::integral_constant<int, 4>());
        };
        if (D == 128) with_d(std::integral_constant<int, 128>());
        else with_d(std::integral_constant<int, 64>());
    };
    if (kv8 && dtype == RSA_BF16) with_tag(kv8_tag<bf16_tag>());
    else if (kv8) with_tag(kv8_tag<fp16_tag>());
    else if (dtype == RSA_BF16) with_tag(bf16_tag());
    else with_tag(fp16_tag());
}

// An e4m3 cache view as the loads need it: K is read 8 bytes a lane, V 16 (strides in elements = bytes).
static int dec_check_cache8(const rsa_tensor4& t, int align) {
    if (!t.ptr || (reinterpret_cast<uintptr_t>(t.ptr) & (align - 1))) return RSA_ERR_BAD_ARG;
    if ((t.stride_b % align) || (t.stride_h % align) || (t.stride_s % align)) return RSA_ERR_BAD_ARG;
    return RSA_OK;
}

// What the eight entries hand to dec_run: their own arguments by name, and kind -- decode, extend, or the packed extend call: Sq is
// then M, T the rows of q, and q / out are read through stride_h and stride_s (the row's); kv8: the cache holds e4m3 codes and the two
// scale arrays are there; q_len_dev: the ragged call's rows per batch item (null: Sq); cu: the packed call's cu_seqlens_q [B + 1].
struct DecCall {
    DecKind kind;
    bool kv8;
    int T, B, H, Hkv, Hl, Sq, Sk, D, dtype, block, NK;
    const int32_t* kv_len_dev;
    int kv_valid, causal;
    double sm_scale;
    rsa_tensor4 q, k, v;
    const int32_t* block_table;
    int64_t table_stride_b;
    int num_pages;
    const int32_t *cols, *counts;
    int blocks_per_split;
    void* ws;
    size_t ws_bytes;
    rsa_out4 out;
    float* lse;
    const float *k_scale, *v_scale;
    const int32_t *q_len_dev, *cu;
    void* stream;
};

static int dec_run(const DecCall& c) {
    const bool pk = c.kind == DEC_PACKED;
    const int B = c.B, H = c.H, Hkv = c.Hkv, Hl = c.Hl, Sq = c.Sq, Sk = c.Sk, D = c.D, block = c.block, NK = c.NK;
    const rsa_tensor4 &q = c.q, &k = c.k, &v = c.v;
    const rsa_out4& out = c.out;
    if (B <= 0 || H <= 0 || Hkv <= 0 || Hl <= 0 || Sq <= 0 || Sk <= 0 || NK <= 0) return RSA_ERR_BAD_ARG;
    if (H % Hkv || (Hl != 1 && Hl != Hkv && Hl != H)) return RSA_ERR_BAD_ARG;
    if (block != 64 && block != 128) return RSA_ERR_UNSUPPORTED;
    if (c.dtype != RSA_BF16 && c.dtype != RSA_FP16) return RSA_ERR_UNSUPPORTED;
    if (D != 64 && D != 128) return RSA_ERR_UNSUPPORTED;
    const long nkmax = ((long)Sk + block - 1) / block;
    if (NK > (nkmax < DEC_MAX_NK ? nkmax : DEC_MAX_NK)) return RSA_ERR_BAD_ARG;
    if ((c.kind == DEC_DECODE && Sq > block) || c.blocks_per_split < 0) return RSA_ERR_BAD_ARG;
    if (!c.kv_len_dev && (c.kv_valid < 0 || c.kv_valid > Sk)) return RSA_ERR_BAD_ARG;
    DecPlan p;
    const int st = dec_plan(c.kind, c.T, B, H, Hkv, Hl, Sq, D, block, NK, c.blocks_per_split, &p);
    if (st != RSA_OK) return st;
    if (pk && (!c.cu || (reinterpret_cast<uintptr_t>(c.cu) & 3))) return RSA_ERR_BAD_ARG;
    if (!c.cols || !c.counts || !c.ws || !out.ptr) return RSA_ERR_BAD_ARG;
    if (rsa_check_tensor(q) != RSA_OK) return RSA_ERR_BAD_ARG;
    if (c.kv8) {
        if (!c.k_scale || !c.v_scale || ((reinterpret_cast<uintptr_t>(c.k_scale) | reinterpret_cast<uintptr_t>(c.v_scale)) & 3))
            return RSA_ERR_BAD_ARG;
        if (dec_check_cache8(k, 8) != RSA_OK || dec_check_cache8(v, 16) != RSA_OK) return RSA_ERR_BAD_ARG;
    } else if (rsa_check_tensor(k) != RSA_OK || rsa_check_tensor(v) != RSA_OK) {
        return RSA_ERR_BAD_ARG;
    }
    if (q.stride_b < 0 || q.stride_h < 0 || q.stride_s < 0 || k.stride_b < 0 || k.stride_h < 0 || k.stride_s < 0 ||
        v.stride_b < 0 || v.stride_h < 0 || v.stride_s < 0 || out.stride_b < 0 || out.stride_h < 0 || out.stride_s < 0)
        return RSA_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(out.ptr) & 7) || (out.stride_b % 4) || (out.stride_h % 4) || (out.stride_s % 4))
        return RSA_ERR_BAD_ARG;         // 8-byte stores of four channels
    if ((reinterpret_cast<uintptr_t>(c.cols) | reinterpret_cast<uintptr_t>(c.counts) | reinterpret_cast<uintptr_t>(c.kv_len_dev) |
         reinterpret_cast<uintptr_t>(c.block_table) | reinterpret_cast<uintptr_t>(c.lse) | reinterpret_cast<uintptr_t>(c.q_len_dev)) & 3)
        return RSA_ERR_BAD_ARG;
    if (c.block_table && (c.num_pages <= 0 || c.table_stride_b < 0)) return RSA_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(c.ws) & 15) return RSA_ERR_BAD_ARG;
    if (c.ws_bytes < p.bytes) return RSA_ERR_WORKSPACE;

    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const long parts = p.groups * p.nsplit;
    DecArgs8 a;                         // (the 2-byte kernels take the base structs)
    a.q = static_cast<const unsigned short*>(q.ptr);
    a.k = static_cast<const unsigned short*>(k.ptr);
    a.v = static_cast<const unsigned short*>(v.ptr);
    a.qsb = q.stride_b; a.qsh = q.stride_h; a.qss = q.stride_s;
    a.ksb = k.stride_b; a.ksh = k.stride_h; a.kss = k.stride_s;
    a.vsb = v.stride_b; a.vsh = v.stride_h; a.vss = v.stride_s;
    a.table = c.block_table;
    a.tsb = c.table_stride_b;
    a.num_pages = c.num_pages;
    a.cols = c.cols;
    a.counts = c.counts;
    a.kv_len = c.kv_len_dev;
    a.kv_valid = c.kv_valid;
    a.H = H; a.Hkv = Hkv; a.Hl = Hl; a.U = p.U; a.Sq = Sq; a.Sk = Sk; a.NK = NK; a.blk = block; a.causal = c.causal != 0;
    a.C = p.C; a.nsplit = p.nsplit; a.R16 = 16 * p.MT;
    a.qk_scale = (float)(c.sm_scale * 1.44269504);  // (as rsa_block_sparse_plain_fwd)
    // (packed: row_start and piece_start stand at the head of the workspace, the partials 16-byte aligned behind them)
    int32_t* const pk_head = static_cast<int32_t*>(c.ws);
    a.ws_o = reinterpret_cast<float*>(static_cast<unsigned char*>(c.ws) + (pk ? pk_head_bytes(2 * ((long)B + 1)) : 0));
    a.ws_ml = reinterpret_cast<float2*>(a.ws_o + parts * a.R16 * D);
    a.k_scale = c.k_scale;
    a.v_scale = c.v_scale;
    DecMergeArgs8 g;
    g.v_scale = c.v_scale;
    g.Hkv = Hkv;
    g.ws_o = a.ws_o;
    g.ws_ml = a.ws_ml;
    g.out = static_cast<unsigned short*>(out.ptr);
    g.osb = out.stride_b; g.osh = out.stride_h; g.oss = out.stride_s;
    g.lse = c.lse;
    g.counts = c.counts;
    g.Hl = Hl; g.NK = NK; g.C = p.C;
    g.H = H; g.U = p.U; g.Sq = Sq; g.nsplit = p.nsplit; g.R16 = a.R16;
    g.rows = pk ? (long)c.T * H : (long)B * H * Sq;
    const dim3 grid((unsigned)p.groups, (unsigned)p.nsplit), mgrid((unsigned)((g.rows * (D / 4) + DEC_NT - 1) / DEC_NT));

    // the two kernels of one row form, over the call's types
    auto launch = [&](auto form) {
        using Form = decltype(form);
        dec_with_shape(c.kv8, c.dtype, D, p.MT, [&](auto ctag, auto d, auto mt) {
            using CTag = decltype(ctag);
            typename Form::template Args<typename DecCache<CTag>::Args> sa;
            typename Form::template Args<typename DecCache<CTag>::MergeArgs> ma;
            static_cast<typename DecCache<CTag>::Args&>(sa) = a;
            static_cast<typename DecCache<CTag>::MergeArgs&>(ma) = g;
            if constexpr (Form::EXT) {
                sa.g = ma.g = p.g;
                sa.qblk = ma.qblk = block;
                sa.src = ma.src = form.rows;
            }
            decode_split_kernel<CTag, decltype(d)::value, decltype(mt)::value, Form><<<grid, DEC_NT, 0, s>>>(sa);
            decode_merge_kernel<CTag, decltype(d)::value, Form><<<mgrid, DEC_NT, 0, s>>>(ma);
        });
    };
    if (c.kind == DEC_DECODE) {
        launch(DecodeForm{});
    } else if (pk) {        // behind the scan of cu_seqlens_q: three launches
        pk_scan_launch(c.cu, B, c.T, Sq, block, p.g.qg, p.g.cpb, pk_head, nullptr, pk_head + B + 1, s);
        launch(ExtendForm<RowsPacked>{{pk_head, pk_head + B + 1, B, pk_steps(B)}});
    } else if (c.q_len_dev) {
        launch(ExtendForm<RowsCounted>{{c.q_len_dev}});
    } else {
        launch(ExtendForm<RowsPadded>{});
    }
    return rsa_launch_status();
}

extern "C" int rsa_block_sparse_decode(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                       const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                       rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                       int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws,
                                       size_t ws_bytes, rsa_out4 out, float* lse, void* stream) {
    return dec_run({.kind = DEC_DECODE, .kv8 = false, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = Sq, .Sk = Sk, .D = D,
                    .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid, .causal = causal,
                    .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table, .table_stride_b = table_stride_b,
                    .num_pages = num_pages, .cols = cols, .counts = counts, .blocks_per_split = blocks_per_split, .ws = ws,
                    .ws_bytes = ws_bytes, .out = out, .lse = lse, .stream = stream});
}

// The e4m3 cache: dtype names q's type; k / v hold one-byte codes (strides in bytes) and the scales are DEVICE fp32 [Hkv].
extern "C" int rsa_block_sparse_decode_kv8(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                           const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                           rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                           int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split,
                                           void* ws, size_t ws_bytes, rsa_out4 out, float* lse, const float* k_scale,
                                           const float* v_scale, void* stream) {
    return dec_run({.kind = DEC_DECODE, .kv8 = true, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = Sq, .Sk = Sk, .D = D,
                    .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid, .causal = causal,
                    .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table, .table_stride_b = table_stride_b,
                    .num_pages = num_pages, .cols = cols, .counts = counts, .blocks_per_split = blocks_per_split, .ws = ws,
                    .ws_bytes = ws_bytes, .out = out, .lse = lse, .k_scale = k_scale, .v_scale = v_scale, .stream = stream});
}

// ---- extend: any number of query rows.  The decode entries' argument lists; NQ = ceil(Sq / block) and cols /
// counts hold NQ list rows per (b, list head).
extern "C" int rsa_block_sparse_extend(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                       const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                       rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                       int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws,
                                       size_t ws_bytes, rsa_out4 out, float* lse, void* stream) {
    return dec_run({.kind = DEC_EXTEND, .kv8 = false, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = Sq, .Sk = Sk, .D = D,
                    .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid, .causal = causal,
                    .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table, .table_stride_b = table_stride_b,
                    .num_pages = num_pages, .cols = cols, .counts = counts, .blocks_per_split = blocks_per_split, .ws = ws,
                    .ws_bytes = ws_bytes, .out = out, .lse = lse, .stream = stream});
}

extern "C" int rsa_block_sparse_extend_kv8(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                           const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                           rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                           int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split,
                                           void* ws, size_t ws_bytes, rsa_out4 out, float* lse, const float* k_scale,
                                           const float* v_scale, void* stream) {
    return dec_run({.kind = DEC_EXTEND, .kv8 = true, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = Sq, .Sk = Sk, .D = D,
                    .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid, .causal = causal,
                    .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table, .table_stride_b = table_stride_b,
                    .num_pages = num_pages, .cols = cols, .counts = counts, .blocks_per_split = blocks_per_split, .ws = ws,
                    .ws_bytes = ws_bytes, .out = out, .lse = lse, .k_scale = k_scale, .v_scale = v_scale, .stream = stream});
}

// ---- ragged extend: a row count per batch item.  The extend entries' argument lists with q_len_dev, DEVICE
// int32 [B] (clamped into [0, Sq] on the device; NULL: the extend entry's call), in front of the stream.
extern "C" int rsa_block_sparse_extend_ragged(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                              const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale, rsa_tensor4 q,
                                              rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table, int64_t table_stride_b,
                                              int num_pages, const int32_t* cols, const int32_t* counts, int blocks_per_split,
                                              void* ws, size_t ws_bytes, rsa_out4 out, float* lse, const int32_t* q_len_dev,
                                              void* stream) {
    return dec_run({.kind = DEC_EXTEND, .kv8 = false, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = Sq, .Sk = Sk, .D = D,
                    .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid, .causal = causal,
                    .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table, .table_stride_b = table_stride_b,
                    .num_pages = num_pages, .cols = cols, .counts = counts, .blocks_per_split = blocks_per_split, .ws = ws,
                    .ws_bytes = ws_bytes, .out = out, .lse = lse, .q_len_dev = q_len_dev, .stream = stream});
}

extern "C" int rsa_block_sparse_extend_ragged_kv8(int B, int H, int Hkv, int Hl, int Sq, int Sk, int D, int dtype, int block, int NK,
                                                  const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale,
                                                  rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table,
                                                  int64_t table_stride_b, int num_pages, const int32_t* cols, const int32_t* counts,
                                                  int blocks_per_split, void* ws, size_t ws_bytes, rsa_out4 out, float* lse,
                                                  const float* k_scale, const float* v_scale, const int32_t* q_len_dev,
                                                  void* stream) {
    return dec_run({.kind = DEC_EXTEND, .kv8 = true, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = Sq, .Sk = Sk, .D = D,
                    .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid, .causal = causal,
                    .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table, .table_stride_b = table_stride_b,
                    .num_pages = num_pages, .cols = cols, .counts = counts, .blocks_per_split = blocks_per_split, .ws = ws,
                    .ws_bytes = ws_bytes, .out = out, .lse = lse, .k_scale = k_scale, .v_scale = v_scale, .q_len_dev = q_len_dev,
                    .stream = stream});
}

// ---- packed extend: q [T, H, D] with cu_seqlens_q.  The extend entries' argument lists with T in front, M
// = max_q_len where Sq stood, and cu_seqlens_q_dev, DEVICE int32 [B + 1], in front of the stream; q and out are read through
// stride_h and stride_s (a row of the packed tensor), stride_b is not read.
extern "C" int rsa_block_sparse_extend_packed(int T, int B, int H, int Hkv, int Hl, int max_q_len, int Sk, int D, int dtype, int block,
                                              int NK, const int32_t* kv_len_dev, int kv_valid, int causal, double sm_scale,
                                              rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v, const int32_t* block_table,
                                              int64_t table_stride_b, int num_pages, const int32_t* cols, const int32_t* counts,
                                              int blocks_per_split, void* ws, size_t ws_bytes, rsa_out4 out, float* lse,
                                              const int32_t* cu_seqlens_q_dev, void* stream) {
    q.stride_b = 0, out.stride_b = 0;
    return dec_run({.kind = DEC_PACKED, .kv8 = false, .T = T, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = max_q_len, .Sk = Sk,
                    .D = D, .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid,
                    .causal = causal, .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table,
                    .table_stride_b = table_stride_b, .num_pages = num_pages, .cols = cols, .counts = counts,
                    .blocks_per_split = blocks_per_split, .ws = ws, .ws_bytes = ws_bytes, .out = out, .lse = lse,
                    .cu = cu_seqlens_q_dev, .stream = stream});
}

extern "C" int rsa_block_sparse_extend_packed_kv8(int T, int B, int H, int Hkv, int Hl, int max_q_len, int Sk, int D, int dtype,
                                                  int block, int NK, const int32_t* kv_len_dev, int kv_valid, int causal,
                                                  double sm_scale, rsa_tensor4 q, rsa_tensor4 k, rsa_tensor4 v,
                                                  const int32_t* block_table, int64_t table_stride_b, int num_pages,
                                                  const int32_t* cols, const int32_t* counts, int blocks_per_split, void* ws,
                                                  size_t ws_bytes, rsa_out4 out, float* lse, const float* k_scale,
                                                  const float* v_scale, const int32_t* cu_seqlens_q_dev, void* stream) {
    q.stride_b = 0, out.stride_b = 0;
    return dec_run({.kind = DEC_PACKED, .kv8 = true, .T = T, .B = B, .H = H, .Hkv = Hkv, .Hl = Hl, .Sq = max_q_len, .Sk = Sk,
                    .D = D, .dtype = dtype, .block = block, .NK = NK, .kv_len_dev = kv_len_dev, .kv_valid = kv_valid,
                    .causal = causal, .sm_scale = sm_scale, .q = q, .k = k, .v = v, .block_table = block_table,
                    .table_stride_b = table_stride_b, .num_pages = num_pages, .cols = cols, .counts = counts,
                    .blocks_per_split = blocks_per_split, .ws = ws, .ws_bytes = ws_bytes, .out = out, .lse = lse,
                    .k_scale = k_scale, .v_scale = v_scale, .cu = cu_seqlens_q_dev, .stream = stream});
}
