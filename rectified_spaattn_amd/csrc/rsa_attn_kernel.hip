// K5 at 64-token blocks: block-sparse flash attention forward for gfx950 (MI355X) with the rectification epilogue fused, 32
// query rows per wave.  (128-token blocks and dense calls run the 64-rows-per-wave kernel, rsa_attn_kernel64.hip.)
//
// One workgroup (4 waves, 256 threads, two workgroups per CU) owns the PAIR of 64-row query blocks (2 qblk, 2 qblk + 1): waves
// 0-1 the first, waves 2-3 the second, wave w rows 32w..32w+31 of the pair's 128.  It walks the UNION of the two blocks' kept
// lists -- one 64-key tile per entry, staged once for both; the entries carry which of the two kept them (bits 14 / 15 of the LDS
// list), and a wave pair masks the tiles of the other's list to -inf (exact: they add 0 to O and l, and -inf leaves the running
// maximum alone), so every row gets the bytes its own list would give.  Dense text rows: 128-row units from row
// NBv * 64 on (a.txt0), every key block theirs, optionally split over the key range (split-KV partials, rsa_attn.hip).
//
// Both GEMMs run on v_mfma_f32_32x32x16_{bf16,f16} in the "key on the register, query row on the lane" orientation:
//      S^T[key][q]  = K . Q^T      A = K rows (ds_read_b128 from an XOR-swizzled row-major tile), B = Q (registers)
//      O^T[d][q]   += V^T . P^T    A = V^T (ds_read_b64_tr_b16 transposing reads), B = P^T = the S^T accumulator
//                                      converted in place (no LDS round trip, no cross-lane traffic)
// so the softmax state (m, l) of a query row lives on one lane pair and the only cross-lane operation per
// 32 keys is one v_permlane32_swap for the row max.
//
// Software pipeline (per wave, at 32-key granularity, S double-buffered in registers, loop unrolled by two
// 64-key tiles so every LDS address is a loop-invariant VGPR plus an immediate):
//      MFMA stream:  S(u+1)^T = K(u+1) . Q^T      then   O^T += V(u)^T . P(u)^T
//      VALU stream:  P(u) = exp2(S(u) - m) (+ row sums, 2-byte packing)   then   row max of S(u+1)
// That block is ONE hand-placed instruction stream (gen_k5_block.py -> rsa_attn_block.h: inline asm, every register
// pinned): round 2 showed that leaving it to hipcc makes the kernel's speed a matter of which schedule the compiler
// happens to emit (profiles/r03_k5_r1_vs_head.md: the same source went from read-ahead operand reads to one
// lgkmcnt(0) per MFMA between two rounds, -8 %).  The running max is deferred: the reference max only moves when some
// row's max grew by more than 2^8 since it was set (P <= 2^8: same relative precision in bf16/fp16 P, fp32
// accumulators); that rare rescale and the mask (boundary tiles, tiles of the other wave pair's list) sit in branches in front
// of the block.
//
// Staging: K/V tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction) issued
// from inline asm so that hipcc neither counts nor drains them; LDS = [K0 K1 V0 V1 | union list (u16)], 64-key tiles.  At the
// head of sub-step (t,0) V(t+1) is issued into V(t-1)'s slot, at the head of (t,1) K(t+2) into K(t)'s slot, each behind a
// counted vmcnt (the group issued half a tile ago stays in flight) + barrier; every tile has a full tile time to land.
// (One wait + barrier + issue point per 64-key TILE -- half the barriers, 8 pieces per issue point -- measured the same:
// 16.33 vs 16.23 ms, profiles/r03_k5_block.md; not kept.)  The LDS image is lane-linear, so the XOR swizzle is applied to
// the per-lane SOURCE chunk (same involution as tile_off on the read side); per-lane source offsets are tile-invariant
// 32-bit values and the tile only moves a scalar base.
//
// The chip runs this loop at its board power cap (tools/clock_probe.py), so cycles saved from stalls come back as a lower
// clock; what pays is fewer instructions per MFMA.  Head dim 128: the score chain starts from -m (a 16-register block, C
// operand of the first QK^T MFMA), so the accumulator is S - m and the softmax needs no subtraction; the row sums are added
// into l.  Head dim 64: the classic arithmetic (S, then S - m by v_sub), which measures faster there, with the row sums on the
// matrix pipe (lacc).
//
// Semantics kept from the reference kernel (rectified_hunyuan_attn.py:15-105): Q is pre-multiplied by
// sm_scale*log2(e) and rounded to the input dtype (:61-62), P is rounded to the input dtype before PV (:97),
// fp32 softmax statistics and accumulators, kv columns beyond the valid keys are -inf (:86-87), rows
// beyond the sequence are not stored (:105).  Added: a NaN-free fully-masked path, the fused O*R+comp epilogue (hunyuan :365)
// and a strided [B,S,H,D] store (hunyuan :383-387).
//
// (Forms measured and NOT kept in this library -- a ping-pong 8-wave kernel, paired 256-row workgroups over union lists,
// persistent workgroups, a 256-row dense tile, non-temporal K/V loads, the LDS-DMA pieces spread over the block's MFMA
// shadows, 16x16x32 MFMAs, one staging point per tile: commit c37b5bb / profiles/r02_experiments.md, profiles/r03_k5_block.md.)
#include "rsa_attn.h"
#include "rsa_attn_block.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The hand-placed pipelined block (gen_k5_block.py): one asm statement per sub-step with every register pinned (register
// map and operand lists: rsa_attn_block.h, RSA_K5_OPS*; e.g. D = 128: O v[0:63], Q v[64:95], SA v[96:111], SB v[112:127],
// -m v[128:143]).  S_cur = SA on even sub-steps, SB on odd ones.
#define RSA_K5_PICK(NAME, DD, TT, OPS, CLOB) \
    do { \
        if constexpr (VS == 0 && SUB == 0) asm volatile(NAME##_##DD##_##TT##_V0_S0 OPS : CLOB, "memory"); \
        else if constexpr (VS == 0 && SUB == 1) asm volatile(NAME##_##DD##_##TT##_V0_S1 OPS : CLOB, "memory"); \
        else if constexpr (VS == 1 && SUB == 0) asm volatile(NAME##_##DD##_##TT##_V1_S0 OPS : CLOB, "memory"); \
        else asm volatile(NAME##_##DD##_##TT##_V1_S1 OPS : CLOB, "memory"); \
    } while (0)

// head dim 128: S_cur / S_nxt hold S - m (nm = -m in 16 registers), no subtraction in the softmax; the row sums go into l
template <typename Tag, int VS, int SUB>
__device__ __forceinline__ void k5_block_nm(f32x16 (&o)[4], const s16x8 (&q)[8], f32x16& S_cur, f32x16& S_nxt, const f32x16& nm,
                                            float& l, float& mx, const i32x8& ka, const i32x8& va) {
    f32x16& SA = SUB == 0 ? S_cur : S_nxt;
    f32x16& SB = SUB == 0 ? S_nxt : S_cur;
    if constexpr (std::is_same<Tag, bf16_tag>::value) RSA_K5_PICK(RSA_K5_BLOCKN, 128, BF16, RSA_K5_OPSN_128, RSA_K5_CLOBBERN_128);
    else RSA_K5_PICK(RSA_K5_BLOCKN, 128, F16, RSA_K5_OPSN_128, RSA_K5_CLOBBERN_128);
}
// head dim 64: the classic form (S, then S - m by v_sub: the arithmetic of round 2's compiled block, bit for bit), which measures
// 4 % faster there than the -m form (at 128 the -m form wins by 3.7 %).  The row sums ride the matrix pipe: lacc = four registers
// with the lane's complete row sum of the rounded P, onesv the ones operand of those products.
template <typename Tag, int VS, int SUB>
__device__ __forceinline__ void k5_block(f32x16 (&o)[2], const s16x8 (&q)[4], f32x16& S_cur, f32x16& S_nxt, float m, f32x4& lacc,
                                         const s16x8& onesv, float& mx, const i32x4& ka, const i32x4& va) {
    f32x16& SA = SUB == 0 ? S_cur : S_nxt;
    f32x16& SB = SUB == 0 ? S_nxt : S_cur;
    if constexpr (std::is_same<Tag, bf16_tag>::value) RSA_K5_PICK(RSA_K5_BLOCK, 64, BF16, RSA_K5_OPS_64, RSA_K5_CLOBBER_64);
    else RSA_K5_PICK(RSA_K5_BLOCK, 64, F16, RSA_K5_OPS_64, RSA_K5_CLOBBER_64);
}

// NEGM (head dim 128): the score chain starts from -m and the row sums are added into l_run.  Head dim 64: the classic
// arithmetic with the row sums in lacc.  The two differ by the rounding order of S - m.
// WIDE: 16-byte output stores after a permlane32_swap regroup (needs 16-byte aligned output rows), else 8-byte stores.
// GQA: grouped-query K/V heads of a sparse call (AttnArgs::kv_group / list_group; rsa_block_sparse_gqa_fwd): the walk of query head
// h with the K/V head h / kv_group and the lists of list head h / list_group; nothing else changes.
template <int D, typename Tag, bool WIDE, bool GQA = false>
__global__ __launch_bounds__(256, 2) void bsfwd_kernel(AttnArgs) {
    const AttnArgs& a = rsa_kernargs<AttnArgs>();
    constexpr bool NEGM = D == 128;
    constexpr int NW = 4;                   // 4 waves x 32 query rows
    constexpr int KS = D / 16;
    constexpr int DT = D / 32;
    constexpr int CHR = D / 8;
    constexpr int RPI = 1024 / (D * 2);     // rows per 1-KiB piece
    constexpr int TILE_BYTES = 64 * D * 2;
    constexpr int NPC = TILE_BYTES / 1024 / NW;  // 1-KiB pieces per wave per tile operand (4 at head dim 128, 2 at 64)
    using E = Elem<Tag>;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    unsigned short* lds_list = reinterpret_cast<unsigned short*>(lds + 4 * TILE_BYTES);

    const int work = blockIdx.x;
    const GsyncTicket gs_tk = rsa_gsync_announce(a.gsync, a.gsync_gen);   // aligned starts (rsa_attn.h)
    // ---------------- work mapping (rsa_attn.h) ----------------
    // qblk: the PAIR of query blocks, or the 128-row text unit; tsp: which part of a text unit's key range this workgroup walks.
    // `tail` is ignored: this kernel has no partial store for a tail piece, and the host plans a tail split for the kernels that have
    int bh, qblk, tsp, tail;
    const int walk = rsa_walk_map(a, work, (a.NBv + 1) >> 1, bh, qblk, tsp, tail);
    if (walk == WALK_NONE) return;
    const bool text = walk == WALK_TEXT;
    const int b = bh / a.H, h = bh % a.H;
    long lbh = bh;                          // list head of this head: its own, or the one it shares (h / list_group)
    if constexpr (GQA) lbh = (long)b * (a.H / a.list_group) + h / a.list_group;
    const int t = threadIdx.x, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int grow = (text ? a.txt0 + (qblk - a.NBv) * 128 : qblk * 128) + 32 * wv + r;
    const int qw = 2 * qblk + (wv >> 1);   // this wave's own query block (sparse walks)

    // ---------------- per-row plan ----------------
    // hi: one past the last key the rows may see; a list (sparse pair) or the key blocks first_blk .. + n_items - 1 (text unit)
    bool store_r = false, zero_r = false;
    int n_items, first_blk = 0, hi;
    const int32_t* list = nullptr;
    bool rectify = false;
    if (!text) {
        rsa_walk_list(a, lbh * a.NBv + 2 * qblk, -1, 0, list, n_items);
        hi = a.kv_valid;
        rectify = a.R != nullptr;
        store_r = grow < a.Sq && qw < a.NBv;
    } else {
        rsa_walk_text(a, 64, tsp, first_blk, n_items);
        hi = a.kv_text_valid;
        store_r = grow < a.q_text_end;
        zero_r = !store_r && grow < a.Sq;
    }
    n_items = __builtin_amdgcn_readfirstlane(n_items);
    const bool use_list = list != nullptr;
    if (use_list) {
        // union of the pair's lists: both scattered into two bitmaps (in the K/V tile area, free until the first staging),
        // one word per thread (NB_total <= 8 192: <= 256 words), a workgroup prefix sum of the popcounts, then each thread
        // writes its word's entries in ascending order: block | kept by 2 qblk << 14 | kept by 2 qblk + 1 << 15
        unsigned* bm = reinterpret_cast<unsigned*>(lds);
        int* wsum = reinterpret_cast<int*>(lds + 2 * 256 * 4);
        const int nw = (a.NB_total + 31) >> 5;
        for (int i = t; i < 2 * nw; i += 64 * NW) bm[i] = 0u;
        __syncthreads();
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int qb = 2 * qblk + hb;
            if (qb < a.NBv) {
                const long ri = lbh * a.NBv + qb;
                const int32_t* li = a.cols + ri * a.NB_total;
                const int n = a.counts[ri];
                for (int i = t; i < n; i += 64 * NW) {
                    const int c = li[i];
                    atomicOr(&bm[hb * nw + (c >> 5)], 1u << (c & 31));
                }
            }
        }
        __syncthreads();
        const unsigned w0 = t < nw ? bm[t] : 0u, w1 = t < nw ? bm[nw + t] : 0u;
        unsigned u = w0 | w1;
        const int c = __popc(u);
        int x = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[t >> 6] = x;
        __syncthreads();
        int off = x - c;
        for (int ww = 0; ww < (t >> 6); ++ww) off += wsum[ww];
        n_items = __builtin_amdgcn_readfirstlane(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
        while (u) {
            const int bit = __ffs(u) - 1;
            u &= u - 1;
            lds_list[off++] = (unsigned short)((32 * t + bit) | (((w0 >> bit) & 1u) << 14) | (((w1 >> bit) & 1u) << 15));
        }
        __syncthreads();
    }
    // One 64-key tile per item.  The raw entry of tile `tile` (block | owner bits; text walks: both owners), still per lane, index
    // clamped (callers guard tile < n_items), and the KEY WORD the tile queue carries: first key | owner bits << 28
    auto raw_item = [&](int tile) -> int {
        const int it = tile < n_items ? tile : (n_items > 0 ? n_items - 1 : 0);
        return use_list ? (int)lds_list[it] : (first_blk + it) | (3 << 14);
    };
    auto kword = [&](int raw) -> int { return ((raw & 0x3FFF) * 64) | ((raw >> 14) << 28); };
    auto kkey = [&](int kw) -> int { return kw & 0x0FFFFFFF; };
    const int kv_limit = hi < a.Sk ? hi : a.Sk;
    auto key0_of = [&](int tile) -> int { return kword(__builtin_amdgcn_readfirstlane(raw_item(tile))); };

    // ---------------- Q fragments (B operand) ----------------
    s16x8 qf[KS];
    {
        const unsigned short* qp = a.q + (long)b * a.qsb + (long)h * a.qsh + (long)grow * a.qss + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = rsa_q_frag<Tag>(qp + 16 * ks, grow < a.Sq, a.qk_scale);
    }

    // ---------------- LDS-DMA staging ----------------
    int hkv = h;                            // the K/V head
    if constexpr (GQA) hkv = h / a.kv_group;
    const unsigned char* kbase = reinterpret_cast<const unsigned char*>(a.k + (long)b * a.ksb + (long)hkv * a.ksh);
    const unsigned char* vbase = reinterpret_cast<const unsigned char*>(a.v + (long)b * a.vsb + (long)hkv * a.vsh);
    // A region of keys is staged in groups of 4 pieces (4 KiB = 4*RPI rows); in every group wave w moves piece w: rows
    // w*RPI .. +RPI-1 of the group.  The source-chunk swizzle depends on the row inside the group only.
    const int rsub = lane / CHR, cl = lane % CHR;
    const int rowl = wv * RPI + rsub;  // row inside a group
    const int gsw = D == 128 ? (cl ^ (((rowl & 3) << 2) | ((rowl >> 2) & 3))) : (cl ^ ((rowl >> 1) & 7));
    const unsigned voffk = (unsigned)(((long)rowl * a.kss + gsw * 8) * 2);
    const unsigned voffv = (unsigned)(((long)rowl * a.vss + gsw * 8) * 2);
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const long kstep = (long)(4 * RPI) * a.kss * 2, vstep = (long)(4 * RPI) * a.vss * 2;  // bytes per group
    // the 64-key tile starting at key `key_first` -> LDS byte offset `lds_off` (tile slots: K0 K1 V0 V1)
    auto dma = [&](int is_v, int key_word, unsigned lds_off) {
        const int key_first = kkey(key_word);
        const unsigned ld0 = lds_base + lds_off + wv * 1024;
        const unsigned char* base = is_v ? vbase : kbase;
        const long ss = is_v ? a.vss : a.kss;
        if (key_first + 64 <= kv_limit) {
            const unsigned char* tb = base + (long)key_first * ss * 2;
            const long step = is_v ? vstep : kstep;
            const unsigned vo = is_v ? voffv : voffk;
#pragma unroll
            for (int j = 0; j < NPC; ++j) rsa_lds_dma16(vo, tb + j * step, ld0 + j * 4096);
        } else {   // the tile runs past the last valid key: rows clamped (their scores are masked)
#pragma unroll
            for (int j = 0; j < NPC; ++j) {
                int krow = key_first + j * 4 * RPI + rowl;
                krow = krow < kv_limit ? krow : kv_limit - 1;
                rsa_lds_dma16((unsigned)(((long)krow * ss + gsw * 8) * 2), base, ld0 + j * 4096);
            }
        }
    };

    // ---------------- state ----------------
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;
    // Row sums on the matrix pipe (head dim 64, gen_k5_block.py::rsm_form): lacc = the lane's complete
    // row sum of the rounded P in all four registers.  A operand of v_mfma_f32_16x16x32 (lane: row a = l & 15, k-block l >> 4): ones
    // iff (k-block & 1) == ((a >> 2) & 1) -- the B operand is the P . V product's P fragment, whose k-blocks 0 / 2 are the two lane
    // halves of query row n and 1 / 3 those of row n + 16, and the lane that owns C rows 4 (l >> 4) .. + 3 of column l & 15 is the
    // lane of exactly that query row (the construction of the e4m3 kernel's row-sum product).
    f32x4 lacc = {0.0f, 0.0f, 0.0f, 0.0f};
    s16x8 onesv;
    {
        const short one = std::is_same<Tag, bf16_tag>::value ? (short)0x3F80 : (short)0x3C00;
        const short w = (((lane >> 4) & 1) == ((lane >> 2) & 1)) ? one : (short)0;
#pragma unroll
        for (int i = 0; i < 8; ++i) onesv[i] = w;
    }
    // m_ref = the finite reference the scores are taken against (S_cur, S_nxt hold S - m_ref), nm = its negation in 16
    // registers (C operand of the first QK^T MFMA), thr = how far a new row maximum may exceed it before the rescale (-inf
    // until the row has seen a finite score: the first finite maximum always becomes the reference).  m_run is the running
    // maximum itself (-inf = nothing seen): what the split-KV partials carry, and the classic form's reference.
    float m_ref = 0.0f, thr = -INFINITY;
    f32x16 nm;
#pragma unroll
    for (int i = 0; i < 16; ++i) nm[i] = 0.0f;

    // per-lane read addressing
    const int kswz = ((r & 3) << 2) | ((r >> 2) & 3);
    const int g4 = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
    int vrd[DT][2];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int ch = 4 * dt + 2 * (g4 & 1) + (tp >> 1);
        vrd[dt][0] = tile_off<D>(4 * hh + tq, ch) + 8 * (tp & 1);
        vrd[dt][1] = tile_off<D>(4 * hh + tq + 8, ch) + 8 * (tp & 1);
    }
    auto k_off = [&](int ks, int sub) {
        if constexpr (D == 128) return (32 * sub + r) * 256 + (((2 * ks + hh) ^ kswz) << 4);
        else return tile_off<D>(32 * sub + r, 2 * ks + hh);
    };
    // read addresses of the hand-placed block: LDS byte addresses of sub-tile 0 / slot 0; slot, sub-tile and k-step are immediates
    using AddrV = typename std::conditional<D == 128, i32x8, i32x4>::type;   // KS K addresses, 2 DT V addresses
    AddrV ka, va;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) ka[ks] = (int)lds_base + k_off(ks, 0);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { va[2 * dt] = (int)lds_base + vrd[dt][0]; va[2 * dt + 1] = (int)lds_base + vrd[dt][1]; }

    // S^T (32 keys x 32 rows) = K[sub-tile SUB of K slot] . Q^T
    auto qk_sub = [&](auto KSLOT, auto SUB, f32x16& S) {
        constexpr int slot = decltype(KSLOT)::value, sub = decltype(SUB)::value;
        const unsigned char* kt_ = lds + slot * TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const s16x8 a0 = *reinterpret_cast<const s16x8*>(kt_ + k_off(ks, sub));
            S = E::mfma(a0, qf[ks], S);
        }
    };
    auto rowmax_sub = [&](const f32x16& S, float& mx) {
        float m = S[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) m = fmaxf(m, S[i]);
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    };
    auto apply_mask_sub = [&](f32x16& S, int key_first, bool mine) {
        int kbase = key_first + 4 * hh;
        asm volatile("" : "+v"(kbase));   // rare branch: keep its 16 key indices out of the loop's live registers
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = kbase + (i & 3) + 8 * (i >> 2);
            if (kk >= hi || !mine) S[i] = -INFINITY;
        }
    };

    int kq1 = 0, kq2 = 0;  // first keys of tile+1 / tile+2 (fetched from LDS ahead of use)

    // The part of a sub-step u = 2*tile + SUB behind its staging: rare branches (boundary mask, deferred rescale), then the
    // pipelined block: consumes S_cur (scores of 32 keys, row max in mx_cur), produces S_nxt / mx_nxt for sub-step u+1.
    // VS = slot parity of `tile` (its K and V slots); next scores = K(tile) sub-tile 1 (SUB 0) / K(tile+1) sub-tile 0 (SUB 1).
    auto half = [&](auto VS, auto SUB, int key0, f32x16& S_cur, float& mx_cur, f32x16& S_nxt, float& mx_nxt) {
        constexpr int vs = decltype(VS)::value, sub = decltype(SUB)::value;
        const int kfirst = kkey(key0) + 32 * sub;
        const bool mine = (key0 >> (28 + (wv >> 1))) & 1;   // the tile is in this wave pair's list
        if (kfirst + 32 > hi || !mine) {
            apply_mask_sub(S_cur, kfirst, mine);
            rowmax_sub(S_cur, mx_cur);
        }
        if constexpr (NEGM) {
            // S_cur, mx_cur are relative to m_ref as it was when they were computed, and that is still m_ref
            if (__builtin_amdgcn_ballot_w64(mx_cur > thr) != 0ull) {
                asm volatile("s_nop 11" ::: "memory");   // the block's last MFMA wrote O: 12 wait states before a VALU touches it
                const bool first = thr == -INFINITY;
                float delta = first ? mx_cur : fmaxf(mx_cur, 0.0f);
                if (delta == -INFINITY) delta = 0.0f;      // nothing but masked keys so far
                else thr = 8.0f;
                const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);   // (first: O and l are still zero)
                m_ref += delta;
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
#pragma unroll
                for (int i = 0; i < 16; ++i) { S_cur[i] -= delta; nm[i] = -m_ref; }
            }
            k5_block_nm<Tag, vs, sub>(o, qf, S_cur, S_nxt, nm, l_run, mx_nxt, ka, va);
        }
        else {   // the classic arithmetic (scores S, reference m_run subtracted in the softmax)
            if (__builtin_amdgcn_ballot_w64(mx_cur > m_run + 8.0f) != 0ull) {
                asm volatile("s_nop 11" ::: "memory");
                const float m_new = fmaxf(m_run, mx_cur);
                const float mu = (m_new == -INFINITY) ? 0.0f : m_new;
                const float alpha = __builtin_amdgcn_exp2f(m_run - mu);
                m_run = m_new;
#pragma unroll
                for (int i = 0; i < 4; ++i) lacc[i] *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
            }
            const float m_use = (m_run == -INFINITY) ? 0.0f : m_run;
            k5_block<Tag, vs, sub>(o, qf, S_cur, S_nxt, m_use, lacc, onesv, mx_nxt, ka, va);
        }
    };

    // staging: a wait + barrier + issue point in front of every sub-step.  SUB 0 issues V(tile+1) into V(tile-1)'s slot,
    // SUB 1 K(tile+2) into K(tile)'s slot; the newest group (issued half a tile ago) may stay in flight, the one issued a
    // tile ago must land.
    auto stage = [&](auto VS, auto SUB, int tile) {
        constexpr int vs = decltype(VS)::value, sub = decltype(SUB)::value;
        if (tile + 1 < n_items) {
            if constexpr (NPC == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if constexpr (sub == 0) {
            if (tile + 1 < n_items) dma(1, kq1, (2 + (vs ^ 1)) * TILE_BYTES);
        } else {
            if (tile + 2 < n_items) dma(0, kq2, vs * TILE_BYTES);
        }
    };

    // ---------------- prologue + main loop ----------------
    if (!text) rsa_gsync_wait(a.gsync, gs_tk, n_items, a.NB_total, a.gsync_ratio);   // aligned starts: in front of the first staging instruction (text-row pieces do not wait, as in the 64-row and e4m3 kernels)
    f32x16 SA, SB;
    float mxA = -INFINITY, mxB = -INFINITY;
    int key0 = 0;
    if (n_items > 0) {
        key0 = key0_of(0);
        kq1 = key0_of(1);
        kq2 = key0_of(2);
        dma(0, key0, 0);
        dma(1, key0, 2 * TILE_BYTES);
        if (n_items > 1) dma(0, kq1, TILE_BYTES);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        qk_sub(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, SA);
        rowmax_sub(SA, mxA);
    }
    // The kept-list entry of tile+3 is read from LDS one advance() EARLY into a register (pref_raw) and only made scalar
    // here: the LDS round trip (~100 cycles, once per tile and wave) is off the wave's critical path.
    int pref_raw = n_items > 0 ? raw_item(3) : 0;
    auto advance = [&](int tile) {  // after finishing `tile`: shift the key queue, tile+3's first key from the prefetched entry
        key0 = kq1;
        kq1 = kq2;
        kq2 = kword(__builtin_amdgcn_readfirstlane(pref_raw));
        pref_raw = raw_item(tile + 4);
    };
    {
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        auto tile_step = [&](auto VS, int tile) {
            stage(VS, I0{}, tile);
            half(VS, I0{}, key0, SA, mxA, SB, mxB);
            stage(VS, I1{}, tile);
            half(VS, I1{}, key0, SB, mxB, SA, mxA);
        };
        int tile = 0;
        for (; tile + 1 < n_items; tile += 2) {
            tile_step(I0{}, tile);
            advance(tile);
            tile_step(I1{}, tile + 1);
            advance(tile + 1);
        }
        if (tile < n_items) tile_step(I0{}, tile);
    }

    // ---------------- epilogue ----------------
    asm volatile("s_nop 11" ::: "memory");   // (the last block's last MFMA -> the reads of O below)
    if constexpr (NEGM) m_run = thr == -INFINITY ? -INFINITY : m_ref;
    const auto swl = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_run), __float_as_uint(l_run), false, false);
    const float l_tot = !NEGM ? lacc[0] : __uint_as_float(swl[0]) + __uint_as_float(swl[1]);   // (lacc: already complete over both lane halves)
    if (a.tsplit > 1 && text) {
        // split-KV partial of a text block: unnormalised O (fp32), m (log2 domain) and l per row; the combine
        // kernel (rsa_attn.hip) merges the tsplit parts
        float* pp = rsa_part_of(a, bh, qblk, tsp, -1, 32 * wv + r, D);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) rsa_part_tile(pp, dt, hh, o[dt]);
        rsa_part_ml(pp, D, hh, m_run, l_tot);
    } else if (store_r || zero_r) {
        // the fused O * R / l + comp store (rsa_attn.h); padded text rows (zero_r) are stored as zeros.  Only sparse walks are
        // rectified, so a text row's compensation values are zeros already
        float4 cv[DT][4];
        float Rv = 1.0f;
        const long rowi = (long)bh * a.NBv + qw;
        rsa_comp_row<DT>(cv, rectify ? a.comp + rowi * D : nullptr, hh);
        if (rectify) Rv = a.R[rowi];
        const float inv = l_tot > 0.0f && !zero_r ? 1.0f / l_tot : 0.0f;
        const float sc = inv * Rv;
        unsigned short* op = a.out + (long)b * a.osb + (long)h * a.osh + (long)grow * a.oss;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) rsa_out_tile<Tag, WIDE>(op, dt, hh, o[dt], sc, cv[dt]);
    }
}

// launch hook used by rsa_attn.hip::launch_attn (64-token blocks only)
int rsa_launch_bsfwd(const AttnArgs& a, dim3 grid, size_t lds_bytes, int D, int dtype, hipStream_t s) {
    if (a.blk != 64 || a.mode != MODE_SPARSE) return RSA_ERR_UNSUPPORTED;
    // the 16-byte output stores need 16-byte aligned rows; anything else takes the 8-byte form
    const bool wide = !(((uintptr_t)a.out & 15) || ((a.osb | a.osh | a.oss) & 7));
    if (a.gqa != RSA_GQA_NONE && (a.gqa != RSA_GQA_HEAD || a.kv_group <= 0 || a.list_group <= 0)) return RSA_ERR_BAD_ARG;   // (no head pairs here)
#define RSA_K5(DD, TT) \
    do { \
        if (a.gqa) { \
            if (wide) RSA_LAUNCH_GSYNC(2, (bsfwd_kernel<DD, TT, true, true>), a, true, grid, 256, lds_bytes, s); \
            else RSA_LAUNCH_GSYNC(2, (bsfwd_kernel<DD, TT, false, true>), a, true, grid, 256, lds_bytes, s); \
        } else if (wide) RSA_LAUNCH_GSYNC(2, (bsfwd_kernel<DD, TT, true>), a, true, grid, 256, lds_bytes, s); \
        else RSA_LAUNCH_GSYNC(2, (bsfwd_kernel<DD, TT, false>), a, true, grid, 256, lds_bytes, s); \
    } while (0)
    if (D == 128) {
        if (dtype == RSA_BF16) RSA_K5(128, bf16_tag); else RSA_K5(128, fp16_tag);
    } else {
        if (dtype == RSA_BF16) RSA_K5(64, bf16_tag); else RSA_K5(64, fp16_tag);
    }
#undef RSA_K5
    return rsa_launch_status();
}
