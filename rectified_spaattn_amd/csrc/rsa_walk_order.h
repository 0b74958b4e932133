// The work mapping of the K5 kernels: grid index -> (batch * head, unit, piece).  No HIP types: a plain C++ compiler can
// include this file (tests/test_walk_order_cpu.py compiles it with the system compiler), rsa_attn.h includes it for the kernels.
#pragma once

#if defined(__HIPCC__)
#define RSA_WALK_FN __host__ __device__ __forceinline__
#else
#define RSA_WALK_FN static inline
#endif

enum { WALK_NONE = 0, WALK_SPARSE = 1, WALK_TEXT = 2 };
enum { RSA_ORDER_PAD = 0xFFFF };   // entry of the order table that is no unit (a padding workgroup)

// The eighth map (no order table): the j-th of a head's NBp sparse workgroups runs on XCD j & 7, which takes the (j & 7)-th
// contiguous eighth of the head's units.
RSA_WALK_FN int rsa_walk_unit(int j, int NBp) { return (j & 7) * (NBp >> 3) + (j >> 3); }
// ... and its inverse: the j at which the eighth map walks `unit`
RSA_WALK_FN int rsa_walk_unit_inv(int unit, int NBp) { return (unit % (NBp >> 3)) * 8 + unit / (NBp >> 3); }

// Run mapping (with an order table; the sparse units start at work index 0).  The whole walks of a launch -- the work indices
// [0, n_whole): all BH * NBp sparse units, or those in front of a split tail -- form one sequence of positions, head after head and
// inside a head in the table's order.  Workgroup v runs on XCD v & 7 as the (v >> 3)-th that XCD receives, `gen` of them at a
// time: the gen slots of (generation g, XCD x) take the RUN of gen consecutive positions (g * 8 + x) * gen .., so that the walks an
// XCD holds together are neighbours in the sequence -- of one head wherever a run does not straddle a head boundary, and, where
// the table sorts by mean kept key block, of nearby key ranges.  Behind the last full generation of 8 * gen positions p = v.
// A bijection of [0, n_whole) for every gen.
RSA_WALK_FN int rsa_walk_pos(int v, int n_whole, int gen) {
    const int per = 8 * gen;
    if (v >= n_whole / per * per) return v;
    const int xcd = v & 7, n = v >> 3, g = n / gen, i = n % gen;
    return (g * 8 + xcd) * gen + i;
}

// Sparse workgroup v -> its head and unit (>= the head's unit count: a padding workgroup).  order: u16 [BH, NBp], rank -> unit, or
// null = the eighth map.  The pieces of a split tail (v >= n_whole) ALWAYS walk the units of the eighth map: which units are split
// does not depend on the table, whose ranks in front of the tail hold the head's other units (walk_order_sort_kernel, rsa_attn.hip;
// RSA_ORDER_PAD where there are fewer of them than ranks).
RSA_WALK_FN int rsa_walk_sparse(const unsigned short* order, int v, int n_whole, int NBp, int gen, int& bh) {
    if (!order || v >= n_whole) {
        bh = v / NBp;
        return rsa_walk_unit(v % NBp, NBp);
    }
    const int p = rsa_walk_pos(v, n_whole, gen);
    bh = p / NBp;
    return order[p];    // (p = bh * NBp + rank)
}

// The whole map, on any struct with WalkArgs' plan members (rsa_attn.h): returns what the workgroup walks (WALK_NONE = padding
// workgroup).  ORDERED = false compiles the table's form out (kernels that are never given one).
template <bool ORDERED, typename A>
RSA_WALK_FN int rsa_walk_map_t(const A& a, int work, int n_units, int& bh, int& unit, int& tsp, int& tail) {
    tsp = 0;
    tail = -1;
    const int n_sparse = a.BH * a.NBp;
    const bool heavy_last = a.heavy_last != 0;
    int wh = heavy_last ? work - n_sparse : work;                 // index among the text-row pieces
    int v = heavy_last ? work : work - a.n_heavy_pad;             // index among the sparse units
    bool text = heavy_last ? work >= n_sparse : work < a.n_heavy_pad;
    if (a.tail_n > 0) {
        const int tail_end = a.tail_first + a.tail_n * a.tail_p;
        text = work >= tail_end;
        wh = work - tail_end;
        if (work >= a.tail_first && !text) {
            tail = work - a.tail_first;
            v = a.tail_first + tail / a.tail_p;
            tsp = tail % a.tail_p;
        }
    }
    if (text) {
        const int ntq = a.NQB - a.NBv;
        const int per_bh = ntq * a.tsplit;      // text blocks x key-range splits (tsplit = 1: no split)
        if (ntq <= 0 || wh >= a.BH * per_bh) return WALK_NONE;
        bh = wh / per_bh;
        const int rem = wh % per_bh;
        unit = a.NBv + rem / a.tsplit;
        tsp = rem % a.tsplit;
    } else {
        unit = rsa_walk_sparse(ORDERED ? a.order : nullptr, v, a.tail_n > 0 ? a.tail_first : n_sparse, a.NBp, a.gsync_gen, bh);
        if (unit >= n_units) return WALK_NONE;
    }
    return text ? WALK_TEXT : WALK_SPARSE;
}
