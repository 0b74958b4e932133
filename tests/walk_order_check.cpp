// Host check of the K5 work mapping (rectified_spaattn_amd/csrc/rsa_walk_order.h), compiled by tests/test_walk_order_cpu.py with the
// system C++ compiler: every grid index of a launch is mapped and the result counted.  Prints one line per failure; exit code 1
// if there was one.
#include <cstdio>
#include <map>
#include <tuple>
#include <vector>

#include "rsa_walk_order.h"

struct Plan {   // the members of WalkArgs that rsa_walk_map_t reads
    int BH, NBp, NBv, NQB, heavy_last, n_heavy_pad, tail_first, tail_n, tail_p, tsplit, gsync_gen;
    const unsigned short* order;
};

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures < 40) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static unsigned rnd_state = 12345u;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

// the host plan's arithmetic (rsa_plan_walk): text pieces last, tail split of the last partial generation of 512
static Plan make_plan(int BH, int NBv, int gen, bool text, bool want_tail, long* nblocks, bool* has_tail) {
    Plan a{};
    a.BH = BH; a.NBv = NBv; a.NBp = (NBv + 7) & ~7; a.gsync_gen = gen;
    const int ntq = text ? 2 : 0;
    a.NQB = NBv + ntq;
    a.tsplit = text ? 4 : 1;
    const int n_heavy = BH * ntq * a.tsplit;
    a.heavy_last = text;
    a.n_heavy_pad = (n_heavy + 7) & ~7;
    const long n_sparse = (long)BH * a.NBp;
    *nblocks = a.n_heavy_pad + n_sparse;
    *has_tail = false;
    if (want_tail) {
        const long full = n_sparse / 512, T = n_sparse % 512, room = 512 - a.n_heavy_pad;
        const long P = T > 0 ? (room / T < 4 ? room / T : 4) : 0;
        if (full >= 1 && T > 0 && P >= 2) {
            a.tail_first = (int)(full * 512); a.tail_n = (int)T; a.tail_p = (int)P;
            *nblocks = (long)a.tail_first + T * P + a.n_heavy_pad;
            *has_tail = true;
        }
    }
    return a;
}

template <bool ORDERED>
static void check_case(int BH, int NBv, int gen, bool text, bool want_tail, int table, int* tails_seen) {
    long nblocks;
    bool has_tail;
    Plan a = make_plan(BH, NBv, gen, text, want_tail, &nblocks, &has_tail);
    if (has_tail) ++*tails_seen;
    const int n_sparse = BH * a.NBp;
    // table: 0 = none, 1 = index order, 2 = a random order per head.  As walk_order_sort_kernel builds it: the ranks of a head in front
    // of the split tail (work index n_whole) hold the units the eighth map does NOT walk in pieces, pads behind them; the ranks of the
    // tail hold the eighth map's units.
    const int n_whole = has_tail ? a.tail_first : n_sparse;
    std::vector<unsigned short> order((size_t)n_sparse, (unsigned short)RSA_ORDER_PAD);
    for (int bh = 0; bh < BH; ++bh) {
        unsigned short* o = order.data() + (size_t)bh * a.NBp;
        const int left = n_whole - bh * a.NBp, r0 = left < 0 ? 0 : (left < a.NBp ? left : a.NBp);
        int cnt = 0;
        for (int u = 0; u < NBv; ++u)
            if (rsa_walk_unit_inv(u, a.NBp) < r0) o[cnt++] = (unsigned short)u;
        CHECK(cnt <= r0, "BH %d NBv %d: %d whole units for %d ranks", BH, NBv, cnt, r0);
        CHECK(NBv == 0 || rsa_walk_unit(rsa_walk_unit_inv(NBv - 1, a.NBp), a.NBp) == NBv - 1, "inverse of the eighth map");
        if (table == 2)
            for (int r = cnt - 1; r > 0; --r) { const int x = (int)(rnd() % (unsigned)(r + 1)); const unsigned short tmp = o[r]; o[r] = o[x]; o[x] = tmp; }
        for (int r = r0; r < a.NBp; ++r) { const int u = rsa_walk_unit(r, a.NBp); o[r] = (unsigned short)(u < NBv ? u : RSA_ORDER_PAD); }
    }
    a.order = table ? order.data() : nullptr;
    const bool ordered = ORDERED && table != 0;
#define TAG "BH %d NBv %d gen %d text %d tail %d table %d ordered %d: "
#define TAGV BH, NBv, gen, (int)text, (int)has_tail, table, (int)ORDERED

    std::map<std::tuple<int, int>, int> whole;                  // (bh, unit) -> walks of the whole list
    std::map<std::tuple<int, int>, std::vector<int>> pieces;    // (bh, unit) -> tail pieces seen
    std::map<std::tuple<int, int, int>, int> texts;             // (bh, text unit, piece)
    long none_sparse = 0;
    for (long work = 0; work < nblocks; ++work) {
        int bh = -1, unit = -1, tsp = -1, tail = -2;
        const int kind = rsa_walk_map_t<ORDERED>(a, (int)work, NBv, bh, unit, tsp, tail);
        const bool in_text = has_tail ? work >= a.tail_first + a.tail_n * a.tail_p : work >= n_sparse;
        if (kind == WALK_TEXT) {
            CHECK(in_text && unit >= NBv && unit < a.NQB && bh >= 0 && bh < BH && tsp >= 0 && tsp < a.tsplit, TAG "text work %ld -> bh %d unit %d tsp %d", TAGV, work, bh, unit, tsp);
            ++texts[std::make_tuple(bh, unit, tsp)];
            continue;
        }
        if (in_text) { CHECK(kind == WALK_NONE, TAG "text pad %ld is kind %d", TAGV, work, kind); continue; }
        // what the issue's arithmetic gives for this sparse work index
        const int v = tail >= 0 ? a.tail_first + tail / a.tail_p : (int)work;
        CHECK((tail >= 0) == (has_tail && work >= a.tail_first), TAG "work %ld tail %d", TAGV, work, tail);
        int want_bh, want_unit;
        if (ordered && tail < 0) {
            int p = v;
            const int per = 8 * gen;
            if (v < n_whole / per * per) {
                const int xcd = v & 7, n = v >> 3, g = n / gen, i = n % gen;
                p = (g * 8 + xcd) * gen + i;
            }
            want_bh = p / a.NBp;
            want_unit = order[(size_t)want_bh * a.NBp + p % a.NBp];
        } else {
            want_bh = v / a.NBp;
            want_unit = rsa_walk_unit(v % a.NBp, a.NBp);     // k5_walk_order = 0, and every piece of a split tail: the eighth map
        }
        CHECK(bh == want_bh, TAG "work %ld bh %d, expected %d", TAGV, work, bh, want_bh);
        if (kind == WALK_NONE) {
            CHECK(want_unit >= NBv, TAG "work %ld is padding, expected unit %d", TAGV, work, want_unit);
            ++none_sparse;
            continue;
        }
        CHECK(kind == WALK_SPARSE && unit == want_unit && unit >= 0 && unit < NBv, TAG "work %ld -> unit %d, expected %d", TAGV, work, unit, want_unit);
        if (tail >= 0) {
            CHECK(tsp == tail % a.tail_p, TAG "work %ld piece %d of tail %d", TAGV, work, tsp, tail);
            pieces[std::make_tuple(bh, unit)].push_back(tsp);
        } else {
            CHECK(tsp == 0, TAG "work %ld whole walk with piece %d", TAGV, work, tsp);
            ++whole[std::make_tuple(bh, unit)];
        }
    }
    // every (bh, unit) exactly once as a whole walk, or exactly tail_p times as the pieces 0 .. tail_p - 1
    for (int bh = 0; bh < BH; ++bh)
        for (int u = 0; u < NBv; ++u) {
            const auto key = std::make_tuple(bh, u);
            const int w = whole.count(key) ? whole[key] : 0;
            const auto pc = pieces.find(key);
            if (pc == pieces.end()) { CHECK(w == 1, TAG "(bh %d, unit %d) walked %d times", TAGV, bh, u, w); continue; }
            CHECK(w == 0, TAG "(bh %d, unit %d) walked whole AND in pieces", TAGV, bh, u);
            std::vector<int> seen((size_t)a.tail_p, 0);
            for (int p : pc->second) if (p >= 0 && p < a.tail_p) ++seen[(size_t)p];
            bool ok = (int)pc->second.size() == a.tail_p;
            for (int c : seen) ok = ok && c == 1;
            CHECK(ok, TAG "(bh %d, unit %d): %d pieces", TAGV, bh, u, (int)pc->second.size());
        }
    const long pad_groups = (long)BH * (a.NBp - NBv);
    if (!has_tail) CHECK(none_sparse == pad_groups, TAG "%ld padding workgroups, expected %ld", TAGV, none_sparse, pad_groups);
    for (int bh = 0; bh < BH && text; ++bh)
        for (int u = NBv; u < a.NQB; ++u)
            for (int p = 0; p < a.tsplit; ++p) {
                const auto key = std::make_tuple(bh, u, p);
                CHECK(texts.count(key) && texts[key] == 1, TAG "text piece (bh %d, unit %d, %d)", TAGV, bh, u, p);
            }
    // the gen slots of one (generation, XCD) take gen consecutive positions; the positions are a bijection of the whole walks
    std::vector<int> hit((size_t)n_whole, 0);
    for (int v = 0; v < n_whole; ++v) {
        const int p = rsa_walk_pos(v, n_whole, gen);
        CHECK(p >= 0 && p < n_whole, TAG "position %d of %d", TAGV, p, v);
        if (p >= 0 && p < n_whole) ++hit[(size_t)p];
    }
    for (int p = 0; p < n_whole; ++p) CHECK(hit[(size_t)p] == 1, TAG "position %d taken %d times", TAGV, p, hit[(size_t)p]);
    for (int g = 0; g < n_whole / (8 * gen); ++g)
        for (int x = 0; x < 8; ++x) {
            const int p0 = rsa_walk_pos((g * gen) * 8 + x, n_whole, gen);
            for (int i = 0; i < gen; ++i)
                CHECK(rsa_walk_pos((g * gen + i) * 8 + x, n_whole, gen) == p0 + i, TAG "generation %d XCD %d slot %d", TAGV, g, x, i);
        }
    for (int v = n_whole / (8 * gen) * (8 * gen); v < n_whole; ++v) CHECK(rsa_walk_pos(v, n_whole, gen) == v, TAG "last position %d", TAGV, v);
}

int main() {
    const int BHs[] = {1, 3, 24}, NBvs[] = {1, 7, 165, 168, 902}, gens[] = {32, 64, 128};   // (128: a generation that does not divide the 512 the tail is cut at)
    int cases = 0, tails = 0;
    for (int BH : BHs)
        for (int NBv : NBvs)
            for (int gen : gens)
                for (int text = 0; text < 2; ++text)
                    for (int tail = 0; tail < 2; ++tail)
                        for (int table = 0; table < 3; ++table) {
                            check_case<true>(BH, NBv, gen, text != 0, tail != 0, table, &tails);
                            check_case<false>(BH, NBv, gen, text != 0, tail != 0, table, &tails);   // a kernel that is never given a table
                            cases += 2;
                        }
    if (tails < 36) { std::printf("only %d cases had a tail split\n", tails); ++failures; }
    std::printf("%d cases, %d with a tail split, %d failures\n", cases, tails, failures);
    return failures ? 1 : 0;
}
