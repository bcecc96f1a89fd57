// Rooted subgraph search over sorted neighbour lists: the arithmetic core of the sparse counting kernel (count_sparse.hip), for the graphs
// that the LDS-resident kernel (count.hip / count_core.h) refuses: more than 768 vertices, tables beyond 160 KiB of LDS, 65 535 columns.
//
// Shared between the HIP kernel and host-side harnesses used ONLY by tests (tests/sparse_harness.cpp and tests/sparse_directed_harness.cpp
// compile this header with g++; they are not a product fallback).  Everything is integer arithmetic; results are exact.
//
// The graph is a CSR of neighbour lists: the neighbours of vertex v are nbr[row_ptr[v] .. row_ptr[v + 1]), 32-bit vertex ids, STRICTLY
// increasing -- no duplicate entries and no self loops (the set-up pass, or the harness, removes both).  Vertex ids are whatever the
// caller numbers the rows of row_ptr with (batch-global in the kernel): only their order within one graph matters, and an offset keeps it.
//
// One lane runs one rooted search of one plan of the packed plan table (gsn_internal.h).  Only the per-level masks
// adj | nonadj << 8 | gt << 16 | lt << 24 of levels n_fixed .. k - 1 are read: they define the result completely.  min_degree, the distance
// bytes and the cores of the LDS kernel only prune work and are ignored here.  Closed forms of the plan's tail (patterns.cpp:
// plan_tail_mode) that are honoured because they are cheap on lists: mode 2 (twin levels: C(|C|, r)) and mode 1 (independent last levels:
// |C1| |C2| - |C1 & C2|); mode 3 (chain) runs the generic search.
//
// Directed plans (header[6] & 2, vertex mode; the functions' DIR = true).  The graph has two lists per vertex, both strictly increasing and
// without self loops: row v of the CSR holds the OUT-neighbours of v, row in_base + v its IN-neighbours (in_base = 0: an undirected graph,
// one list per vertex), so sp_find serves both by an offset.  Level masks:
//   plan[2 + l]                  adjacency bit j: the image of level l is an OUT-neighbour of f_j (pattern arc j -> l); non-adjacency bit j:
//                                it is not; gt / lt as in an undirected plan
//   plan[PLAN_STRIDE_WORDS + l]  in_adj | in_nonadj << 8: the same for IN-neighbours of f_j (pattern arc l -> j)
// and the plans lie plan_stride(header[6]) = PLAN_STRIDE_DIRECTED words apart.  A level takes its candidates from the shortest list among
// the out-lists named by the adjacency mask and the in-lists named by the in-adjacency mask, and checks every remaining bit of both words by
// binary search in the matching list; with neither mask it walks the graph's vertices.  Closed-form tails: modes 1 and 2 are honoured, with
// the candidate sets counted under both words.  Their derivations hold because the plan compiler only emits them for a directed plan when
// they do: mode 1 when NEITHER word of the last level names level k - 2 (patterns.cpp: plan_tail_mode, in_ref), mode 2 when the twin levels
// are equal in BOTH words and neither word of one names the other (twin_link: level_in[b] == level_in[a], in_ref) -- the two candidate sets
// are then fixed once the levels above are placed, exactly as in the undirected case; mode 3 is never emitted for a directed plan.  The
// oracle decides: tests/test_count_sparse_directed_cpu.py compares every cell.
//
// The search is an iterative depth-first walk (no recursion).  Level l takes its candidates from the neighbour list of ONE earlier image named by its
// adjacency mask (the anchor: the one with the shortest list), rejects a candidate equal to an earlier image, checks the other adjacency
// bits by binary search in the earlier images' lists, the non-adjacency bits by a failing binary search, and gt / lt by comparison.  A level
// with an empty adjacency mask (a disconnected pattern; none of the pattern families of the reference has one) walks all vertices of the
// graph instead.  The last level is counted, never descended into.
//
// Per-lane state: for each level 0 .. 7 the image, the cursor and the end of its candidate list, and the masks still to check (the
// level's masks without the anchor's adjacency bit): SP_FIELDS * SP_LEVELS words at st[(field * SP_LEVELS + level) * ss] -- ss = 1 for a
// plain array (host), ss = the lane count with st pointing at the lane's own word of a lane-interleaved LDS array (device).  A directed
// search keeps the in-masks still to check in a fifth field (SP_CHK_IN; SP_FIELDS_DIRECTED * SP_LEVELS words): SP_CHK has no bit free, and
// an undirected search neither reads nor reserves the field.
//
// Plan width.  Every function below takes the format of the plan table as its last template parameter, a struct of four numbers: the
// levels that hold a slot, the width of a mask field, the words per level and the plan stride.  The default, SpNarrow, is the table of
// patterns of at most GSN_KMAX = 9 vertices described above.  SpWide is the wide table (gsn_internal.h: PLAN_MAGIC_WIDE) of pattern lists
// with 10 .. GSN_KMAX_WIDE = 16 vertices: 15 levels with a slot, 16-bit fields, adj | nonadj << 16 at plan[2 + l], gt | lt << 16 in a second
// word at plan[PLAN_WIDE_ORD_OFF + l] and, directed, in_adj | in_nonadj << 16 in a third at plan[PLAN_WIDE_IN_OFF + l].  The order word of
// a level never changes during a search (only an adjacency bit, the anchor's, is ever struck), so a wide search reads it from the plan at
// every turn and keeps the same four (directed: five) state fields per level: (4 or 5) * 15 words per lane.  Anchor choice, binary-search
// checks, the closed-form tails and the edge-mode row rules are the same code for both formats.
#pragma once

#include <stdint.h>

#include "count_core.h"

namespace gsn {

constexpr int SP_LEVELS = 8;          // levels that hold an image or a cursor: 0 .. k - 2 with k <= GSN_KMAX = 9
constexpr int SP_LEVELS_WIDE = 15;    // the same of a wide plan: k <= GSN_KMAX_WIDE = 16
enum { SP_IMG = 0, SP_CUR = 1, SP_END = 2, SP_CHK = 3, SP_FIELDS = 4, SP_CHK_IN = 4, SP_FIELDS_DIRECTED = 5 };
static_assert(GSN_KMAX - 1 <= SP_LEVELS, "the last level is counted, every earlier one has a slot");
static_assert(GSN_KMAX_WIDE - 1 <= SP_LEVELS_WIDE, "the last level is counted, every earlier one has a slot");

// the format of a plan table: LEVELS with a slot, BITS per mask field, WORDS per level (undirected; a directed plan has one more), and the
// plan STRIDE (undirected / directed)
template <int LEVELS_, int BITS_, int WORDS_, int STRIDE_, int STRIDE_DIRECTED_>
struct SpFormat {
    static constexpr int LEVELS = LEVELS_, BITS = BITS_, WORDS = WORDS_, STRIDE = STRIDE_, STRIDE_DIRECTED = STRIDE_DIRECTED_;
    static constexpr uint32_t MASK = (1u << BITS_) - 1u;
    static constexpr bool ORD_WORD = WORDS_ > 1;                          // gt | lt in a word of their own (else in the upper half of the first)
    static constexpr int ORD_OFF = (STRIDE_ - 2) / WORDS_ + 2;            // wide: plan[ORD_OFF + l]
    static constexpr int IN_OFF = STRIDE_;                                // directed: plan[IN_OFF + l]
};
using SpNarrow = SpFormat<SP_LEVELS, 8, 1, PLAN_STRIDE_WORDS, PLAN_STRIDE_DIRECTED>;
using SpWide = SpFormat<SP_LEVELS_WIDE, 16, 2, PLAN_STRIDE_WIDE, PLAN_STRIDE_WIDE_DIRECTED>;
static_assert(SpWide::ORD_OFF == PLAN_WIDE_ORD_OFF && SpWide::IN_OFF == PLAN_WIDE_IN_OFF, "the wide record of gsn_internal.h");
static_assert(SpNarrow::IN_OFF == PLAN_STRIDE_WORDS, "the narrow record of gsn_internal.h");

struct SparseGraph {
    const uint32_t *row_ptr;   // [n + 1] over the caller's vertex numbering; directed: [in_base + n + 1]
    const uint32_t *nbr;       // strictly increasing within a row
    uint32_t v_lo, v_hi;       // the vertices of the graph the roots lie in (walked only by a level without an adjacency mask)
    uint32_t in_base = 0;      // directed: row in_base + v holds the in-neighbours of v, row v its out-neighbours
};

#define GSN_SP(F, L) st[((F) * FMT::LEVELS + (L)) * ss]

// position of b in row a, or -1
GSN_HD int64_t sp_find(const SparseGraph &g, uint32_t a, uint32_t b) {
    uint32_t lo = g.row_ptr[a], hi = g.row_ptr[a + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t x = g.nbr[mid];
        if (x == b) return (int64_t)mid;
        if (x < b) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// does v satisfy the masks `chk` (and, directed, the in-masks `chk_in`) against the images of the levels they name?  `ord`: the order
// word of a format that has one (else the order masks are the upper half of `chk`)
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD bool sp_masks_hold(const SparseGraph &g, const uint32_t *st, int ss, uint32_t chk, uint32_t chk_in, uint32_t ord, uint32_t v) {
    uint32_t m = chk & FMT::MASK;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        if (sp_find(g, GSN_SP(SP_IMG, j), v) < 0) return false;
    }
    m = (chk >> FMT::BITS) & FMT::MASK;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        if (sp_find(g, GSN_SP(SP_IMG, j), v) >= 0) return false;
    }
    if (DIR) {
        m = chk_in & FMT::MASK;
        while (m) {
            const int j = ctz64(m);
            m &= m - 1u;
            if (sp_find(g, g.in_base + GSN_SP(SP_IMG, j), v) < 0) return false;
        }
        m = (chk_in >> FMT::BITS) & FMT::MASK;
        while (m) {
            const int j = ctz64(m);
            m &= m - 1u;
            if (sp_find(g, g.in_base + GSN_SP(SP_IMG, j), v) >= 0) return false;
        }
    }
    m = FMT::ORD_WORD ? ord & FMT::MASK : (chk >> 16) & 0xffu;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        if (!(v > GSN_SP(SP_IMG, j))) return false;
    }
    m = FMT::ORD_WORD ? ord >> FMT::BITS : chk >> 24;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        if (!(v < GSN_SP(SP_IMG, j))) return false;
    }
    return true;
}

// candidate of a level with the images of levels 0 .. nimg - 1 placed: distinct from all of them, and the masks hold
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD bool sp_accept(const SparseGraph &g, const uint32_t *st, int ss, uint32_t chk, uint32_t chk_in, uint32_t ord, int nimg, uint32_t v) {
    for (int j = 0; j < nimg; ++j)
        if (GSN_SP(SP_IMG, j) == v) return false;
    return sp_masks_hold<DIR, FMT>(g, st, ss, chk, chk_in, ord, v);
}

// the candidate list of a level with masks `desc` (directed: and in-masks `din`): positions cur .. end of nbr (or vertex ids, when the
// level has no adjacency mask in either word), and the masks that remain to be checked per candidate
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD void sp_open(const SparseGraph &g, const uint32_t *st, int ss, uint32_t desc, uint32_t din, uint32_t &cur, uint32_t &end, uint32_t &chk,
                    uint32_t &chk_in) {
    uint32_t m = desc & FMT::MASK;
    chk_in = din;
    if (!m && !(DIR && (din & FMT::MASK))) { cur = g.v_lo; end = g.v_hi; chk = desc; return; }
    int best = -1;
    uint32_t blen = 0, bcur = 0;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        const uint32_t a = GSN_SP(SP_IMG, j), lo = g.row_ptr[a], len = g.row_ptr[a + 1] - lo;
        if (best < 0 || len < blen) { best = j; blen = len; bcur = lo; }
    }
    if (DIR) {
        m = din & FMT::MASK;
        while (m) {
            const int j = ctz64(m);
            m &= m - 1u;
            const uint32_t a = g.in_base + GSN_SP(SP_IMG, j), lo = g.row_ptr[a], len = g.row_ptr[a + 1] - lo;
            if (best < 0 || len < blen) { best = FMT::BITS + j; blen = len; bcur = lo; }
        }
    }
    cur = bcur; end = bcur + blen;
    if (DIR && best >= FMT::BITS) { chk = desc; chk_in = din & ~(1u << (best - FMT::BITS)); }
    else chk = desc & ~(1u << best);
}
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD uint32_t sp_at(const SparseGraph &g, uint32_t desc, uint32_t din, uint32_t pos) {
    return ((desc & FMT::MASK) || (DIR && (din & FMT::MASK))) ? g.nbr[pos] : pos;
}

// number of candidates of a level with masks `desc` / `din` / `ord` (images 0 .. nimg - 1 placed) that, with `both`, also satisfy
// `desc2` / `din2` / `ord2`
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD uint64_t sp_count_level(const SparseGraph &g, const uint32_t *st, int ss, uint32_t desc, uint32_t din, uint32_t ord, int nimg,
                               bool both = false, uint32_t desc2 = 0, uint32_t din2 = 0, uint32_t ord2 = 0) {
    uint32_t cur, end, chk, chk_in;
    sp_open<DIR, FMT>(g, st, ss, desc, din, cur, end, chk, chk_in);
    uint64_t c = 0;
    for (; cur < end; ++cur) {
        const uint32_t v = sp_at<DIR, FMT>(g, desc, din, cur);
        if (!sp_accept<DIR, FMT>(g, st, ss, chk, chk_in, ord, nimg, v)) continue;
        if (both && !sp_masks_hold<DIR, FMT>(g, st, ss, desc2, din2, ord2, v)) continue;
        ++c;
    }
    return c;
}

// One rooted search, resumable: sp_begin places the roots, every sp_step runs one turn of the walk (opens a level -- or counts it, when it
// is the last or the head of a closed-form tail -- or tries one candidate), s.l < 0 = finished, s.cnt holds the maps.  The kernel's lanes
// interleave turns of different searches; sp_search is the same thing run to the end.
struct SparseLane {
    const uint32_t *plan;
    int k, nfix, tm, tl;      // tail mode honoured by this search (0: none) and the level it starts at
    int l;                    // level being opened or consumed; < 0: no search in progress
    bool enter;               // level l is to be opened
    uint64_t cnt;             // accumulates over the plans of a cell
};

// the roots: r0 = level 0, r1 = level 1 (plans with two fixed levels)
template <class FMT = SpNarrow>
GSN_HD void sp_begin(SparseLane &s, const uint32_t *plan, uint32_t r0, uint32_t r1, uint32_t *st, int ss) {
    s.plan = plan;
    s.k = (int)(plan[0] & 0xffu); s.nfix = (int)((plan[0] >> 8) & 0xffu);
    GSN_SP(SP_IMG, 0) = r0;
    if (s.nfix > 1) GSN_SP(SP_IMG, 1) = r1;
    s.l = -1;
    if (s.nfix >= s.k) { s.cnt += 1; return; }
    s.tm = plan_tail(plan); s.tl = -1;
    if (s.tm == 2) s.tl = plan_tail_level(plan, s.k);
    if (s.tm == 1) s.tl = s.k - 2;
    if (s.tl < s.nfix) s.tm = 0;                 // (mode 3, or a tail that starts inside the roots: the generic walk)
    s.l = s.nfix;
    s.enter = true;
}

template <bool DIR = false, class FMT = SpNarrow>
GSN_HD void sp_step(const SparseGraph &g, SparseLane &s, uint32_t *st, int ss) {
    const int l = s.l, k = s.k;
    const uint32_t desc = s.plan[2 + l], din = DIR ? s.plan[FMT::IN_OFF + l] : 0u, ord = FMT::ORD_WORD ? s.plan[FMT::ORD_OFF + l] : 0u;
    if (s.enter) {
        s.enter = false;
        if (l == k - 1) {
            s.cnt += sp_count_level<DIR, FMT>(g, st, ss, desc, din, ord, l);
        } else if (s.tm == 2 && l == s.tl) {     // r twin levels: any r of the candidates, in one order
            const uint64_t n1 = sp_count_level<DIR, FMT>(g, st, ss, desc, din, ord, l);
            const int r = 2 + (int)(s.plan[1] >> 30);
            if (n1 >= (uint64_t)r) {
                uint64_t c = 1;
                for (int i = 0; i < r; ++i) c = c * (n1 - (uint64_t)i) / (uint64_t)(i + 1);     // (exact at every step)
                s.cnt += c;
            }
        } else if (s.tm == 1 && l == s.tl) {     // the last level's masks do not name level k - 2: pairs minus the coinciding ones
            const uint32_t d2 = s.plan[2 + k - 1], d2in = DIR ? s.plan[FMT::IN_OFF + k - 1] : 0u;
            const uint32_t ord2 = FMT::ORD_WORD ? s.plan[FMT::ORD_OFF + k - 1] : 0u;
            const uint64_t n1 = sp_count_level<DIR, FMT>(g, st, ss, desc, din, ord, l);
            if (n1)
                s.cnt += n1 * sp_count_level<DIR, FMT>(g, st, ss, d2, d2in, ord2, l) -
                         sp_count_level<DIR, FMT>(g, st, ss, desc, din, ord, l, true, d2, d2in, ord2);
        } else {
            uint32_t cur, end, chk, chk_in;
            sp_open<DIR, FMT>(g, st, ss, desc, din, cur, end, chk, chk_in);
            GSN_SP(SP_CUR, l) = cur; GSN_SP(SP_END, l) = end; GSN_SP(SP_CHK, l) = chk;
            if (DIR) GSN_SP(SP_CHK_IN, l) = chk_in;
            return;
        }
        s.l = l - 1 < s.nfix ? -1 : l - 1;       // counted: back to the level above
        return;
    }
    const uint32_t cur = GSN_SP(SP_CUR, l);
    if (cur >= GSN_SP(SP_END, l)) {
        s.l = l - 1 < s.nfix ? -1 : l - 1;
        return;
    }
    GSN_SP(SP_CUR, l) = cur + 1;
    const uint32_t v = sp_at<DIR, FMT>(g, desc, din, cur);
    if (!sp_accept<DIR, FMT>(g, st, ss, GSN_SP(SP_CHK, l), DIR ? GSN_SP(SP_CHK_IN, l) : 0u, ord, l, v)) return;
    GSN_SP(SP_IMG, l) = v;
    s.l = l + 1;
    s.enter = true;
}

// the number of maps of one plan
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD uint64_t sp_search(const SparseGraph &g, const uint32_t *plan, uint32_t r0, uint32_t r1, uint32_t *st, int ss) {
    SparseLane s;
    s.cnt = 0; s.tm = 0; s.tl = -1;
    sp_begin<FMT>(s, plan, r0, r1, st, ss);
    while (s.l >= 0) sp_step<DIR, FMT>(g, s, st, ss);
    return s.cnt;
}

// one cell: the plans col_ptr[col] .. col_ptr[col + 1] of the table all add to output column `col`.  DIR must agree with the table's
// header (table[6] & 2): it sets the plan stride and the size of st (SP_FIELDS_DIRECTED * FMT::LEVELS words, else SP_FIELDS * FMT::LEVELS);
// FMT must agree with its magic word
template <bool DIR = false, class FMT = SpNarrow>
GSN_HD uint64_t sp_cell(const SparseGraph &g, const uint32_t *table, int col, uint32_t r0, uint32_t r1, uint32_t *st, int ss) {
    constexpr int stride = DIR ? FMT::STRIDE_DIRECTED : FMT::STRIDE;
    const uint32_t *col_ptr = table + PLAN_HEADER_WORDS;
    const uint32_t *plans = table + table[7];
    uint64_t cnt = 0;
    for (uint32_t p = col_ptr[col]; p < col_ptr[col + 1]; ++p) cnt += sp_search<DIR, FMT>(g, plans + (size_t)p * stride, r0, r1, st, ss);
    return cnt;
}

// Edge mode: what the lane that draws column c = (u, v) does with the row.  arc_col[slot] = the LAST column that holds the arc of that
// slot of nbr (utils_graph_processing.py:142-144: the last duplicate carries the counts), -1 = none.
//   SP_ROW_ZERO    the row carries nothing: a self loop, an earlier duplicate
//   SP_ROW_MIRROR  undirected orbit classes (sym) and u > v with the reverse column present: that column's lane writes this row too
//   SP_ROW_SEARCH  search; `mirror` = the reverse column to write as well (sym), else -1; `rev_missing`: a non-zero count is a KeyError
enum { SP_ROW_ZERO = 0, SP_ROW_MIRROR = 1, SP_ROW_SEARCH = 2 };
GSN_HD int sp_edge_row(const SparseGraph &g, const int32_t *arc_col, int64_t c, uint32_t u, uint32_t v, bool sym, int64_t &mirror, bool &rev_missing) {
    mirror = -1; rev_missing = false;
    if (u == v) return SP_ROW_ZERO;
    const int64_t s = sp_find(g, u, v);
    if (s < 0 || (int64_t)arc_col[s] != c) return SP_ROW_ZERO;
    const int64_t rs = sp_find(g, v, u);          // (the graph is symmetric: the slot exists)
    const int64_t rev = rs < 0 ? -1 : (int64_t)arc_col[rs];
    rev_missing = rev < 0;
    if (sym && rev >= 0) {
        if (u > v) return SP_ROW_MIRROR;
        mirror = rev;
    }
    return SP_ROW_SEARCH;
}

#undef GSN_SP

}  // namespace gsn
