// Per-lane rooted subgraph search: the arithmetic core of the counting kernel.
//
// Shared between the HIP kernel (count.hip) and a host-side logic harness used ONLY by tests
// (tests/host_harness.cpp compiles this header with g++ to check plans + search against the oracle on CPU;
// it is not a product fallback -- the product path launches the HIP kernel or fails).
//
// A "lane" owns one rooted search at a time:
//   * the target graph is a bit matrix A[n][W] of 64-bit words (LDS on device),
//   * the partial map f is packed 8 bits per level into one 64-bit register (n <= 256; 16 bits / two registers above),
//   * a frame per level holds the not-yet-tried candidates of that level (LDS stack on device, lane-interleaved),
//   * one call to lane_step() pops one candidate, and either descends one level or -- at the last-but-one
//     level -- adds popcount(candidates of the last level) to the lane's counter (the last level is never
//     enumerated one by one).
// Everything is integer / bit arithmetic; results are exact.
#pragma once

#include <stdint.h>

#include "gsn_internal.h"

#if defined(__HIPCC__)
#define GSN_HD __host__ __device__ __forceinline__
#else
#define GSN_HD inline
#endif

namespace gsn {

GSN_HD int popc64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}
GSN_HD int ctz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)x) - 1;
#else
    return __builtin_ctzll(x);
#endif
}

// bits strictly below position p, restricted to word wi
GSN_HD uint64_t below_word(int p, int wi) {
    const int pw = p >> 6;
    return wi < pw ? ~0ull : (wi == pw ? ((1ull << (p & 63)) - 1ull) : 0ull);
}

// A column endpoint against its graph's vertex range: is  base <= x < base + width ?  d = x - base where it is.  One 64-bit subtraction,
// then the high word against zero and ONE unsigned 32-bit compare -- not two 64-bit compares (a 64-bit compare is two vector instructions
// and a carry chain on gfx9).  The subtraction wraps (unsigned): an x below base, INT64_MIN included, leaves 2^64 - (base - x), whose high
// word is not zero for every base a batch can have (0 <= base < 2^62); an x of base + 2^32 and more leaves a high word >= 1.  width 0:
// nothing is inside.
GSN_HD bool endpoint_local(const int64_t x, const int64_t base, const uint32_t width, uint32_t &d) {
    const uint64_t diff = (uint64_t)x - (uint64_t)base;
    d = (uint32_t)diff;
    return (uint32_t)(diff >> 32) == 0u && d < width;
}
// the width of [lo, hi) for endpoint_local: an empty or inverted range (a pointer array that is not monotone) holds nothing
GSN_HD uint32_t endpoint_width(const int64_t lo, const int64_t hi) { return hi > lo ? (uint32_t)(hi - lo) : 0u; }

// bit planes of the vertices' degrees inside each d-core: plane p of core d has bit v set iff bit p of |N(v) & core_d| is set (v in core_d);
// layout [CORE_MAX + 1][DEG_PLANES][W] words (n <= 768 < 2^10).  sum_{v in S} deg(v) = sum_p 2^p popc(S & plane_p).
constexpr int DEG_PLANES = 10;

template <int W>
struct Bits {
    uint64_t w[W];
};

template <int W>
GSN_HD int popc(const Bits<W> &b) {
    int c = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) c += popc64(b.w[i]);
    return c;
}

// Packed partial map: the image of level l sits at bits [VB*l, VB*l + VB) with VB = 8 for graphs of <= 256 vertices
// (W <= 4: one 64-bit register for k <= 8) and VB = 16 above (two registers).
template <int W>
struct FVec {
    static constexpr int VB = W <= 4 ? 8 : 16;
    uint64_t lo, hi;   // hi is dead code for VB == 8
};
template <int W>
GSN_HD int fv_get(const FVec<W> &f, int l) {
    if (FVec<W>::VB == 8) return (int)((f.lo >> (8 * l)) & 0xffu);
    const uint64_t w = l < 4 ? f.lo : f.hi;
    return (int)((w >> (16 * (l & 3))) & 0xffffu);
}
template <int W>
GSN_HD void fv_set(FVec<W> &f, int l, int v) {
    if (FVec<W>::VB == 8) {
        f.lo = (f.lo & ~(0xffull << (8 * l))) | ((uint64_t)v << (8 * l));
    } else {
        const int sh = 16 * (l & 3);
        if (l < 4) f.lo = (f.lo & ~(0xffffull << sh)) | ((uint64_t)v << sh);
        else f.hi = (f.hi & ~(0xffffull << sh)) | ((uint64_t)v << sh);
    }
}
template <int W>
GSN_HD FVec<W> fv_roots(int a, int b) {
    FVec<W> f;
    f.lo = (uint64_t)a | ((uint64_t)b << FVec<W>::VB);
    f.hi = 0;
    return f;
}

// Candidate set of level l given the packed partial map fvec (levels 0..l-1 assigned) and the set `used` of their images.
//   desc = adj_mask | nonadj_mask<<8 | gt_mask<<16 | lt_mask<<24  (bit j <-> earlier level j)
//   adj    : candidate must be a neighbour of f_j          (pattern edge)
//   nonadj : candidate must NOT be a neighbour of f_j      (induced matching, pattern non-edge)
//   gt/lt  : symmetry breaking, candidate id must be > / < f_j
// Only the levels named in desc are visited (a cycle or path level has one or two), everything else is covered by
// `valid & ~used` -- the kernel is VALU-issue bound, so the per-step instruction count is what matters.
// `ball` = j | r<<3 (r = 0: none) with `balls` = the r-hop balls of the target graph, radius 2 at balls[v*W], radius 3 at
// balls[(ball_n + v)*W] (nullptr: pruning off -- it never changes the result, only the work).
// DIR (digraph patterns and targets): A holds the OUT-neighbour rows, A_in the IN-neighbour rows, and desc_in =
// in_adj_mask | in_nonadj_mask<<8 names the earlier levels whose image the candidate must (not) have an arc TO.
template <int W, bool DIR = false>
GSN_HD void candidates(Bits<W> &C, uint32_t desc, uint32_t ball, const FVec<W> &fvec, const Bits<W> &used, const uint64_t *A,
                       const uint64_t *valid, const uint64_t *balls, int ball_n, uint32_t desc_in = 0, const uint64_t *A_in = nullptr) {
#pragma unroll
    for (int w = 0; w < W; ++w) C.w[w] = valid[w] & ~used.w[w];
    if (balls && (ball >> 3)) {
        const int fj = fv_get<W>(fvec, (int)(ball & 7u));
        const uint64_t *row = balls + (size_t)(((ball >> 3) == 3 ? ball_n : 0) + fj) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) C.w[w] &= row[w];
    }
    uint32_t m = desc & 0xffu;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        const uint64_t *row = A + fv_get<W>(fvec, j) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) C.w[w] &= row[w];
    }
    m = (desc >> 8) & 0xffu;
    while (m) {
        const int j = ctz64(m);
        m &= m - 1u;
        const uint64_t *row = A + fv_get<W>(fvec, j) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) C.w[w] &= ~row[w];
    }
    if (DIR) {
        m = desc_in & 0xffu;
        while (m) {
            const int j = ctz64(m);
            m &= m - 1u;
            const uint64_t *row = A_in + fv_get<W>(fvec, j) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) C.w[w] &= row[w];
        }
        m = (desc_in >> 8) & 0xffu;
        while (m) {
            const int j = ctz64(m);
            m &= m - 1u;
            const uint64_t *row = A_in + fv_get<W>(fvec, j) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) C.w[w] &= ~row[w];
        }
    }
    m = desc >> 16;
    while (m) {
        const int jj = ctz64(m);
        m &= m - 1u;
        const bool lt = jj >= 8;
        const int fj = fv_get<W>(fvec, jj & 7);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t bl = below_word(fj, w);                       // ids < fj
            C.w[w] &= lt ? bl : ~(bl | ((w == (fj >> 6)) ? (1ull << (fj & 63)) : 0ull));
        }
    }
}

// r-hop balls of vertex v from the adjacency bit matrix: ball2 = v + N(v) + N(N(v)), ball3 = one more hop (needs every
// ball2 first).  One call per vertex; the caller parallelises over v.
template <int W>
GSN_HD void ball_expand(const uint64_t *A, const uint64_t *from /* [n][W] or nullptr: the adjacency itself */, int v, uint64_t *out) {
    Bits<W> acc;
#pragma unroll
    for (int w = 0; w < W; ++w) acc.w[w] = (from ? from[v * W + w] : A[v * W + w]) | ((w == (v >> 6)) ? (1ull << (v & 63)) : 0ull);
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint64_t m = A[v * W + w];
        while (m) {
            const int u = w * 64 + ctz64(m);
            m &= m - 1ull;
#pragma unroll
            for (int x = 0; x < W; ++x) acc.w[x] |= from ? from[u * W + x] : A[u * W + x];
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) out[v * W + w] = acc.w[w];
}

// One peeling round of the d-core: does vertex v (a member of `core`) keep at least d neighbours inside `core`?
template <int W>
GSN_HD bool core_keeps(const uint64_t *A, const uint64_t *core, int v, int d) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) c += popc64(A[v * W + w] & core[w]);
    return c >= d;
}

// degree planes of ONE vertex v of core d (caller: every v of every needed core; planes zeroed before).  `orfn(word_ptr, bit)` sets a bit.
template <int W, class OrFn>
GSN_HD void deg_planes_vertex(const uint64_t *A, const uint64_t *core, int v, uint64_t *planes /* of this core */, OrFn orfn) {
    if (!((core[v >> 6] >> (v & 63)) & 1ull)) return;
    int deg = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) deg += popc64(A[v * W + w] & core[w]);
    for (int p = 0; p < DEG_PLANES; ++p)
        if ((deg >> p) & 1) orfn(planes + p * W + (v >> 6), 1ull << (v & 63));
}

// The last two levels without a closed form, in ONE tight loop instead of one lane_step per image of level k - 2: the last level's candidate
// set minus everything that names level k - 2 is made once (`base`), then every d in C1 costs an AND with its adjacency row (or its
// complement: induced non-edge), the order mask when the two levels are ordered, and a popcount.
// Where the loop pays: graphs of more than 64 vertices (W >= 2), whose candidate sets are long and whose generic step (frame load / store,
// candidates() from scratch) costs several times an iteration of the loop: ER G(128,1000), edge mode 45.7 -> 57.3 k graphs/s.  On
// molecules (W == 1, sets of one or two vertices) the loop only makes a wave's steps uneven -- the headline's counting kernel went from
// 0.249 to 0.271 ms with it -- so there level k - 2 keeps its frame and is stepped through like the levels above.
template <int W>
struct TailLoop { static constexpr bool on = W >= 2; };

template <int W, bool DIR>
GSN_HD uint64_t tail_loop(const Bits<W> &C1, const uint32_t *plan, int k, const FVec<W> &fvec, const Bits<W> &used, const uint64_t *A,
                          const uint64_t *valid, const uint64_t *balls, int ball_n, const uint64_t *A_in) {
    const int a = k - 2;
    const uint32_t bit = 1u << a, d1 = plan[2 + k - 1], d1_in = DIR ? plan[PLAN_STRIDE_WORDS + k - 1] : 0u;
    uint32_t ball = (plan[2 + GSN_KMAX + ((k - 1) >> 2)] >> (8 * ((k - 1) & 3))) & 0xffu;
    if ((ball >> 3) && (int)(ball & 7u) == a) ball = 0;          // (a distance bound never changes the result: dropped when it names level k - 2)
    const bool adj = (d1 & bit) != 0, non = ((d1 >> 8) & bit) != 0, gt = ((d1 >> 16) & bit) != 0, lt = ((d1 >> 24) & bit) != 0;
    const bool adj_in = DIR && (d1_in & bit) != 0, non_in = DIR && ((d1_in >> 8) & bit) != 0;
    Bits<W> base;
    candidates<W, DIR>(base, d1 & ~(bit | (bit << 8) | (bit << 16) | (bit << 24)), ball, fvec, used, A, valid, balls, ball_n,
                       d1_in & ~(bit | (bit << 8)), A_in);
    uint64_t cnt = 0;
#pragma unroll
    for (int wi = 0; wi < W; ++wi) {
        uint64_t m = C1.w[wi];
        while (m) {
            const int d = wi * 64 + ctz64(m);
            m &= m - 1ull;
            const uint64_t *row = A + d * W;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t c = base.w[w];
                if (adj) c &= row[w];
                if (non) c &= ~row[w];
                if (DIR) {
                    const uint64_t rin = A_in[d * W + w];
                    if (adj_in) c &= rin;
                    if (non_in) c &= ~rin;
                }
                const uint64_t self = (w == (d >> 6)) ? (1ull << (d & 63)) : 0ull;
                const uint64_t bl = below_word(d, w);
                if (gt) c &= ~(bl | self);
                if (lt) c &= bl;
                c &= ~self;
                cnt += (uint64_t)popc64(c);
            }
        }
    }
    return cnt;
}

template <int W>
struct Lane {
    int l;          // level whose frame is being consumed; < 0: no search in progress
    int k, nfix;
    FVec<W> fvec;   // partial map, VB bits per level
    uint64_t cnt;   // matches found so far for the current task (accumulates over the task's plans)
    Bits<W> used;   // images of levels 0 .. l-1
    const uint32_t *plan;
    const uint64_t *balls;   // distance-pruning tables of the target graph or nullptr
    int ball_n;              // vertex capacity of one table
    const uint64_t *degp;    // degree bit planes of the cores (plans with a chain tail) or nullptr
    int loop;                // W == 1: the last two levels in tail_loop all the same (dense small graphs: the launcher decides)
#if defined(COUNT_PROF_STEP) && defined(__HIPCC__)
    unsigned long long prof[12];   // wave-level: [0..2] tail_loop cycles / visits / active lanes, [3] its iterations summed over lanes, [4] max iterations per visit summed,
                                   // [5..7] tail_pairs cycles / visits / lanes, [8..10] rest of lane_step (candidates + frames + climb) cycles / visits / lanes
#endif
};
#if defined(COUNT_PROF_STEP) && defined(__HIP_DEVICE_COMPILE__)
#define CP_T0() const unsigned long long cp_t0 = __builtin_amdgcn_s_memtime()
#define CP_ADD(S, I) do { (S).prof[I] += __builtin_amdgcn_s_memtime() - cp_t0; (S).prof[(I) + 1] += 1; (S).prof[(I) + 2] += (unsigned long long)__popcll(__ballot(1)); } while (0)
#else
#define CP_T0()
#define CP_ADD(S, I)
#endif

// core index of a plan: images must lie in the min-degree(H) core of the target; cores 0..CORE_MAX are tabulated
// (core d for d > CORE_MAX uses core CORE_MAX, a superset)
constexpr int CORE_MAX = 4;
GSN_HD int plan_core(const uint32_t *plan) {
    const int d = (int)((plan[1] >> 20) & 0xfu);
    return d > CORE_MAX ? CORE_MAX : d;
}
GSN_HD uint32_t plan_ball(const uint32_t *plan, int l) { return (plan[2 + GSN_KMAX + (l >> 2)] >> (8 * (l & 3))) & 0xffu; }
// closed form of the last two levels (patterns.cpp: plan_tail_mode): 0 none, 1 independent candidate sets, 2 twins, 3 chain
GSN_HD int plan_tail(const uint32_t *plan) { return (int)((plan[1] >> 28) & 3u); }
// the level at which the closed form replaces the search: k - 2, or k - r for a run of r twin levels (mode 2, r = 2 .. 5)
GSN_HD int plan_tail_level(const uint32_t *plan, int k) { return ((plan[1] >> 28) & 3u) == 2u ? k - 2 - (int)(plan[1] >> 30) : k - 2; }

// Number of ways to place the last two levels given C1 = the candidates of level k - 2 (levels 0 .. k - 3 are in fvec / used):
// independent sets: |C1| |C2| - |C1 & C2| with C2 = the candidates of level k - 1 (whose constraints do not name level k - 2);
// twins: C(|C1|, 2).
template <int W, bool DIR>
GSN_HD uint64_t tail_pairs(int mode, const Bits<W> &C1, const uint32_t *plan, int k, const FVec<W> &fvec, const Bits<W> &used, const uint64_t *A,
                           const uint64_t *valid, const uint64_t *balls, int ball_n, const uint64_t *A_in, const uint64_t *degp) {
    const uint64_t n1 = (uint64_t)popc<W>(C1);
    if (mode == 2) {                                    // C(n1, r): r twin levels
        const int r = 2 + (int)(plan[1] >> 30);
        if (n1 < (uint64_t)r) return 0;
        uint64_t c = 1;
        for (int i = 0; i < r; ++i) c = c * (n1 - (uint64_t)i) / (uint64_t)(i + 1);     // (exact at every step: i + 1 consecutive integers)
        return c;
    }
    if (mode == 3) {
        // chain: sum over d in C1 of |N(d) & core \ placed| -- d itself is no neighbour of d, the placed images f_0 .. f_{k-3} are
        const uint64_t *pl = degp + (size_t)plan_core(plan) * DEG_PLANES * W;
        uint64_t s = 0;
#pragma unroll
        for (int p = 0; p < DEG_PLANES; ++p) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) c += popc64(C1.w[w] & pl[p * W + w]);
            s += (uint64_t)c << p;
        }
        for (int j = 0; j < k - 2; ++j) {
            const uint64_t *row = A + fv_get<W>(fvec, j) * W;
            int c = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) c += popc64(C1.w[w] & row[w]);
            s -= (uint64_t)c;
        }
        return s;
    }
    Bits<W> C2;
    candidates<W, DIR>(C2, plan[2 + k - 1], plan_ball(plan, k - 1), fvec, used, A, valid, balls, ball_n,
                       DIR ? plan[PLAN_STRIDE_WORDS + k - 1] : 0u, A_in);
    int both = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) both += popc64(C1.w[w] & C2.w[w]);
    return n1 * (uint64_t)popc<W>(C2) - (uint64_t)both;
}

template <int W>
GSN_HD void bit_set(Bits<W> &b, int v) {
#pragma unroll
    for (int w = 0; w < W; ++w) b.w[w] |= (w == (v >> 6)) ? (1ull << (v & 63)) : 0ull;
}
template <int W>
GSN_HD void bit_clear(Bits<W> &b, int v) {
#pragma unroll
    for (int w = 0; w < W; ++w) b.w[w] &= ~((w == (v >> 6)) ? (1ull << (v & 63)) : 0ull);
}

// frame addressing: word w of level l of lane `tid` lives at stack[((l * W + w) * sstride) + tid]
template <int W>
GSN_HD void frame_store(uint64_t *stack, int sstride, int tid, int l, const Bits<W> &b) {
#pragma unroll
    for (int w = 0; w < W; ++w) stack[(l * W + w) * sstride + tid] = b.w[w];
}
template <int W>
GSN_HD void frame_load(const uint64_t *stack, int sstride, int tid, int l, Bits<W> &b) {
#pragma unroll
    for (int w = 0; w < W; ++w) b.w[w] = stack[(l * W + w) * sstride + tid];
}

// Start the rooted search of `plan` with the root levels already in fvec.  May finish immediately (s.l < 0).
// TAIL = false compiles the closed forms and the tail loop of the last two levels out (the kernel instantiation of the molecule
// workloads, whose plans have none and whose graphs are below 65 vertices: their code and registers cost the headline kernel 7 %)
template <int W, bool DIR = false, bool TAIL = true>
GSN_HD void lane_begin(Lane<W> &s, const uint32_t *plan, const FVec<W> &fvec_roots, const uint64_t *A, const uint64_t *valid,
                       uint64_t *stack, int sstride, int tid, const uint64_t *A_in = nullptr) {
    const uint32_t h = plan[0];
    s.k = (int)(h & 0xffu);
    s.nfix = (int)((h >> 8) & 0xffu);
    s.plan = plan;
    s.fvec = fvec_roots;
    s.l = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) s.used.w[w] = 0ull;
    bit_set<W>(s.used, fv_get<W>(fvec_roots, 0));
    if (s.nfix > 1) bit_set<W>(s.used, fv_get<W>(fvec_roots, 1));
    {   // a root outside the plan's core cannot be the image of anything
        const int ra = fv_get<W>(fvec_roots, 0);
        bool in = (valid[ra >> 6] >> (ra & 63)) & 1ull;
        if (s.nfix > 1) { const int rb = fv_get<W>(fvec_roots, 1); in = in && ((valid[rb >> 6] >> (rb & 63)) & 1ull); }
        if (!in) return;
    }
    if (s.nfix == s.k) { s.cnt += 1; return; }
    Bits<W> C;
    candidates<W, DIR>(C, plan[2 + s.nfix], plan_ball(plan, s.nfix), s.fvec, s.used, A, valid, s.balls, s.ball_n,
                       DIR ? plan[PLAN_STRIDE_WORDS + s.nfix] : 0u, A_in);
    if (s.nfix == s.k - 1) { s.cnt += (uint64_t)popc<W>(C); return; }
    if (TAIL && plan_tail(plan) == 2 && s.nfix == plan_tail_level(plan, s.k)) {            // a run of twin levels: C(|C|, r)
        s.cnt += tail_pairs<W, DIR>(2, C, plan, s.k, s.fvec, s.used, A, valid, s.balls, s.ball_n, A_in, s.degp);
        return;
    }
    if (TAIL && s.nfix == s.k - 2 && (TailLoop<W>::on || s.loop || plan_tail(plan))) {     // the last two levels: closed form or one tight loop, no frame
        const int tm = plan_tail(plan);
        s.cnt += tm ? tail_pairs<W, DIR>(tm, C, plan, s.k, s.fvec, s.used, A, valid, s.balls, s.ball_n, A_in, s.degp)
                    : tail_loop<W, DIR>(C, plan, s.k, s.fvec, s.used, A, valid, s.balls, s.ball_n, A_in);
        return;
    }
    bool cempty = true;
#pragma unroll
    for (int w = 0; w < W; ++w) cempty = cempty && (C.w[w] == 0ull);
    if (cempty) return;  // invariant: the frame of the current level is never empty when lane_step runs
    s.l = s.nfix;
    frame_store<W>(stack, sstride, tid, s.l, C);
}

// One search step.  Precondition: s.l >= 0.  Pops one candidate of the current level; at the last-but-one level the
// whole last level is counted by popcount.  A level that runs empty backtracks in the same step (no wasted iteration).
template <int W, bool DIR = false, bool TAIL = true>
GSN_HD void lane_step(Lane<W> &s, const uint64_t *A, const uint64_t *valid, uint64_t *stack, int sstride, int tid,
                      const uint64_t *A_in = nullptr) {
    Bits<W> M;
    frame_load<W>(stack, sstride, tid, s.l, M);
    int v = -1;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        if (v < 0 && M.w[w]) {
            v = w * 64 + ctz64(M.w[w]);
            M.w[w] &= M.w[w] - 1ull;
        }
    }
    bool empty = true;
#pragma unroll
    for (int w = 0; w < W; ++w) empty = empty && (M.w[w] == 0ull);
    // v >= 0 always: a frame is only ever stored non-empty or left through the `empty` path below
    const int l = s.l;
    fv_set<W>(s.fvec, l, v);
    const int nl = l + 1;
    Bits<W> used2 = s.used;
    bit_set<W>(used2, v);
    Bits<W> C;
    candidates<W, DIR>(C, s.plan[2 + nl], plan_ball(s.plan, nl), s.fvec, used2, A, valid, s.balls, s.ball_n,
                       DIR ? s.plan[PLAN_STRIDE_WORDS + nl] : 0u, A_in);
    bool descend = false;
    if (nl == s.k - 1) {
        s.cnt += (uint64_t)popc<W>(C);
    } else if (TAIL && plan_tail(s.plan) == 2 && nl == plan_tail_level(s.plan, s.k)) {
        s.cnt += tail_pairs<W, DIR>(2, C, s.plan, s.k, s.fvec, used2, A, valid, s.balls, s.ball_n, A_in, s.degp);      // r twin levels: C(|C|, r)
    } else if (TAIL && nl == s.k - 2 && (TailLoop<W>::on || s.loop || plan_tail(s.plan))) {
        // the last two levels: in closed form where the plan allows it (level k - 2 is not enumerated), else in one tight loop over its images
        const int tm = plan_tail(s.plan);
        if (tm) {
            CP_T0();
            s.cnt += tail_pairs<W, DIR>(tm, C, s.plan, s.k, s.fvec, used2, A, valid, s.balls, s.ball_n, A_in, s.degp);
            CP_ADD(s, 5);
        } else {
            CP_T0();
            s.cnt += tail_loop<W, DIR>(C, s.plan, s.k, s.fvec, used2, A, valid, s.balls, s.ball_n, A_in);
            CP_ADD(s, 0);
#if defined(COUNT_PROF_STEP) && defined(__HIP_DEVICE_COMPILE__)
            {   // (inside a divergent branch: ballots over the active lanes, no shuffles)
                const int it = popc<W>(C);
                unsigned long long alive = __ballot(1), sm = 0;
                int mx = 0;
                for (int b = 10; b >= 0; --b) {
                    const unsigned long long hb = __ballot((it >> b) & 1);
                    sm += (unsigned long long)__popcll(hb) << b;
                    if (hb & alive) { mx |= 1 << b; alive &= hb; }
                }
                s.prof[3] += sm; s.prof[4] += (unsigned long long)mx;
            }
#endif
        }
    } else {
        bool cempty = true;
#pragma unroll
        for (int w = 0; w < W; ++w) cempty = cempty && (C.w[w] == 0ull);
        descend = !cempty;
    }
    if (descend) {
        frame_store<W>(stack, sstride, tid, l, M);   // possibly empty: the climb below finds it so on the way back
        s.used = used2;
        s.l = nl;
        frame_store<W>(stack, sstride, tid, nl, C);
        return;
    }
    if (!empty) {
        frame_store<W>(stack, sstride, tid, l, M);
        return;
    }
    // this level is exhausted: climb to the nearest level that still has candidates
    int cl = l - 1;
    while (cl >= s.nfix) {
        bit_clear<W>(s.used, fv_get<W>(s.fvec, cl));
        Bits<W> P;
        frame_load<W>(stack, sstride, tid, cl, P);
        bool pe = true;
#pragma unroll
        for (int w = 0; w < W; ++w) pe = pe && (P.w[w] == 0ull);
        if (!pe) break;
        --cl;
    }
    s.l = cl >= s.nfix ? cl : -1;
}

// ---- cycle columns of one-word graphs: bitset path walks instead of the plan interpreter ---------------------------------------
// A non-induced k-cycle rooted at one of its arcs has no automorphism that fixes the arc, so its edge-mode identifier of row (u, v)
// is the number of simple k-cycles through the edge {u, v} = the number of simple paths of k - 1 edges from v to u whose inner
// vertices avoid u and v.  On a graph of <= 64 vertices (A[x] = the one-word adjacency row of x) one depth-first walk from v counts
// the paths of every length 2 .. L - 1 at once: at a vertex reached by d edges, popc(A[x] & A[u] & ~used) closes the (d + 2)-cycles.
// `mask` prunes the inner vertices (the 2-core: every vertex of a cycle lies in it; ~0 = no pruning -- it never changes the result).
// cnt[k - 3] = the count for length k, k = 3 .. L.  L is a compile-time bound: the loops unroll, nothing but A is read from memory.
template <int L, int D, class Acc>
GSN_HD void cycle_walk_level(const uint64_t *A, const uint64_t au, const uint64_t mask, const int x, const uint64_t used, Acc *cnt) {
    const uint64_t row = A[x] & ~used;
    cnt[D] += (Acc)popc64(row & au);
    if constexpr (D + 1 < L - 2) {
        uint64_t m = row & mask;
        while (m) {
            const int y = ctz64(m);
            m &= m - 1ull;
            cycle_walk_level<L, D + 1, Acc>(A, au, mask, y, used | (1ull << y), cnt);
        }
    }
}
// (counter width: a cell for length k is at most the number of ordered choices of the k - 2 inner vertices among the 62 others, K64's value;
//  k = 6: 62 * 61 * 60 * 59 = 13 388 280 < 2^32, so 32 bits hold every count of a one-word graph for L <= 6 -- no launch condition is
//  needed (tests/test_cycle_counter_width_cpu.py); k = 8: 62 * ... * 57 = 4.4e10 does not fit: 64-bit counters above 6)
template <int L>
struct CycleAcc { typedef uint64_t type; };
template <> struct CycleAcc<3> { typedef uint32_t type; };
template <> struct CycleAcc<4> { typedef uint32_t type; };
template <> struct CycleAcc<5> { typedef uint32_t type; };
template <> struct CycleAcc<6> { typedef uint32_t type; };
// Out: the caller's counter type -- uint64_t, or CycleAcc<L>::type itself (the kernel: no 64-bit copies of counters that fit 32 bits)
template <int L, class Out>
GSN_HD void cycle_walk(const uint64_t *A, const int u, const int v, const uint64_t mask, Out *cnt /* [L - 2] */) {
    static_assert(L >= 3 && L <= GSN_KMAX, "cycle lengths 3 .. GSN_KMAX");
    static_assert(sizeof(Out) >= sizeof(typename CycleAcc<L>::type), "the caller's counters hold what the walk's do");
    typename CycleAcc<L>::type c[L - 2];
#pragma unroll
    for (int i = 0; i < L - 2; ++i) c[i] = 0;
    cycle_walk_level<L, 0, typename CycleAcc<L>::type>(A, A[u] & mask, mask, v, (1ull << u) | (1ull << v), c);
#pragma unroll
    for (int i = 0; i < L - 2; ++i) cnt[i] = (Out)c[i];
}

// ---- a finished row of a cycle launch leaving LDS: the four staged 16-bit counts (lo = cells 0, 1; hi = cells 2, 3: one 8-byte read) ------
// A staged 0xffff means "this cell's count did not fit 16 bits and went to memory by itself" (count.hip: emit_row), so it is not stored again.
// Does one of the four cells hold 0xffff?  (the zero-halfword test on the complement)
GSN_HD bool cyc_row_has_direct(const uint32_t lo, const uint32_t hi) {
    return ((((~lo) - 0x00010001u) & lo & 0x80008000u) | (((~hi) - 0x00010001u) & hi & 0x80008000u)) != 0u;
}
// The int64 row d[0 .. 3].  wide: d is 16-byte aligned -- two 16-byte stores, 32 contiguous bytes per lane; else four 8-byte stores.  A row
// with a 0xffff cell goes cell by cell and skips those cells.
typedef int64_t cyc_i64x2 __attribute__((vector_size(16)));
GSN_HD void cyc_row_store(int64_t *d, const uint32_t lo, const uint32_t hi, const bool wide) {
    const uint32_t c0 = lo & 0xffffu, c1 = lo >> 16, c2 = hi & 0xffffu, c3 = hi >> 16;
    if (cyc_row_has_direct(lo, hi)) {
        if (c0 != 0xffffu) d[0] = (int64_t)c0;
        if (c1 != 0xffffu) d[1] = (int64_t)c1;
        if (c2 != 0xffffu) d[2] = (int64_t)c2;
        if (c3 != 0xffffu) d[3] = (int64_t)c3;
    } else if (wide) {
        cyc_i64x2 *d2 = reinterpret_cast<cyc_i64x2 *>(d);
        d2[0] = cyc_i64x2{(int64_t)c0, (int64_t)c1};
        d2[1] = cyc_i64x2{(int64_t)c2, (int64_t)c3};
    } else {
        d[0] = (int64_t)c0; d[1] = (int64_t)c1; d[2] = (int64_t)c2; d[3] = (int64_t)c3;
    }
}
// The row's hot columns as bits: column c owns the bits  sum of the classes before it .. + its own; its class is the count, the last class
// when clamped and beyond, none when not clamped and beyond (0xffff = 65 535 and more: beyond every class count, which fit a byte).
// ncls_w: the four columns' class counts, a byte each.  The caller shifts the mask to its first pack column.
GSN_HD uint32_t cyc_row_mask(const uint32_t lo, const uint32_t hi, const uint32_t ncls_w, const bool clamp) {
    const uint32_t cell[4] = {lo & 0xffffu, lo >> 16, hi & 0xffffu, hi >> 16};
    uint32_t m = 0u, first = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t n = (ncls_w >> (8 * c)) & 0xffu;
        const uint32_t cls = cell[c] < n ? cell[c] : n - 1u;
        if (cell[c] < n || clamp) m |= 1u << (first + cls);
        first += n;
    }
    return m;
}

// Is this plan table a set of such columns?  Judged from the plans' structure, not from pattern names: edge mode, non-induced, undirected
// orbit classes; every column has exactly one plan (a cycle has one arc orbit: a second plan would ADD to the column), rooted at an arc,
// without non-adjacency or order masks, and the pattern rebuilt from its levels' adjacency masks plus the root edge is one cycle: k
// vertices, k edges, every degree 2, connected.  len[c] = the cycle length of column c; returns the largest length, 0 = not recognised.
inline int cycle_plan_lengths(const uint32_t *plan, int64_t plan_words, uint8_t *len, int len_cap) {
    if (!plan || plan_words < PLAN_HEADER_WORDS || plan[0] != PLAN_MAGIC) return 0;
    if (plan[1] != (uint32_t)GSN_MODE_EDGE || plan[2] != 0u || plan[6] != 0u) return 0;
    const int n_plans = (int)plan[3], n_cols = (int)plan[4], plans_off = (int)plan[7];
    if (n_cols < 1 || n_cols > len_cap || n_plans != n_cols || plan_words < plans_off + (int64_t)n_plans * PLAN_STRIDE_WORDS) return 0;
    int lmax = 0;
    for (int c = 0; c < n_cols; ++c) {
        if (plan[PLAN_HEADER_WORDS + c] != (uint32_t)c) return 0;            // col_ptr: plan c is the one plan of column c
        const uint32_t *w = plan + plans_off + c * PLAN_STRIDE_WORDS;
        const int k = (int)(w[0] & 0xffu), nfix = (int)((w[0] >> 8) & 0xffu);
        if (k < 3 || k > GSN_KMAX || nfix != 2 || (int)(w[0] >> 16) != c) return 0;
        uint32_t nb[GSN_KMAX];
        for (int l = 0; l < k; ++l) nb[l] = 0;
        nb[0] |= 2u; nb[1] |= 1u;                                             // the root edge
        for (int l = 0; l < k; ++l) {
            if (w[2 + l] >> 8) return 0;                                      // non-adjacency (induced) or order (symmetry) constraints
            const uint32_t adj = w[2 + l] & 0xffu;
            if (adj >> l) return 0;                                           // (a level names earlier levels only)
            for (int j = 0; j < l; ++j)
                if ((adj >> j) & 1u) { nb[l] |= 1u << j; nb[j] |= 1u << l; }
        }
        for (int l = 0; l < k; ++l)
            if (popc64(nb[l]) != 2) return 0;                                 // 2-regular: k vertices, k edges
        uint32_t seen = 1u;                                                   // connected: one cycle, not several
        for (int prev = 0, cur = ctz64(nb[0]), i = 1; i < k; ++i) {
            if ((seen >> cur) & 1u) return 0;
            seen |= 1u << cur;
            const int nxt = ctz64(nb[cur] & ~(1u << prev));
            prev = cur; cur = nxt;
        }
        len[c] = (uint8_t)k;
        lmax = k > lmax ? k : lmax;
    }
    return lmax;
}

}  // namespace gsn
