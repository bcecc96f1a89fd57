// TEST-ONLY logic harness (not product code, never shipped in libgsn_hip.so).
// Compiles the sparse kernel's search core (gsn_amd/csrc/count_sparse_core.h) for the HOST with DIRECTED plans: builds the out-lists (rows
// 0 .. n - 1) and the in-lists (rows n .. 2 n - 1) of one CSR the way the kernel's set-up pass does -- column (u, v) is the arc u -> v only,
// repeated columns merge, self loops drop out; here with std::sort -- and runs every (vertex, column) cell sequentially through the same
// functions the kernel's lanes call.  An undirected vertex-mode plan takes the undirected instantiation of the same core (both directions of
// a column keyed, no in-lists): the symmetric-digraph test compares the two.  The HIP set-up pass itself is covered by the -m gpu tests.
//
// Two builds: a shared object for ctypes (sparse_directed_harness_count), and with -DSPARSE_HARNESS_MAIN, linked with the plan compiler
// (gsn_amd/csrc/patterns.cpp), a stand-alone program that builds a seeded digraph and a bidirected one and runs both searches -- the form
// that runs under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gsn_amd/csrc/count_sparse_core.h"

namespace gsn {
int set_error(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr);
    return code;
}
}
using namespace gsn;

// -> the graph's status (GSN_ST_OK / GSN_ST_BAD_INDEX), or -1: not a vertex-mode plan
extern "C" int sparse_directed_harness_count(const uint32_t *plan, int64_t n, int64_t E, const int64_t *src, const int64_t *dst, int64_t *out) {
    if (plan[0] != PLAN_MAGIC || plan[1] != (uint32_t)GSN_MODE_VERTEX) return -1;
    const bool directed = (plan[6] & 2u) != 0;
    const int n_cols = (int)plan[4];
    for (int64_t i = 0; i < n * n_cols; ++i) out[i] = 0;
    uint32_t n_active = 0;
    std::vector<uint64_t> keys;
    for (int64_t c = 0; c < E; ++c) {
        if (src[c] < 0 || dst[c] < 0 || src[c] >= n || dst[c] >= n) return GSN_ST_BAD_INDEX;
        const uint64_t u = (uint64_t)src[c], v = (uint64_t)dst[c];
        n_active = std::max(n_active, (uint32_t)std::max(u, v) + 1u);
        if (u == v) continue;
        keys.push_back(u << 32 | v);                                              // v joins the out-list of u
        keys.push_back(directed ? ((uint64_t)n + v) << 32 | u : v << 32 | u);     // u joins the in-list of v
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const size_t n_rows = (size_t)(directed ? 2 * n : n);
    std::vector<uint32_t> row_ptr(n_rows + 1, 0), nbr(keys.size() + 1, 0);
    for (size_t i = 0; i < keys.size(); ++i) { nbr[i] = (uint32_t)keys[i]; row_ptr[(size_t)(keys[i] >> 32) + 1] += 1; }
    for (size_t r = 0; r < n_rows; ++r) row_ptr[r + 1] += row_ptr[r];
    SparseGraph g{row_ptr.data(), nbr.data(), 0u, n_active};
    if (directed) g.in_base = (uint32_t)n;
    uint32_t st[SP_FIELDS_DIRECTED * SP_LEVELS];
    for (int col = 0; col < n_cols; ++col)
        for (int64_t row = 0; row < (int64_t)n_active; ++row)     // (graph-tool creates vertices 0 .. the largest id of a column: the rest are no vertices)
            out[row * n_cols + col] = (int64_t)(directed ? sp_cell<true>(g, plan, col, (uint32_t)row, 0u, st, 1) : sp_cell<false>(g, plan, col, (uint32_t)row, 0u, st, 1));
    return GSN_ST_OK;
}

#ifdef SPARSE_HARNESS_MAIN
extern "C" int gsn_count_plan_build(int mode, int induced, int directed_orbits, int64_t n_patterns, const int64_t *pat_ptr, const int64_t *pat_edges,
                                    uint32_t *plan, int64_t capacity, int64_t *out_words, int64_t *out_n_cols);

static std::vector<uint32_t> build_plan(const std::vector<std::vector<int64_t>> &pats, int induced, int flags, int64_t &n_cols) {
    std::vector<int64_t> ptr{0}, edges;
    for (auto &p : pats) { edges.insert(edges.end(), p.begin(), p.end()); ptr.push_back((int64_t)edges.size() / 2); }
    int64_t words = 0;
    if (gsn_count_plan_build(GSN_MODE_VERTEX, induced, flags, (int64_t)pats.size(), ptr.data(), edges.data(), nullptr, 0, &words, &n_cols)) exit(2);
    std::vector<uint32_t> plan((size_t)words);
    if (gsn_count_plan_build(GSN_MODE_VERTEX, induced, flags, (int64_t)pats.size(), ptr.data(), edges.data(), plan.data(), words, &words, &n_cols)) exit(2);
    return plan;
}

static std::vector<int64_t> run(const std::vector<uint32_t> &plan, int64_t n_cols, int64_t n, const std::vector<int64_t> &src, const std::vector<int64_t> &dst) {
    std::vector<int64_t> out((size_t)(n * n_cols));
    if (sparse_directed_harness_count(plan.data(), n, (int64_t)src.size(), src.data(), dst.data(), out.data()) != GSN_ST_OK) exit(2);
    return out;
}

// A seeded digraph (repeated arcs, self loops, antiparallel pairs) under digraph patterns, and a bidirected graph under bidirected patterns
// next to the undirected patterns on the same edges: the two must agree.
int main() {
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto rnd = [&x](uint64_t m) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (int64_t)(x % m); };
    const std::vector<std::vector<int64_t>> und = {{0, 1, 1, 2, 2, 0}, {0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0}, {0, 1, 0, 2, 0, 3}, {0, 1, 1, 2, 2, 3}};
    std::vector<std::vector<int64_t>> both = und;
    for (size_t p = 0; p < und.size(); ++p)
        for (size_t i = 0; i < und[p].size(); i += 2) { both[p].push_back(und[p][i + 1]); both[p].push_back(und[p][i]); }
    const std::vector<std::vector<int64_t>> dir = {{0, 1, 1, 2, 2, 0}, {0, 1, 1, 2}, {0, 1, 0, 2}, {1, 0, 2, 0}, {0, 1, 1, 0, 1, 2}, {0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 0},
                                                    {0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 0, 5}, {0, 1, 0, 2, 0, 3, 0, 4}};
    long long total = 0;
    for (int induced = 0; induced < 2; ++induced) {
        const int64_t n = 300;
        std::vector<int64_t> src, dst;
        for (int i = 0; i < 900; ++i) { src.push_back(rnd(n)); dst.push_back(rnd(n)); }
        for (int i = 0; i < 20; ++i) { src.push_back(src[(size_t)i]); dst.push_back(dst[(size_t)i]); }           // repeated arcs
        for (int i = 20; i < 60; ++i) { src.push_back(dst[(size_t)i]); dst.push_back(src[(size_t)i]); }          // antiparallel pairs
        for (int i = 0; i < 5; ++i) { const int64_t v = rnd(n); src.push_back(v); dst.push_back(v); }            // self loops
        int64_t n_cols = 0;
        const std::vector<uint32_t> plan = build_plan(dir, induced, 2, n_cols);
        for (int64_t c : run(plan, n_cols, n, src, dst)) total += c;

        std::vector<int64_t> s2, d2, s1, d1;
        for (int i = 0; i < 400; ++i) {
            const int64_t u = rnd(n), v = rnd(n);
            s1.push_back(u); d1.push_back(v);
            s2.push_back(u); d2.push_back(v); s2.push_back(v); d2.push_back(u);
        }
        int64_t nc_b = 0, nc_u = 0;
        const std::vector<uint32_t> plan_b = build_plan(both, induced, 2, nc_b), plan_u = build_plan(und, induced, 0, nc_u);
        const std::vector<int64_t> got_b = run(plan_b, nc_b, n, s2, d2), got_u = run(plan_u, nc_u, n, s1, d1);
        if (nc_b != nc_u || got_b != got_u) { fprintf(stderr, "bidirected and undirected counts differ (induced %d)\n", induced); return 1; }
        for (int64_t c : got_b) total += c;
    }
    if (total <= 0) { fprintf(stderr, "no occurrence counted\n"); return 1; }
    printf("sparse directed harness ok: %lld occurrences\n", total);
    return 0;
}
#endif
