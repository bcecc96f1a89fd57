// TEST-ONLY logic harness (not product code, never shipped in libgsn_hip.so).
// Compiles the WIDE instantiation of the sparse kernel's search core (gsn_amd/csrc/count_sparse_core.h: SpWide, plan tables of pattern lists
// with 10 .. 16 vertices) for the HOST.  Undirected tables (vertex and edge mode) and directed ones (vertex mode) alike: the CSR of sorted,
// duplicate-free neighbour lists -- directed: out-lists in rows 0 .. n - 1, in-lists in rows n .. 2 n - 1 -- and the "last column of every
// arc" table are built the way the kernel's set-up pass builds them (here with std::sort), then every (column, row) cell runs sequentially
// through the same functions the kernel's lanes call.  The HIP set-up pass itself is covered by the -m gpu tests.
//
// Two builds: a shared object for ctypes (sparse_wide_harness_count), and with -DSPARSE_HARNESS_MAIN a stand-alone program that reads one
// case from a file -- the form that runs under -fsanitize=address,undefined.
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

// -> the graph's status (GSN_ST_OK / GSN_ST_KEYERROR / GSN_ST_BAD_INDEX), or -1: not a wide plan table
extern "C" int sparse_wide_harness_count(const uint32_t *plan, int64_t n, int64_t E, const int64_t *src, const int64_t *dst, int64_t *out) {
    if (plan[0] != PLAN_MAGIC_WIDE) return -1;
    const int mode = (int)plan[1], n_cols = (int)plan[4];
    const bool directed = (plan[6] & 2u) != 0;
    if (directed && mode != GSN_MODE_VERTEX) return -1;
    const bool sym = mode == GSN_MODE_EDGE && (plan[6] & 1u) == 0;
    const int64_t rows = mode == GSN_MODE_EDGE ? E : n;
    for (int64_t i = 0; i < rows * n_cols; ++i) out[i] = 0;
    uint32_t n_active = 0;
    std::vector<uint64_t> arcs;
    for (int64_t c = 0; c < E; ++c) {
        if (src[c] < 0 || dst[c] < 0 || src[c] >= n || dst[c] >= n) return GSN_ST_BAD_INDEX;
        const uint64_t u = (uint64_t)src[c], v = (uint64_t)dst[c];
        n_active = std::max(n_active, (uint32_t)std::max(u, v) + 1u);
        if (u == v) continue;
        arcs.push_back(u << 32 | v);
        arcs.push_back(directed ? ((uint64_t)n + v) << 32 | u : v << 32 | u);
    }
    std::sort(arcs.begin(), arcs.end());
    arcs.erase(std::unique(arcs.begin(), arcs.end()), arcs.end());
    const size_t n_rows = (size_t)(directed ? 2 * n : n);
    std::vector<uint32_t> row_ptr(n_rows + 1, 0), nbr(arcs.size() + 1, 0);
    for (size_t i = 0; i < arcs.size(); ++i) { nbr[i] = (uint32_t)arcs[i]; row_ptr[(size_t)(arcs[i] >> 32) + 1] += 1; }
    for (size_t r = 0; r < n_rows; ++r) row_ptr[r + 1] += row_ptr[r];
    SparseGraph g{row_ptr.data(), nbr.data(), 0u, n_active};
    if (directed) g.in_base = (uint32_t)n;
    uint32_t st[SP_FIELDS_DIRECTED * SpWide::LEVELS];
    if (directed) {
        for (int col = 0; col < n_cols; ++col)
            for (int64_t row = 0; row < (int64_t)n_active; ++row)
                out[row * n_cols + col] = (int64_t)sp_cell<true, SpWide>(g, plan, col, (uint32_t)row, 0u, st, 1);
        return GSN_ST_OK;
    }
    std::vector<int32_t> arc_col(arcs.size() + 1, -1);
    for (int64_t c = 0; c < E; ++c) {
        if (src[c] == dst[c]) continue;
        const int64_t s = sp_find(g, (uint32_t)src[c], (uint32_t)dst[c]);
        arc_col[(size_t)s] = std::max(arc_col[(size_t)s], (int32_t)c);
    }
    int status = GSN_ST_OK;
    for (int col = 0; col < n_cols; ++col)
        for (int64_t row = 0; row < rows; ++row) {
            if (mode == GSN_MODE_EDGE) {
                const uint32_t u = (uint32_t)src[row], v = (uint32_t)dst[row];
                int64_t mirror;
                bool rev_missing;
                if (sp_edge_row(g, arc_col.data(), row, u, v, sym, mirror, rev_missing) != SP_ROW_SEARCH) continue;
                const uint64_t cnt = sp_cell<false, SpWide>(g, plan, col, u, v, st, 1);
                out[row * n_cols + col] = (int64_t)cnt;
                if (mirror >= 0) out[mirror * n_cols + col] = (int64_t)cnt;
                if (rev_missing && cnt) status = GSN_ST_KEYERROR;
            } else if (row < (int64_t)n_active) {     // (graph-tool creates vertices 0 .. the largest id of a column: the rest are no vertices)
                out[row * n_cols + col] = (int64_t)sp_cell<false, SpWide>(g, plan, col, (uint32_t)row, 0u, st, 1);
            }
        }
    return status;
}

#ifdef SPARSE_HARNESS_MAIN
// case file: int64 plan_words, n, E, n_cols, status; uint32 plan[plan_words] (padded to 8 bytes); int64 src[E], dst[E], expected[rows * n_cols]
int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t h[5];
    if (fread(h, 8, 5, f) != 5) return 2;
    const int64_t plan_words = h[0], n = h[1], E = h[2], n_cols = h[3];
    std::vector<uint32_t> plan((size_t)(plan_words + 1) / 2 * 2);
    if (fread(plan.data(), 4, plan.size(), f) != plan.size()) return 2;
    const int64_t rows = plan[1] == (uint32_t)GSN_MODE_EDGE ? E : n;
    std::vector<int64_t> src((size_t)E), dst((size_t)E), want((size_t)(rows * n_cols)), got((size_t)(rows * n_cols));
    if (fread(src.data(), 8, src.size(), f) != src.size() || fread(dst.data(), 8, dst.size(), f) != dst.size() ||
        fread(want.data(), 8, want.size(), f) != want.size())
        return 2;
    fclose(f);
    const int st = sparse_wide_harness_count(plan.data(), n, E, src.data(), dst.data(), got.data());
    if (st != (int)h[4]) { fprintf(stderr, "status %d, expected %d\n", st, (int)h[4]); return 1; }
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i] != want[i]) { fprintf(stderr, "cell %zu: %lld, expected %lld\n", i, (long long)got[i], (long long)want[i]); return 1; }
    printf("sparse wide harness ok: %lld cells\n", (long long)got.size());
    return 0;
}
#endif
