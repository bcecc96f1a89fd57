// Sparse counting kernel: substructure counts of the graphs the LDS-resident kernel (count.hip) refuses -- more than 768 vertices, tables
// beyond 160 KiB of LDS, 65 535 columns per graph.  Nothing here is sized by LDS: the graph lives in HBM as sorted neighbour lists and one
// lane runs one rooted search over them (count_sparse_core.h).  Opt-in: gsn_count_hip keeps refusing; callers ask for this entry.
//
// One launch = a set-up pass and a search kernel, all on the device, on the caller's stream:
//   set-up   sparse_mark_kernel    status words of the processed graphs, their pointers checked, rows -> graph
//            sparse_check_kernel   every endpoint inside its graph (else GSN_ST_BAD_INDEX on the graph), the largest id per graph
//            sparse_keys_kernel    per column the arcs (u, v) and (v, u) as 64-bit keys u << 32 | v -- either direction of a column makes the
//                                  edge; self loops, columns of a bad graph and of graphs outside the launch become an end marker.
//                                  A directed plan: column (u, v) is the arc u -> v only -- keys u << 32 | v (row u: out-neighbours) and
//                                  (nv + v) << 32 | u (row nv + v: in-neighbours of v); the end marker is row 2 nv
//            rocPRIM               device radix sort of the keys, then unique: parallel columns merged, lists strictly increasing
//            sparse_csr_kernel     row_ptr by binary search over the sorted keys, nbr = their low halves
//            sparse_arc_kernel     edge mode: per arc slot the LAST column that holds that direction (utils_graph_processing.py:142-144)
//   search   sparse_search_kernel  <DIR, WIDE>: undirected / directed plans (vertex mode only: there are no directed edge counts), narrow
//                                  tables (patterns of <= 9 vertices) / wide ones (10 .. 16: gsn_internal.h).  Persistent waves; lanes
//                                  pull (output column, row) cells from one global counter with a wave-aggregated atomic; every cell is written by exactly one lane, no atomics on counts: deterministic
// Vertices and columns are numbered from the first pointer of the launch (node_ptr[0], edge_ptr[0]), 32 bits each.  The launcher reads
// those two and the two last pointers back (one stream synchronisation): the launch cannot be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "count_sparse_core.h"

namespace gsn {
namespace {

constexpr int64_t SP_MAX_VERTICES = ((int64_t)1 << 31) - 2;
constexpr int64_t SP_MAX_COLUMNS = (int64_t)1 << 30;            // two arcs per column, 32-bit positions in nbr
constexpr int SP_CHUNKS = 16;                                    // blocks per graph of the set-up kernels (grid y)
constexpr int SP_T = 256;

inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

struct SparseLayout {
    int64_t keys_a, keys_b, nbr, arc_col, row_ptr, row_graph, vmax, misc, temp, temp_bytes, total;
};
// (n_cols: no table of this layout depends on it)
SparseLayout sparse_layout(int64_t nv, int64_t ec) {
    const int64_t arcs = 2 * ec, rows = nv > ec ? nv : ec;
    SparseLayout L;
    int64_t o = 0;
    L.keys_a = o; o += up256(arcs * 8 + 8);
    L.keys_b = o; o += up256(arcs * 8 + 8);
    L.nbr = o; o += up256(arcs * 4 + 4);
    L.arc_col = o; o += up256(arcs * 4 + 4);
    L.row_ptr = o; o += up256((2 * nv + 2) * 4);                         // (two row sets, out and in, when the plan is directed)
    L.row_graph = o; o += up256(rows * 4 + 4);
    L.vmax = o; o += up256((nv + 1) * 4);
    L.misc = o; o += 256;
    L.temp = o; L.temp_bytes = up256(arcs * 4 + ((int64_t)4 << 20));     // rocPRIM's scratch (sort with both key buffers given, unique): checked at launch
    L.total = o + L.temp_bytes;
    return L;
}

struct SparseArgs {
    const uint32_t *plan;
    int mode, n_cols, sym, ids_are_global, directed;
    const int64_t *node_ptr, *edge_ptr, *src, *dst;
    const int32_t *graph_ids;
    int64_t n_graphs;
    int64_t n0, e0, nv, ec;            // first vertex / column of the launch, their numbers
    int64_t nr;                        // rows of row_ptr: nv, or 2 nv for a directed plan (row nv + v: the in-neighbours of v)
    int64_t *out;
    int32_t *status;
    uint64_t *keys_a, *keys_b;
    uint32_t *nbr, *row_ptr, *vmax;
    int32_t *arc_col, *row_graph;
    unsigned long long *cell_counter;  // misc[0]
    unsigned int *n_unique;            // misc + 8
};

__device__ __forceinline__ int64_t item_graph(const SparseArgs &a, int64_t item) {
    const int64_t g = a.graph_ids ? (int64_t)a.graph_ids[item] : item;
    return (g < 0 || g >= a.n_graphs) ? -1 : g;
}

// the graph's vertex and column ranges, numbered from the launch's first; false: pointers outside the launch
__device__ __forceinline__ bool graph_ranges(const SparseArgs &a, int64_t g, int64_t &v0, int64_t &v1, int64_t &c0, int64_t &c1) {
    v0 = a.node_ptr[g] - a.n0; v1 = a.node_ptr[g + 1] - a.n0;
    c0 = a.edge_ptr[g] - a.e0; c1 = a.edge_ptr[g + 1] - a.e0;
    return v0 >= 0 && v0 <= v1 && v1 <= a.nv && c0 >= 0 && c0 <= c1 && c1 <= a.ec;
}

__global__ __launch_bounds__(SP_T) void sparse_fill_kernel(SparseArgs a) {
    const uint64_t endmark = (uint64_t)a.nr << 32;
    const int64_t stride = (int64_t)gridDim.x * SP_T;
    for (int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x; i < 2 * a.ec; i += stride) a.keys_a[i] = endmark;
    const int64_t rows = a.mode == GSN_MODE_EDGE ? a.ec : a.nv;
    for (int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x; i < rows; i += stride) a.row_graph[i] = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) { *a.cell_counter = 0ull; *a.n_unique = 0u; }
}

__global__ __launch_bounds__(SP_T) void sparse_mark_kernel(SparseArgs a) {
    const int64_t g = item_graph(a, blockIdx.x);
    if (g < 0) return;
    int64_t v0, v1, c0, c1;
    const bool ok = graph_ranges(a, g, v0, v1, c0, c1);
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        a.status[g] = ok ? GSN_ST_OK : GSN_ST_BAD_INDEX;
        if (ok && v1 > v0) a.vmax[v0] = 0u;
    }
    if (!ok) return;
    const int64_t r0 = a.mode == GSN_MODE_EDGE ? c0 : v0, r1 = a.mode == GSN_MODE_EDGE ? c1 : v1;
    for (int64_t r = r0 + (int64_t)blockIdx.y * SP_T + threadIdx.x; r < r1; r += (int64_t)SP_CHUNKS * SP_T) a.row_graph[r] = (int32_t)g;
}

// local endpoints of column c (numbered from the launch's first column) of graph g whose first vertex is v0
__device__ __forceinline__ void column_ends(const SparseArgs &a, int64_t c, int64_t v0, int64_t &u, int64_t &v) {
    const int64_t off = a.ids_are_global ? a.n0 + v0 : 0;
    u = a.src[a.e0 + c] - off; v = a.dst[a.e0 + c] - off;
}

__global__ __launch_bounds__(SP_T) void sparse_check_kernel(SparseArgs a) {
    const int64_t g = item_graph(a, blockIdx.x);
    if (g < 0) return;
    int64_t v0, v1, c0, c1;
    if (!graph_ranges(a, g, v0, v1, c0, c1)) return;
    const int64_t n = v1 - v0;
    int64_t big = 0;
    bool bad = false;
    for (int64_t c = c0 + (int64_t)blockIdx.y * SP_T + threadIdx.x; c < c1; c += (int64_t)SP_CHUNKS * SP_T) {
        int64_t u, v;
        column_ends(a, c, v0, u, v);
        if (u < 0 || v < 0 || u >= n || v >= n) bad = true;
        else big = max(big, max(u, v) + 1);          // graph-tool creates vertices 0 .. the largest id, self-loop columns included
    }
    if (bad) atomicMax(&a.status[g], (int)GSN_ST_BAD_INDEX);
    if (big > 0) atomicMax(&a.vmax[v0], (unsigned int)big);      // (big <= n: v0 < v1, the word exists)
}

__global__ __launch_bounds__(SP_T) void sparse_keys_kernel(SparseArgs a) {
    const int64_t g = item_graph(a, blockIdx.x);
    if (g < 0) return;
    int64_t v0, v1, c0, c1;
    if (!graph_ranges(a, g, v0, v1, c0, c1)) return;
    if (a.status[g] == GSN_ST_BAD_INDEX) return;     // (its columns keep the end marker: the graph has no edges)
    for (int64_t c = c0 + (int64_t)blockIdx.y * SP_T + threadIdx.x; c < c1; c += (int64_t)SP_CHUNKS * SP_T) {
        int64_t u, v;
        column_ends(a, c, v0, u, v);
        if (u == v) continue;
        const uint64_t gu = (uint64_t)(v0 + u), gv = (uint64_t)(v0 + v);
        a.keys_a[2 * c] = gu << 32 | gv;
        a.keys_a[2 * c + 1] = a.directed ? ((uint64_t)a.nv + gv) << 32 | gu : gv << 32 | gu;      // directed: u joins the in-list of v
    }
}

// keys: the sorted, duplicate-free arcs, *n_unique of them, the end marker (row nr) last when any slot held it
__global__ __launch_bounds__(SP_T) void sparse_csr_kernel(SparseArgs a, const uint64_t *keys) {
    const int64_t nk = (int64_t)*a.n_unique;
    const int64_t stride = (int64_t)gridDim.x * SP_T;
    for (int64_t v = (int64_t)blockIdx.x * SP_T + threadIdx.x; v <= a.nr; v += stride) {
        const uint64_t want = (uint64_t)v << 32;
        int64_t lo = 0, hi = nk;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < want) lo = mid + 1; else hi = mid;
        }
        a.row_ptr[v] = (uint32_t)lo;
    }
    for (int64_t i = (int64_t)blockIdx.x * SP_T + threadIdx.x; i < nk; i += stride) {
        a.nbr[i] = (uint32_t)keys[i];
        a.arc_col[i] = -1;
    }
}

__global__ __launch_bounds__(SP_T) void sparse_arc_kernel(SparseArgs a) {
    const int64_t g = item_graph(a, blockIdx.x);
    if (g < 0) return;
    int64_t v0, v1, c0, c1;
    if (!graph_ranges(a, g, v0, v1, c0, c1)) return;
    if (a.status[g] == GSN_ST_BAD_INDEX) return;
    const SparseGraph gr{a.row_ptr, a.nbr, 0u, 0u};
    for (int64_t c = c0 + (int64_t)blockIdx.y * SP_T + threadIdx.x; c < c1; c += (int64_t)SP_CHUNKS * SP_T) {
        int64_t u, v;
        column_ends(a, c, v0, u, v);
        if (u == v) continue;
        const int64_t s = sp_find(gr, (uint32_t)(v0 + u), (uint32_t)(v0 + v));
        if (s >= 0) atomicMax(&a.arc_col[s], (int)c);
    }
}

constexpr int SP_PULL_BATCH = 8;      // idle lanes are refilled when this many wait, or when no lane of the wave is inside a search

// One wave per workgroup.  A lane is idle, or owns one cell: the plans of its column run one after the other, a turn of the walk per trip.
// DIR: a directed plan (vertex mode): a fifth state field for the in-masks, the longer plan stride, in-lists at rows nv + v.
// WIDE: a wide plan table: 15 levels with a slot instead of 8 -- (4 or 5) * 15 * 64 state words, 15 360 B or 19 200 B of LDS a workgroup.
template <bool WIDE>
using SparseFormat = typename std::conditional<WIDE, SpWide, SpNarrow>::type;
template <bool DIR, bool WIDE>
constexpr int sparse_state_words() { return (DIR ? SP_FIELDS_DIRECTED : SP_FIELDS) * SparseFormat<WIDE>::LEVELS * 64; }

template <bool DIR, bool WIDE = false>
__global__ __launch_bounds__(64) void sparse_search_kernel(SparseArgs a) {
    using FMT = SparseFormat<WIDE>;
    __shared__ uint32_t st_all[sparse_state_words<DIR, WIDE>()];
    constexpr int stride = DIR ? FMT::STRIDE_DIRECTED : FMT::STRIDE;
    const int lane = threadIdx.x;
    uint32_t *st = st_all + lane;
    const bool edge_mode = !DIR && a.mode == GSN_MODE_EDGE;
    const int64_t rows = edge_mode ? a.ec : a.nv;
    const unsigned long long n_cells = (unsigned long long)rows * (unsigned long long)a.n_cols;
    const uint32_t *col_ptr = a.plan + PLAN_HEADER_WORDS;
    const uint32_t *col_order = col_ptr + a.n_cols + 1;
    const uint32_t *plans = a.plan + a.plan[7];
    const uint64_t lane_lt = (1ull << lane) - 1ull;

    SparseGraph gr{a.row_ptr, a.nbr, 0u, 0u};
    if (DIR) gr.in_base = (uint32_t)a.nv;
    SparseLane s;
    s.plan = plans; s.k = 0; s.nfix = 0; s.tm = 0; s.tl = -1; s.l = -1; s.enter = false; s.cnt = 0;
    bool has = false, exhausted = false, rev_missing = false;
    uint32_t p_i = 0, p_e = 0, r0 = 0, r1 = 0;
    int col = 0;
    int64_t row = 0, mirror = -1, g = -1;

    for (;;) {
        const bool need = !has && !exhausted;
        uint64_t m = __ballot(need);
        if (m && __popcll(m) < SP_PULL_BATCH && __ballot(has) != 0ull) m = 0ull;
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            unsigned long long base = 0;
            if (lane == leader) base = atomicAdd(a.cell_counter, (unsigned long long)__popcll(m));
            base = __shfl(base, leader);
            if (need) {
                const unsigned long long t = base + (unsigned long long)__popcll(m & lane_lt);
                if (t >= n_cells) {
                    exhausted = true;
                } else {
                    // columns in the plan compiler's order of falling estimated cost: the long searches start first
                    col = (int)col_order[t / (unsigned long long)rows];
                    row = (int64_t)(t % (unsigned long long)rows);
                    g = a.row_graph[row];
                    if (g >= 0) {                                // (a row of a graph outside the launch: untouched)
                        int64_t *cell = a.out + ((edge_mode ? a.e0 : a.n0) + row) * a.n_cols + col;
                        const int64_t v0 = a.node_ptr[g] - a.n0;
                        bool search = a.status[g] != GSN_ST_BAD_INDEX;      // (a bad graph: zero rows)
                        mirror = -1; rev_missing = false;
                        if (search && edge_mode) {
                            int64_t u, v;
                            column_ends(a, row, v0, u, v);
                            r0 = (uint32_t)(v0 + u); r1 = (uint32_t)(v0 + v);
                            const int role = sp_edge_row(gr, a.arc_col, row, r0, r1, a.sym != 0, mirror, rev_missing);
                            if (role == SP_ROW_MIRROR) cell = nullptr;       // the reverse column's lane writes this row
                            search = role == SP_ROW_SEARCH;
                        } else if (search) {
                            r0 = (uint32_t)row; r1 = 0u;
                            search = row - v0 < (int64_t)a.vmax[v0];          // beyond the largest id of a column: not a vertex of the matched graph
                        }
                        if (search) {
                            const uint32_t vm = a.vmax[v0];
                            gr.v_lo = (uint32_t)v0; gr.v_hi = (uint32_t)v0 + vm;
                            has = true;
                            s.cnt = 0; s.l = -1;
                            p_i = col_ptr[col]; p_e = col_ptr[col + 1];
                        } else if (cell) {
                            *cell = 0;
                        }
                    }
                }
            }
        }
        if (__ballot(has) == 0ull) {
            if (__ballot(!exhausted) == 0ull) break;
            continue;
        }
        if (has) {
            if (s.l < 0) {
                if (p_i < p_e) { sp_begin<FMT>(s, plans + (size_t)p_i * stride, r0, r1, st, 64); ++p_i; }
            } else {
                sp_step<DIR, FMT>(gr, s, st, 64);
            }
            if (s.l < 0 && p_i >= p_e) {                         // the cell's last plan ended in this trip (or it had none)
                const int64_t rbase = edge_mode ? a.e0 : a.n0;
                a.out[(rbase + row) * a.n_cols + col] = (int64_t)s.cnt;
                if (mirror >= 0) a.out[(rbase + mirror) * a.n_cols + col] = (int64_t)s.cnt;
                if (edge_mode && rev_missing && s.cnt != 0) atomicMax(&a.status[g], (int)GSN_ST_KEYERROR);
                has = false;
            }
        }
    }
}

}  // namespace
}  // namespace gsn

using namespace gsn;

extern "C" int64_t gsn_count_sparse_workspace_bytes(int64_t n_vertices_total, int64_t n_columns_processed, int64_t n_cols) {
    (void)n_cols;
    if (n_vertices_total < 0 || n_columns_processed < 0 || n_vertices_total > SP_MAX_VERTICES || n_columns_processed > SP_MAX_COLUMNS) return -1;
    return sparse_layout(n_vertices_total, n_columns_processed).total;
}

#define SP_HIP(call, what)                                                                                             \
    do {                                                                                                               \
        const hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) return set_error(GSN_E_HIP, "gsn_count_sparse_hip: %s: %s", what, hipGetErrorString(e_)); \
    } while (0)

extern "C" int gsn_count_sparse_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                    const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                    int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                                    int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status, void *workspace,
                                    int64_t workspace_bytes, void *stream) {
    (void)max_nodes; (void)max_edges;                 // (no table here is sized by a single graph)
    if (!plan_host || !plan_dev || plan_words < PLAN_HEADER_WORDS || (plan_host[0] != PLAN_MAGIC && plan_host[0] != PLAN_MAGIC_WIDE))
        return set_error(GSN_E_INVALID, "gsn_count_sparse_hip: not a plan table (build it with gsn_count_plan_build)");
    const bool wide = plan_host[0] == PLAN_MAGIC_WIDE;      // patterns of 10 .. 16 vertices: the wide instantiation of the search kernel
    if (!node_ptr || !edge_ptr || !out || !status || !workspace) return set_error(GSN_E_INVALID, "gsn_count_sparse_hip: null pointer argument");
    const bool directed = (plan_host[6] & 2u) != 0;
    if (directed && plan_host[1] != (uint32_t)GSN_MODE_VERTEX)
        return set_error(GSN_E_UNSUPPORTED, "gsn_count_sparse_hip: directed plans are vertex-mode plans (no directed edge counts)");
    if (!graph_ids) n_items = n_graphs;
    if (n_graphs <= 0 || n_items <= 0) return GSN_OK;
    if (n_items >= ((int64_t)1 << 31)) return set_error(GSN_E_UNSUPPORTED, "gsn_count_sparse_hip: %lld graphs in one launch", (long long)n_items);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return set_error(GSN_E_INVALID, "gsn_count_sparse_hip: the workspace must be 256-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    // the launch's vertex and column spans: the only host reads of the call
    int64_t ends[4] = {0, 0, 0, 0};
    SP_HIP(hipMemcpyAsync(&ends[0], node_ptr, 8, hipMemcpyDeviceToHost, st), "read node_ptr");
    SP_HIP(hipMemcpyAsync(&ends[1], node_ptr + n_graphs, 8, hipMemcpyDeviceToHost, st), "read node_ptr");
    SP_HIP(hipMemcpyAsync(&ends[2], edge_ptr, 8, hipMemcpyDeviceToHost, st), "read edge_ptr");
    SP_HIP(hipMemcpyAsync(&ends[3], edge_ptr + n_graphs, 8, hipMemcpyDeviceToHost, st), "read edge_ptr");
    SP_HIP(hipStreamSynchronize(st), "synchronise");
    const int64_t nv = ends[1] - ends[0], ec = ends[3] - ends[2];
    if (ends[0] < 0 || ends[2] < 0 || nv < 0 || ec < 0) return set_error(GSN_E_INVALID, "gsn_count_sparse_hip: node_ptr / edge_ptr do not rise");
    if (nv > SP_MAX_VERTICES || ec > SP_MAX_COLUMNS)
        return set_error(GSN_E_UNSUPPORTED, "gsn_count_sparse_hip: %lld vertices / %lld columns in one launch (32-bit ids: <= %lld / %lld)", (long long)nv,
                         (long long)ec, (long long)SP_MAX_VERTICES, (long long)SP_MAX_COLUMNS);
    if (ec > 0 && !edge_index) return set_error(GSN_E_INVALID, "gsn_count_sparse_hip: edge_index is null");
    const SparseLayout L = sparse_layout(nv, ec);
    if (workspace_bytes < L.total)
        return set_error(GSN_E_NOSPACE, "gsn_count_sparse_hip: workspace of %lld bytes, %lld needed (gsn_count_sparse_workspace_bytes(%lld, %lld, .))",
                         (long long)workspace_bytes, (long long)L.total, (long long)nv, (long long)ec);

    char *ws = static_cast<char *>(workspace);
    SparseArgs a{};
    a.plan = plan_dev; a.mode = (int)plan_host[1]; a.n_cols = (int)plan_host[4];
    a.sym = (a.mode == GSN_MODE_EDGE && (plan_host[6] & 1u) == 0) ? 1 : 0;
    a.ids_are_global = ids_are_global; a.directed = directed ? 1 : 0;
    a.node_ptr = node_ptr; a.edge_ptr = edge_ptr; a.src = edge_index; a.dst = edge_index ? edge_index + edge_row_stride : nullptr;
    a.graph_ids = graph_ids; a.n_graphs = n_graphs;
    a.n0 = ends[0]; a.e0 = ends[2]; a.nv = nv; a.ec = ec; a.nr = directed ? 2 * nv : nv;
    a.out = out; a.status = status;
    a.keys_a = reinterpret_cast<uint64_t *>(ws + L.keys_a); a.keys_b = reinterpret_cast<uint64_t *>(ws + L.keys_b);
    a.nbr = reinterpret_cast<uint32_t *>(ws + L.nbr); a.arc_col = reinterpret_cast<int32_t *>(ws + L.arc_col);
    a.row_ptr = reinterpret_cast<uint32_t *>(ws + L.row_ptr); a.row_graph = reinterpret_cast<int32_t *>(ws + L.row_graph);
    a.vmax = reinterpret_cast<uint32_t *>(ws + L.vmax);
    a.cell_counter = reinterpret_cast<unsigned long long *>(ws + L.misc);
    a.n_unique = reinterpret_cast<unsigned int *>(ws + L.misc + 8);
    if (a.n_cols < 1 || plan_words < (int64_t)plan_host[7] + (int64_t)plan_host[3] * (wide ? plan_stride_wide(plan_host[6]) : plan_stride(plan_host[6])))
        return set_error(GSN_E_INVALID, "gsn_count_sparse_hip: plan table shorter than its header says");

    const int64_t arcs = 2 * ec, rows = a.mode == GSN_MODE_EDGE ? ec : nv;
    auto blocks_for = [](int64_t n) { const int64_t b = (n + SP_T - 1) / SP_T; return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); };
    const dim3 per_graph((unsigned)n_items, SP_CHUNKS);
    hipLaunchKernelGGL(sparse_fill_kernel, dim3(blocks_for(arcs > rows ? arcs : rows)), dim3(SP_T), 0, st, a);
    if (int rc = launch_check("sparse_fill_kernel launch")) return rc;
    hipLaunchKernelGGL(sparse_mark_kernel, per_graph, dim3(SP_T), 0, st, a);
    if (int rc = launch_check("sparse_mark_kernel launch")) return rc;
    hipLaunchKernelGGL(sparse_check_kernel, per_graph, dim3(SP_T), 0, st, a);
    if (int rc = launch_check("sparse_check_kernel launch")) return rc;
    const uint64_t *sorted = a.keys_a;
    if (arcs > 0) {
        hipLaunchKernelGGL(sparse_keys_kernel, per_graph, dim3(SP_T), 0, st, a);
        if (int rc = launch_check("sparse_keys_kernel launch")) return rc;
        // keys row << 32 | v with row <= nr (the end marker): the bits above those of nr are zero
        unsigned end_bit = 33;
        while (end_bit < 64 && ((uint64_t)a.nr >> (end_bit - 32)) != 0) ++end_bit;
        rocprim::double_buffer<uint64_t> keys(a.keys_a, a.keys_b);
        size_t need_sort = 0, need_unique = 0;
        SP_HIP(rocprim::radix_sort_keys(nullptr, need_sort, keys, (size_t)arcs, 0u, end_bit, st), "rocprim::radix_sort_keys (size)");
        SP_HIP(rocprim::unique(nullptr, need_unique, a.keys_a, a.keys_b, a.n_unique, (size_t)arcs, rocprim::equal_to<uint64_t>(), st), "rocprim::unique (size)");
        if ((int64_t)need_sort > L.temp_bytes || (int64_t)need_unique > L.temp_bytes)
            return set_error(GSN_E_NOSPACE, "gsn_count_sparse_hip: rocPRIM asks for %zu / %zu bytes of scratch, the layout reserves %lld", need_sort, need_unique,
                             (long long)L.temp_bytes);
        size_t tb = (size_t)L.temp_bytes;
        SP_HIP(rocprim::radix_sort_keys(ws + L.temp, tb, keys, (size_t)arcs, 0u, end_bit, st), "rocprim::radix_sort_keys");
        uint64_t *in = keys.current(), *uniq = keys.alternate();
        tb = (size_t)L.temp_bytes;
        SP_HIP(rocprim::unique(ws + L.temp, tb, in, uniq, a.n_unique, (size_t)arcs, rocprim::equal_to<uint64_t>(), st), "rocprim::unique");
        sorted = uniq;
    }
    hipLaunchKernelGGL(sparse_csr_kernel, dim3(blocks_for(arcs > a.nr + 1 ? arcs : a.nr + 1)), dim3(SP_T), 0, st, a, sorted);
    if (int rc = launch_check("sparse_csr_kernel launch")) return rc;
    if (a.mode == GSN_MODE_EDGE && arcs > 0) {
        hipLaunchKernelGGL(sparse_arc_kernel, per_graph, dim3(SP_T), 0, st, a);
        if (int rc = launch_check("sparse_arc_kernel launch")) return rc;
    }
    if (rows > 0) {
        // persistent waves: at most 16 one-wave workgroups per CU's worth of the chip, fewer when the cells are few
        const int64_t cells = rows * (int64_t)a.n_cols, want = (cells + 63) / 64;
        // (a wide search keeps 15 360 B / 19 200 B of state in LDS: 10 / 8 workgroups fit the 160 KiB of a CU, and no more are started)
        const int64_t per_cu = !wide ? 16 : LDS_LIMIT_BYTES / (int64_t)(sizeof(uint32_t) * (directed ? sparse_state_words<true, true>() : sparse_state_words<false, true>()));
        const unsigned grid = (unsigned)(want < 1 ? 1 : (want > 256 * per_cu ? 256 * per_cu : want));
        if (wide && directed) hipLaunchKernelGGL((sparse_search_kernel<true, true>), dim3(grid), dim3(64), 0, st, a);
        else if (wide) hipLaunchKernelGGL((sparse_search_kernel<false, true>), dim3(grid), dim3(64), 0, st, a);
        else if (directed) hipLaunchKernelGGL(sparse_search_kernel<true>, dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL(sparse_search_kernel<false>, dim3(grid), dim3(64), 0, st, a);
        if (int rc = launch_check("sparse_search_kernel launch")) return rc;
    }
    return GSN_OK;
}
