// A collated batch of a device-resident dataset in one launch (gsn_amd/loader.py; gsn_loader_collate_hip in gsn_abi.h).
//
// One wave per (field, slot) pair; the address arithmetic and the per-lane routine are loader_core.h's, shared with the host harness of
// the tests.  The field table is a kernel argument: nothing is uploaded per batch.  Launch shape: workgroups of four waves; the grid
// covers the pairs once up to LD_MAX_BLOCKS workgroups (eight per CU of a 256-CU device) and strides beyond.  At the reference's batch
// sizes (32 - 128 graphs, ~8 fields) that is a few hundred short waves: the launch is latency-bound and one round of waves is the
// shortest it can be.  Copies move single elements of the field's own width (4 or 8 bytes), consecutive lanes on consecutive elements:
// rows of 20 bytes occur, so nothing wider is known to be aligned on both sides.
//
// The same batch collated into static buffers of fixed capacity and filled up with pad graphs (gsn_loader_collate_padded_hip; PaddedDataLoader):
// a second kernel of the same launch shape over all graph slots, its arithmetic in loader_padded_core.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsn_internal.h"
#include "loader_core.h"
#include "loader_padded_core.h"

namespace gsn {

constexpr int LD_THREADS = LD_WAVE * LD_WAVES_PER_BLOCK;
constexpr int64_t LD_MAX_BLOCKS = 2048;

struct LoaderTable {
    gsn_loader_field f[GSN_LOADER_MAX_FIELDS];
};

__global__ __launch_bounds__(LD_THREADS) void loader_collate_kernel(const LoaderTable tab, int n_fields, const int64_t *__restrict__ order,
                                                                    const int64_t *__restrict__ plan, int64_t stride, int64_t first,
                                                                    int64_t batch, int64_t *batch_vec, int64_t *node_ptr_out,
                                                                    int64_t *edge_ptr_out) {
    const int lane = threadIdx.x & (LD_WAVE - 1);
    // (wave-uniform by construction; said to the compiler so that the table is read through scalar loads)
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * LD_WAVES_PER_BLOCK + (threadIdx.x >> 6)));
    const int64_t n_pairs = (int64_t)n_fields * batch;
    const int64_t n_waves = (int64_t)gridDim.x * LD_WAVES_PER_BLOCK;
    for (int64_t pair = wave; pair < n_pairs; pair += n_waves) {
        int field;
        int64_t slot;
        ld_pair_of(pair, batch, &field, &slot);
        ld_run_pair(tab.f[field], order, plan, stride, first, batch, slot, lane, batch_vec, node_ptr_out, edge_ptr_out);
    }
}

// The padded collate (loader_padded_core.h): the same launch shape over n_fields * G_cap pairs.  Fill words and the batch's numbers are
// kernel arguments as the table is: read through scalar loads, nothing uploaded per batch.
struct LoaderFill {
    uint64_t w[GSN_LOADER_MAX_FIELDS];
};

__global__ __launch_bounds__(LD_THREADS) void loader_collate_padded_kernel(const LoaderTable tab, const LoaderFill fill, const gsn_loader_pad pad,
                                                                           int n_fields, const int64_t *__restrict__ order,
                                                                           const int64_t *__restrict__ plan, int64_t stride, int64_t first,
                                                                           int64_t *batch_vec, int64_t *node_ptr_out, int64_t *edge_ptr_out,
                                                                           int64_t *n_valid) {
    const int lane = threadIdx.x & (LD_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * LD_WAVES_PER_BLOCK + (threadIdx.x >> 6)));
    const int64_t n_pairs = (int64_t)n_fields * pad.graph_slots;
    const int64_t n_waves = (int64_t)gridDim.x * LD_WAVES_PER_BLOCK;
    for (int64_t pair = wave; pair < n_pairs; pair += n_waves) {
        int field;
        int64_t slot;
        ld_pair_of(pair, pad.graph_slots, &field, &slot);
        lp_run_pair(tab.f[field], fill.w[field], pad, order, plan, stride, first, slot, lane, batch_vec, node_ptr_out, edge_ptr_out, n_valid);
    }
}

}  // namespace gsn

using namespace gsn;

extern "C" int gsn_loader_collate_hip(int n_fields, const gsn_loader_field *fields, const int64_t *order, const int64_t *plan,
                                      int64_t n_graphs_total, int64_t first, int64_t batch, int64_t *batch_vec, int64_t *node_ptr_out,
                                      int64_t *edge_ptr_out, void *stream) {
    if (n_fields < 0 || n_fields > GSN_LOADER_MAX_FIELDS)
        return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: %d fields (0 .. %d)", n_fields, GSN_LOADER_MAX_FIELDS);
    if (n_graphs_total < 0 || first < 0 || batch < 0 || batch > n_graphs_total || first > n_graphs_total - batch)
        return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: positions [%lld, %lld + %lld) outside the order's %lld", (long long)first,
                         (long long)first, (long long)batch, (long long)n_graphs_total);
    if (n_fields > 0 && !fields) return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: null field table");
    LoaderTable tab = {};
    bool rows = false;
    for (int i = 0; i < n_fields; ++i) {
        const gsn_loader_field &f = fields[i];
        if (f.elem_bytes != 4 && f.elem_bytes != 8)
            return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d moves elements of %d bytes (4 or 8)", i, f.elem_bytes);
        if (f.kind != GSN_LOADER_COPY && f.kind != GSN_LOADER_EDGE_INDEX)
            return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d has unknown kind %d", i, f.kind);
        if (f.row_bytes <= 0 || f.row_bytes % f.elem_bytes != 0)
            return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d has rows of %lld bytes (a positive multiple of its %d-byte elements)", i,
                             (long long)f.row_bytes, f.elem_bytes);
        if (f.ptr_class < 0 || f.dst_rows < 0)
            return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d has a negative pointer class or row count", i);
        if (f.kind == GSN_LOADER_EDGE_INDEX && (f.elem_bytes != 8 || f.row_bytes != 8 || f.inc_class < 0 || f.src_stride < 0 || f.dst_stride < f.dst_rows))
            return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d (edge_index) needs int64 elements, a vertex class and row strides that hold its columns", i);
        if (!f.row_ptr) return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d has no row pointer", i);
        if (f.dst_rows > 0 && (!f.src || !f.dst))
            return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: field %d has %lld rows and a null source or destination", i, (long long)f.dst_rows);
        rows = rows || f.dst_rows > 0;
        tab.f[i] = f;
    }
    if (batch == 0 || n_fields == 0 || (!rows && !node_ptr_out && !edge_ptr_out)) return GSN_OK;
    if (!order || !plan) return set_error(GSN_E_INVALID, "gsn_loader_collate_hip: null order or plan");
    const int64_t n_pairs = (int64_t)n_fields * batch;
    int64_t blocks = (n_pairs + LD_WAVES_PER_BLOCK - 1) / LD_WAVES_PER_BLOCK;
    if (blocks > LD_MAX_BLOCKS) blocks = LD_MAX_BLOCKS;
    hipLaunchKernelGGL(loader_collate_kernel, dim3((unsigned)blocks), dim3(LD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), tab, n_fields,
                       order, plan, n_graphs_total, first, batch, batch_vec, node_ptr_out, edge_ptr_out);
    return launch_check("loader_collate_kernel");
}

extern "C" int gsn_loader_collate_padded_hip(int n_fields, const gsn_loader_field *fields, const uint64_t *fill, const int64_t *order,
                                             const int64_t *plan, int64_t n_graphs_total, int64_t first, const gsn_loader_pad *pad,
                                             int64_t *batch_vec, int64_t *node_ptr_out, int64_t *edge_ptr_out, int64_t *n_valid, void *stream) {
    const char *who = "gsn_loader_collate_padded_hip";
    if (n_fields < 1 || n_fields > GSN_LOADER_MAX_FIELDS) return set_error(GSN_E_INVALID, "%s: %d fields (1 .. %d)", who, n_fields, GSN_LOADER_MAX_FIELDS);
    if (!fields || !fill || !pad || !order || !plan || !node_ptr_out) return set_error(GSN_E_INVALID, "%s: null table, fill, pad, order, plan or node pointer", who);
    const gsn_loader_pad p = *pad;
    if (p.graph_slots < 2 || p.node_capacity < 0 || p.edge_capacity < 0 || p.node_capacity > ((int64_t)1 << 48) || p.edge_capacity > ((int64_t)1 << 48) ||
        p.graph_slots > ((int64_t)1 << 40) || p.n_chunk > ((int64_t)1 << 40) || p.e_chunk > ((int64_t)1 << 40))
        return set_error(GSN_E_INVALID, "%s: capacities of %lld vertices, %lld edge columns, %lld slots", who, (long long)p.node_capacity,
                         (long long)p.edge_capacity, (long long)p.graph_slots);
    if (!lp_fits(p))
        return set_error(GSN_E_INVALID, "%s: %lld graphs of %lld vertices / %lld edge columns do not fit %lld slots, %lld vertices, %lld edge columns in chunks of %lld / %lld",
                         who, (long long)p.n_real, (long long)p.n_real_nodes, (long long)p.n_real_edges, (long long)p.graph_slots,
                         (long long)p.node_capacity, (long long)p.edge_capacity, (long long)p.n_chunk, (long long)p.e_chunk);
    if (n_graphs_total < 0 || first < 0 || p.n_real > n_graphs_total || first > n_graphs_total - p.n_real)
        return set_error(GSN_E_INVALID, "%s: positions [%lld, %lld + %lld) outside the order's %lld", who, (long long)first, (long long)first,
                         (long long)p.n_real, (long long)n_graphs_total);
    LoaderTable tab = {};
    LoaderFill words = {};
    int node_fields = 0;
    for (int i = 0; i < n_fields; ++i) {
        const gsn_loader_field &f = fields[i];
        if (f.elem_bytes != 4 && f.elem_bytes != 8) return set_error(GSN_E_INVALID, "%s: field %d moves elements of %d bytes (4 or 8)", who, i, f.elem_bytes);
        if (f.kind != GSN_LOADER_COPY && f.kind != GSN_LOADER_EDGE_INDEX) return set_error(GSN_E_INVALID, "%s: field %d has unknown kind %d", who, i, f.kind);
        if (f.row_bytes <= 0 || f.row_bytes % f.elem_bytes != 0)
            return set_error(GSN_E_INVALID, "%s: field %d has rows of %lld bytes (a positive multiple of its %d-byte elements)", who, i, (long long)f.row_bytes,
                             f.elem_bytes);
        if (f.ptr_class < 0 || !f.row_ptr) return set_error(GSN_E_INVALID, "%s: field %d has no pointer class or row pointer", who, i);
        const bool edges = f.kind == GSN_LOADER_EDGE_INDEX || (f.flags & GSN_LOADER_F_PAD_EDGES), graph = (f.flags & GSN_LOADER_F_PAD_GRAPH) != 0;
        if (f.kind == GSN_LOADER_EDGE_INDEX && (f.elem_bytes != 8 || f.row_bytes != 8 || f.inc_class < 0 || f.src_stride < 0 || f.dst_stride < f.dst_rows || graph))
            return set_error(GSN_E_INVALID, "%s: field %d (edge_index) needs int64 elements, a vertex class and row strides that hold its columns", who, i);
        if ((edges && graph) || ((f.flags & GSN_LOADER_F_NODES) && (edges || graph)))
            return set_error(GSN_E_INVALID, "%s: field %d is marked as more than one of per-vertex, per-edge, per-graph", who, i);
        const int64_t cap = graph ? p.graph_slots : edges ? p.edge_capacity : p.node_capacity;
        if (f.dst_rows != cap) return set_error(GSN_E_INVALID, "%s: field %d has %lld destination rows, its capacity is %lld", who, i, (long long)f.dst_rows, (long long)cap);
        if (cap > 0 && (!f.src || !f.dst)) return set_error(GSN_E_INVALID, "%s: field %d has %lld rows and a null source or destination", who, i, (long long)cap);
        node_fields += (f.flags & GSN_LOADER_F_NODES) != 0;
        tab.f[i] = f;
        words.w[i] = fill[i];
    }
    if (node_fields != 1) return set_error(GSN_E_INVALID, "%s: %d fields carry GSN_LOADER_F_NODES (exactly one: it owns batch_vec, the node pointer and n_valid)", who, node_fields);
    const int64_t n_pairs = (int64_t)n_fields * p.graph_slots;
    int64_t blocks = (n_pairs + LD_WAVES_PER_BLOCK - 1) / LD_WAVES_PER_BLOCK;
    if (blocks > LD_MAX_BLOCKS) blocks = LD_MAX_BLOCKS;
    hipLaunchKernelGGL(loader_collate_padded_kernel, dim3((unsigned)blocks), dim3(LD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), tab, words, p,
                       n_fields, order, plan, n_graphs_total, first, batch_vec, node_ptr_out, edge_ptr_out, n_valid);
    return launch_check("loader_collate_padded_kernel");
}
