// A collated batch of a device-resident dataset in one launch (gsn_amd/loader.py; gsn_loader_collate_hip in gsn_abi.h).
//
// One wave per (field, slot) pair; the address arithmetic and the per-lane routine are loader_core.h's, shared with the host harness of
// the tests.  The field table is a kernel argument: nothing is uploaded per batch.  Launch shape: workgroups of four waves; the grid
// covers the pairs once up to LD_MAX_BLOCKS workgroups (eight per CU of a 256-CU device) and strides beyond.  At the reference's batch
// sizes (32 - 128 graphs, ~8 fields) that is a few hundred short waves: the launch is latency-bound and one round of waves is the
// shortest it can be.  Copies move single elements of the field's own width (4 or 8 bytes), consecutive lanes on consecutive elements:
// rows of 20 bytes occur, so nothing wider is known to be aligned on both sides.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsn_internal.h"
#include "loader_core.h"

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
