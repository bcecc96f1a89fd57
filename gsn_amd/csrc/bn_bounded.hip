// Train-mode BatchNorm1d bookkeeping of a stage whose rows are a PADDED batch (gsn_amd.loader.PaddedDataLoader): the real rows are the prefix
// [0, v) of the m_rows the stage ran over, v read from device memory (bn_bounded_core.h), and the statistics are those of the real rows.
//
// The producers of the column sums (the product kernels) sum over all m_rows rows; this launch stands where gsn_bn_finalize_count_hip stands
// and corrects them from the materialised pre-BN rows h, over the SHORTER of the two row ranges:
//     v <= m_rows - v :  sums over rows [0, v) taken directly (the given sums are not read)
//     otherwise       :  sums over rows [v, m_rows) taken and subtracted from the given sums, in fp64
// so no more than half the rows are read.  One wave covers 64 adjacent columns of one row, waves stride over rows, four rows' loads in flight
// (bn_act_bwd_reduce_kernel's pattern).  The grid is sized by the capacity m_rows (the launch shape is frozen under stream capture), several
// workgroups per column group once the half range is long: their partials go by fp64 atomics into a zeroed scratch, every workgroup then
// draws a ticket of its column group, and the one that draws the last finalises the group's columns with bn_finalize_kernel's expressions
// (bn_finalize_column).  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bn_bounded_core.h"
#include "gsn_internal.h"

namespace gsn {

constexpr int BNB_MAX_WGS = 64;      // workgroups per column group: one fp64 atomic pair per column each, which the L2 serialises (~20 ns)
constexpr int BNB_ROWS_PER_WG = 64;  // a workgroup takes at least 64 rows of the half range (16 per wave), as backward.hip's bgrid

__global__ __launch_bounds__(256) void bn_finalize_bounded_kernel(int n_cols, int64_t m_rows, double eps, double momentum, const double *stats,
                                                                  const float *h, RowBound bound, double *part, unsigned *tickets,
                                                                  const float *gamma, const float *beta, float *running_mean,
                                                                  float *running_var, float *mean, float *invstd, float *scale, float *shift,
                                                                  int64_t *num_batches_tracked) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool cok = c < n_cols;
    const int64_t v = bound_rows(bound, m_rows);
    const bool direct = v <= m_rows - v;
    const int64_t r_end = direct ? v : m_rows;
    double s1 = 0.0, s2 = 0.0;
    if (cok) {
        const int64_t step = (int64_t)gridDim.x * 4;
        int64_t r = (direct ? 0 : v) + (int64_t)blockIdx.x * 4 + wave;
        for (; r + 3 * step < r_end; r += 4 * step) {
            float h4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) h4[u] = h[(r + u * step) * n_cols + c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s1 += (double)h4[u];
                s2 += (double)h4[u] * (double)h4[u];
            }
        }
        for (; r < r_end; r += step) {
            const float hv = h[r * n_cols + c];
            s1 += (double)hv;
            s2 += (double)hv * (double)hv;
        }
    }
    __shared__ double red[2][4][64];
    __shared__ bool s_last;
    red[0][wave][lane] = s1;
    red[1][wave][lane] = s2;
    __syncthreads();
    if (wave == 0 && cok) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < 4; ++w) { a += red[0][w][lane]; b += red[1][w][lane]; }
        __hip_atomic_fetch_add(&part[c], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&part[n_cols + c], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&tickets[blockIdx.y], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (!s_last || wave != 0 || !cok) return;      // every workgroup of the column group has added its partials
    if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;
    if (v == 0) {      // no real row: nn.BatchNorm1d leaves the running statistics alone and still counts the batch
        mean[c] = 0.f; invstd[c] = 1.f; scale[c] = 1.f; shift[c] = 0.f;
        return;
    }
    const double p1 = __hip_atomic_load(&part[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double p2 = __hip_atomic_load(&part[n_cols + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double t1 = direct ? p1 : stats[c] - p1, t2 = direct ? p2 : stats[n_cols + c] - p2;
    bn_finalize_column(c, t1, t2, (double)v, eps, momentum, gamma, beta, running_mean, running_var, mean, invstd, scale, shift);
}

static int bnb_grid(int64_t m_rows) {
    const int64_t half = (m_rows + 1) / 2, b = (half + BNB_ROWS_PER_WG - 1) / BNB_ROWS_PER_WG;
    return (int)(b < 1 ? 1 : (b > BNB_MAX_WGS ? BNB_MAX_WGS : b));
}

}  // namespace gsn

using namespace gsn;

extern "C" int64_t gsn_bn_finalize_bounded_scratch_bytes(int64_t n_cols) {
    if (n_cols < 1) return 0;
    return 16 * n_cols + (4 * ((n_cols + 63) / 64) + 7) / 8 * 8;
}

extern "C" int gsn_bn_finalize_bounded_hip(int64_t n_cols, int64_t m_rows, double eps, double momentum, const double *stats, const float *h,
                                           const int64_t *n_valid, const int64_t *row_ptr, int64_t n_slots, void *scratch,
                                           const float *gamma, const float *beta, float *running_mean, float *running_var, float *mean,
                                           float *invstd, float *scale, float *shift, int64_t *num_batches_tracked, void *stream) {
    if (n_cols < 1 || n_cols > INT32_MAX || m_rows < 1 || !stats || !h || !n_valid || !scratch || !mean || !invstd || !scale || !shift ||
        ((running_mean != nullptr) != (running_var != nullptr)) || n_slots < 0 || (row_ptr == nullptr && n_slots != 0))
        return set_error(GSN_E_INVALID, "gsn_bn_finalize_bounded_hip: bad arguments");
    if (reinterpret_cast<uintptr_t>(scratch) & 7) return set_error(GSN_E_INVALID, "gsn_bn_finalize_bounded_hip: scratch must be 8-byte aligned");
    double *part = reinterpret_cast<double *>(scratch);
    unsigned *tickets = reinterpret_cast<unsigned *>(part + 2 * n_cols);
    const dim3 grid((unsigned)bnb_grid(m_rows), (unsigned)((n_cols + 63) / 64));
    hipLaunchKernelGGL(bn_finalize_bounded_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (int)n_cols, m_rows, eps, momentum,
                       stats, h, RowBound{n_valid, row_ptr, n_slots}, part, tickets, gamma, beta, running_mean, running_var, mean, invstd, scale,
                       shift, num_batches_tracked);
    return launch_check("bn_finalize_bounded_kernel");
}
