// Dataset-level recoding of int64 columns over their FULL value range (utils_encoding.one_hot_unique, utils_encoding.py:37-59): per column
// np.unique(values[:, c], return_inverse=True) by a keys-only sort, and the lookup of further rows in the sorted distinct values a fit left
// behind.  The presence-table kernels of encode.hip index a table by value - min and stop at 2^28 entries; nothing here depends on the range.
//
//   gsn_unique_sort_hip:   keys = values ^ 2^63 per column            (tile kernel of unique_sort_kernels.h: loads, sorts every tile in LDS)
//                          bitonic merge stages in one direction      (unique_sort_core.h: global steps at distance >= US_TILE, the rest in LDS)
//                          run starts -> counts per chunk -> scan -> compaction into `uniques`, n_distinct
//                          codes[r][c] = position of values[r][c] in uniques[c]   (one binary search per element)
//   gsn_lookup_codes_hip:  the same search against given sorted values; strict (unseen -> -1 + status) or clamp
//
// No atomics on data, no scatter that depends on arrival order, no loop that waits for another workgroup: two runs give the same bytes.
// Every loop is bounded by M, C, or the key width (stages k <= 63, 64 halvings of a search).  Run once per dataset: HBM-bound passes, not tuned.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsn_internal.h"
#include "unique_sort_core.h"
#include "unique_sort_kernels.h"

namespace gsn {

// the key load of the first tile pass (unique_sort_kernels.h): signed int64 order as unsigned words
struct UsValueLoad {
    const int64_t *values;
    __device__ __forceinline__ uint64_t operator()(int64_t row, int64_t n_cols, int64_t col) const { return us_key(values[row * n_cols + col]); }
};

// exclusive prefix of v over the 256 threads of a workgroup, *total = the sum (all threads call; ends with a barrier)
__device__ __forceinline__ int64_t us_block_scan(int64_t v, int64_t *total) {
    __shared__ int64_t wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int64_t off = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

__global__ __launch_bounds__(256) void us_count_kernel(int64_t m, const uint64_t *keys, int64_t *chunk_count, int64_t n_chunks) {
    const int64_t c = blockIdx.y;
    const uint64_t *kc = keys + c * m;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int flags = us_run_starts(kc, m, ch * US_CHUNK + 4 * (int64_t)threadIdx.x);
        int64_t total;
        us_block_scan(__popc(flags), &total);
        if (threadIdx.x == 0) chunk_count[c * n_chunks + ch] = total;
    }
}

// one workgroup per column: chunk counts -> exclusive prefix in place, their sum to n_distinct
__global__ __launch_bounds__(256) void us_scan_kernel(int64_t n_chunks, int64_t *chunk_count, int64_t *n_distinct) {
    const int64_t c = blockIdx.x;
    int64_t *cc = chunk_count + c * n_chunks;
    int64_t carry = 0;
    for (int64_t base = 0; base < n_chunks; base += 256) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < n_chunks ? cc[i] : 0;
        int64_t total;
        const int64_t ex = us_block_scan(v, &total);
        if (i < n_chunks) cc[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) n_distinct[c] = carry;
}

__global__ __launch_bounds__(256) void us_compact_kernel(int64_t m, const uint64_t *keys, const int64_t *chunk_offset, int64_t n_chunks,
                                                         int64_t *uniques) {
    const int64_t c = blockIdx.y;
    const uint64_t *kc = keys + c * m;
    int64_t *uc = uniques + c * m;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t i0 = ch * US_CHUNK + 4 * (int64_t)threadIdx.x;
        const int flags = us_run_starts(kc, m, i0);
        int64_t total;
        int64_t pos = chunk_offset[c * n_chunks + ch] + us_block_scan(__popc(flags), &total);
        for (int u = 0; u < 4; ++u)
            if ((flags >> u) & 1) uc[pos++] = us_value(kc[i0 + u]);      // (pos < number of run starts <= m; i0 + u < m where the bit is set)
    }
}

__global__ __launch_bounds__(256) void us_codes_kernel(int64_t m, int64_t n_cols, const int64_t *values, const int64_t *uniques,
                                                       const int64_t *n_distinct, int64_t *codes) {
    const int64_t total = m * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i % n_cols;
        bool unseen;
        codes[i] = us_lookup(uniques + c * m, n_distinct[c], values[i], 0, &unseen);
    }
}

__global__ __launch_bounds__(256) void us_lookup_kernel(int64_t n_rows, int64_t n_cols, const int64_t *values, const int64_t *uniques,
                                                        const int64_t *col_ptr, int clamp, int64_t *codes, int32_t *status,
                                                        int64_t *first_unseen) {
    const int64_t total = n_rows * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t c = i % n_cols;
        const int64_t p0 = col_ptr[c], n = col_ptr[c + 1] - p0;
        bool unseen;
        codes[i] = us_lookup(uniques + p0, n, values[i], clamp, &unseen);
        if (unseen && !clamp) {
            atomicMax(status, (int32_t)GSN_ST_UNSEEN);
            atomicMin(reinterpret_cast<unsigned long long *>(first_unseen), (unsigned long long)i);
        }
    }
}

static int64_t us_chunks(int64_t m) { return (m + US_CHUNK - 1) / US_CHUNK; }
static int64_t us_keys_bytes(int64_t m, int64_t c) { return (8 * m * c + 255) / 256 * 256; }

}  // namespace gsn

using namespace gsn;

extern "C" int64_t gsn_unique_sort_scratch_bytes(int64_t m_rows, int64_t n_cols) {
    if (m_rows <= 0 || n_cols <= 0) return 0;
    return us_keys_bytes(m_rows, n_cols) + (8 * us_chunks(m_rows) * n_cols + 255) / 256 * 256;
}

extern "C" int gsn_unique_sort_hip(int64_t m_rows, int64_t n_cols, const int64_t *values, int64_t *uniques, int64_t *n_distinct,
                                   int64_t *codes, void *scratch, int64_t scratch_bytes, void *stream) {
    if (m_rows < 0 || n_cols < 0) return set_error(GSN_E_INVALID, "gsn_unique_sort_hip: negative shape");
    if (m_rows == 0 || n_cols == 0) return GSN_OK;
    if (n_cols > 65535 || m_rows > ((int64_t)1 << 40) / n_cols)
        return set_error(GSN_E_UNSUPPORTED, "gsn_unique_sort_hip: more than 65535 columns or 2^40 elements");
    if (!values || !uniques || !n_distinct || !codes || !scratch)
        return set_error(GSN_E_INVALID, "gsn_unique_sort_hip: null pointer with %lld x %lld values", (long long)m_rows, (long long)n_cols);
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) != 0) return set_error(GSN_E_INVALID, "gsn_unique_sort_hip: scratch must be 8-byte aligned");
    const int64_t need = gsn_unique_sort_scratch_bytes(m_rows, n_cols);
    if (scratch_bytes < need)
        return set_error(GSN_E_NOSPACE, "gsn_unique_sort_hip: scratch of %lld bytes < %lld", (long long)scratch_bytes, (long long)need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t *keys = reinterpret_cast<uint64_t *>(scratch);
    int64_t *chunk_count = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(scratch) + us_keys_bytes(m_rows, n_cols));
    UsLaunches<UsValueLoad> ops{m_rows, n_cols, UsValueLoad{values}, keys, s};
    us_schedule(m_rows, ops);
    const int64_t n_chunks = us_chunks(m_rows);
    const dim3 cgrid(us_grid(n_chunks), (unsigned)n_cols);
    hipLaunchKernelGGL(us_count_kernel, cgrid, dim3(256), 0, s, m_rows, keys, chunk_count, n_chunks);
    hipLaunchKernelGGL(us_scan_kernel, dim3((unsigned)n_cols), dim3(256), 0, s, n_chunks, chunk_count, n_distinct);
    hipLaunchKernelGGL(us_compact_kernel, cgrid, dim3(256), 0, s, m_rows, keys, chunk_count, n_chunks, uniques);
    hipLaunchKernelGGL(us_codes_kernel, dim3(us_grid((m_rows * n_cols + 255) / 256)), dim3(256), 0, s, m_rows, n_cols, values, uniques,
                       n_distinct, codes);
    return launch_check("unique sort kernels");
}

extern "C" int gsn_lookup_codes_hip(int64_t n_rows, int64_t n_cols, const int64_t *values, const int64_t *uniques, const int64_t *col_ptr,
                                    int mode, int64_t *codes, int32_t *status, int64_t *first_unseen, void *stream) {
    if (n_rows < 0 || n_cols < 0 || (mode != GSN_LOOKUP_STRICT && mode != GSN_LOOKUP_CLAMP))
        return set_error(GSN_E_INVALID, "gsn_lookup_codes_hip: negative shape or unknown mode %d", mode);
    if (n_rows == 0 || n_cols == 0) return GSN_OK;
    if (n_rows > ((int64_t)1 << 40) / n_cols) return set_error(GSN_E_UNSUPPORTED, "gsn_lookup_codes_hip: more than 2^40 elements");
    // (`uniques` may be null when every column is empty: it is then never read)
    if (!values || !col_ptr || !codes || (mode == GSN_LOOKUP_STRICT && (!status || !first_unseen)))
        return set_error(GSN_E_INVALID, "gsn_lookup_codes_hip: null pointer with %lld x %lld values", (long long)n_rows, (long long)n_cols);
    hipLaunchKernelGGL(us_lookup_kernel, dim3(us_grid((n_rows * n_cols + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       n_rows, n_cols, values, uniques, col_ptr, mode == GSN_LOOKUP_CLAMP ? 1 : 0, codes, status, first_unseen);
    return launch_check("us_lookup_kernel");
}
