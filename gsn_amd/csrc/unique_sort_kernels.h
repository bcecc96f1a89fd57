// The sort kernels of unique_sort_core.h's network and their launcher, shared by the translation units that sort uint64 key columns
// (unique_sort.hip: keys from int64 values; evaluate.hip: keys from scores and labels).  A caller supplies the key LOAD of the first tile
// pass -- a trivially copyable functor  uint64_t operator()(int64_t row, int64_t n_cols, int64_t col) const  -- everything behind it works
// on the key columns alone.  Kernels have internal linkage (templates / static): every translation unit carries its own copies.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "unique_sort_core.h"

namespace gsn {

constexpr int64_t US_MAX_GRID_X = 1 << 20;

__device__ __forceinline__ void us_cmpswap_lds(uint64_t *s, int lo, int hi) {
    const uint64_t a = s[lo], b = s[hi];
    if (a > b) { s[lo] = b; s[hi] = a; }
}

// FIRST: keys from `load`, stages 1 .. US_LOG_TILE (a full sort of the tile).  Otherwise: the steps US_LOG_TILE-1 .. 0 of a later stage.
// Positions >= m hold the largest key in LDS: they never move (every pair leaves its smaller key low) and are not written back.
template <bool FIRST, class Load>
__global__ __launch_bounds__(256) void us_tile_kernel(int64_t m, int64_t n_cols, Load load, uint64_t *keys, int64_t n_tiles) {
    __shared__ uint64_t s[US_TILE];
    const int64_t c = blockIdx.y;
    uint64_t *kc = keys + c * m;
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * US_TILE;
        for (int i = tid; i < US_TILE; i += 256) {
            const int64_t g = base + i;
            s[i] = g < m ? (FIRST ? load(g, n_cols, c) : kc[g]) : ~0ull;
        }
        __syncthreads();
        const int k_first = FIRST ? 1 : US_LOG_TILE + 1, k_last = FIRST ? US_LOG_TILE : US_LOG_TILE + 1;
        for (int k = k_first; k <= k_last; ++k) {
            if (FIRST) {
                for (int t = tid; t < US_TILE / 2; t += 256) {
                    int64_t lo, hi;
                    us_pair_flip(t, k, lo, hi);
                    us_cmpswap_lds(s, (int)lo, (int)hi);
                }
                __syncthreads();
            }
            for (int j = FIRST ? k - 2 : US_LOG_TILE - 1; j >= 0; --j) {
                for (int t = tid; t < US_TILE / 2; t += 256) {
                    int64_t lo, hi;
                    us_pair_step(t, j, lo, hi);
                    us_cmpswap_lds(s, (int)lo, (int)hi);
                }
                __syncthreads();
            }
        }
        for (int i = tid; i < US_TILE; i += 256) {
            const int64_t g = base + i;
            if (g < m) kc[g] = s[i];
        }
        __syncthreads();
    }
}

// one step over whole columns: flip of stage kj, or step kj
static __global__ __launch_bounds__(256) void us_global_kernel(int64_t m, uint64_t *keys, int kj, int flip, int64_t n_pairs) {
    uint64_t *kc = keys + (int64_t)blockIdx.y * m;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_pairs; t += (int64_t)gridDim.x * 256) {
        int64_t lo, hi;
        if (flip) us_pair_flip(t, kj, lo, hi); else us_pair_step(t, kj, lo, hi);
        if (hi < m) {
            const uint64_t a = kc[lo], b = kc[hi];
            if (a > b) { kc[lo] = b; kc[hi] = a; }
        }
    }
}

static inline unsigned us_grid(int64_t blocks) { return (unsigned)(blocks < 1 ? 1 : (blocks > US_MAX_GRID_X ? US_MAX_GRID_X : blocks)); }

// the `ops` of us_schedule: one sort of the m keys of each of n_cols columns (n_cols <= 65535: the grid's y extent)
template <class Load>
struct UsLaunches {
    int64_t m, n_cols;
    Load load;
    uint64_t *keys;
    hipStream_t s;
    int64_t n_tiles() const { return (m + US_TILE - 1) / US_TILE; }
    void tile_sort() { hipLaunchKernelGGL((us_tile_kernel<true, Load>), dim3(us_grid(n_tiles()), (unsigned)n_cols), dim3(256), 0, s, m, n_cols, load, keys, n_tiles()); }
    void tile_merge() { hipLaunchKernelGGL((us_tile_kernel<false, Load>), dim3(us_grid(n_tiles()), (unsigned)n_cols), dim3(256), 0, s, m, n_cols, load, keys, n_tiles()); }
    void global(int kj, int flip, int64_t n_pairs) {
        hipLaunchKernelGGL(us_global_kernel, dim3(us_grid((n_pairs + 255) / 256), (unsigned)n_cols), dim3(256), 0, s, m, keys, kj, flip, n_pairs);
    }
    void global_flip(int k) { global(k, 1, us_pair_count(m, k - 1)); }
    void global_step(int j) { global(j, 0, us_pair_count(m, j)); }
};

}  // namespace gsn
