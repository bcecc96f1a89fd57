// Sorted distinct values of int64 columns over their full range: the index arithmetic of the sorting network, its launch schedule and
// the searches, shared between the HIP kernels (unique_sort.hip) and a host-side logic harness used ONLY by tests
// (tests/unique_sort_harness.cpp compiles this header with g++; it is not a product fallback).
//
// The sort is the bitonic network in its one-direction form: stage k = 1, 2, ... merges sorted runs of 2^(k-1) keys into runs of 2^k,
//   first a FLIP step    pairs (i, i ^ (2^k - 1))  inside every 2^k block,
//   then  steps j = k-2 .. 0   pairs (i, i + 2^j),
// and EVERY pair leaves its smaller key at the lower index.  Positions >= M therefore behave as +infinity that never moves: a pair whose
// upper position is >= M is skipped, and any M is sorted without padding.  The pairs of a step are disjoint, no step depends on the order
// in which its pairs run, and the keys are compared as biased unsigned words (value ^ 2^63: signed int64 order, no subtraction anywhere).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define US_HD __host__ __device__ __forceinline__
#else
#define US_HD inline
#endif

namespace gsn {

constexpr int US_LOG_TILE = 12;
constexpr int US_TILE = 1 << US_LOG_TILE;      // keys of one LDS tile (32 KiB): steps whose pairs are closer than this run inside a tile
constexpr int US_CHUNK = 1024;                 // keys per workgroup of the compaction passes (256 threads x 4)
constexpr uint64_t US_BIAS = 0x8000000000000000ull;

US_HD uint64_t us_key(int64_t v) { return (uint64_t)v ^ US_BIAS; }
US_HD int64_t us_value(uint64_t k) { return (int64_t)(k ^ US_BIAS); }

// pair t of the flip step of stage k (t counts the lower halves of the 2^k blocks)
US_HD void us_pair_flip(int64_t t, int k, int64_t &lo, int64_t &hi) {
    const int64_t half = (int64_t)1 << (k - 1);
    const int64_t b = t >> (k - 1), o = t & (half - 1);
    lo = (b << k) + o;
    hi = (b << k) + 2 * half - 1 - o;
}
// pair t of step j
US_HD void us_pair_step(int64_t t, int j, int64_t &lo, int64_t &hi) {
    const int64_t d = (int64_t)1 << j;
    lo = ((t >> j) << (j + 1)) + (t & (d - 1));
    hi = lo + d;
}
// pair indices t = 0 .. us_pair_count - 1 cover every pair of a step at distance (or block half) 2^j whose lower position is < m
US_HD int64_t us_pair_count(int64_t m, int j) {
    const int64_t d = (int64_t)1 << j;
    return ((m + 2 * d - 1) >> (j + 1)) << j;
}

// The launches of one sort of m keys per column, in order.  ops: tile_sort() -- stages 1 .. US_LOG_TILE of every tile; global_flip(k),
// global_step(j) -- one step over the whole column; tile_merge() -- steps US_LOG_TILE-1 .. 0 of every tile.  Every loop is bounded by the key
// width: 2^(k-1) < m <= 2^63.
template <class Ops>
inline void us_schedule(int64_t m, Ops &ops) {
    ops.tile_sort();
    for (int k = US_LOG_TILE + 1; k <= 63 && ((int64_t)1 << (k - 1)) < m; ++k) {
        ops.global_flip(k);
        for (int j = k - 2; j >= US_LOG_TILE; --j) ops.global_step(j);
        ops.tile_merge();
    }
}

// bit u of the result: position i0 + u (< m) of the sorted column kc starts a run of equal keys (u < 4: a thread's share of a chunk)
US_HD int us_run_starts(const uint64_t *kc, int64_t m, int64_t i0) {
    int flags = 0;
    uint64_t prev = i0 > 0 && i0 < m ? kc[i0 - 1] : 0;
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u;
        if (i < m) {
            const uint64_t k = kc[i];
            if (i == 0 || k != prev) flags |= 1 << u;
            prev = k;
        }
    }
    return flags;
}

// number of entries of the sorted u[0 .. n) that are <= v  (at most 64 halvings: n < 2^63)
US_HD int64_t us_count_le(const int64_t *u, int64_t n, int64_t v) {
    int64_t lo = 0, hi = n;
    for (int it = 0; it < 64 && lo < hi; ++it) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (u[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// code of v among the sorted distinct u[0 .. n); *unseen is set when v is not one of them
//   clamp == 0: the index of v, or -1           clamp != 0: the index of the largest entry <= v, 0 below the smallest and for n == 0
US_HD int64_t us_lookup(const int64_t *u, int64_t n, int64_t v, int clamp, bool *unseen) {
    const int64_t cnt = us_count_le(u, n, v);
    const bool hit = cnt > 0 && u[cnt - 1] == v;
    *unseen = !hit;
    if (clamp) return cnt > 0 ? cnt - 1 : 0;
    return hit ? cnt - 1 : -1;
}

}  // namespace gsn
