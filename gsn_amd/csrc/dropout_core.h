// The random stream of the native dropout, stated once: shared between the HIP kernels (dropout.hip) and a host-side harness used ONLY by
// tests (tests/dropout_harness.cpp compiles this header with g++; it is not a product fallback).
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped by the Weyl
// constants between rounds.  Known answers: counter {0,0,0,0}, key {0,0} -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; counter {243f6a88, 85a308d3,
// 13198a2e, 03707344}, key {a4093822, 299f31d0} -> d16cfe09 94fdcceb 5001e420 24126ea1.
//
// Mask of one call with state (seed, calls), both 64 bits: element e -- counted from the start of the TENSOR, never from an address --
// belongs to group q = e >> 2; the group's four words are Philox(counter = (lo32 q, hi32 q, lo32 calls, hi32 calls), key = (lo32 seed,
// hi32 seed)); element e takes word e & 3 and is KEPT iff word >= thr, thr = min(2^32 - 1, round(p 2^32)).  The mask is a function of
// (seed, calls, e, thr) alone: not of the grid, the alignment or the shape.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DR_HD __host__ __device__ __forceinline__
#else
#define DR_HD inline
#endif

namespace gsn {

constexpr uint32_t DR_PHILOX_M0 = 0xD2511F53u, DR_PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t DR_PHILOX_W0 = 0x9E3779B9u, DR_PHILOX_W1 = 0xBB67AE85u;      // Weyl constants of the key schedule

struct DrWords {
    uint32_t w[4];
};

DR_HD DrWords dr_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)DR_PHILOX_M0 * c0, p1 = (uint64_t)DR_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += DR_PHILOX_W0;      // (unsigned: wraps)
        k1 += DR_PHILOX_W1;
    }
    DrWords r;
    r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
    return r;
}

// the four words of group q of the call (seed, calls)
DR_HD DrWords dr_group_words(uint64_t seed, uint64_t calls, uint64_t q) {
    return dr_philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)calls, (uint32_t)(calls >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

DR_HD bool dr_keep_word(uint32_t word, uint32_t thr) { return word >= thr; }

// the keep decision of element e (what the kernels compute a group at a time)
DR_HD bool dr_keep(uint64_t seed, uint64_t calls, uint64_t e, uint32_t thr) {
    return dr_keep_word(dr_group_words(seed, calls, e >> 2).w[e & 3u], thr);
}

}  // namespace gsn
