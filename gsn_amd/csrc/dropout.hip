// Dropout with the residual add in one launch, and its adjoint (gsn_amd/dropout.py; the reference's F.dropout calls,
// models_graph_classification_ogb_original.py:243-259 and dgn_layer.py:81).  No mask tensor exists: the forward draws the mask from the
// stream of dropout_core.h at the call's (seed, calls) and leaves that pair in `used`; the adjoint draws the same mask from `used`.
//
// Call counter without a second launch, the scheme of optim.hip: every workgroup reads state[1] BEFORE its elements and adds 1 to the `done`
// word (agent scope) AFTER them.  The workgroup that draws grid - 1 knows that every other workgroup has read the counter: it writes
// state[1] = calls + 1 and puts the word back to 0.  Nobody waits for anybody; a grid of one workgroup runs the same code.  The add is
// relaxed here where optim.hip's is acquire-release: see the comment at the add.
//
// Values: v = keep ? x * scale : +0 is a select (a NaN or Inf in a dropped element does not propagate); with a residual out = res + v, the
// product and the sum rounded separately (__fmul_rn / __fadd_rn are never contracted): bit for bit res + mask * x * scale in fp32.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dropout_core.h"
#include "gsn_internal.h"

namespace gsn {

// 1 024 lanes on a chunk of 8 192 elements: two Philox calls per lane.  The batches of 32 graphs make calls of 10 k - 250 k elements, 2 - 31 workgroups
// on 256 CUs, and such a call lasts as long as one lane's serial work (256 lanes, eight calls per lane: 4.5 - 4.9 us per launch inside the molhiv step)
constexpr int DROPOUT_THREADS = 1024;
constexpr int DROPOUT_CHUNK = GSN_DROPOUT_CHUNK_ELEMS;
constexpr int DROPOUT_GROUPS = DROPOUT_CHUNK / 4;                          // Philox calls of a workgroup
constexpr int DROPOUT_ITERS = DROPOUT_GROUPS / DROPOUT_THREADS;            // groups per lane
static_assert(DROPOUT_CHUNK % (4 * DROPOUT_THREADS) == 0, "a chunk is a whole number of groups per lane");

static inline bool dr_aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// elements [4 q, 4 q + 4) of a tensor of n elements: a whole group as 16 bytes when `vec`, else word by word, clipped to n
__device__ __forceinline__ float4 dr_load(const float *p, int64_t q, int64_t n, bool vec) {
    const int64_t e = 4 * q;
    if (vec && e + 4 <= n) return *reinterpret_cast<const float4 *>(p + e);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < n) v.x = p[e];
    if (e + 1 < n) v.y = p[e + 1];
    if (e + 2 < n) v.z = p[e + 2];
    if (e + 3 < n) v.w = p[e + 3];
    return v;
}

__device__ __forceinline__ void dr_store(float *p, int64_t q, int64_t n, bool vec, const float4 &v) {
    const int64_t e = 4 * q;
    if (vec && e + 4 <= n) {
        *reinterpret_cast<float4 *>(p + e) = v;
        return;
    }
    if (e < n) p[e] = v.x;
    if (e + 1 < n) p[e + 1] = v.y;
    if (e + 2 < n) p[e + 2] = v.z;
    if (e + 3 < n) p[e + 3] = v.w;
}

__device__ __forceinline__ float dr_value(float x, uint32_t word, uint32_t thr, float scale) {
    return dr_keep_word(word, thr) ? __fmul_rn(x, scale) : 0.0f;
}

// the masked, scaled group q of `src` at (seed, calls)
__device__ __forceinline__ float4 dr_apply(const float4 &x, uint64_t seed, uint64_t calls, int64_t q, uint32_t thr, float scale) {
    const DrWords r = dr_group_words(seed, calls, (uint64_t)q);
    return make_float4(dr_value(x.x, r.w[0], thr, scale), dr_value(x.y, r.w[1], thr, scale), dr_value(x.z, r.w[2], thr, scale),
                       dr_value(x.w, r.w[3], thr, scale));
}

// HAS_RES: out = res + v.  Workgroup b owns groups [b * DROPOUT_GROUPS, (b + 1) * DROPOUT_GROUPS) clipped to the n_groups of the tensor.
template <bool HAS_RES>
__global__ __launch_bounds__(DROPOUT_THREADS) void dropout_fwd_kernel(int64_t n, const float *__restrict__ x, const float *__restrict__ res,
                                                                      float *__restrict__ out, uint32_t thr, float scale, int64_t *state,
                                                                      unsigned *done, int64_t *used, bool vec) {
    __shared__ int s_last;
    const int tid = threadIdx.x;
    // (agent-scope loads: the pair is written by the last workgroup of the launch in front of this one)
    const uint64_t seed = (uint64_t)__hip_atomic_load(state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t calls = (uint64_t)__hip_atomic_load(state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // before this workgroup's `done` add
    const int64_t n_groups = (n + 3) >> 2;
    const int64_t q0 = (int64_t)blockIdx.x * DROPOUT_GROUPS;

    if (vec && 4 * (q0 + DROPOUT_GROUPS) <= n) {      // (uniform) a whole chunk of 16-byte groups: no bound inside, every load in flight at once
        const float4 *x4 = reinterpret_cast<const float4 *>(x) + q0 + tid;
        const float4 *r4 = HAS_RES ? reinterpret_cast<const float4 *>(res) + q0 + tid : nullptr;
        float4 *o4 = reinterpret_cast<float4 *>(out) + q0 + tid;
        float4 X[DROPOUT_ITERS], R[DROPOUT_ITERS];
#pragma unroll
        for (int k = 0; k < DROPOUT_ITERS; ++k) {
            X[k] = x4[k * DROPOUT_THREADS];
            if (HAS_RES) R[k] = r4[k * DROPOUT_THREADS];
        }
#pragma unroll
        for (int k = 0; k < DROPOUT_ITERS; ++k) {
            float4 v = dr_apply(X[k], seed, calls, q0 + tid + k * DROPOUT_THREADS, thr, scale);
            if (HAS_RES) {
                v.x = __fadd_rn(R[k].x, v.x); v.y = __fadd_rn(R[k].y, v.y); v.z = __fadd_rn(R[k].z, v.z); v.w = __fadd_rn(R[k].w, v.w);
            }
            o4[k * DROPOUT_THREADS] = v;
        }
    } else {      // the last chunk of the tensor, or a misaligned tensor: group by group, clipped to n
#pragma unroll 1
        for (int k = 0; k < DROPOUT_ITERS; ++k) {
            const int64_t q = q0 + tid + k * DROPOUT_THREADS;
            if (q < n_groups) {
                float4 v = dr_apply(dr_load(x, q, n, vec), seed, calls, q, thr, scale);
                if (HAS_RES) {
                    const float4 r = dr_load(res, q, n, vec);
                    v.x = __fadd_rn(r.x, v.x); v.y = __fadd_rn(r.y, v.y); v.z = __fadd_rn(r.z, v.z); v.w = __fadd_rn(r.w, v.w);
                }
                dr_store(out, q, n, vec, v);
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        used[0] = (int64_t)seed;
        used[1] = (int64_t)calls;
    }
    // Every lane that has a group has USED `calls` for the values it stored above, so its load has returned when it arrives at this barrier, and
    // the add below is issued behind the barrier: a relaxed add orders everything the scheme needs (a read against the one later write of the
    // same word).  Nothing is handed from workgroup to workgroup inside the launch, so no release or acquire is paid: with acquire-release the
    // add writes the XCD's L2 back and drops the L1 once per workgroup -- 270 instead of 68 us on 105 000 x 300 with a residual.
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (s_last && tid == 0) {      // every workgroup of the launch has read the counter
        __hip_atomic_store(state + 1, (int64_t)(calls + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(DROPOUT_THREADS) void dropout_bwd_kernel(int64_t n, const float *__restrict__ grad_out, float *__restrict__ grad_x,
                                                                      uint32_t thr, float scale, const int64_t *__restrict__ used, bool vec) {
    const int tid = threadIdx.x;
    const uint64_t seed = (uint64_t)used[0], calls = (uint64_t)used[1];      // written by the forward launch, read-only here
    const int64_t n_groups = (n + 3) >> 2;
    const int64_t q0 = (int64_t)blockIdx.x * DROPOUT_GROUPS;
    if (vec && 4 * (q0 + DROPOUT_GROUPS) <= n) {      // (uniform) a whole chunk of 16-byte groups
        const float4 *g4 = reinterpret_cast<const float4 *>(grad_out) + q0 + tid;
        float4 *o4 = reinterpret_cast<float4 *>(grad_x) + q0 + tid;
        float4 G[DROPOUT_ITERS];
#pragma unroll
        for (int k = 0; k < DROPOUT_ITERS; ++k) G[k] = g4[k * DROPOUT_THREADS];
#pragma unroll
        for (int k = 0; k < DROPOUT_ITERS; ++k) o4[k * DROPOUT_THREADS] = dr_apply(G[k], seed, calls, q0 + tid + k * DROPOUT_THREADS, thr, scale);
    } else {
#pragma unroll 1
        for (int k = 0; k < DROPOUT_ITERS; ++k) {
            const int64_t q = q0 + tid + k * DROPOUT_THREADS;
            if (q < n_groups) dr_store(grad_x, q, n, vec, dr_apply(dr_load(grad_out, q, n, vec), seed, calls, q, thr, scale));
        }
    }
}

static int dropout_grid(const char *who, int64_t n, unsigned *grid) {
    const int64_t chunks = (n + DROPOUT_CHUNK - 1) / DROPOUT_CHUNK;
    if (chunks > INT32_MAX)
        return set_error(GSN_E_UNSUPPORTED, "%s: %lld elements (at most (2^31 - 1) * %d)", who, (long long)n, DROPOUT_CHUNK);
    *grid = (unsigned)chunks;
    return GSN_OK;
}

}  // namespace gsn

using namespace gsn;

extern "C" int64_t gsn_dropout_chunk_elems(void) { return DROPOUT_CHUNK; }

extern "C" int gsn_dropout_fwd_hip(int64_t n, const float *x, const float *res, float *out, uint32_t thr, float scale, int64_t *state,
                                   unsigned *done, int64_t *used, void *stream) {
    if (n < 0) return set_error(GSN_E_INVALID, "gsn_dropout_fwd_hip: negative element count %lld", (long long)n);
    if (n == 0) return GSN_OK;      // no launch: the state does not advance
    if (!x || !out || !state || !done || !used) return set_error(GSN_E_INVALID, "gsn_dropout_fwd_hip: null tensor, state or counter pointer");
    unsigned grid = 0;
    if (int rc = dropout_grid("gsn_dropout_fwd_hip", n, &grid)) return rc;
    const bool vec = dr_aligned16(x) && dr_aligned16(out) && (!res || dr_aligned16(res));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (res)
        hipLaunchKernelGGL(dropout_fwd_kernel<true>, dim3(grid), dim3(DROPOUT_THREADS), 0, s, n, x, res, out, thr, scale, state, done, used, vec);
    else
        hipLaunchKernelGGL(dropout_fwd_kernel<false>, dim3(grid), dim3(DROPOUT_THREADS), 0, s, n, x, res, out, thr, scale, state, done, used, vec);
    return launch_check("dropout_fwd_kernel");
}

extern "C" int gsn_dropout_bwd_hip(int64_t n, const float *grad_out, float *grad_x, uint32_t thr, float scale, const int64_t *used,
                                   void *stream) {
    if (n < 0) return set_error(GSN_E_INVALID, "gsn_dropout_bwd_hip: negative element count %lld", (long long)n);
    if (n == 0) return GSN_OK;
    if (!grad_out || !grad_x || !used) return set_error(GSN_E_INVALID, "gsn_dropout_bwd_hip: null gradient or state pointer");
    unsigned grid = 0;
    if (int rc = dropout_grid("gsn_dropout_bwd_hip", n, &grid)) return rc;
    const bool vec = dr_aligned16(grad_out) && dr_aligned16(grad_x);
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3(grid), dim3(DROPOUT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), n, grad_out, grad_x, thr,
                       scale, used, vec);
    return launch_check("dropout_bwd_kernel");
}
