// Adam update of all parameters of all parameter groups in one launch (gsn_amd/optim.py; the reference's torch.optim.Adam,
// train_test_funcs.py:22, :106).  Multi-tensor layout as in fingerprint.hip -- a device table of base pointers and sizes -- plus a chunk
// table that maps a workgroup to (tensor, first element): a 180 000-element weight and a 0-d parameter share the launch, and no workgroup
// is idle.  Learning rate and the other hyper-parameters are read from a float64 device record per group and the step counters from a
// device array, so a replayed HIP graph follows what the host writes there between replays.
//
// Step counters without a second launch: every workgroup reads its tensor's counter BEFORE its element loop and adds 1 to the `done` word
// (agent scope, acquire-release) AFTER it.  The workgroup that draws n_chunks - 1 knows that every other workgroup has read its counter:
// it advances the counters of the tensors that had a gradient and puts the word back to 0.  Nobody waits for anybody.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsn_internal.h"

namespace gsn {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = GSN_ADAM_CHUNK_ELEMS;
constexpr int ADAM_VEC_ITERS = ADAM_CHUNK / (4 * ADAM_THREADS);      // 16-byte groups per thread
static_assert(ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a chunk is a whole number of 16-byte groups per thread");

// per chunk, from the group's float64 record (what torch's non-capturable path computes on the host per step)
struct AdamCoef {
    float b1, omb1, b2, omb2;
    float step_size;      // lr / bc1
    float bc2_sqrt;       // sqrt(bc2)
    float eps;
    float wd;             // L2 form: g' = g + wd p    (0 when decoupled)
    float decay;          // decoupled form: p <- p (1 - lr wd)    (1 otherwise)
};

__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const AdamCoef &c) {
    p *= c.decay;
    g = fmaf(c.wd, p, g);
    m = fmaf(c.b1, m, c.omb1 * g);
    v = fmaf(c.b2, v, (c.omb2 * g) * g);
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = fmaf(-c.step_size, m / denom, p);
}

__device__ __forceinline__ float4 ld4(const float *q, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4 *>(q);
    return make_float4(q[0], q[1], q[2], q[3]);
}

__device__ __forceinline__ void st4(float *q, bool aligned, const float4 &x) {
    if (aligned) {
        *reinterpret_cast<float4 *>(q) = x;
    } else {
        q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = x.w;
    }
}

__device__ __forceinline__ bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(int n_tensors, const int64_t *__restrict__ tensors, int n_chunks,
                                                                 const int32_t *__restrict__ chunks, const double *__restrict__ groups,
                                                                 float *exp_avg, float *exp_avg_sq, float *steps, unsigned *done) {
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int t = chunks[2 * blockIdx.x];
    const int64_t first = chunks[2 * blockIdx.x + 1];
    const int64_t *rec = tensors + (int64_t)t * GSN_ADAM_TENSOR_WORDS;
    const float *g = reinterpret_cast<const float *>(rec[1]);
    if (g) {      // (uniform over the workgroup)
        const float step_old = steps[t];      // read before this workgroup's `done` increment: see the head of the file
        const double *hp = groups + rec[5] * GSN_ADAM_GROUP_DOUBLES;
        const double lr = hp[0], beta1 = hp[1], beta2 = hp[2], wd = hp[4];
        const bool decoupled = hp[5] != 0.0;
        const double tt = (double)step_old + 1.0;
        const double bc1 = 1.0 - pow(beta1, tt), bc2 = 1.0 - pow(beta2, tt);
        AdamCoef c;
        c.b1 = (float)beta1; c.omb1 = (float)(1.0 - beta1);
        c.b2 = (float)beta2; c.omb2 = (float)(1.0 - beta2);
        c.step_size = (float)(lr / bc1);
        c.bc2_sqrt = (float)sqrt(bc2);
        c.eps = (float)hp[3];
        c.wd = decoupled ? 0.0f : (float)wd;
        c.decay = decoupled ? (float)(1.0 - lr * wd) : 1.0f;

        const int64_t left = rec[4] - first;
        const int len = left < ADAM_CHUNK ? (int)left : ADAM_CHUNK;      // elements of this chunk: [0, len) behind the four bases below
        float *p = reinterpret_cast<float *>(rec[0]) + first;
        g += first;
        float *m = exp_avg + rec[2] + first, *v = exp_avg_sq + rec[3] + first;
        // scalar head up to the parameter's first 16-byte boundary, 16-byte groups behind it, scalar tail.  A stream whose pointer is
        // not 16-byte aligned at the first group (a gradient or a state slot that is misaligned differently) moves its groups as four words.
        int head = (int)((0u - (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2)) & 3u);
        head = head < len ? head : len;
        const int nvec = (len - head) >> 2;
        const int tail0 = head + 4 * nvec;
        const bool ag = aligned16(g + head), am = aligned16(m + head), av = aligned16(v + head);

        float4 P[ADAM_VEC_ITERS], G[ADAM_VEC_ITERS], M[ADAM_VEC_ITERS], V[ADAM_VEC_ITERS];
#pragma unroll
        for (int k = 0; k < ADAM_VEC_ITERS; ++k) {
            const int i = tid + k * ADAM_THREADS;
            if (i < nvec) {      // elements head + 4 i .. head + 4 i + 3 < tail0 <= len
                const int e = head + 4 * i;
                P[k] = ld4(p + e, true); G[k] = ld4(g + e, ag); M[k] = ld4(m + e, am); V[k] = ld4(v + e, av);
            }
        }
#pragma unroll
        for (int k = 0; k < ADAM_VEC_ITERS; ++k) {
            const int i = tid + k * ADAM_THREADS;
            if (i < nvec) {
                const int e = head + 4 * i;
                adam_elem(P[k].x, G[k].x, M[k].x, V[k].x, c);
                adam_elem(P[k].y, G[k].y, M[k].y, V[k].y, c);
                adam_elem(P[k].z, G[k].z, M[k].z, V[k].z, c);
                adam_elem(P[k].w, G[k].w, M[k].w, V[k].w, c);
                st4(p + e, true, P[k]); st4(m + e, am, M[k]); st4(v + e, av, V[k]);
            }
        }
        // head: elements [0, head) on lanes 0 .. 2 of wave 0; tail: elements [tail0, len) on lanes 0 .. 2 of wave 1
        int e = -1;
        if (tid < head) e = tid;
        else if (tid >= 64 && tail0 + (tid - 64) < len) e = tail0 + (tid - 64);
        if (e >= 0) {
            float pe = p[e], me = m[e], ve = v[e];
            adam_elem(pe, g[e], me, ve, c);
            p[e] = pe; m[e] = me; v[e] = ve;
        }
    }
    __syncthreads();
    if (tid == 0)
        s_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(n_chunks - 1);
    __syncthreads();
    if (s_last) {      // every workgroup of the launch has read its counter and stored its elements
        for (int i = tid; i < n_tensors; i += ADAM_THREADS)
            if (tensors[(int64_t)i * GSN_ADAM_TENSOR_WORDS + 1]) steps[i] += 1.0f;
        if (tid == 0) __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace gsn

using namespace gsn;

extern "C" int gsn_adam_step_hip(int n_tensors, const int64_t *tensors, int64_t n_chunks, const int32_t *chunks, int n_groups,
                                 const double *groups, float *exp_avg, float *exp_avg_sq, float *steps, unsigned *done, int64_t max_elems,
                                 void *stream) {
    if (n_tensors < 0 || n_groups < 0 || n_chunks < 0 || max_elems < 0)
        return set_error(GSN_E_INVALID, "gsn_adam_step_hip: negative count (n_tensors %d, n_groups %d, n_chunks %lld, max_elems %lld)", n_tensors,
                         n_groups, (long long)n_chunks, (long long)max_elems);
    if (!tensors || !chunks || !groups || !exp_avg || !exp_avg_sq || !steps || !done)
        return set_error(GSN_E_INVALID, "gsn_adam_step_hip: null table or state pointer");
    if (max_elems > INT32_MAX)
        return set_error(GSN_E_UNSUPPORTED, "gsn_adam_step_hip: a tensor of %lld elements (at most 2^31 - 1 per tensor)", (long long)max_elems);
    if (n_chunks > INT32_MAX) return set_error(GSN_E_UNSUPPORTED, "gsn_adam_step_hip: %lld chunks (at most 2^31 - 1)", (long long)n_chunks);
    if (n_chunks == 0) return GSN_OK;
    if (n_tensors < 1 || n_groups < 1) return set_error(GSN_E_INVALID, "gsn_adam_step_hip: chunks without tensors or groups");
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(ADAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), n_tensors,
                       tensors, (int)n_chunks, chunks, groups, exp_avg, exp_avg_sq, steps, done);
    return launch_check("adam_step_kernel");
}
