// Laplacian eigenvector fields of the directional GSN (directional_gsn/data/HIV.py:21-51, positional_encoding): the k eigenpairs of
// smallest eigenvalue of every graph's Laplacian, many graphs per launch, one workgroup per graph.
//
// What is solved.  A[u, v] = number of arcs u -> v (duplicates add, self loops count), d = max(in-degree, 1), and
//   none: L = diag(d) - A        sym: L = I - D^-1/2 A D^-1/2        walk: L = I - D^-1 A.
// Only symmetric arc sets are in scope (A != A^T -> GSN_ST_ASYMMETRIC).  L_walk = D^-1/2 L_sym D^1/2, so 'walk' solves L_sym and
// returns D^-1/2 u, renormalised: one symmetric solver serves the three norms.
//
// Solver.  Parallel two-sided cyclic Jacobi in fp32 on A := L, V := I.  The n vertices (padded to an even m) meet in a round-robin
// tournament: a sweep is m - 1 steps of m / 2 disjoint pairs (p, q), and every pair of a step is rotated at once:
//   1. one thread per pair reads a_pp, a_qq, a_pq and leaves (c, s), the pair and the two new diagonal entries in LDS     | barrier
//   2. the column pairs of A and of V are rotated: one work item per (pair, row), consecutive lanes on consecutive rows    | barrier
//   3. the row pairs of A are rotated: one work item per (pair, column), consecutive lanes on consecutive columns; the items at
//      the pair's own columns write the exact values instead (a_pq = a_qp = 0, a_pp - t a_pq, a_qq + t a_pq)                | barrier
// A pair with |a_pq| <= 2^-24 |L|_F / n is left alone (rotating rounding noise never settles).  A graph has converged when
// off(A) <= 2^-24 |L|_F or a whole sweep rotated nothing.  Every loop is bounded: sweeps by the argument max_sweeps, steps and items by
// the graph's size, which is bounded by the class.  A graph that has not converged at max_sweeps gets GSN_ST_NO_CONVERGENCE, its rows
// are written all the same, and the workgroup ends.
//
// Layout.  A and V are [n][PITCH] floats with PITCH = NMAX + 1: odd, so the column pass (lane stride PITCH) and the row pass (lane
// stride 1) both touch 32 distinct banks per half wave.  Classes NMAX = 32, 64, 128 keep both matrices in LDS (8.3, 32.5, 129 KiB);
// NMAX = 256 does the same rotations on 2 * 256 * 257 floats of caller scratch per graph (0.5 MiB: it stays in L2), with the loads of
// eight work items in flight per thread and the column pass laid along rows (see the passes).
//
// Determinism.  The only floating-point atomics are the +1.0f per arc that build A (integer-valued sums, exact in any order).  Norms
// are reduced by a fixed butterfly and a fixed order over the waves; rotation counts are integers.  Two runs are bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "gsn_internal.h"

namespace gsn {
namespace {

constexpr float EIG_EPS = 5.9604644775390625e-08f;   // 2^-24
constexpr int EIG_MAX_SWEEPS = 64;

struct EigArgs {
    int64_t n_graphs_total;
    const int64_t *node_ptr, *edge_ptr, *edge_index;
    int64_t n_edges;
    const int32_t *graph_ids;
    int64_t n_ids;
    int norm, k, max_sweeps;
    float *vec, *val;
    int32_t *status, *sweeps_used;
    float *scratch;
};

template <int NMAX>
struct EigShared {
    float c[NMAX / 2], s[NMAX / 2], app[NMAX / 2], aqq[NMAX / 2];
    int pq[NMAX / 2];          // p | q << 16, or -1: the pair is left alone in this step
    float deg[NMAX];           // d = max(in-degree, 1), later d^-1/2 ('walk')
    float diag[NMAX];
    float red[16];
    int sel[GSN_EIG_KMAX];
    int flags;                 // bit 0: a vertex id outside the graph, bit 1: A != A^T
    int rotations;
};

// idx / n for 0 <= idx < 2^16, 1 <= n <= 256, inv_n = 1.0f / n: (idx + 0.5) / n lies at least 1 / 512 from an integer, the fp32 error of the
// product stays below 1e-4
__device__ __forceinline__ int div_n(int idx, float inv_n) { return (int)(((float)idx + 0.5f) * inv_n); }

// the sum of x over the workgroup, the same bits in every thread: butterfly inside the wave, then the waves in order
template <int THREADS>
__device__ __forceinline__ float block_sum(float x, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if constexpr (THREADS == 64) return x;
    __syncthreads();                       // (red may still be read from the previous reduction)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) r += red[w];
    return r;
}

template <int NMAX, int THREADS>
__device__ __forceinline__ float off_norm2(const float *A, int n, float inv_n, float *red) {
    constexpr int PITCH = NMAX + 1;
    float x = 0.f;
    for (int idx = threadIdx.x; idx < n * n; idx += THREADS) {
        const int i = div_n(idx, inv_n), j = idx - i * n;
        const float a = A[i * PITCH + j];
        if (i != j) x += a * a;
    }
    return block_sum<THREADS>(x, red);
}

// zero rows and NaN values for a graph that is not solved (its rows lie inside the output: the caller checked)
template <int THREADS>
__device__ __forceinline__ void write_refused(const EigArgs &a, int64_t g, int64_t node0, int64_t n, int st) {
    for (int64_t idx = threadIdx.x; idx < n * a.k; idx += THREADS) a.vec[node0 * a.k + idx] = 0.f;
    if ((int)threadIdx.x < a.k) a.val[g * a.k + threadIdx.x] = nanf("");
    if (threadIdx.x == 0) {
        a.status[g] = st;
        if (a.sweeps_used) a.sweeps_used[g] = 0;
    }
}

template <int NMAX, int THREADS, bool IN_LDS>
__global__ void __launch_bounds__(THREADS) laplacian_eig_kernel(EigArgs a) {
    constexpr int PITCH = NMAX + 1;
    extern __shared__ float eig_lds[];
    __shared__ EigShared<NMAX> sh;
    const int tid = threadIdx.x;
    const int64_t g = a.graph_ids ? (int64_t)a.graph_ids[blockIdx.x] : (int64_t)blockIdx.x;
    if (g < 0 || g >= a.n_graphs_total) return;      // a graph id outside the batch owns no output
    const int64_t n_total = a.node_ptr[a.n_graphs_total];
    const int64_t node0 = a.node_ptr[g], n64 = a.node_ptr[g + 1] - node0;
    if (node0 < 0 || n64 < 0 || node0 + n64 > n_total) {   // rows outside the output: nothing but the status can be written
        if (tid == 0) {
            a.status[g] = GSN_ST_BAD_INDEX;
            if (a.sweeps_used) a.sweeps_used[g] = 0;
        }
        if (tid < a.k) a.val[g * a.k + tid] = nanf("");
        return;
    }
    if (n64 > NMAX) {
        write_refused<THREADS>(a, g, node0, n64, GSN_ST_TOO_LARGE);
        return;
    }
    const int n = (int)n64, k = a.k;
    const float inv_n = 1.f / (float)(n > 0 ? n : 1);
    float *A = IN_LDS ? eig_lds : a.scratch + (int64_t)blockIdx.x * (2 * NMAX * PITCH);
    float *V = A + NMAX * PITCH;

    // ---- A := adjacency counts, V := I
    for (int idx = tid; idx < n * PITCH; idx += THREADS) {
        const int i = idx / PITCH, j = idx - i * PITCH;
        A[idx] = 0.f;
        V[idx] = i == j ? 1.f : 0.f;
    }
    if (tid == 0) {
        sh.flags = 0;
        sh.rotations = 0;
    }
    __syncthreads();
    int64_t e0 = a.edge_ptr[g], e1 = a.edge_ptr[g + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > a.n_edges) e1 = a.n_edges;
    if constexpr (IN_LDS) {
        for (int64_t e = e0 + tid; e < e1; e += THREADS) {
            const int64_t u = a.edge_index[e] - node0, v = a.edge_index[a.n_edges + e] - node0;
            if (u < 0 || u >= n || v < 0 || v >= n) atomicOr(&sh.flags, 1);
            else atomicAdd(&A[(int)u * PITCH + (int)v], 1.0f);
        }
    } else if (tid < n || tid == 0) {
        // A in global memory: no atomics -- thread u walks the graph's arcs and adds those leaving u onto its own row
        bool bad = false;
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t u = a.edge_index[e] - node0, v = a.edge_index[a.n_edges + e] - node0;
            if (u < 0 || u >= n || v < 0 || v >= n) bad = true;
            else if (u == tid) A[tid * PITCH + (int)v] += 1.0f;
        }
        if (bad) atomicOr(&sh.flags, 1);
    }
    __syncthreads();
    // ---- degrees (column sums: in-degree), symmetry
    for (int v = tid; v < n; v += THREADS) {
        float d = 0.f;
        for (int u = 0; u < n; ++u) d += A[u * PITCH + v];
        sh.deg[v] = fmaxf(d, 1.f);
    }
    {
        bool asym = false;
        for (int idx = tid; idx < n * n; idx += THREADS) {
            const int i = div_n(idx, inv_n), j = idx - i * n;
            asym |= A[i * PITCH + j] != A[j * PITCH + i];
        }
        if (asym) atomicOr(&sh.flags, 2);
    }
    __syncthreads();
    const int flags = sh.flags;
    if (flags) {
        write_refused<THREADS>(a, g, node0, n, (flags & 1) ? GSN_ST_BAD_INDEX : GSN_ST_ASYMMETRIC);
        return;
    }
    // ---- A := L, |L|_F
    float f2 = 0.f;
    for (int idx = tid; idx < n * n; idx += THREADS) {
        const int i = div_n(idx, inv_n), j = idx - i * n;
        const float x = A[i * PITCH + j];
        float l;
        if (a.norm == GSN_EIG_NORM_NONE) l = (i == j ? sh.deg[i] : 0.f) - x;
        else l = (i == j ? 1.f : 0.f) - __fdiv_rn(x, __fsqrt_rn(sh.deg[i] * sh.deg[j]));   // (d_i d_j: an exact integer, the same for (j, i))
        A[i * PITCH + j] = l;
        f2 += l * l;
    }
    f2 = block_sum<THREADS>(f2, sh.red);     // (its barriers also publish L)
    if constexpr (THREADS == 64) __syncthreads();
    const float fro = __fsqrt_rn(f2);
    const float skip = EIG_EPS * fro * inv_n;
    const float done2 = (EIG_EPS * fro) * (EIG_EPS * fro);

    // ---- the sweeps
    const int m = n + (n & 1), half = m >> 1, ring = m - 1;
    constexpr int U = 8;                   // work items a thread of the scratch class has in flight
    const float inv_half = 1.f / (float)(half > 0 ? half : 1);
    bool converged = false;
    int used = 0;
    for (int sw = 0;; ++sw) {
        const float off2 = off_norm2<NMAX, THREADS>(A, n, inv_n, sh.red);
        if (off2 <= done2) {
            converged = true;
            break;
        }
        if (sw >= a.max_sweeps) break;
        int my_rot = 0;
        for (int step = 0; step < ring; ++step) {
            for (int pr = tid; pr < half; pr += THREADS) {
                int x = pr == 0 ? ring : (step + pr) % ring, y = pr == 0 ? step : (step - pr + ring) % ring;
                const int p = x < y ? x : y, q = x < y ? y : x;
                int code = -1;
                if (q < n) {
                    const float apq = A[p * PITCH + q];
                    if (fabsf(apq) > skip) {
                        const float app = A[p * PITCH + p], aqq = A[q * PITCH + q];
                        const float theta = __fdiv_rn(aqq - app, 2.f * apq);
                        const float t = __fdiv_rn(copysignf(1.f, theta), fabsf(theta) + __fsqrt_rn(theta * theta + 1.f));   // (theta^2 = inf: t = 0)
                        const float c = __fdiv_rn(1.f, __fsqrt_rn(t * t + 1.f));
                        sh.c[pr] = c;
                        sh.s[pr] = t * c;
                        sh.app[pr] = app - t * apq;
                        sh.aqq[pr] = aqq + t * apq;
                        code = p | (q << 16);
                        ++my_rot;
                    }
                }
                sh.pq[pr] = code;
            }
            __syncthreads();
            // columns p, q of A and V:  [x_p, x_q] := [c x_p - s x_q, s x_p + c x_q], then (after a barrier) rows p, q of A
            if constexpr (IN_LDS) {
                // consecutive lanes take consecutive rows of one pair (lane stride PITCH: conflict-free), then consecutive columns
                for (int idx = tid; idx < half * n; idx += THREADS) {
                    const int pr = div_n(idx, inv_n), i = idx - pr * n;
                    const int code = sh.pq[pr];
                    if (code < 0) continue;
                    const int p = code & 0xffff, q = code >> 16;
                    const float c = sh.c[pr], s = sh.s[pr];
                    float *ra = A + i * PITCH, *rv = V + i * PITCH;
                    const float ap = ra[p], aq = ra[q], vp = rv[p], vq = rv[q];
                    ra[p] = c * ap - s * aq;
                    ra[q] = s * ap + c * aq;
                    rv[p] = c * vp - s * vq;
                    rv[q] = s * vp + c * vq;
                }
                __syncthreads();
                for (int idx = tid; idx < half * n; idx += THREADS) {
                    const int pr = div_n(idx, inv_n), j = idx - pr * n;
                    const int code = sh.pq[pr];
                    if (code < 0) continue;
                    const int p = code & 0xffff, q = code >> 16;
                    const float c = sh.c[pr], s = sh.s[pr];
                    const float ap = A[p * PITCH + j], aq = A[q * PITCH + j];
                    float np_ = c * ap - s * aq, nq_ = s * ap + c * aq;
                    if (j == p) {
                        np_ = sh.app[pr];
                        nq_ = 0.f;
                    } else if (j == q) {
                        np_ = 0.f;
                        nq_ = sh.aqq[pr];
                    }
                    A[p * PITCH + j] = np_;
                    A[q * PITCH + j] = nq_;
                }
            } else {
                // the same two passes on global memory: U items per thread at a time, all loads before the first store (the round trips
                // overlap), and in the column pass consecutive lanes take consecutive pairs of one row (a wave then stays inside that
                // row's few cache lines).  Measured on one MI355X against this form for every class: 64 graphs of 160 .. 256 vertices
                // 225 -> 50 ms, but the LDS classes 6 - 15 % slower, hence the two forms.
                for (int base = tid; base < half * n; base += THREADS * U) {
                    float ap[U], aq[U], vp[U], vq[U], c[U], s[U];
                    int op[U], oq[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int idx = base + u * THREADS;
                        op[u] = -1;
                        if (idx >= half * n) continue;
                        const int i = div_n(idx, inv_half), pr = idx - i * half;
                        const int code = sh.pq[pr];
                        if (code < 0) continue;
                        op[u] = i * PITCH + (code & 0xffff);
                        oq[u] = i * PITCH + (code >> 16);
                        c[u] = sh.c[pr];
                        s[u] = sh.s[pr];
                        ap[u] = A[op[u]];
                        aq[u] = A[oq[u]];
                        vp[u] = V[op[u]];
                        vq[u] = V[oq[u]];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (op[u] < 0) continue;
                        A[op[u]] = c[u] * ap[u] - s[u] * aq[u];
                        A[oq[u]] = s[u] * ap[u] + c[u] * aq[u];
                        V[op[u]] = c[u] * vp[u] - s[u] * vq[u];
                        V[oq[u]] = s[u] * vp[u] + c[u] * vq[u];
                    }
                }
                __syncthreads();
                // rows p, q of A
                for (int base = tid; base < half * n; base += THREADS * U) {
                    float np_[U], nq_[U];
                    int op[U], oq[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int idx = base + u * THREADS;
                        op[u] = -1;
                        if (idx >= half * n) continue;
                        const int pr = div_n(idx, inv_n), j = idx - pr * n;
                        const int code = sh.pq[pr];
                        if (code < 0) continue;
                        const int p = code & 0xffff, q = code >> 16;
                        const float c = sh.c[pr], s = sh.s[pr];
                        op[u] = p * PITCH + j;
                        oq[u] = q * PITCH + j;
                        const float ap = A[op[u]], aq = A[oq[u]];
                        np_[u] = c * ap - s * aq;
                        nq_[u] = s * ap + c * aq;
                        if (j == p) {
                            np_[u] = sh.app[pr];
                            nq_[u] = 0.f;
                        } else if (j == q) {
                            np_[u] = 0.f;
                            nq_[u] = sh.aqq[pr];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (op[u] < 0) continue;
                        A[op[u]] = np_[u];
                        A[oq[u]] = nq_[u];
                    }
                }
            }
            __syncthreads();
        }
        ++used;
        if (my_rot) atomicAdd(&sh.rotations, my_rot);     // (an integer count)
        __syncthreads();
        const int rot = sh.rotations;
        __syncthreads();
        if (tid == 0) sh.rotations = 0;
        if (rot == 0) {
            converged = true;
            break;
        }
    }

    // ---- the k smallest diagonal entries, ties by position
    for (int i = tid; i < n; i += THREADS) {
        sh.diag[i] = A[i * PITCH + i];
        if (a.norm == GSN_EIG_NORM_WALK) sh.deg[i] = __fdiv_rn(1.f, __fsqrt_rn(sh.deg[i]));
    }
    if (tid < GSN_EIG_KMAX) sh.sel[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += THREADS) {
        const float di = sh.diag[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float dj = sh.diag[j];
            rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        if (rank < k) sh.sel[rank] = i;
    }
    __syncthreads();
    // ---- one wave per output column: scale ('walk'), normalise, fix the sign, write
    const int lane = tid & 63;
    for (int j = tid >> 6; j < k; j += THREADS / 64) {
        if (j >= n) {       // fewer vertices than columns: a zero vector and no eigenvalue
            for (int i = lane; i < n; i += 64) a.vec[(node0 + i) * k + j] = 0.f;
            if (lane == 0) a.val[g * k + j] = nanf("");
            continue;
        }
        const int col = sh.sel[j];
        float x[NMAX / 64 > 0 ? NMAX / 64 : 1];
        float s2 = 0.f;
#pragma unroll
        for (int r = 0; r < (NMAX + 63) / 64; ++r) {
            const int i = lane + 64 * r;
            float v = 0.f;
            if (i < n) {
                v = V[i * PITCH + col];
                if (a.norm == GSN_EIG_NORM_WALK) v *= sh.deg[i];
            }
            x[r] = v;
            s2 += v * v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
        const float inv = __fdiv_rn(1.f, __fsqrt_rn(s2));
        // the component of largest magnitude (lowest index on ties) becomes positive
        float best = -1.f;
        int best_i = 0x7fffffff;
        float best_v = 0.f;
#pragma unroll
        for (int r = 0; r < (NMAX + 63) / 64; ++r) {
            const int i = lane + 64 * r;
            x[r] *= inv;
            if (i < n && fabsf(x[r]) > best) {      // (ascending i: the first of equal magnitudes stays)
                best = fabsf(x[r]);
                best_i = i;
                best_v = x[r];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o), ov = __shfl_xor(best_v, o);
            const int oi = __shfl_xor(best_i, o);
            if (ob > best || (ob == best && oi < best_i)) {
                best = ob;
                best_i = oi;
                best_v = ov;
            }
        }
        const float sgn = best_v < 0.f ? -1.f : 1.f;
#pragma unroll
        for (int r = 0; r < (NMAX + 63) / 64; ++r) {
            const int i = lane + 64 * r;
            if (i < n) a.vec[(node0 + i) * k + j] = sgn * x[r];
        }
        if (lane == 0) a.val[g * k + j] = sh.diag[col];
    }
    if (tid == 0) {
        a.status[g] = converged ? GSN_ST_OK : GSN_ST_NO_CONVERGENCE;
        if (a.sweeps_used) a.sweeps_used[g] = used;
    }
}

template <int NMAX, int THREADS, bool IN_LDS>
int eig_launch(const EigArgs &a, hipStream_t stream) {
    const size_t lds = IN_LDS ? sizeof(float) * 2 * NMAX * (NMAX + 1) : 0;
    if (lds > 48 * 1024) {      // (a constant of the instantiation: once per device)
        static DeviceOnce once;
        if (int rc = lds_limit(&once, {kernel_ptr(&laplacian_eig_kernel<NMAX, THREADS, IN_LDS>)}, nullptr, (int)lds)) return rc;
    }
    hipLaunchKernelGGL((laplacian_eig_kernel<NMAX, THREADS, IN_LDS>), dim3((unsigned)a.n_ids), dim3(THREADS), lds, stream, a);
    return launch_check("laplacian_eig_kernel<%d> launch", NMAX);
}

}  // namespace
}  // namespace gsn

using namespace gsn;

extern "C" int64_t gsn_laplacian_eig_scratch_floats(int n_class, int64_t n_ids) {
    if (n_class != 256 || n_ids <= 0) return 0;
    return n_ids * (int64_t)(2 * 256 * 257);
}

extern "C" int gsn_laplacian_eig_hip(int64_t n_graphs_total, const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                     int64_t n_edges, const int32_t *graph_ids, int64_t n_ids, int n_class, int norm, int k, int max_sweeps,
                                     float *vec, float *val, int32_t *status, int32_t *sweeps_used, float *scratch, int64_t scratch_floats,
                                     void *stream) {
    const char *who = "gsn_laplacian_eig_hip";
    if (n_graphs_total < 0 || n_edges < 0 || n_ids < 0) return set_error(GSN_E_INVALID, "%s: negative sizes", who);
    if (norm < GSN_EIG_NORM_NONE || norm > GSN_EIG_NORM_WALK) return set_error(GSN_E_INVALID, "%s: norm %d", who, norm);
    if (k < 1 || k > GSN_EIG_KMAX) return set_error(GSN_E_INVALID, "%s: k = %d outside 1 .. %d", who, k, GSN_EIG_KMAX);
    if (max_sweeps < 1 || max_sweeps > EIG_MAX_SWEEPS)
        return set_error(GSN_E_INVALID, "%s: max_sweeps = %d outside 1 .. %d", who, max_sweeps, EIG_MAX_SWEEPS);
    if (n_class != 32 && n_class != 64 && n_class != 128 && n_class != 256)
        return set_error(GSN_E_INVALID, "%s: n_class %d is not 32, 64, 128 or 256", who, n_class);
    if (!graph_ids) n_ids = n_graphs_total;
    if (n_ids == 0) return GSN_OK;
    if (n_ids > INT32_MAX) return set_error(GSN_E_UNSUPPORTED, "%s: more than 2^31 graphs in a launch", who);
    if (!node_ptr || !edge_ptr || (n_edges > 0 && !edge_index) || !vec || !val || !status)
        return set_error(GSN_E_INVALID, "%s: null pointers", who);
    if (n_class == 256 && (!scratch || scratch_floats < gsn_laplacian_eig_scratch_floats(256, n_ids)))
        return set_error(GSN_E_NOSPACE, "%s: class 256 needs %lld floats of scratch", who,
                         (long long)gsn_laplacian_eig_scratch_floats(256, n_ids));
    EigArgs a{n_graphs_total, node_ptr, edge_ptr, edge_index, n_edges, graph_ids, n_ids, norm, k, max_sweeps,
              vec, val, status, sweeps_used, scratch};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (n_class) {
    case 32: return eig_launch<32, 64, true>(a, s);
    case 64: return eig_launch<64, 256, true>(a, s);
    case 128: return eig_launch<128, 512, true>(a, s);
    default: return eig_launch<256, 1024, false>(a, s);
    }
}
