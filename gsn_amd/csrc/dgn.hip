// Directional GSN aggregation (directional_gsn/nets/dgn_layer.py:30-56, nets/aggregators.py, nets/scalers.py): every
// aggregator of a DGNLayerSimple over the in-edges of each node, forward and backward, in one kernel family.
//
// Layout.  The edges come as the target-sorted CSR of edge_index[1] (seg_ptr, perm = edge ids stable by target, src = sources in
// that order); a node's mailbox is its CSR segment, i.e. its in-edges in edge-id order -- the order DGL's degree buckets put them in.
// The vector field of an edge e = (u -> v) is cat(F_node[u] - F_node[v], F_edge[e]) (dgn_layer.py:30-36); a column of it is read
// where it lies (the node difference is formed on the fly, the [E, C] concatenation never exists).
//
// Schedule (forward).  L lanes own one node (L = the power of two >= d / VEC, at most 64; VEC = 4, 2 or 1 floats per lane by the
// row's alignment); a lane owns VEC consecutive features, and more than 64 * VEC features are walked in chunks.  Per node:
//   1. a scalar pass over its few in-edges forms the per-aggregator normalisers of the directional kinds (sum |w|, sum relu(+-w),
//      the online softmax max / denominator);
//   2. one streaming pass over the h[src] rows accumulates, in registers, sum, sum of squares, max, min and one weighted sum per
//      directional aggregator;
//   3. the epilogue applies the aggregator formulas and the scalers and writes the node's whole output row [S][A][d].
// Nodes without an in-edge get a zero row (DGL zero-fills nodes that receive no message).
//
// Backward.  Pass 1 (target side) recomputes the node's statistics and writes, per in-edge, the gradient of its message h[src] at
// the edge id (grad_msg [E, d]), and the node's own term (the h_in of the dx kinds) into grad_h.  Pass 2 (source side, the CSR of
// edge_index[0]) adds each node's out-edge message gradients onto grad_h.  Every element has one writer and a fixed summation order:
// no atomics, bit-identical run to run.  max / min send the gradient to the first CSR position holding the extremum (lowest edge id).
//
// More than DGN_MAXA aggregators are handled as several launches over slices of the descriptor list (each writes its own output
// columns; the backward's later slices add onto the first's results in stream order).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "gsn_internal.h"

// No fused multiply-add contraction in this file: mean(h^2) - mean(h)^2 must be the difference of two ROUNDED values, as in PyTorch,
// for D = 1 and tied neighbourhoods to give a variance of exactly 0 (a contracted fma(-m1, m1, m2) leaves the rounding error of m1^2).
#pragma clang fp contract(off)

namespace gsn {
namespace {

constexpr int DGN_MAXA = 8;       // aggregators per launch
constexpr int DGN_MAXS = 4;       // scalers
constexpr int DGN_BLOCK = 256;
constexpr float DGN_EPS = 1e-8f;  // aggregators.py:5

struct DgnArgs {
    int64_t n_nodes;
    int d;
    int lanes;                     // lanes per node (power of two)
    const int32_t *seg_ptr, *perm, *src;
    const float *h;
    const float *nf;               // node field [N, nf_width] (row stride nf_stride), or null
    int64_t nf_stride;
    int nf_width;
    const float *ef;               // edge field [E, *] by edge id (row stride ef_stride), or null
    int64_t ef_stride;
    int n_agg;
    int kind[DGN_MAXA];
    int col[DGN_MAXA];
    float alpha[DGN_MAXA];
    int slot[DGN_MAXA];
    int n_scal;
    int scal[DGN_MAXS];
    float avg_log;
    int n_out_agg;                 // A: aggregators of the whole layer (output row = n_scal * A * d)
    float *out;                    // forward: [N, n_scal * A * d]
    const float *gout;             // backward: same layout
    float *gmsg;                   // backward: [E, d] by edge id
    float *gh;                     // backward: [N, d]
    int first;                     // backward: this slice writes (1) or adds onto (0) grad_msg / grad_h
    const int32_t *seg_src, *perm_src;
};

__device__ __forceinline__ bool is_dir(int k) { return k >= GSN_DGN_DIR_AV; }

// column c of the vector field of the edge at CSR position (u -> v, edge id e)
__device__ __forceinline__ float field_w(const DgnArgs &a, int c, int64_t u, int64_t v, int64_t e) {
    if (c < a.nf_width) return a.nf[u * a.nf_stride + c] - a.nf[v * a.nf_stride + c];
    return a.ef[e * a.ef_stride + (c - a.nf_width)];
}

// per directional aggregator: n1 / n2 after pass 1, then (at the end of node_norms) the factors the weight formula uses
//   av:       n1 = sum|w|                         -> wt = |w| * n1'             n1' = 1 / (sum|w| + EPS)
//   softmax:  n1 = max a|w|, n2 = sum exp(a|w|-m) -> wt = exp(a|w| - n1) * n2'  n2' = 1 / n2
//   dx(-no-abs): n1 = sum|w|, n2 = sum w          -> wt = w * n1'               n2' = sum w' = n2 * n1'
//   balanced: n1 = sum relu(w), n2 = sum relu(-w) -> wt = (relu(w) n1' + relu(-w) n2') / 2, sum wt = (n1 n1' + n2 n2') / 2 (in sw)
__device__ __forceinline__ void node_norms(const DgnArgs &a, int64_t v, int beg, int end, float (&n1)[DGN_MAXA], float (&n2)[DGN_MAXA],
                                           float (&sw)[DGN_MAXA]) {
#pragma unroll
    for (int j = 0; j < DGN_MAXA; ++j) {
        n1[j] = a.kind[j] == GSN_DGN_DIR_SOFTMAX ? -INFINITY : 0.f;
        n2[j] = 0.f;
        sw[j] = 0.f;
    }
    for (int k = beg; k < end; ++k) {
        const int64_t u = a.src[k], e = a.perm[k];
#pragma unroll
        for (int j = 0; j < DGN_MAXA; ++j) {
            if (j >= a.n_agg || !is_dir(a.kind[j])) continue;
            const float w = field_w(a, a.col[j], u, v, e);
            switch (a.kind[j]) {
            case GSN_DGN_DIR_SOFTMAX: {
                const float x = a.alpha[j] * fabsf(w);
                if (x > n1[j]) {
                    n2[j] = n2[j] * expf(n1[j] - x) + 1.f;
                    n1[j] = x;
                } else {
                    n2[j] += expf(x - n1[j]);
                }
                break;
            }
            case GSN_DGN_DIR_DX_BALANCED:
                n1[j] += fmaxf(w, 0.f);
                n2[j] += fmaxf(-w, 0.f);
                break;
            default:
                n1[j] += fabsf(w);
                n2[j] += w;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < DGN_MAXA; ++j) {
        if (j >= a.n_agg || !is_dir(a.kind[j])) continue;
        switch (a.kind[j]) {
        case GSN_DGN_DIR_AV: n1[j] = 1.f / (n1[j] + DGN_EPS); break;
        case GSN_DGN_DIR_SOFTMAX: n2[j] = 1.f / n2[j]; break;
        case GSN_DGN_DIR_DX_BALANCED: {
            const float ip = 1.f / (n1[j] + DGN_EPS), in = 1.f / (n2[j] + DGN_EPS);
            sw[j] = (n1[j] * ip + n2[j] * in) * 0.5f;
            n1[j] = ip;
            n2[j] = in;
            break;
        }
        default: {  // dx, dx-no-abs
            const float inv = 1.f / (n1[j] + DGN_EPS);
            sw[j] = n2[j] * inv;
            n1[j] = inv;
        }
        }
    }
}

// weight of the edge in directional aggregator j (after node_norms)
__device__ __forceinline__ float edge_wt(const DgnArgs &a, int j, float w, const float (&n1)[DGN_MAXA], const float (&n2)[DGN_MAXA]) {
    switch (a.kind[j]) {
    case GSN_DGN_DIR_AV: return fabsf(w) * n1[j];
    case GSN_DGN_DIR_SOFTMAX: return expf(a.alpha[j] * fabsf(w) - n1[j]) * n2[j];
    case GSN_DGN_DIR_DX_BALANCED: return (fmaxf(w, 0.f) * n1[j] + fmaxf(-w, 0.f) * n2[j]) * 0.5f;
    default: return w * n1[j];
    }
}

template <int VEC>
struct Vec {
    float x[VEC];
};

template <int VEC>
__device__ __forceinline__ Vec<VEC> load_vec(const float *p) {
    Vec<VEC> r;
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r.x[0] = t.x; r.x[1] = t.y; r.x[2] = t.z; r.x[3] = t.w;
    } else if constexpr (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        r.x[0] = t.x; r.x[1] = t.y;
    } else {
        r.x[0] = *p;
    }
    return r;
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *p, const Vec<VEC> &r) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(r.x[0], r.x[1], r.x[2], r.x[3]);
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(r.x[0], r.x[1]);
    } else {
        *p = r.x[0];
    }
}

// fp32 log(D + 1) / avg, avg / log(D + 1): scalers.py:10-18 (the factor is a float32 tensor there: avg_d['log'] is one)
__device__ __forceinline__ float scaler_factor(int code, int D, float avg) {
    const float l = (float)log((double)D + 1.0);
    return code == GSN_DGN_AMPLIFICATION ? l / avg : (code == GSN_DGN_ATTENUATION ? avg / l : 1.f);
}

// The streaming statistics of one node over one feature chunk: sum, sum of squares (products rounded before the sum, as
// torch.mean(h * h) does: no fused multiply-add, so D = 1 and tied rows give mean(h^2) - mean(h)^2 == 0 exactly), max, min, and the
// weighted sums of the directional aggregators.  The mean, var and std epilogues use correctly rounded division and square root
// (__fdiv_rn / __fsqrt_rn), so that those rows come out exactly as PyTorch's: std of a zero variance is sqrtf(EPS) to the bit.
template <int VEC>
struct Stats {
    float s1[VEC], s2[VEC], mx[VEC], mn[VEC], acc[DGN_MAXA][VEC];
};

template <int VEC>
__device__ __forceinline__ void node_stats(const DgnArgs &a, int64_t v, int beg, int end, int f, const float (&n1)[DGN_MAXA],
                                           const float (&n2)[DGN_MAXA], Stats<VEC> &st) {
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        st.s1[q] = 0.f; st.s2[q] = 0.f; st.mx[q] = -INFINITY; st.mn[q] = INFINITY;
#pragma unroll
        for (int j = 0; j < DGN_MAXA; ++j) st.acc[j][q] = 0.f;
    }
#pragma unroll 2
    for (int k = beg; k < end; ++k) {
        const int64_t u = a.src[k], e = a.perm[k];
        const Vec<VEC> x = load_vec<VEC>(a.h + u * a.d + f);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            st.s1[q] += x.x[q];
            st.s2[q] += __fmul_rn(x.x[q], x.x[q]);
            st.mx[q] = fmaxf(st.mx[q], x.x[q]);
            st.mn[q] = fminf(st.mn[q], x.x[q]);
        }
#pragma unroll
        for (int j = 0; j < DGN_MAXA; ++j) {
            if (j >= a.n_agg || !is_dir(a.kind[j])) continue;
            const float wt = edge_wt(a, j, field_w(a, a.col[j], u, v, e), n1, n2);
#pragma unroll
            for (int q = 0; q < VEC; ++q) st.acc[j][q] += __fmul_rn(wt, x.x[q]);
        }
    }
}

template <int VEC>
__global__ void __launch_bounds__(DGN_BLOCK) dgn_aggregate_fwd_kernel(DgnArgs a) {
    const int lane = threadIdx.x & (a.lanes - 1);
    const int64_t v = (int64_t)blockIdx.x * (DGN_BLOCK / a.lanes) + threadIdx.x / a.lanes;
    if (v >= a.n_nodes) return;
    const int beg = a.seg_ptr[v], end = a.seg_ptr[v + 1], D = end - beg;
    const int64_t row = (int64_t)a.n_scal * a.n_out_agg * a.d;
    float *out = a.out + v * row;
    float n1[DGN_MAXA], n2[DGN_MAXA], sw[DGN_MAXA];
    if (D > 0) node_norms(a, v, beg, end, n1, n2, sw);
    float sc[DGN_MAXS];
#pragma unroll
    for (int s = 0; s < DGN_MAXS; ++s) sc[s] = (s < a.n_scal && D > 0) ? scaler_factor(a.scal[s], D, a.avg_log) : 0.f;  // (D = 0: a zero row, not 0 * inf)
    for (int f = lane * VEC; f < a.d; f += a.lanes * VEC) {
        Stats<VEC> st;
        Vec<VEC> hin;
        if (D > 0) {
            node_stats<VEC>(a, v, beg, end, f, n1, n2, st);
            hin = load_vec<VEC>(a.h + v * a.d + f);
        }
#pragma unroll
        for (int j = 0; j < DGN_MAXA; ++j) {
            if (j >= a.n_agg) continue;
            Vec<VEC> y;
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                float r = 0.f;
                if (D > 0) {
                    const float m1 = __fdiv_rn(st.s1[q], (float)D);
                    switch (a.kind[j]) {
                    case GSN_DGN_MEAN: r = m1; break;
                    case GSN_DGN_SUM: r = st.s1[q]; break;
                    case GSN_DGN_MAX: r = st.mx[q]; break;
                    case GSN_DGN_MIN: r = st.mn[q]; break;
                    case GSN_DGN_VAR:
                    case GSN_DGN_STD: {
                        const float var = fmaxf(__fdiv_rn(st.s2[q], (float)D) - __fmul_rn(m1, m1), 0.f);
                        r = a.kind[j] == GSN_DGN_VAR ? var : __fsqrt_rn(var + DGN_EPS);
                        break;
                    }
                    case GSN_DGN_DIR_AV:
                    case GSN_DGN_DIR_SOFTMAX: r = st.acc[j][q]; break;
                    case GSN_DGN_DIR_DX_NOABS: r = st.acc[j][q] - __fmul_rn(sw[j], hin.x[q]); break;
                    default: r = fabsf(st.acc[j][q] - __fmul_rn(sw[j], hin.x[q]));  // dx, dx-balanced
                    }
                }
                y.x[q] = r;
            }
            for (int s = 0; s < a.n_scal; ++s) {
                Vec<VEC> ys;
#pragma unroll
                for (int q = 0; q < VEC; ++q) ys.x[q] = y.x[q] * sc[s];
                store_vec<VEC>(out + ((int64_t)s * a.n_out_agg + a.slot[j]) * a.d + f, ys);
            }
        }
    }
}

// Pass 1 of the backward: per target node, the message gradients of its in-edges (at their edge ids) and its own h_in term.
template <int VEC>
__global__ void __launch_bounds__(DGN_BLOCK) dgn_aggregate_bwd_target_kernel(DgnArgs a) {
    const int lane = threadIdx.x & (a.lanes - 1);
    const int64_t v = (int64_t)blockIdx.x * (DGN_BLOCK / a.lanes) + threadIdx.x / a.lanes;
    if (v >= a.n_nodes) return;
    const int beg = a.seg_ptr[v], end = a.seg_ptr[v + 1], D = end - beg;
    const int64_t row = (int64_t)a.n_scal * a.n_out_agg * a.d;
    float n1[DGN_MAXA], n2[DGN_MAXA], sw[DGN_MAXA];
    if (D > 0) node_norms(a, v, beg, end, n1, n2, sw);
    float sc[DGN_MAXS];
#pragma unroll
    for (int s = 0; s < DGN_MAXS; ++s) sc[s] = (s < a.n_scal && D > 0) ? scaler_factor(a.scal[s], D, a.avg_log) : 0.f;  // (D = 0: a zero row, not 0 * inf)
    for (int f = lane * VEC; f < a.d; f += a.lanes * VEC) {
        Vec<VEC> self;
#pragma unroll
        for (int q = 0; q < VEC; ++q) self.x[q] = 0.f;
        if (D > 0) {
            Stats<VEC> st;
            node_stats<VEC>(a, v, beg, end, f, n1, n2, st);
            const Vec<VEC> hin = load_vec<VEC>(a.h + v * a.d + f);
            // per-feature coefficients: every edge gets U + V (h_k - m1) + sum_j G_j wt_j(k), the first max / min position gMX / gMN
            float U[VEC], V[VEC], m1[VEC], gMX[VEC], gMN[VEC], G[DGN_MAXA][VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                U[q] = 0.f; V[q] = 0.f; gMX[q] = 0.f; gMN[q] = 0.f;
                m1[q] = __fdiv_rn(st.s1[q], (float)D);
            }
#pragma unroll
            for (int j = 0; j < DGN_MAXA; ++j) {
                if (j >= a.n_agg) continue;
                Vec<VEC> g;
#pragma unroll
                for (int q = 0; q < VEC; ++q) g.x[q] = 0.f;
                for (int s = 0; s < a.n_scal; ++s) {
                    const Vec<VEC> t = load_vec<VEC>(a.gout + v * row + ((int64_t)s * a.n_out_agg + a.slot[j]) * a.d + f);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) g.x[q] += t.x[q] * sc[s];
                }
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    G[j][q] = 0.f;
                    switch (a.kind[j]) {
                    case GSN_DGN_MEAN: U[q] += g.x[q] / (float)D; break;
                    case GSN_DGN_SUM: U[q] += g.x[q]; break;
                    case GSN_DGN_MAX: gMX[q] += g.x[q]; break;
                    case GSN_DGN_MIN: gMN[q] += g.x[q]; break;
                    case GSN_DGN_VAR:
                    case GSN_DGN_STD: {
                        // var = relu(mean(h^2) - mean(h)^2): d var / d h_k = 2 (h_k - m1) / D where the relu passes (relu'(0) = 0);
                        // std = sqrt(var + EPS): d std / d var = 1 / (2 std)
                        const float raw = __fdiv_rn(st.s2[q], (float)D) - __fmul_rn(m1[q], m1[q]);
                        if (raw > 0.f) {
                            const float gv = a.kind[j] == GSN_DGN_VAR ? g.x[q] : g.x[q] * 0.5f / __fsqrt_rn(raw + DGN_EPS);
                            V[q] += gv * 2.f / (float)D;
                        }
                        break;
                    }
                    case GSN_DGN_DIR_AV:
                    case GSN_DGN_DIR_SOFTMAX:
                    case GSN_DGN_DIR_DX_NOABS: G[j][q] = g.x[q]; break;
                    default: {  // |T|: abs'(0) = 0
                        const float T = st.acc[j][q] - __fmul_rn(sw[j], hin.x[q]);
                        G[j][q] = T > 0.f ? g.x[q] : (T < 0.f ? -g.x[q] : 0.f);
                    }
                    }
                    if (a.kind[j] == GSN_DGN_DIR_DX || a.kind[j] == GSN_DGN_DIR_DX_NOABS || a.kind[j] == GSN_DGN_DIR_DX_BALANCED)
                        self.x[q] -= G[j][q] * sw[j];
                }
            }
            bool mx_done[VEC], mn_done[VEC];
#pragma unroll
            for (int q = 0; q < VEC; ++q) { mx_done[q] = false; mn_done[q] = false; }
            for (int k = beg; k < end; ++k) {
                const int64_t u = a.src[k], e = a.perm[k];
                const Vec<VEC> x = load_vec<VEC>(a.h + u * a.d + f);
                Vec<VEC> gm;
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    float r = U[q] + V[q] * (x.x[q] - m1[q]);
                    if (!mx_done[q] && x.x[q] == st.mx[q]) { r += gMX[q]; mx_done[q] = true; }
                    if (!mn_done[q] && x.x[q] == st.mn[q]) { r += gMN[q]; mn_done[q] = true; }
                    gm.x[q] = r;
                }
#pragma unroll
                for (int j = 0; j < DGN_MAXA; ++j) {
                    if (j >= a.n_agg || !is_dir(a.kind[j])) continue;
                    const float wt = edge_wt(a, j, field_w(a, a.col[j], u, v, e), n1, n2);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) gm.x[q] += G[j][q] * wt;
                }
                float *dst = a.gmsg + e * a.d + f;
                if (!a.first) {
                    const Vec<VEC> old = load_vec<VEC>(dst);
#pragma unroll
                    for (int q = 0; q < VEC; ++q) gm.x[q] += old.x[q];
                }
                store_vec<VEC>(dst, gm);
            }
        }
        float *dst = a.gh + v * a.d + f;
        if (!a.first) {
            const Vec<VEC> old = load_vec<VEC>(dst);
#pragma unroll
            for (int q = 0; q < VEC; ++q) self.x[q] += old.x[q];
        }
        store_vec<VEC>(dst, self);
    }
}

// Pass 2 of the backward: grad_h[u] += the message gradients of u's out-edges, in the source CSR's (edge-id) order.
template <int VEC>
__global__ void __launch_bounds__(DGN_BLOCK) dgn_aggregate_bwd_source_kernel(DgnArgs a) {
    const int lane = threadIdx.x & (a.lanes - 1);
    const int64_t u = (int64_t)blockIdx.x * (DGN_BLOCK / a.lanes) + threadIdx.x / a.lanes;
    if (u >= a.n_nodes) return;
    const int beg = a.seg_src[u], end = a.seg_src[u + 1];
    for (int f = lane * VEC; f < a.d; f += a.lanes * VEC) {
        float *dst = a.gh + u * a.d + f;
        Vec<VEC> r = load_vec<VEC>(dst);
        for (int k = beg; k < end; ++k) {
            const Vec<VEC> t = load_vec<VEC>(a.gmsg + (int64_t)a.perm_src[k] * a.d + f);
#pragma unroll
            for (int q = 0; q < VEC; ++q) r.x[q] += t.x[q];
        }
        store_vec<VEC>(dst, r);
    }
}

int dgn_vec(int64_t d, std::initializer_list<const void *> ptrs) {
    uintptr_t m = 0;
    for (const void *p : ptrs) m |= (uintptr_t)p;
    if (d % 4 == 0 && m % 16 == 0) return 4;
    if (d % 2 == 0 && m % 8 == 0) return 2;
    return 1;
}

int dgn_lanes(int64_t d, int vec) {
    int l = 1;
    while (l < 64 && (int64_t)l * vec < d) l *= 2;
    return l;
}

// argument checks shared by both directions; fills everything of `a` but the descriptor slice
int dgn_setup(const char *who, DgnArgs &a, int64_t n_nodes, int64_t n_edges, int64_t d, const int32_t *seg_ptr, const int32_t *perm,
              const int32_t *src, const float *h, const float *node_field, int64_t node_stride, int64_t node_width, const float *edge_field,
              int64_t edge_stride, int64_t edge_width, const gsn_dgn_agg *aggs, int n_aggs, const int32_t *scalers, int n_scalers,
              double avg_d_log) {
    if (n_nodes < 0 || n_edges < 0 || d < 1 || d > (1 << 24) || n_aggs < 1 || !aggs || n_scalers < 1 || !scalers)
        return set_error(GSN_E_INVALID, "%s: bad sizes", who);
    if (n_scalers > DGN_MAXS) return set_error(GSN_E_UNSUPPORTED, "%s: %d scalers (at most %d)", who, n_scalers, DGN_MAXS);
    if (n_nodes > INT32_MAX || n_edges > INT32_MAX) return set_error(GSN_E_UNSUPPORTED, "%s: more than 2^31 nodes or edges", who);
    if (node_width < 0 || edge_width < 0 || (node_width > 0 && ((n_nodes > 0 && !node_field) || node_stride < node_width)) ||
        (edge_width > 0 && ((n_edges > 0 && !edge_field) || edge_stride < edge_width)))
        return set_error(GSN_E_INVALID, "%s: bad field", who);
    const int64_t width = node_width + edge_width;
    for (int j = 0; j < n_aggs; ++j) {
        const gsn_dgn_agg &g = aggs[j];
        if (g.kind < GSN_DGN_MEAN || g.kind > GSN_DGN_DIR_DX_BALANCED || g.slot < 0 || g.slot >= n_aggs)
            return set_error(GSN_E_INVALID, "%s: bad aggregator descriptor %d", who, j);
        // the reference indexes vector_field[:, :, eig_idx] and raises IndexError (aggregators.py:38-70)
        if (g.kind >= GSN_DGN_DIR_AV && (g.col < 0 || g.col >= width))
            return set_error(GSN_E_INVALID, "%s: aggregator %d reads field column %d of a %lld-column field", who, j, g.col, (long long)width);
    }
    for (int s = 0; s < n_scalers; ++s)
        if (scalers[s] < GSN_DGN_IDENTITY || scalers[s] > GSN_DGN_ATTENUATION) return set_error(GSN_E_INVALID, "%s: bad scaler %d", who, s);
    if (n_nodes > 0 && (!seg_ptr || !h)) return set_error(GSN_E_INVALID, "%s: null node pointers", who);
    if (n_edges > 0 && (!perm || !src)) return set_error(GSN_E_INVALID, "%s: null CSR pointers", who);
    a = DgnArgs{};
    a.n_nodes = n_nodes; a.d = (int)d;
    a.seg_ptr = seg_ptr; a.perm = perm; a.src = src; a.h = h;
    a.nf = node_width > 0 ? node_field : nullptr; a.nf_stride = node_stride; a.nf_width = (int)node_width;
    a.ef = edge_width > 0 ? edge_field : nullptr; a.ef_stride = edge_stride;
    a.n_scal = n_scalers;
    for (int s = 0; s < n_scalers; ++s) a.scal[s] = scalers[s];
    a.avg_log = (float)avg_d_log;
    a.n_out_agg = n_aggs;
    return GSN_OK;
}

void dgn_slice(DgnArgs &a, const gsn_dgn_agg *aggs, int j0, int n) {
    a.n_agg = n;
    for (int j = 0; j < DGN_MAXA; ++j) {
        const bool on = j < n;
        a.kind[j] = on ? aggs[j0 + j].kind : GSN_DGN_MEAN;
        a.col[j] = on ? aggs[j0 + j].col : 0;
        a.alpha[j] = on ? aggs[j0 + j].alpha : 0.f;
        a.slot[j] = on ? aggs[j0 + j].slot : 0;
    }
}

template <template <int> class K>
void dgn_launch(const DgnArgs &a, int vec, hipStream_t s) {
    const unsigned grid = (unsigned)((a.n_nodes + DGN_BLOCK / a.lanes - 1) / (DGN_BLOCK / a.lanes));
    if (vec == 4) hipLaunchKernelGGL(K<4>::fn, dim3(grid), dim3(DGN_BLOCK), 0, s, a);
    else if (vec == 2) hipLaunchKernelGGL(K<2>::fn, dim3(grid), dim3(DGN_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(K<1>::fn, dim3(grid), dim3(DGN_BLOCK), 0, s, a);
}

template <int V> struct FwdK { static constexpr auto fn = dgn_aggregate_fwd_kernel<V>; };
template <int V> struct BwdTK { static constexpr auto fn = dgn_aggregate_bwd_target_kernel<V>; };
template <int V> struct BwdSK { static constexpr auto fn = dgn_aggregate_bwd_source_kernel<V>; };

}  // namespace
}  // namespace gsn

using namespace gsn;

extern "C" int gsn_dgn_aggregate_fwd_hip(int64_t n_nodes, int64_t n_edges, int64_t d, const int32_t *seg_ptr, const int32_t *perm,
                                         const int32_t *src, const float *h, const float *node_field, int64_t node_stride,
                                         int64_t node_width, const float *edge_field, int64_t edge_stride, int64_t edge_width,
                                         const gsn_dgn_agg *aggs, int n_aggs, const int32_t *scalers, int n_scalers, double avg_d_log,
                                         float *out, void *stream) {
    DgnArgs a;
    int rc = dgn_setup("gsn_dgn_aggregate_fwd_hip", a, n_nodes, n_edges, d, seg_ptr, perm, src, h, node_field, node_stride, node_width,
                       edge_field, edge_stride, edge_width, aggs, n_aggs, scalers, n_scalers, avg_d_log);
    if (rc != GSN_OK) return rc;
    if (n_nodes == 0) return GSN_OK;
    if (!out) return set_error(GSN_E_INVALID, "gsn_dgn_aggregate_fwd_hip: null output");
    a.out = out;
    const int vec = dgn_vec(d, {h, out});
    a.lanes = dgn_lanes(d, vec);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (int j0 = 0; j0 < n_aggs; j0 += DGN_MAXA) {
        dgn_slice(a, aggs, j0, n_aggs - j0 < DGN_MAXA ? n_aggs - j0 : DGN_MAXA);
        dgn_launch<FwdK>(a, vec, s);
        if (int rc = launch_check("dgn_aggregate_fwd_kernel")) return rc;
    }
    return GSN_OK;
}

extern "C" int gsn_dgn_aggregate_bwd_hip(int64_t n_nodes, int64_t n_edges, int64_t d, const int32_t *seg_ptr, const int32_t *perm,
                                         const int32_t *src, const int32_t *src_seg_ptr, const int32_t *src_perm, const float *h,
                                         const float *node_field, int64_t node_stride, int64_t node_width, const float *edge_field,
                                         int64_t edge_stride, int64_t edge_width, const gsn_dgn_agg *aggs, int n_aggs,
                                         const int32_t *scalers, int n_scalers, double avg_d_log, const float *grad_out, float *grad_msg,
                                         float *grad_h, void *stream) {
    DgnArgs a;
    int rc = dgn_setup("gsn_dgn_aggregate_bwd_hip", a, n_nodes, n_edges, d, seg_ptr, perm, src, h, node_field, node_stride, node_width,
                       edge_field, edge_stride, edge_width, aggs, n_aggs, scalers, n_scalers, avg_d_log);
    if (rc != GSN_OK) return rc;
    if (n_nodes == 0) return GSN_OK;
    if (!grad_out || !grad_h || !src_seg_ptr || (n_edges > 0 && (!grad_msg || !src_perm)))
        return set_error(GSN_E_INVALID, "gsn_dgn_aggregate_bwd_hip: null gradient / source CSR pointers");
    a.gout = grad_out; a.gmsg = grad_msg; a.gh = grad_h;
    a.seg_src = src_seg_ptr; a.perm_src = src_perm;
    const int vec = dgn_vec(d, {h, grad_out, grad_msg, grad_h});
    a.lanes = dgn_lanes(d, vec);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (int j0 = 0; j0 < n_aggs; j0 += DGN_MAXA) {
        dgn_slice(a, aggs, j0, n_aggs - j0 < DGN_MAXA ? n_aggs - j0 : DGN_MAXA);
        a.first = j0 == 0;
        dgn_launch<BwdTK>(a, vec, s);
        if (int rc = launch_check("dgn_aggregate_bwd_target_kernel")) return rc;
    }
    dgn_launch<BwdSK>(a, vec, s);
    return launch_check("dgn_aggregate_bwd_source_kernel");
}
