// Device pieces shared by the BatchNorm kernels that take their row count from device memory (bn_bounded.hip, the bounded instantiations of
// backward.hip) and by the kernels they must agree with bit for bit (bn_finalize_kernel in encode.hip):
//   * the row bound of a padded batch, whose real rows are a prefix of the capacity,
//   * one column of the train-mode BatchNorm1d bookkeeping from its two fp64 sums.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gsn {

// (n_valid, row_ptr, n_slots): v = row_ptr ? row_ptr[clamp(*n_valid, 0, n_slots)] : *n_valid, clamped to [0, m_rows].  row_ptr has n_slots + 1
// entries; no device value, however wrong, indexes outside it.
struct RowBound {
    const int64_t *n_valid;
    const int64_t *row_ptr;
    int64_t n_slots;
};
__device__ __forceinline__ int64_t bound_rows(const RowBound &b, int64_t m_rows) {
    int64_t v = *b.n_valid;
    if (b.row_ptr) {
        v = v < 0 ? 0 : (v > b.n_slots ? b.n_slots : v);
        v = b.row_ptr[v];
    }
    return v < 0 ? 0 : (v > m_rows ? m_rows : v);
}

// Column c of nn.BatchNorm1d's train-mode bookkeeping from s1 = sum of the column and s2 = sum of its squares over m_rows rows: batch mean,
// biased variance, invstd, scale = gamma * invstd, shift = beta, running statistics with the unbiased variance.
__device__ __forceinline__ void bn_finalize_column(int c, double s1, double s2, double m_rows, double eps, double momentum, const float *gamma,
                                                   const float *beta, float *running_mean, float *running_var, float *mean, float *invstd,
                                                   float *scale, float *shift) {
    const double mu = s1 / m_rows;
    double var = s2 / m_rows - mu * mu;
    var = var > 0.0 ? var : 0.0;
    const float is = (float)(1.0 / sqrt(var + eps));
    mean[c] = (float)mu;
    invstd[c] = is;
    scale[c] = gamma ? is * gamma[c] : is;
    shift[c] = beta ? beta[c] : 0.f;
    if (running_mean) {
        const double unbiased = var * (m_rows / (m_rows > 1.0 ? m_rows - 1.0 : 1.0));
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * (double)(float)mu);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (double)(float)unbiased);
    }
}

}  // namespace gsn
