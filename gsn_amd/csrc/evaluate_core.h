// Evaluation arithmetic shared between the HIP kernels (evaluate.hip) and a host-side logic harness used ONLY by tests
// (tests/evaluate_harness.cpp compiles this header with g++; it is not a product fallback):
//   * the per-element loss of the reference's --loss_fn kinds (utils.py:164-175) and its derivative,
//   * the map from an fp32 score and its label to a sort key,
//   * the walk over a sorted key column that turns runs of equal scores into the rank statistic U2 (ROC-AUC) and the AP sum.
//
// Formulas are evaluated in float64 from the fp32 inputs and rounded ONCE to fp32 (the per-element value that is then summed in float64):
// an element is within half an fp32 ulp of the exact value whatever the magnitudes of its parts.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define EV_HD __host__ __device__ __forceinline__
#else
#define EV_HD inline
#endif

namespace gsn {

constexpr int EV_CHUNK = 1024;                 // consecutive elements (rows for CrossEntropyLoss) of one float64 partial sum: 256 threads x 4
constexpr int64_t EV_ONE_LAUNCH_ELEMS = 65536; // up to here one workgroup takes the whole reduction (a second launch costs more than it saves)

// ---- losses (kind = GSN_LOSS_*: 0 BCEWithLogitsLoss, 1 L1Loss, 2 MSELoss; CrossEntropyLoss is row-wise, below) ----
EV_HD float ev_loss_elem(int kind, float xf, float yf) {
    const double x = xf, y = yf;
    if (kind == 0) return (float)(fmax(x, 0.0) - x * y + log1p(exp(-fabs(x))));      // stable: finite at |x| = 100 and beyond
    const double d = x - y;
    return (float)(kind == 1 ? fabs(d) : d * d);
}
// d loss_elem / d x, float64 (the caller multiplies by upstream / count and rounds once)
EV_HD double ev_dloss_elem(int kind, float xf, float yf) {
    const double x = xf, y = yf;
    if (kind == 0) {
        const double e = exp(-fabs(x));                       // sigmoid(x) without overflow on either side
        return (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - y;
    }
    const double d = x - y;
    if (kind == 1) return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);      // (a NaN difference gives 0, torch gives NaN: never reached, NaN = unlabelled)
    return 2.0 * d;
}
// the fp32 metric terms of utils.py:177-183 with reduction='sum': |x - y| (kind 1) or (x - y)^2 (kind 2), over EVERY element (no mask)
EV_HD float ev_metric_elem(int kind, float xf, float yf) {
    const double d = (double)xf - (double)yf;
    return (float)(kind == 1 ? fabs(d) : d * d);
}

// One row of CrossEntropyLoss: log-sum-exp with the row maximum subtracted.  *row_max / *sum_exp for the derivative, *arg_max = the FIRST
// index of the maximum (torch.max / argmax on ties).  A target outside [0, C) gives NaN (and the caller a zero gradient row): no fault.
EV_HD float ev_ce_row(const float *x, int64_t n_classes, int64_t target, double *row_max, double *sum_exp, int64_t *arg_max) {
    double m = x[0];
    int64_t am = 0;
    for (int64_t j = 1; j < n_classes; ++j)
        if ((double)x[j] > m) { m = x[j]; am = j; }
    double s = 0.0;
    for (int64_t j = 0; j < n_classes; ++j) s += exp((double)x[j] - m);
    *row_max = m; *sum_exp = s; *arg_max = am;
    if (target < 0 || target >= n_classes) return NAN;
    return (float)(log(s) + m - (double)x[target]);
}
// d loss_row / d x[j]
EV_HD double ev_ce_drow(float xj, double row_max, double sum_exp, bool is_target) { return exp((double)xj - row_max) / sum_exp - (is_target ? 1.0 : 0.0); }

// ---- score -> key -------------------------------------------------------------------------------------------------------------------
// Monotone image of an fp32 score: a < b  <=>  image(a) < image(b), and -0.0 == +0.0 have ONE image (they are tied for `==` and for sklearn).
EV_HD uint32_t ev_score_image(float s) {
    uint32_t b;
    memcpy(&b, &s, 4);
    if ((b << 1) == 0) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
constexpr uint64_t EV_KEY_UNLABELLED = ~0ull;          // NaN label: sorts last, counted out
constexpr uint64_t EV_KEY_BAD_LABEL = ~0ull - 1;       // a label other than 0, 1, NaN
constexpr uint64_t EV_KEY_NONFINITE = ~0ull - 2;       // a NaN / infinite prediction in a labelled row
constexpr uint64_t EV_KEY_VALID_END = 1ull << 33;      // every valid key is below
EV_HD uint64_t ev_key(float score, float label) {
    if (label != label) return EV_KEY_UNLABELLED;
    if (label != 0.0f && label != 1.0f) return EV_KEY_BAD_LABEL;
    if (!(fabsf(score) <= 3.402823466e+38f)) return EV_KEY_NONFINITE;
    return ((uint64_t)ev_score_image(score) << 1) | (label == 1.0f ? 1u : 0u);
}

// ---- the walk over a sorted column --------------------------------------------------------------------------------------------------
// The n valid keys kc[0 .. n) ascending; a run = the keys of one score (key >> 1), negatives before positives.  Logical position j is
// kc[j], or kc[n - 1 - j] when `mirror` (the column from the highest score down; positives then come first in a run).  A thread owns the
// four positions j0 .. j0 + 3 of a 1 024-position chunk, and three steps with two scans between them give, at every run END,
//   pos_r, neg_r: the run's positives / negatives      start: the run's first position      pos_before: positives before the run
// from which    ascending:  U2 += pos_r (2 neg_below + neg_r)                  neg_below = start - pos_before
//               descending: AP += (pos_r / n_pos) (tp / (tp + fp))             tp = positives so far, tp + fp = j + 1
struct EvQuad {
    uint64_t k[4];
    uint64_t prev, next;      // keys at j0 - 1 and j0 + cnt (valid with has_prev / has_next)
    int cnt;                  // positions of the quad below n
    bool has_prev, has_next;
};
EV_HD uint64_t ev_key_at(const uint64_t *kc, int64_t n, int mirror, int64_t j) { return kc[mirror ? n - 1 - j : j]; }
EV_HD void ev_quad_load(const uint64_t *kc, int64_t n, int mirror, int64_t j0, EvQuad &q) {
    q.cnt = 0; q.prev = q.next = 0;
    for (int u = 0; u < 4; ++u) {
        q.k[u] = 0;
        if (j0 + u < n) { q.k[u] = ev_key_at(kc, n, mirror, j0 + u); q.cnt = u + 1; }
    }
    q.has_prev = q.cnt > 0 && j0 > 0;
    q.has_next = q.cnt > 0 && j0 + q.cnt < n;
    if (q.has_prev) q.prev = ev_key_at(kc, n, mirror, j0 - 1);
    if (q.has_next) q.next = ev_key_at(kc, n, mirror, j0 + q.cnt);
}
// step 1: the quad's positives (summed over the threads before it: pos_before of step 2 and 3)
EV_HD int ev_quad_pos(const EvQuad &q) {
    int p = 0;
    for (int u = 0; u < q.cnt; ++u) p += (int)(q.k[u] & 1);
    return p;
}
// a run start as one word: (position + 1) << 32 | positives before it.  Both grow along the column, so the latest start is the MAXIMUM.
EV_HD uint64_t ev_start_pack(int64_t j, int64_t pos_before) { return ((uint64_t)(j + 1) << 32) | (uint64_t)pos_before; }
// step 2: the latest run start inside the quad (0: none), given the positives before position j0
EV_HD uint64_t ev_quad_start(const EvQuad &q, int64_t j0, int64_t pos_before) {
    uint64_t pack = 0, prev = q.prev;
    for (int u = 0; u < q.cnt; ++u) {
        if ((u == 0 && !q.has_prev) || (q.k[u] >> 1) != (prev >> 1)) pack = ev_start_pack(j0 + u, pos_before);
        prev = q.k[u];
        pos_before += (int64_t)(q.k[u] & 1);
    }
    return pack;
}
// step 3: the run ends inside the quad.  start_in: the latest run start before position j0 (maximum over the earlier quads and chunks).
EV_HD void ev_quad_emit(const EvQuad &q, int64_t j0, int64_t pos_before, uint64_t start_in, int mirror, int64_t n_pos, int64_t *u2, double *ap) {
    uint64_t start = start_in, prev = q.prev;
    for (int u = 0; u < q.cnt; ++u) {
        const int64_t j = j0 + u;
        if ((u == 0 && !q.has_prev) || (q.k[u] >> 1) != (prev >> 1)) start = ev_start_pack(j, pos_before);
        prev = q.k[u];
        pos_before += (int64_t)(q.k[u] & 1);      // now: positives up to and including j
        const bool end = u + 1 < q.cnt ? (q.k[u + 1] >> 1) != (q.k[u] >> 1) : (!q.has_next || (q.next >> 1) != (q.k[u] >> 1));
        if (end) {
            const int64_t j_start = (int64_t)(start >> 32) - 1, pos_start = (int64_t)(start & 0xffffffffu);
            const int64_t pos_r = pos_before - pos_start, neg_r = (j + 1 - j_start) - pos_r;
            if (!mirror) *u2 += pos_r * (2 * (j_start - pos_start) + neg_r);
            else if (pos_r > 0) *ap += ((double)pos_r / (double)n_pos) * ((double)pos_before / (double)(j + 1));
        }
    }
}

}  // namespace gsn
