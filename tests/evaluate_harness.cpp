// Test-only host harness of gsn_amd/csrc/evaluate_core.h: the loss formulas and derivatives, the score -> key map and the walk over a
// sorted key column, executed on the CPU the way evaluate.hip runs them (chunks of 1 024 positions, 256 quads per chunk, a sum scan and a
// maximum scan between the three steps, carries from chunk to chunk).  Not a product path.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../gsn_amd/csrc/evaluate_core.h"

using namespace gsn;

extern "C" void harness_loss(int kind, int64_t n, const float *x, const float *y, float *loss, double *dloss) {
    for (int64_t i = 0; i < n; ++i) {
        loss[i] = ev_loss_elem(kind, x[i], y[i]);
        dloss[i] = ev_dloss_elem(kind, x[i], y[i]);
    }
}

extern "C" void harness_metric(int kind, int64_t n, const float *x, const float *y, float *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = ev_metric_elem(kind, x[i], y[i]);
}

extern "C" void harness_ce(int64_t rows, int64_t n_classes, const float *x, const int64_t *target, float *loss, double *drow, int64_t *arg_max) {
    for (int64_t r = 0; r < rows; ++r) {
        double m, s;
        loss[r] = ev_ce_row(x + r * n_classes, n_classes, target[r], &m, &s, arg_max + r);
        for (int64_t j = 0; j < n_classes; ++j) drow[r * n_classes + j] = ev_ce_drow(x[r * n_classes + j], m, s, j == target[r]);
    }
}

extern "C" void harness_keys(int64_t n, const float *score, const float *label, uint64_t *keys) {
    for (int64_t i = 0; i < n; ++i) keys[i] = ev_key(score[i], label[i]);
}

// one column: scores and labels -> out_i = {n_labelled, n_pos, U2, refused rows}, out_d = {ap}
extern "C" void harness_rank(int64_t m, const float *score, const float *label, int64_t *out_i, double *out_d) {
    std::vector<uint64_t> k(m);
    for (int64_t i = 0; i < m; ++i) k[i] = ev_key(score[i], label[i]);
    std::sort(k.begin(), k.end());
    int64_t n = 0, n_pos = 0, refused = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (k[i] < EV_KEY_VALID_END) { ++n; n_pos += (int64_t)(k[i] & 1); }
        refused += k[i] == EV_KEY_BAD_LABEL || k[i] == EV_KEY_NONFINITE;
    }
    const int64_t n_chunks = (n + EV_CHUNK - 1) / EV_CHUNK;
    int64_t u2_total = 0;
    double ap_total = 0.0;
    for (int mirror = 0; mirror < 2; ++mirror) {
        int64_t pos_carry = 0;
        uint64_t start_carry = 0;
        for (int64_t ch = 0; ch < n_chunks; ++ch) {
            EvQuad q[256];
            int64_t pos_before[256];
            uint64_t start_in[256];
            int64_t run = pos_carry;
            for (int t = 0; t < 256; ++t) {      // step 1 and the sum scan
                ev_quad_load(k.data(), n, mirror, ch * EV_CHUNK + 4 * t, q[t]);
                pos_before[t] = run;
                run += ev_quad_pos(q[t]);
            }
            uint64_t best = start_carry;
            for (int t = 0; t < 256; ++t) {      // step 2 and the maximum scan
                start_in[t] = best;
                best = std::max(best, ev_quad_start(q[t], ch * EV_CHUNK + 4 * t, pos_before[t]));
            }
            double ap_chunk = 0.0;
            for (int t = 0; t < 256; ++t) {      // step 3
                int64_t u2 = 0;
                double ap = 0.0;
                ev_quad_emit(q[t], ch * EV_CHUNK + 4 * t, pos_before[t], start_in[t], mirror, n_pos, &u2, &ap);
                u2_total += u2;
                ap_chunk += ap;
            }
            ap_total += ap_chunk;
            pos_carry = run;
            start_carry = best;
        }
    }
    out_i[0] = n; out_i[1] = n_pos; out_i[2] = u2_total; out_i[3] = refused;
    out_d[0] = ap_total;
}
