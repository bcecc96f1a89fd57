// Evaluation on the device (gsn_amd/evaluation.py): the masked mean loss of the reference's OGB branch as one capturable node
// (train_test_funcs.py:98-101), one batch of an evaluation epoch per call (:193-202, :234-251) and ROC-AUC / average precision per column
// from exact integer rank statistics (:257-259, ogb's Evaluator through sklearn).  Formulas, key map and the run walk: evaluate_core.h.
//
//   loss          per element fp32 -> float64 sum of each chunk of EV_CHUNK consecutive elements (thread: its 4 elements in order, wave: a
//                 shuffle tree, workgroup: its 4 waves in order) -> chunk sums added in chunk order -> one division, one rounding.
//                 <= EV_ONE_LAUNCH_ELEMS elements: one workgroup walks the chunks, one launch.  Beyond: one workgroup per chunk leaves its
//                 partial, a second launch adds them in the same order.
//   accumulate    the same chunk function (the same bits), the metric term beside it, the batch's rows copied behind a device-resident cursor
//   rank metrics  keys -> the sort of unique_sort_kernels.h -> one workgroup per column: counts, then the chunks of the column in order,
//                 ascending for U2 and descending for AP, with a sum scan (positives) and a maximum scan (latest run start) per chunk
//
// No float atomics, no atomics at all; no loop waits for another workgroup; every loop is bounded by the shape.  Two runs give the same bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "evaluate_core.h"
#include "gsn_internal.h"
#include "unique_sort_kernels.h"

namespace gsn {

struct EvPart {
    double loss, metric;
    int64_t count, correct;
};
__device__ __forceinline__ void ev_add(EvPart &a, const EvPart &b) { a.loss += b.loss; a.metric += b.metric; a.count += b.count; a.correct += b.correct; }

struct EvArgs {
    int kind, metric;
    int64_t rows, cols;      // units = rows * cols elements, or rows for CE
    const float *y_hat;
    const void *y;
};
// (CE rows without a class column are refused on the host, ev_check; should one get here it has no unit, so nothing is read)
__device__ __forceinline__ int64_t ev_units(const EvArgs &a) { return a.kind == GSN_LOSS_CE ? (a.cols > 0 ? a.rows : 0) : a.rows * a.cols; }

// sum of v over the 256 threads, the same value in every thread: wave tree, then the waves in order (all threads call; `buf`: 4 entries)
template <class T>
__device__ __forceinline__ T ev_block_sum(T v, T *buf) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();      // (buf may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((buf[0] + buf[1]) + buf[2]) + buf[3];
}

// the partial of chunk ch, the same in every thread
__device__ __forceinline__ EvPart ev_chunk(const EvArgs &a, int64_t ch, double *dbuf, int64_t *ibuf) {
    const int64_t n = ev_units(a), u0 = ch * EV_CHUNK + 4 * (int64_t)threadIdx.x;
    EvPart p{0.0, 0.0, 0, 0};
    for (int u = 0; u < 4; ++u) {
        const int64_t i = u0 + u;
        if (i >= n) break;
        if (a.kind == GSN_LOSS_CE) {
            const int64_t target = reinterpret_cast<const int64_t *>(a.y)[i];
            double m, s;
            int64_t am;
            p.loss += (double)ev_ce_row(a.y_hat + i * a.cols, a.cols, target, &m, &s, &am);
            p.count += 1;
            p.correct += am == target;
        } else {
            const float x = a.y_hat[i], y = reinterpret_cast<const float *>(a.y)[i];
            if (y == y) {
                p.loss += (double)ev_loss_elem(a.kind, x, y);
                p.count += 1;
            }
            if (a.metric == GSN_METRIC_L1 || a.metric == GSN_METRIC_MSE) p.metric += (double)ev_metric_elem(a.metric, x, y);
        }
    }
    EvPart r;
    r.loss = ev_block_sum(p.loss, dbuf);
    r.metric = a.metric == GSN_METRIC_NONE || a.metric == GSN_METRIC_ACCURACY ? 0.0 : ev_block_sum(p.metric, dbuf);
    r.count = ev_block_sum(p.count, ibuf);
    r.correct = a.metric == GSN_METRIC_ACCURACY ? ev_block_sum(p.correct, ibuf) : 0;
    return r;
}

struct EvAcc {
    int64_t num_graphs;
    double *f64;
    int64_t *i64;
    float *pred_buf;
    void *true_buf;
    int64_t capacity, y_words;      // y_words: 4-byte words of one row of y
    float *loss_out;
    const int64_t *n_valid;         // COUNTED kernels only: the batch's valid rows, read on the device
};

// COUNTED: the first v = clamp(*n_valid, 0, rows) rows are the batch, and its weight.  False when there is none (uniform: nothing is done).
__device__ __forceinline__ bool ev_count_rows(EvArgs &a, EvAcc &c) {
    int64_t v = *c.n_valid;
    v = v < 0 ? 0 : (v > a.rows ? a.rows : v);
    a.rows = v;
    c.num_graphs = v;
    return v > 0;
}

__device__ __forceinline__ bool ev_overflow(const EvAcc &c, int64_t rows) {
    const int64_t cur = c.i64[GSN_EVAL_CURSOR];
    return cur < 0 || cur > c.capacity - rows;
}

// the batch's rows behind the cursor, by the threads [t0, t0 + nt) of the launch
__device__ __forceinline__ void ev_append(const EvArgs &a, const EvAcc &c, int64_t t0, int64_t nt) {
    const int64_t cur = c.i64[GSN_EVAL_CURSOR];      // (cur + rows <= capacity: checked by the caller)
    if (c.pred_buf) {
        float *dst = c.pred_buf + cur * a.cols;
        for (int64_t i = t0; i < a.rows * a.cols; i += nt) dst[i] = a.y_hat[i];
    }
    if (c.true_buf) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.y);
        uint32_t *dst = reinterpret_cast<uint32_t *>(c.true_buf) + cur * c.y_words;
        for (int64_t i = t0; i < a.rows * c.y_words; i += nt) dst[i] = src[i];
    }
}

// one thread: the mean, and the accumulators of an evaluation batch
__device__ __forceinline__ void ev_finish(const EvArgs &a, const EvPart &t, float *loss, int64_t *count, const EvAcc *c) {
    const float l = (float)(t.loss / (double)t.count);      // (no labelled element: 0 / 0 = NaN, as torch's mean of nothing)
    if (loss) *loss = l;
    if (count) *count = t.count;
    if (c) {
        if (c->loss_out) *c->loss_out = l;
        c->f64[GSN_EVAL_WEIGHTED_LOSS] += (double)l * (double)c->num_graphs;
        c->f64[GSN_EVAL_BATCH_LOSS] += (double)l;
        if (a.metric == GSN_METRIC_L1 || a.metric == GSN_METRIC_MSE) c->f64[GSN_EVAL_METRIC] += (double)(float)t.metric;
        if (a.metric == GSN_METRIC_ACCURACY) c->i64[GSN_EVAL_CORRECT] += t.correct;
        c->i64[GSN_EVAL_BATCHES] += 1;
        c->i64[GSN_EVAL_CURSOR] += a.rows;
    }
}

template <bool ACC, bool COUNTED = false>
__global__ __launch_bounds__(256) void ev_small_kernel(EvArgs a, float *loss, int64_t *count, EvAcc c) {
    __shared__ double dbuf[4];
    __shared__ int64_t ibuf[4];
    if (COUNTED && !ev_count_rows(a, c) && ACC) return;      // (the plain loss of no valid row is still written: NaN, count 0)
    if (ACC) {
        if (ev_overflow(c, a.rows)) {      // (uniform: nobody has written the cursor yet)
            if (threadIdx.x == 0) c.i64[GSN_EVAL_STATUS] |= GSN_EVAL_OVERFLOW;
            return;
        }
        ev_append(a, c, threadIdx.x, 256);
    }
    const int64_t n_chunks = (ev_units(a) + EV_CHUNK - 1) / EV_CHUNK;
    EvPart t{0.0, 0.0, 0, 0};
    for (int64_t ch = 0; ch < n_chunks; ++ch) ev_add(t, ev_chunk(a, ch, dbuf, ibuf));
    __syncthreads();      // (every thread has read the cursor before thread 0 moves it)
    if (threadIdx.x == 0) ev_finish(a, t, loss, count, ACC ? &c : nullptr);
}

template <bool ACC, bool COUNTED = false>
__global__ __launch_bounds__(256) void ev_partial_kernel(EvArgs a, EvPart *parts, int64_t n_chunks, EvAcc c) {
    __shared__ double dbuf[4];
    __shared__ int64_t ibuf[4];
    if (COUNTED) {
        if (!ev_count_rows(a, c) && ACC) return;
        n_chunks = (ev_units(a) + EV_CHUNK - 1) / EV_CHUNK;      // (the chunks of the valid rows: the host sized the scratch for all rows)
    }
    if (ACC) {
        if (ev_overflow(c, a.rows)) return;      // (the combine launch sets the flag; the cursor is only written there)
        ev_append(a, c, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
    }
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const EvPart p = ev_chunk(a, ch, dbuf, ibuf);
        if (threadIdx.x == 0) parts[ch] = p;
    }
}

template <bool ACC, bool COUNTED = false>
__global__ __launch_bounds__(64) void ev_combine_kernel(EvArgs a, const EvPart *parts, int64_t n_chunks, float *loss, int64_t *count, EvAcc c) {
    if (threadIdx.x != 0) return;
    if (COUNTED) {
        if (!ev_count_rows(a, c) && ACC) return;
        n_chunks = (ev_units(a) + EV_CHUNK - 1) / EV_CHUNK;
    }
    if (ACC && ev_overflow(c, a.rows)) {
        c.i64[GSN_EVAL_STATUS] |= GSN_EVAL_OVERFLOW;
        return;
    }
    EvPart t{0.0, 0.0, 0, 0};
    for (int64_t ch = 0; ch < n_chunks; ++ch) ev_add(t, parts[ch]);      // chunk order, as ev_small_kernel
    ev_finish(a, t, loss, count, ACC ? &c : nullptr);
}

// COUNTED: the units of the first v = clamp(*n_valid, 0, rows) rows are the batch; the units behind them get +0 and neither y_hat nor y is
// read there
template <bool COUNTED = false>
__global__ __launch_bounds__(256) void ev_bwd_kernel(EvArgs a, const float *grad_loss, const int64_t *count, float *grad, const int64_t *n_valid) {
    const int64_t n = ev_units(a), cnt = *count;
    [[maybe_unused]] int64_t n_in = n;
    if constexpr (COUNTED) {
        int64_t v = *n_valid;
        v = v < 0 ? 0 : (v > a.rows ? a.rows : v);
        n_in = a.kind == GSN_LOSS_CE ? (a.cols > 0 ? v : 0) : v * a.cols;
    }
    const double scale = cnt > 0 ? (double)*grad_loss / (double)cnt : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if constexpr (COUNTED) {
            if (i >= n_in) {
                if (a.kind == GSN_LOSS_CE) {
                    for (int64_t j = 0; j < a.cols; ++j) grad[i * a.cols + j] = 0.0f;
                } else {
                    grad[i] = 0.0f;
                }
                continue;
            }
        }
        if (a.kind == GSN_LOSS_CE) {
            const int64_t target = reinterpret_cast<const int64_t *>(a.y)[i];
            const float *x = a.y_hat + i * a.cols;
            float *g = grad + i * a.cols;
            const bool ok = cnt > 0 && target >= 0 && target < a.cols;
            double m = 0.0, s = 1.0;
            int64_t am;
            if (ok) ev_ce_row(x, a.cols, target, &m, &s, &am);
            for (int64_t j = 0; j < a.cols; ++j) g[j] = ok ? (float)(scale * ev_ce_drow(x[j], m, s, j == target)) : 0.0f;
        } else {
            const float y = reinterpret_cast<const float *>(a.y)[i];
            grad[i] = (y == y && cnt > 0) ? (float)(scale * ev_dloss_elem(a.kind, a.y_hat[i], y)) : 0.0f;
        }
    }
}

// ---- rank metrics ----
struct EvKeyLoad {
    const float *pred, *label;
    __device__ __forceinline__ uint64_t operator()(int64_t row, int64_t n_cols, int64_t col) const {
        const int64_t i = row * n_cols + col;
        return ev_key(pred[i], label[i]);
    }
};

// exclusive prefix of v over the 256 threads under OP (sum or max of unsigned words), *total = the whole; all threads call
template <bool MAX>
__device__ __forceinline__ uint64_t ev_block_scan(uint64_t v, uint64_t *total, uint64_t *wbuf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x = MAX ? (x > y ? x : y) : x + y;
    }
    const uint64_t up = __shfl_up(x, 1, 64);      // inclusive value of the lane before
    __syncthreads();
    if (lane == 63) wbuf[wave] = x;
    __syncthreads();
    uint64_t off = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
        const uint64_t s = wbuf[w];
        if (w < wave) off = MAX ? (off > s ? off : s) : off + s;
        tot = MAX ? (tot > s ? tot : s) : tot + s;
    }
    *total = tot;
    const uint64_t before = lane > 0 ? up : 0;
    return MAX ? (off > before ? off : before) : off + before;
}

// one workgroup per column of sorted keys
__global__ __launch_bounds__(256) void ev_rank_kernel(int64_t m, const uint64_t *keys, int64_t *out_i, double *out_d, int32_t *status) {
    __shared__ uint64_t wbuf[4];
    __shared__ int64_t ibuf[4];
    __shared__ double dbuf[4];
    const int64_t c = blockIdx.x;
    const uint64_t *kc = keys + c * m;
    const int tid = threadIdx.x;
    // counts: valid keys (they come first), positives among them, and the two kinds of refused rows
    int64_t nv = 0, np = 0, nbad = 0, nnf = 0;
    for (int64_t i = tid; i < m; i += 256) {
        const uint64_t k = kc[i];
        if (k < EV_KEY_VALID_END) { nv += 1; np += (int64_t)(k & 1); }
        nbad += k == EV_KEY_BAD_LABEL;
        nnf += k == EV_KEY_NONFINITE;
    }
    const int64_t n = ev_block_sum(nv, ibuf), n_pos = ev_block_sum(np, ibuf);
    const int64_t n_bad = ev_block_sum(nbad, ibuf), n_nf = ev_block_sum(nnf, ibuf);
    const int64_t n_chunks = (n + EV_CHUNK - 1) / EV_CHUNK;
    int64_t u2_total = 0;
    double ap_total = 0.0;
    for (int mirror = 0; mirror < 2; ++mirror) {
        uint64_t pos_carry = 0, start_carry = 0;
        for (int64_t ch = 0; ch < n_chunks; ++ch) {
            const int64_t j0 = ch * EV_CHUNK + 4 * (int64_t)tid;
            EvQuad q;
            ev_quad_load(kc, n, mirror, j0, q);
            uint64_t pos_chunk, start_chunk;
            const int64_t pos_before = (int64_t)(pos_carry + ev_block_scan<false>((uint64_t)ev_quad_pos(q), &pos_chunk, wbuf));
            uint64_t start_in = ev_block_scan<true>(ev_quad_start(q, j0, pos_before), &start_chunk, wbuf);
            start_in = start_in > start_carry ? start_in : start_carry;
            int64_t u2 = 0;
            double ap = 0.0;
            ev_quad_emit(q, j0, pos_before, start_in, mirror, n_pos, &u2, &ap);
            if (!mirror) u2_total += ev_block_sum(u2, ibuf);
            else ap_total += ev_block_sum(ap, dbuf);      // chunks from the highest scores down, in order
            pos_carry += pos_chunk;
            start_carry = start_chunk > start_carry ? start_chunk : start_carry;
        }
    }
    if (tid == 0) {
        const int64_t n_neg = n - n_pos;
        int32_t st = 0;
        if (n_pos == 0 || n_neg == 0) st |= GSN_RANK_ONE_CLASS;
        if (n_pos == 0) st |= GSN_RANK_NO_POSITIVE;
        if (n_nf > 0) st |= GSN_RANK_NONFINITE;
        if (n_bad > 0) st |= GSN_RANK_BAD_LABEL;
        out_i[3 * c] = n; out_i[3 * c + 1] = n_pos; out_i[3 * c + 2] = u2_total;
        out_d[2 * c] = (st & GSN_RANK_ONE_CLASS) ? (double)NAN : (double)u2_total / (2.0 * (double)n_pos * (double)n_neg);
        out_d[2 * c + 1] = (st & GSN_RANK_NO_POSITIVE) ? (double)NAN : ap_total;
        status[c] = st;
    }
}

static int64_t ev_chunks(int kind, int64_t rows, int64_t cols) {
    const int64_t units = kind == GSN_LOSS_CE ? rows : rows * cols;
    return (units + EV_CHUNK - 1) / EV_CHUNK;
}
static int64_t ev_scratch(int kind, int64_t rows, int64_t cols) {
    if (kind < GSN_LOSS_BCE || kind > GSN_LOSS_CE || rows <= 0 || cols <= 0 || rows > INT64_MAX / 64 / cols) return 0;
    if (rows * cols <= EV_ONE_LAUNCH_ELEMS) return 0;
    return ((int64_t)sizeof(EvPart) * ev_chunks(kind, rows, cols) + 255) / 256 * 256;
}

// shape and pointer checks common to the loss entries (with_scratch: the entry takes the workspace of the two-launch path)
static int ev_check(const char *who, int kind, int64_t rows, int64_t cols, const void *y_hat, const void *y, bool with_scratch, const void *scratch,
                    int64_t scratch_bytes) {
    if (kind < GSN_LOSS_BCE || kind > GSN_LOSS_CE) return set_error(GSN_E_INVALID, "%s: unknown loss kind %d", who, kind);
    if (rows < 0 || cols < 0) return set_error(GSN_E_INVALID, "%s: negative shape", who);
    // (a row's loss reads its target's class and its maximum: rows without classes have neither.  torch refuses the shape as well)
    if (kind == GSN_LOSS_CE && rows > 0 && cols == 0) return set_error(GSN_E_INVALID, "%s: CrossEntropyLoss over %lld rows of 0 classes", who, (long long)rows);
    if (rows > 0 && cols > 0 && rows > ((int64_t)1 << 40) / cols) return set_error(GSN_E_UNSUPPORTED, "%s: more than 2^40 elements", who);
    if (rows > 0 && cols > 0 && (!y_hat || !y)) return set_error(GSN_E_INVALID, "%s: null pointer with %lld x %lld predictions", who, (long long)rows, (long long)cols);
    const int64_t need = with_scratch ? ev_scratch(kind, rows, cols) : 0;
    if (need > 0 && !scratch) return set_error(GSN_E_INVALID, "%s: null scratch with %lld x %lld predictions", who, (long long)rows, (long long)cols);
    if (need > 0 && (reinterpret_cast<uintptr_t>(scratch) & 7) != 0) return set_error(GSN_E_INVALID, "%s: scratch must be 8-byte aligned", who);
    if (scratch_bytes < need) return set_error(GSN_E_NOSPACE, "%s: scratch of %lld bytes < %lld", who, (long long)scratch_bytes, (long long)need);
    return GSN_OK;
}

template <bool ACC, bool COUNTED = false>
static int ev_launch(const EvArgs &a, float *loss, int64_t *count, const EvAcc &c, void *scratch, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a.rows * a.cols <= EV_ONE_LAUNCH_ELEMS) {
        hipLaunchKernelGGL((ev_small_kernel<ACC, COUNTED>), dim3(1), dim3(256), 0, s, a, loss, count, c);
        return launch_check("ev_small_kernel");
    }
    const int64_t n_chunks = ev_chunks(a.kind, a.rows, a.cols);
    EvPart *parts = reinterpret_cast<EvPart *>(scratch);
    hipLaunchKernelGGL((ev_partial_kernel<ACC, COUNTED>), dim3(us_grid(n_chunks)), dim3(256), 0, s, a, parts, n_chunks, c);
    hipLaunchKernelGGL((ev_combine_kernel<ACC, COUNTED>), dim3(1), dim3(64), 0, s, a, parts, n_chunks, loss, count, c);
    return launch_check("ev_partial_kernel / ev_combine_kernel");
}

}  // namespace gsn

using namespace gsn;

extern "C" int64_t gsn_masked_loss_scratch_bytes(int kind, int64_t rows, int64_t cols) { return ev_scratch(kind, rows, cols); }
extern "C" int64_t gsn_eval_accumulate_scratch_bytes(int kind, int64_t rows, int64_t cols) { return ev_scratch(kind, rows, cols); }

extern "C" int gsn_masked_loss_fwd_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, float *loss, int64_t *count,
                                       void *scratch, int64_t scratch_bytes, void *stream) {
    const int rc = ev_check("gsn_masked_loss_fwd_hip", kind, rows, cols, y_hat, y, true, scratch, scratch_bytes);
    if (rc != GSN_OK) return rc;
    // (an empty shape with somewhere to write still launches: the mean of nothing is NaN and the count 0, as torch)
    if ((rows == 0 || cols == 0) && (!loss || !count)) return GSN_OK;
    if (!loss || !count) return set_error(GSN_E_INVALID, "gsn_masked_loss_fwd_hip: null loss or count pointer");
    EvArgs a{kind, GSN_METRIC_NONE, rows, cols, y_hat, y};
    return ev_launch<false>(a, loss, count, EvAcc{}, scratch, stream);
}

extern "C" int gsn_masked_loss_bwd_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, const float *grad_loss,
                                       const int64_t *count, float *grad_y_hat, void *stream) {
    const int rc = ev_check("gsn_masked_loss_bwd_hip", kind, rows, cols, y_hat, y, false, nullptr, 0);
    if (rc != GSN_OK) return rc;
    if (rows == 0 || cols == 0) return GSN_OK;
    if (!grad_loss || !count || !grad_y_hat) return set_error(GSN_E_INVALID, "gsn_masked_loss_bwd_hip: null gradient or count pointer");
    EvArgs a{kind, GSN_METRIC_NONE, rows, cols, y_hat, y};
    const int64_t units = kind == GSN_LOSS_CE ? rows : rows * cols;
    hipLaunchKernelGGL(ev_bwd_kernel<false>, dim3(us_grid((units + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, grad_loss, count,
                       grad_y_hat, (const int64_t *)nullptr);
    return launch_check("ev_bwd_kernel");
}

// The two launches of the masked loss with the row count READ FROM DEVICE MEMORY: rows >= clamp(*n_valid, 0, rows) are unlabelled whatever
// they hold (the integer pad targets of CrossEntropyLoss are 0, not NaN).  The host `rows` picks the launch shape and the scratch size.
extern "C" int gsn_masked_loss_fwd_counted_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, const int64_t *n_valid,
                                               float *loss, int64_t *count, void *scratch, int64_t scratch_bytes, void *stream) {
    if (!n_valid) return set_error(GSN_E_INVALID, "gsn_masked_loss_fwd_counted_hip: null n_valid");
    const int rc = ev_check("gsn_masked_loss_fwd_counted_hip", kind, rows, cols, y_hat, y, true, scratch, scratch_bytes);
    if (rc != GSN_OK) return rc;
    if ((rows == 0 || cols == 0) && (!loss || !count)) return GSN_OK;
    if (!loss || !count) return set_error(GSN_E_INVALID, "gsn_masked_loss_fwd_counted_hip: null loss or count pointer");
    EvArgs a{kind, GSN_METRIC_NONE, rows, cols, y_hat, y};
    EvAcc c{};
    c.n_valid = n_valid;
    return ev_launch<false, true>(a, loss, count, c, scratch, stream);
}

extern "C" int gsn_masked_loss_bwd_counted_hip(int kind, int64_t rows, int64_t cols, const float *y_hat, const void *y, const int64_t *n_valid,
                                               const float *grad_loss, const int64_t *count, float *grad_y_hat, void *stream) {
    if (!n_valid) return set_error(GSN_E_INVALID, "gsn_masked_loss_bwd_counted_hip: null n_valid");
    const int rc = ev_check("gsn_masked_loss_bwd_counted_hip", kind, rows, cols, y_hat, y, false, nullptr, 0);
    if (rc != GSN_OK) return rc;
    if (rows == 0 || cols == 0) return GSN_OK;
    if (!grad_loss || !count || !grad_y_hat) return set_error(GSN_E_INVALID, "gsn_masked_loss_bwd_counted_hip: null gradient or count pointer");
    EvArgs a{kind, GSN_METRIC_NONE, rows, cols, y_hat, y};
    const int64_t units = kind == GSN_LOSS_CE ? rows : rows * cols;
    hipLaunchKernelGGL(ev_bwd_kernel<true>, dim3(us_grid((units + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, grad_loss,
                       count, grad_y_hat, n_valid);
    return launch_check("ev_bwd_kernel<counted>");
}

static int ev_accumulate(const char *who, const int64_t *n_valid, int kind, int metric, int64_t rows, int64_t cols, int64_t y_cols, const float *y_hat, const void *y,
                                       int64_t num_graphs, double *acc_f64, int64_t *acc_i64, float *pred_buf, void *true_buf,
                                       int64_t capacity, float *loss_out, void *scratch, int64_t scratch_bytes, void *stream) {
    const int rc = ev_check(who, kind, rows, cols, y_hat, y, true, scratch, scratch_bytes);
    if (rc != GSN_OK) return rc;
    if (metric < GSN_METRIC_NONE || metric > GSN_METRIC_ACCURACY) return set_error(GSN_E_INVALID, "%s: unknown metric %d", who, metric);
    if ((metric == GSN_METRIC_ACCURACY) != (kind == GSN_LOSS_CE) && metric != GSN_METRIC_NONE)
        return set_error(GSN_E_INVALID, "%s: the accuracy metric goes with integer targets (GSN_LOSS_CE), the L1 / MSE sums with the element-wise kinds", who);
    if (capacity < 0 || y_cols < 0 || num_graphs < 0) return set_error(GSN_E_INVALID, "%s: negative capacity, target width or graph count", who);
    if (rows == 0 || cols == 0) return GSN_OK;
    if (y_cols != (kind == GSN_LOSS_CE ? 1 : cols))
        return set_error(GSN_E_INVALID, "%s: %lld target columns for %lld x %lld predictions", who, (long long)y_cols, (long long)rows, (long long)cols);
    if (!acc_f64 || !acc_i64) return set_error(GSN_E_INVALID, "%s: null accumulator pointer", who);
    EvArgs a{kind, metric, rows, cols, y_hat, y};
    EvAcc c{num_graphs, acc_f64, acc_i64, pred_buf, true_buf, capacity, kind == GSN_LOSS_CE ? 2 : y_cols, loss_out, n_valid};
    return n_valid ? ev_launch<true, true>(a, nullptr, nullptr, c, scratch, stream) : ev_launch<true>(a, nullptr, nullptr, c, scratch, stream);
}

extern "C" int gsn_eval_accumulate_hip(int kind, int metric, int64_t rows, int64_t cols, int64_t y_cols, const float *y_hat, const void *y,
                                       int64_t num_graphs, double *acc_f64, int64_t *acc_i64, float *pred_buf, void *true_buf,
                                       int64_t capacity, float *loss_out, void *scratch, int64_t scratch_bytes, void *stream) {
    return ev_accumulate("gsn_eval_accumulate_hip", nullptr, kind, metric, rows, cols, y_cols, y_hat, y, num_graphs, acc_f64, acc_i64, pred_buf, true_buf,
                         capacity, loss_out, scratch, scratch_bytes, stream);
}

extern "C" int gsn_eval_accumulate_counted_hip(int kind, int metric, int64_t rows, int64_t cols, int64_t y_cols, const float *y_hat, const void *y,
                                               const int64_t *n_valid, double *acc_f64, int64_t *acc_i64, float *pred_buf, void *true_buf,
                                               int64_t capacity, float *loss_out, void *scratch, int64_t scratch_bytes, void *stream) {
    if (!n_valid) return set_error(GSN_E_INVALID, "gsn_eval_accumulate_counted_hip: null n_valid");
    return ev_accumulate("gsn_eval_accumulate_counted_hip", n_valid, kind, metric, rows, cols, y_cols, y_hat, y, 0, acc_f64, acc_i64, pred_buf, true_buf,
                         capacity, loss_out, scratch, scratch_bytes, stream);
}

static int64_t ev_rank_keys_bytes(int64_t m, int64_t c) { return (8 * m * c + 255) / 256 * 256; }

extern "C" int64_t gsn_rank_metrics_scratch_bytes(int64_t m_rows, int64_t n_cols) {
    if (m_rows <= 0 || n_cols <= 0 || n_cols > 65535 || m_rows >= ((int64_t)1 << 31)) return 0;
    return ev_rank_keys_bytes(m_rows, n_cols);
}

extern "C" int gsn_rank_metrics_hip(int64_t m_rows, int64_t n_cols, const float *y_pred, const float *y_true, int64_t *out_i64, double *out_f64,
                                    int32_t *status, void *scratch, int64_t scratch_bytes, void *stream) {
    const char *who = "gsn_rank_metrics_hip";
    if (m_rows < 0 || n_cols < 0) return set_error(GSN_E_INVALID, "%s: negative shape", who);
    if (n_cols == 0) return GSN_OK;
    if (n_cols > 65535 || m_rows >= ((int64_t)1 << 31)) return set_error(GSN_E_UNSUPPORTED, "%s: more than 65535 columns or 2^31 - 1 rows", who);
    if (!out_i64 || !out_f64 || !status || (m_rows > 0 && (!y_pred || !y_true || !scratch)))
        return set_error(GSN_E_INVALID, "%s: null pointer with %lld x %lld predictions", who, (long long)m_rows, (long long)n_cols);
    if (m_rows > 0 && (reinterpret_cast<uintptr_t>(scratch) & 7) != 0) return set_error(GSN_E_INVALID, "%s: scratch must be 8-byte aligned", who);
    const int64_t need = gsn_rank_metrics_scratch_bytes(m_rows, n_cols);
    if (scratch_bytes < need) return set_error(GSN_E_NOSPACE, "%s: scratch of %lld bytes < %lld", who, (long long)scratch_bytes, (long long)need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint64_t *keys = reinterpret_cast<uint64_t *>(scratch);
    if (m_rows > 0) {
        UsLaunches<EvKeyLoad> ops{m_rows, n_cols, EvKeyLoad{y_pred, y_true}, keys, s};
        us_schedule(m_rows, ops);
    }
    // (no rows: every column is empty -- one class, no positive -- and the kernel reads no key)
    hipLaunchKernelGGL(ev_rank_kernel, dim3((unsigned)n_cols), dim3(256), 0, s, m_rows, keys, out_i64, out_f64, status);
    return launch_check("rank metric kernels");
}
