// Internal declarations shared by the translation units of libgsn_hip.so (not part of the ABI).
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <atomic>
#include <initializer_list>
#include <vector>

#include "../../include/gsn_abi.h"
#include "switches.h"

namespace gsn {

// packed counting-plan table (uint32 words) -- written by gsn_count_plan_build, read by the kernel
//   header : [0] magic  [1] mode  [2] induced  [3] n_plans  [4] n_cols  [5] kmax  [6] directed_orbits | directed<<1  [7] plans_off
//   col_ptr: [8 .. 8+n_cols]  plans col_ptr[c]..col_ptr[c+1] all write output column c (plans are sorted by column)
//   col_order: [9+n_cols .. 9+2 n_cols)  the columns by falling estimated search cost (the order the kernel hands cells out in)
//   plan p : at plans_off + p*plan_stride(header[6]): [0] k | n_fixed<<8 | out_col<<16     [1] pattern | root_a<<16 | min_degree<<20 | root_b<<24 | tail_mode<<28 (closed form of the last two levels: patterns.cpp)
//            [2+l] level l: adj_mask | nonadj_mask<<8 | gt_mask<<16 | lt_mask<<24   (bit j = earlier level j)
//            [2+KMAX + l/4] byte l%4: distance constraint of level l:  j | r<<3  (r = 0 none, 2 or 3): the image of level
//                         l must lie within r hops of the image of level j (r = their distance in the pattern)
constexpr uint32_t PLAN_MAGIC = 0x47534e31u;  // 'GSN1'
constexpr int PLAN_HEADER_WORDS = 8;
//            directed patterns only: [PLAN_STRIDE_WORDS + l] level l: in_adj_mask | in_nonadj_mask<<8 -- the image must (not) be
//                         an IN-neighbour of f_j (pattern arc level l -> level j); [2+l] then speaks of OUT-neighbours of f_j
constexpr int PLAN_BALL_WORDS = (GSN_KMAX + 3) / 4;
constexpr int PLAN_STRIDE_WORDS = 2 + GSN_KMAX + PLAN_BALL_WORDS;
// (the partial map of a search holds levels 0 .. 7 -- 8 bits each, or 16 in two registers: count_core.h FVec -- and the masks of a level name
//  EARLIER levels by bit: a ninth level (GSN_KMAX = 9) needs neither a ninth slot nor a ninth bit, because the last level of a plan is never
//  enumerated: it is counted by popcount or by a closed form)
static_assert(GSN_KMAX <= 9, "level masks are 8 bits wide: the last level may be the ninth, no more");
constexpr int PLAN_STRIDE_DIRECTED = PLAN_STRIDE_WORDS + GSN_KMAX;
inline int plan_stride(uint32_t flags) { return (flags & 2u) ? PLAN_STRIDE_DIRECTED : PLAN_STRIDE_WORDS; }

// WIDE plan table: pattern lists whose largest pattern has 10 .. GSN_KMAX_WIDE = 16 vertices (gsn_count_plan_build with GSN_FLAG_WIDE).
// Executed by the sparse kernel only (count_sparse.hip: sparse_search_kernel<DIR, true>); its magic word makes every consumer of the narrow
// table refuse it.  Header, col_ptr and col_order as above (header[5] = kmax > GSN_KMAX); ALL plans of the table, those of its <= 9-vertex
// patterns included, are wide records:
//   plan p : at plans_off + p*plan_stride_wide(header[6]): [0] k | n_fixed<<8 | out_col<<16   [1] pattern | root_a<<16 | root_b<<24 |
//            tail_mode<<28 | (twin_run - 2)<<30 as in the narrow record (min_degree = 0: cores, like distance balls, are pruning hints of
//            the LDS kernel and are left out -- the tail mode is therefore decided without them)
//            [2 + l]                        level l: adj_mask | nonadj_mask<<16          (bit j = earlier level j, j <= 14)
//            [2 + GSN_KMAX_WIDE + l]        level l: gt_mask | lt_mask<<16
//            directed patterns only: [2 + 2 GSN_KMAX_WIDE + l]  level l: in_adj_mask | in_nonadj_mask<<16
// A search holds levels 0 .. 14 (the sixteenth is counted, never placed), so 15 bits of every 16-bit field are used.
constexpr uint32_t PLAN_MAGIC_WIDE = 0x47534e32u;  // 'GSN2'
constexpr int PLAN_WIDE_ORD_OFF = 2 + GSN_KMAX_WIDE;
constexpr int PLAN_WIDE_IN_OFF = 2 + 2 * GSN_KMAX_WIDE;
constexpr int PLAN_STRIDE_WIDE = 2 + 2 * GSN_KMAX_WIDE;
constexpr int PLAN_STRIDE_WIDE_DIRECTED = 2 + 3 * GSN_KMAX_WIDE;
static_assert(GSN_KMAX_WIDE <= 16, "wide level masks are 16 bits wide: the last level may be the sixteenth, no more");
inline int plan_stride_wide(uint32_t flags) { return (flags & 2u) ? PLAN_STRIDE_WIDE_DIRECTED : PLAN_STRIDE_WIDE; }
// what every entry but gsn_count_sparse_hip answers to a wide table (GSN_E_UNSUPPORTED)
#define GSN_WIDE_PLAN_REFUSAL "wide plan (patterns of more than 9 vertices): gsn_count_sparse_hip only"

int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// "done once per DEVICE" flag for per-device kernel attributes (hipFuncSetAttribute applies to the current device only; a
// process may drive several GPUs).  Lock-free: a racing second setter merely repeats the idempotent call.
struct DeviceOnce {
    std::atomic<unsigned long long> mask{0};
    bool done(int dev) const { return dev >= 0 && dev < 64 && ((mask.load(std::memory_order_acquire) >> dev) & 1ull); }
    void mark(int dev) { if (dev >= 0 && dev < 64) mask.fetch_or(1ull << dev, std::memory_order_release); }
};
int current_device();   // hipGetDevice, -1 on error (abi.cpp)

// ---- launch plumbing (abi.cpp); streams travel as void * so that this header needs no HIP include ----
constexpr int LDS_LIMIT_BYTES = 160 * 1024;
template <class... A> const void *kernel_ptr(void (*kernel)(A...)) { return reinterpret_cast<const void *>(kernel); }
// raises the dynamic-LDS limit of `kernels` to `bytes` on the current device, once per device under the caller's static flag
// (`once` null: at every call, for count.hip, whose size varies per call).  The error names the attribute call, (<label>) and the
// HIP error string; a null label stands for "<bytes> B LDS".  After a failure nothing is marked done.
int lds_limit(DeviceOnce *once, std::initializer_list<const void *> kernels, const char *label, int bytes = LDS_LIMIT_BYTES);
// hipGetLastError after a launch: GSN_OK, or GSN_E_HIP with "<label>: <hip string>" (the label is a printf format)
int launch_check(const char *label_fmt, ...) __attribute__((format(printf, 1, 2)));
// a line on stderr when GSN_CHAIN_TRACE is present (read at every call)
void trace(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// device counters of a profiling build: n zeroed unsigned long long on `stream` (n == 0: none, ptr() is null; so it is when the
// allocation fails, and fetch() then returns n zeros)
struct ProfCounters {
    ProfCounters(size_t n, void *stream);
    ~ProfCounters();
    ProfCounters(const ProfCounters &) = delete;
    ProfCounters &operator=(const ProfCounters &) = delete;
    unsigned long long *ptr() const { return dev_; }
    std::vector<unsigned long long> fetch(void *stream);   // waits for the stream, copies the counters out, frees them
private:
    unsigned long long *dev_ = nullptr;
    size_t n_ = 0;
};
// true at every n-th call: the profiling builds print one launch in n
struct EveryNth {
    int n, calls = 0;
    bool operator()() { return calls++ % n == n - 1; }
};
int64_t gsn_wgrad_slab_rows(int64_t m_rows, int64_t tiles, int64_t wg_target);   // backward.hip: rows per slab of a weight-gradient call

}  // namespace gsn
