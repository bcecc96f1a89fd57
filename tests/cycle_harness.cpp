// TEST-ONLY logic harness (not product code, never shipped in libgsn_hip.so).
// Compiles the cycle path walk and the plan recognition of gsn_amd/csrc/count_core.h for the HOST, so that both can be checked
// against the oracle and against plan tables from gsn_count_plan_build on a machine without a GPU.  The graph set-up mirrors the
// kernel's phases 1-2 (self loops dropped, parallel edges merged, last duplicate wins, reverse-row lookup, 2-core filter).
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "../gsn_amd/csrc/count_core.h"

namespace gsn {
int set_error(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr);
    return code;
}
}
using namespace gsn;

template <int L>
static int run(int64_t n, int64_t E, const int64_t *src, const int64_t *dst, int prune, int64_t *out) {
    std::vector<uint64_t> A((size_t)(n ? n : 1), 0);
    int n_active = 0;
    for (int64_t c = 0; c < E; ++c) {
        const int u = (int)src[c], v = (int)dst[c];
        n_active = std::max(n_active, std::max(u, v) + 1);
        if (u == v) continue;
        A[u] |= 1ull << v;
        A[v] |= 1ull << u;
    }
    uint64_t core = below_word(n_active, 0);
    for (bool changed = prune != 0; changed;) {
        changed = false;
        uint64_t drop = 0;
        for (int v = 0; v < (int)n; ++v)
            if (((core >> v) & 1ull) && !core_keeps<1>(A.data(), &core, v, 2)) drop |= 1ull << v;
        if (drop) { core &= ~drop; changed = true; }
    }
    std::vector<int64_t> last((size_t)(n * n ? n * n : 1), -1);
    for (int64_t c = 0; c < E; ++c) last[(size_t)src[c] * n + dst[c]] = c;
    int status = 0;
    for (int64_t row = 0; row < E; ++row) {
        const int u = (int)src[row], v = (int)dst[row];
        uint64_t cnt[L - 2];
        for (int i = 0; i < L - 2; ++i) cnt[i] = 0;
        const bool live = u != v && last[(size_t)u * n + v] == row;
        // (the kernel's root filter: a row with a root outside the 2-core never walks)
        if (live && (!prune || (((core >> u) & (core >> v)) & 1ull))) cycle_walk<L>(A.data(), u, v, prune ? core : ~0ull, cnt);
        bool any = false;
        for (int i = 0; i < L - 2; ++i) { out[row * (L - 2) + i] = (int64_t)cnt[i]; any = any || cnt[i] != 0; }
        if (live && last[(size_t)v * n + u] < 0 && any) status = 1;
    }
    return status;
}

// out[E][L - 2]: column k - 3 = the k-cycle identifier of every row; returns 1 where the reference raises KeyError, -1 on bad arguments
extern "C" int cycle_harness_walk(int L, int64_t n, int64_t E, const int64_t *src, const int64_t *dst, int prune, int64_t *out) {
    if (n > 64) return -1;
    if (L == 6) return run<6>(n, E, src, dst, prune, out);
    if (L == 8) return run<8>(n, E, src, dst, prune, out);
    return -1;
}

extern "C" int cycle_harness_recognise(const uint32_t *plan, int64_t plan_words, uint8_t *len, int len_cap) {
    return cycle_plan_lengths(plan, plan_words, len, len_cap);
}
