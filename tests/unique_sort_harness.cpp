// Test-only host harness of gsn_amd/csrc/unique_sort_core.h: the sorting network's pair arithmetic, its launch schedule, the run-start
// compaction and the searches, executed on the CPU step by step the way unique_sort.hip launches them (tiles with +infinity padding,
// whole-column steps that skip pairs reaching past M, chunks of four keys per thread).  Not a product path.
#include <cstdint>
#include <utility>
#include <vector>

#include "../gsn_amd/csrc/unique_sort_core.h"

using namespace gsn;

namespace {

struct HostOps {
    int64_t m;
    std::vector<uint64_t> &k;
    int launches = 0;
    void tile(bool first) {
        ++launches;
        std::vector<uint64_t> s(US_TILE);
        for (int64_t base = 0; base < m; base += US_TILE) {
            for (int i = 0; i < US_TILE; ++i) s[i] = base + i < m ? k[base + i] : ~0ull;
            const int k_first = first ? 1 : US_LOG_TILE + 1, k_last = first ? US_LOG_TILE : US_LOG_TILE + 1;
            for (int kk = k_first; kk <= k_last; ++kk) {
                if (first)
                    for (int t = 0; t < US_TILE / 2; ++t) {
                        int64_t lo, hi;
                        us_pair_flip(t, kk, lo, hi);
                        if (s[lo] > s[hi]) std::swap(s[lo], s[hi]);
                    }
                for (int j = first ? kk - 2 : US_LOG_TILE - 1; j >= 0; --j)
                    for (int t = 0; t < US_TILE / 2; ++t) {
                        int64_t lo, hi;
                        us_pair_step(t, j, lo, hi);
                        if (s[lo] > s[hi]) std::swap(s[lo], s[hi]);
                    }
            }
            for (int i = 0; i < US_TILE; ++i)
                if (base + i < m) k[base + i] = s[i];
        }
    }
    void global(int kj, bool flip, int64_t n_pairs) {
        ++launches;
        for (int64_t t = 0; t < n_pairs; ++t) {
            int64_t lo, hi;
            if (flip) us_pair_flip(t, kj, lo, hi); else us_pair_step(t, kj, lo, hi);
            if (hi < m && k[lo] > k[hi]) std::swap(k[lo], k[hi]);
        }
    }
    void tile_sort() { tile(true); }
    void tile_merge() { tile(false); }
    void global_flip(int kk) { global(kk, true, us_pair_count(m, kk - 1)); }
    void global_step(int j) { global(j, false, us_pair_count(m, j)); }
};

}  // namespace

// one column: values[m] -> uniques (first return-value entries), codes[m]; returns the number of distinct values; *launches = sort launches
extern "C" int64_t harness_unique_sort(int64_t m, const int64_t *values, int64_t *uniques, int64_t *codes, int *launches) {
    std::vector<uint64_t> k(m);
    for (int64_t i = 0; i < m; ++i) k[i] = us_key(values[i]);
    HostOps ops{m, k};
    if (m > 0) us_schedule(m, ops);
    if (launches) *launches = ops.launches;
    const int64_t n_chunks = (m + US_CHUNK - 1) / US_CHUNK;
    std::vector<int64_t> off(n_chunks + 1, 0);
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
        int64_t cnt = 0;
        for (int t = 0; t < 256; ++t) cnt += __builtin_popcount(us_run_starts(k.data(), m, ch * US_CHUNK + 4 * t));
        off[ch + 1] = off[ch] + cnt;
    }
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
        int64_t pos = off[ch];
        for (int t = 0; t < 256; ++t) {
            const int64_t i0 = ch * US_CHUNK + 4 * t;
            const int flags = us_run_starts(k.data(), m, i0);
            for (int u = 0; u < 4; ++u)
                if ((flags >> u) & 1) uniques[pos++] = us_value(k[i0 + u]);
        }
    }
    const int64_t nd = off[n_chunks];
    for (int64_t i = 0; i < m; ++i) {
        bool unseen;
        codes[i] = us_lookup(uniques, nd, values[i], 0, &unseen);
    }
    return nd;
}

// codes of r values against n sorted distinct values; returns the number of unseen values
extern "C" int64_t harness_lookup(int64_t r, const int64_t *values, int64_t n, const int64_t *uniques, int clamp, int64_t *codes) {
    int64_t bad = 0;
    for (int64_t i = 0; i < r; ++i) {
        bool unseen;
        codes[i] = us_lookup(uniques, n, values[i], clamp, &unseen);
        bad += unseen;
    }
    return bad;
}
