// Host harness of gsn_amd/csrc/loader_core.h (test-only; built with -fsanitize=address,undefined by tests/test_loader_cpu.py and run as a
// process of its own).  It runs the per-(field, slot) routine of the collate kernel for every pair and every lane of generated datasets
// and compares every output byte with a plain concatenation; a last case checks the int64 arithmetic alone with row pointers and plan
// offsets beyond 2^32 on a fake address base (nothing is dereferenced there).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../gsn_amd/csrc/loader_core.h"

using namespace gsn;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, "\n");                    \
            ++failures;                                    \
        }                                                  \
    } while (0)

struct HostField {
    int cls, kind, elem_bytes, flags;
    int64_t row_bytes;
    std::vector<unsigned char> data;      // COPY: rows * row_bytes; EDGE_INDEX: int64 [2, total]
};

// classes: 0 vertices, 1 edge columns, 2 one row per graph, 3 a per-vertex field cut short
static void run_case(int64_t G, int64_t bs, bool drop_last, unsigned seed, int64_t long_graph) {
    std::mt19937_64 rng(seed);
    const int C = 4;
    std::vector<std::vector<int64_t>> sizes(C, std::vector<int64_t>(G)), rp(C, std::vector<int64_t>(G + 1, 0));
    for (int64_t g = 0; g < G; ++g) {
        const int64_t n = g == long_graph ? 700 : 1 + (int64_t)(rng() % 9);
        sizes[0][g] = n;
        sizes[1][g] = g == long_graph ? 1500 : (int64_t)(rng() % 12);      // zero-edge graphs occur
        sizes[2][g] = 1;
        sizes[3][g] = n - (int64_t)(rng() % 2);                            // may be one row shorter (and empty)
    }
    for (int c = 0; c < C; ++c)
        for (int64_t g = 0; g < G; ++g) rp[c][g + 1] = rp[c][g] + sizes[c][g];
    std::vector<HostField> fields = {
        {1, GSN_LOADER_EDGE_INDEX, 8, 0, 8, {}},      // edge_index
        {0, GSN_LOADER_COPY, 8, GSN_LOADER_F_NODES, 8, {}},      // x int64 [n, 1]
        {0, GSN_LOADER_COPY, 4, 0, 20, {}},           // float32 [n, 5]: 20-byte rows
        {3, GSN_LOADER_COPY, 4, 0, 4, {}},            // degrees
        {1, GSN_LOADER_COPY, 8, 0, 40, {}},           // identifiers int64 [E, 5]
        {1, GSN_LOADER_COPY, 4, 0, 12, {}},           // int32 [E, 3]
        {2, GSN_LOADER_COPY, 4, 0, 4, {}},            // y
        {2, GSN_LOADER_COPY, 8, 0, 8, {}},            // graph_size
    };
    const int F = (int)fields.size();
    for (auto &f : fields) {
        const int64_t total = rp[f.cls][G];
        if (f.kind == GSN_LOADER_EDGE_INDEX) {
            f.data.resize((size_t)(2 * total * 8));
            int64_t *ei = reinterpret_cast<int64_t *>(f.data.data());
            for (int64_t g = 0; g < G; ++g)
                for (int64_t e = rp[1][g]; e < rp[1][g + 1]; ++e)
                    for (int r = 0; r < 2; ++r) ei[r * total + e] = (int64_t)(rng() % (uint64_t)sizes[0][g]);
        } else {
            f.data.resize((size_t)(total * f.row_bytes));
            for (auto &b : f.data) b = (unsigned char)(rng() & 0xff);
        }
    }
    std::vector<int64_t> order(G);
    for (int64_t i = 0; i < G; ++i) order[i] = i;
    for (int64_t i = G - 1; i > 0; --i) std::swap(order[i], order[(int64_t)(rng() % (uint64_t)(i + 1))]);
    // the epoch plan, as gsn_amd/loader.py: epoch_plan builds it
    std::vector<int64_t> plan((size_t)(C * G));
    for (int c = 0; c < C; ++c) {
        int64_t run = 0;
        for (int64_t i = 0; i < G; ++i) {
            if (i % bs == 0) run = 0;
            plan[c * G + i] = run;
            run += sizes[c][order[i]];
        }
    }
    const int64_t n_batches = drop_last ? G / bs : (G + bs - 1) / bs;
    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t first = b * bs, B = std::min(bs, G - first);
        int64_t tot[C] = {0, 0, 0, 0};
        for (int64_t s = 0; s < B; ++s)
            for (int c = 0; c < C; ++c) tot[c] += sizes[c][order[first + s]];
        // expected: a plain concatenation
        std::vector<std::vector<unsigned char>> want(F), got(F);
        std::vector<int64_t> want_batch, want_nptr(1, 0), want_eptr(1, 0);
        for (int64_t s = 0; s < B; ++s) {
            const int64_t g = order[first + s];
            want_batch.insert(want_batch.end(), (size_t)sizes[0][g], s);
            want_nptr.push_back(want_nptr.back() + sizes[0][g]);
            want_eptr.push_back(want_eptr.back() + sizes[1][g]);
        }
        for (int fi = 0; fi < F; ++fi) {
            const HostField &f = fields[fi];
            if (f.kind == GSN_LOADER_EDGE_INDEX) {
                want[fi].resize((size_t)(2 * tot[1] * 8));
                int64_t *w = reinterpret_cast<int64_t *>(want[fi].data());
                const int64_t *ei = reinterpret_cast<const int64_t *>(f.data.data());
                int64_t col = 0;
                for (int64_t s = 0; s < B; ++s) {
                    const int64_t g = order[first + s];
                    for (int64_t e = rp[1][g]; e < rp[1][g + 1]; ++e, ++col)
                        for (int r = 0; r < 2; ++r) w[r * tot[1] + col] = ei[r * rp[1][G] + e] + want_nptr[(size_t)s];
                }
            } else {
                for (int64_t s = 0; s < B; ++s) {
                    const int64_t g = order[first + s];
                    want[fi].insert(want[fi].end(), f.data.begin() + rp[f.cls][g] * f.row_bytes, f.data.begin() + rp[f.cls][g + 1] * f.row_bytes);
                }
            }
            got[fi].assign(want[fi].size(), 0xCD);      // exact size: ASan sees any byte past a destination
        }
        std::vector<int64_t> got_batch((size_t)tot[0], -7), got_nptr((size_t)B + 1, -7), got_eptr((size_t)B + 1, -7);
        std::vector<gsn_loader_field> tab((size_t)F);
        for (int fi = 0; fi < F; ++fi) {
            const HostField &f = fields[fi];
            gsn_loader_field &t = tab[(size_t)fi];
            std::memset(&t, 0, sizeof t);
            t.src = f.data.data();
            t.row_ptr = rp[f.cls].data();
            t.dst_rows = tot[f.cls];
            t.dst = t.dst_rows ? got[fi].data() : nullptr;
            t.row_bytes = f.row_bytes;
            t.elem_bytes = f.elem_bytes;
            t.ptr_class = f.cls;
            t.kind = f.kind;
            t.inc_class = 0;
            t.flags = f.flags;
            t.src_stride = rp[1][G];
            t.dst_stride = tot[1];
        }
        // every pair, every lane -- in an order no launch would promise (pairs backwards, lanes backwards)
        const int64_t n_pairs = (int64_t)F * B;
        for (int64_t pair = n_pairs - 1; pair >= 0; --pair) {
            int field;
            int64_t slot;
            ld_pair_of(pair, B, &field, &slot);
            CHECK(field >= 0 && field < F && slot >= 0 && slot < B, "pair %" PRId64 " -> (%d, %" PRId64 ")", pair, field, slot);
            for (int lane = LD_WAVE - 1; lane >= 0; --lane)
                ld_run_pair(tab[(size_t)field], order.data(), plan.data(), G, first, B, slot, lane, got_batch.data(), got_nptr.data(), got_eptr.data());
        }
        for (int fi = 0; fi < F; ++fi)
            CHECK(got[fi] == want[fi], "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": field %d differs", G, bs, b, fi);
        CHECK(got_batch == want_batch, "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": batch vector differs", G, bs, b);
        CHECK(got_nptr == want_nptr, "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": node pointer differs", G, bs, b);
        CHECK(got_eptr == want_eptr, "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": edge pointer differs", G, bs, b);
    }
}

// offsets beyond 2^32 (rows of a field of tens of GB): the arithmetic only, on a fake base
static void big_offsets() {
    const int64_t big = (int64_t)1 << 33;
    const int64_t row_ptr[2] = {big + 3, big + 10};
    const int64_t order[1] = {0};
    const int64_t stride = 1;
    const int64_t plan[3] = {big + 11, 5 * big + 1, 77};      // class 0, 1, 2 at position 0
    const LdSeg s = ld_segment(row_ptr, order, plan, stride, 1, 0);
    CHECK(s.src_row == big + 3 && s.n_rows == 7 && s.dst_row == 5 * big + 1, "segment");
    CHECK(ld_plan_at(plan, stride, 0, 0) == big + 11, "increment");
    CHECK(ld_copy_elems(s, 20, 4) == 35, "elements of 7 rows of 20 bytes");
    CHECK(ld_copy_src_elem(s, 20, 4) == 5 * (big + 3), "source element");
    CHECK(ld_copy_dst_elem(s, 20, 4) == 5 * (5 * big + 1), "destination element");
    CHECK(ld_copy_dst_elem(s, 40, 8) == 5 * (5 * big + 1), "destination element, 8-byte units");
    const int64_t estride = 6 * big;
    CHECK(ld_edge_src_elem(s, 1, estride) == 6 * big + big + 3 && ld_edge_src_elem(s, 0, estride) == big + 3, "edge source row");
    CHECK(ld_edge_dst_elem(s, 1, estride) == 6 * big + 5 * big + 1, "edge destination row");
    CHECK(ld_fits(s, 5 * big + 8) && !ld_fits(s, 5 * big + 7), "bound of the destination");
    const uintptr_t base = (uintptr_t)1 << 44;
    const uintptr_t addr = base + (uintptr_t)ld_copy_dst_elem(s, 20, 4) * 4u;
    CHECK(addr == base + (uintptr_t)20 * (uintptr_t)(5 * big + 1), "byte address on a fake base");
    CHECK((uint64_t)(addr - base) > ((uint64_t)1 << 39), "the offset does pass 2^32");
    int field;
    int64_t slot;
    ld_pair_of(3 * big + 5, big, &field, &slot);
    CHECK(field == 3 && slot == 5, "pair of a batch of 2^33 slots");
}

int main() {
    run_case(1, 1, false, 1, -1);
    run_case(5, 7, false, 2, -1);
    run_case(40, 7, false, 3, 17);       // a 700-vertex / 1 500-column graph: many passes of a wave
    run_case(40, 7, true, 4, -1);
    run_case(40, 40, false, 5, 0);
    run_case(40, 64, false, 6, -1);
    run_case(40, 1, false, 7, 39);
    run_case(131, 32, true, 8, 64);
    big_offsets();
    if (failures) {
        std::fprintf(stderr, "loader harness: %d failures\n", failures);
        return 1;
    }
    std::printf("loader harness ok\n");
    return 0;
}
