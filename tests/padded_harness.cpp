// Host harness of gsn_amd/csrc/loader_padded_core.h (test-only; built with -fsanitize=address,undefined by tests/test_padded_loader_cpu.py and
// run as a process of its own).  It runs the per-(field, slot) routine of the padded collate kernel for every pair and every lane of
// generated datasets into destinations of exactly the capacities, poisoned with 0xA5 (and again with 0x5A: a byte left unwritten shows
// under one of them), and compares every byte with a plain concatenation followed by pad graphs built from the rule's statement by loops.
// Small cases also count the writers of every byte, one (pair, lane) unit at a time: exactly one everywhere.  A last case repeats the
// address arithmetic with offsets beyond 2^32 (nothing is dereferenced there).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../gsn_amd/csrc/loader_padded_core.h"

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

typedef std::vector<unsigned char> Bytes;

struct HostField {
    int cls, kind, elem_bytes, flags;      // cls: 0 vertices, 1 edge columns, 2 one row per graph
    int64_t row_bytes;
    uint64_t fill;
    Bytes data;                            // COPY: rows * row_bytes; EDGE_INDEX: int64 [2, total]
};

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static void put(Bytes &b, const void *p, size_t n) { b.insert(b.end(), (const unsigned char *)p, (const unsigned char *)p + n); }

// every output of a batch, one after the other: the fields, batch_vec, node pointer, edge pointer, n_valid
struct Outputs {
    std::vector<Bytes> field;
    std::vector<int64_t> batch, nptr, eptr, n_valid;
    void poison(unsigned char v) {
        for (auto &f : field)
            if (!f.empty()) std::memset(f.data(), v, f.size());
        std::memset(batch.data(), v, batch.size() * 8);
        std::memset(nptr.data(), v, nptr.size() * 8);
        std::memset(eptr.data(), v, eptr.size() * 8);
        std::memset(n_valid.data(), v, 8);
    }
    Bytes flat() const {
        Bytes b;
        for (auto &f : field) put(b, f.data(), f.size());
        put(b, batch.data(), batch.size() * 8);
        put(b, nptr.data(), nptr.size() * 8);
        put(b, eptr.data(), eptr.size() * 8);
        put(b, n_valid.data(), 8);
        return b;
    }
};

// tight: 0 default capacities; 1 the capacities the largest batch of the epoch needs with the least slack the rule allows
static void run_case(int64_t G, int64_t bs, unsigned seed, int64_t long_graph, bool single_vertex, bool edgeless, bool count_writers) {
    std::mt19937_64 rng(seed);
    const int C = 3;
    std::vector<std::vector<int64_t>> sizes(C, std::vector<int64_t>(G)), rp(C, std::vector<int64_t>(G + 1, 0));
    for (int64_t g = 0; g < G; ++g) {
        sizes[0][g] = single_vertex ? 1 : (g == long_graph ? 300 : 1 + (int64_t)(rng() % 7));
        sizes[1][g] = edgeless ? 0 : (g == long_graph ? 700 : (int64_t)(rng() % 9));      // zero-edge graphs occur
        sizes[2][g] = 1;
    }
    for (int c = 0; c < C; ++c)
        for (int64_t g = 0; g < G; ++g) rp[c][g + 1] = rp[c][g] + sizes[c][g];
    const float nan32 = __builtin_nanf("");
    uint32_t nan_bits;
    std::memcpy(&nan_bits, &nan32, 4);
    std::vector<HostField> fields = {
        {1, GSN_LOADER_EDGE_INDEX, 8, 0, 8, 0, {}},                                  // edge_index
        {0, GSN_LOADER_COPY, 8, GSN_LOADER_F_NODES, 8, 0, {}},                       // x int64 [n, 1]
        {0, GSN_LOADER_COPY, 4, 0, 20, 0, {}},                                       // float32 [n, 5]: 20-byte rows
        {0, GSN_LOADER_COPY, 8, 0, 16, 0x1122334455667788ull, {}},                   // float64 [n, 2] with a fill of its own
        {1, GSN_LOADER_COPY, 8, GSN_LOADER_F_PAD_EDGES, 40, 0, {}},                  // identifiers int64 [E, 5]
        {1, GSN_LOADER_COPY, 4, GSN_LOADER_F_PAD_EDGES, 12, 0xDEADBEEFull, {}},      // int32 [E, 3] with a fill of its own
        {2, GSN_LOADER_COPY, 4, GSN_LOADER_F_PAD_GRAPH, 4, nan_bits, {}},            // y: NaN in the pad slots
        {2, GSN_LOADER_COPY, 8, GSN_LOADER_F_PAD_GRAPH, 8, 0, {}},                   // graph_size
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
    std::vector<int64_t> plan((size_t)(C * G));
    for (int c = 0; c < C; ++c) {
        int64_t run = 0;
        for (int64_t i = 0; i < G; ++i) {
            if (i % bs == 0) run = 0;
            plan[c * G + i] = run;
            run += sizes[c][order[i]];
        }
    }
    // the static shape, from the rule's statement
    int64_t n_max = 0, e_max = 0;
    for (int64_t g = 0; g < G; ++g) { n_max = std::max(n_max, sizes[0][g]); e_max = std::max(e_max, sizes[1][g]); }
    const int64_t n_chunk = std::max<int64_t>(n_max, 2), e_chunk = std::max<int64_t>(e_max, 1);
    const int64_t n_batches = (G + bs - 1) / bs;
    int64_t M = 0, E_cap = 0;
    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t first = b * bs, B = std::min(bs, G - first);
        int64_t nr = 0, er = 0;
        for (int64_t s = 0; s < B; ++s) { nr += sizes[0][order[first + s]]; er += sizes[1][order[first + s]]; }
        M = std::max(M, nr + bs - B);
        E_cap = std::max(E_cap, er);
    }
    const int64_t N_cap = M + std::max<int64_t>(1, std::max(ceil_div(M, n_chunk - 1), ceil_div(E_cap, e_chunk)));
    const int64_t P = std::max<int64_t>(1, std::max(ceil_div(N_cap, n_chunk), ceil_div(E_cap, e_chunk))), G_cap = bs + P;
    const int64_t cap[3] = {N_cap, E_cap, G_cap};

    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t first = b * bs, B = std::min(bs, G - first), S = G_cap - B;
        int64_t N_r = 0, E_r = 0;
        for (int64_t s = 0; s < B; ++s) { N_r += sizes[0][order[first + s]]; E_r += sizes[1][order[first + s]]; }
        gsn_loader_pad pad = {B, G_cap, N_r, E_r, N_cap, E_cap, n_chunk, e_chunk};
        CHECK(N_r + S <= N_cap && E_r <= E_cap && lp_fits(pad), "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": does not fit the default capacities", G, bs, b);
        // the pad graphs, by the rule
        const int64_t r_n = N_cap - N_r - S, r_e = E_cap - E_r;
        std::vector<int64_t> pv((size_t)S), pe((size_t)S);
        int64_t sum_v = 0, sum_e = 0;
        for (int64_t k = 0; k < S; ++k) {
            pv[(size_t)k] = 1 + std::min(n_chunk - 1, std::max<int64_t>(0, r_n - k * (n_chunk - 1)));
            pe[(size_t)k] = std::min(e_chunk, std::max<int64_t>(0, r_e - k * e_chunk));
            sum_v += pv[(size_t)k];
            sum_e += pe[(size_t)k];
        }
        CHECK(N_r + sum_v == N_cap && E_r + sum_e == E_cap, "the pad graphs do not use up the capacities");
        // expected: a plain concatenation, then the pad graphs
        Outputs want;
        want.field.resize((size_t)F);
        want.nptr.assign(1, 0);
        want.eptr.assign(1, 0);
        for (int64_t s = 0; s < B; ++s) {
            const int64_t g = order[first + s];
            want.batch.insert(want.batch.end(), (size_t)sizes[0][g], s);
            want.nptr.push_back(want.nptr.back() + sizes[0][g]);
            want.eptr.push_back(want.eptr.back() + sizes[1][g]);
        }
        for (int64_t k = 0; k < S; ++k) {
            want.batch.insert(want.batch.end(), (size_t)pv[(size_t)k], B + k);
            want.nptr.push_back(want.nptr.back() + pv[(size_t)k]);
            want.eptr.push_back(want.eptr.back() + pe[(size_t)k]);
        }
        want.n_valid.assign(1, B);
        for (int fi = 0; fi < F; ++fi) {
            const HostField &f = fields[(size_t)fi];
            Bytes &w = want.field[(size_t)fi];
            if (f.kind == GSN_LOADER_EDGE_INDEX) {
                std::vector<int64_t> m((size_t)(2 * E_cap));
                const int64_t *ei = reinterpret_cast<const int64_t *>(f.data.data());
                int64_t col = 0;
                for (int64_t s = 0; s < B; ++s) {
                    const int64_t g = order[first + s];
                    for (int64_t e = rp[1][g]; e < rp[1][g + 1]; ++e, ++col)
                        for (int r = 0; r < 2; ++r) m[(size_t)(r * E_cap + col)] = ei[r * rp[1][G] + e] + want.nptr[(size_t)s];
                }
                for (int64_t k = 0; k < S; ++k)
                    for (int64_t t = 0; t < pe[(size_t)k]; ++t, ++col)
                        for (int r = 0; r < 2; ++r) m[(size_t)(r * E_cap + col)] = want.nptr[(size_t)(B + k)] + t % pv[(size_t)k];
                CHECK(col == E_cap, "edge columns");
                put(w, m.data(), m.size() * 8);
            } else {
                for (int64_t s = 0; s < B; ++s) {
                    const int64_t g = order[first + s];
                    w.insert(w.end(), f.data.begin() + rp[f.cls][g] * f.row_bytes, f.data.begin() + rp[f.cls][g + 1] * f.row_bytes);
                }
                const int64_t pad_rows = f.cls == 0 ? sum_v : f.cls == 1 ? sum_e : S;
                for (int64_t i = 0; i < pad_rows * (f.row_bytes / f.elem_bytes); ++i) put(w, &f.fill, (size_t)f.elem_bytes);      // (little endian: the low bytes)
            }
            CHECK((int64_t)w.size() == cap[f.cls] * f.row_bytes * (f.kind == GSN_LOADER_EDGE_INDEX ? 2 : 1), "field %d: expected size", fi);
        }
        Outputs got;      // exact sizes: ASan sees any byte past a destination
        got.field.resize((size_t)F);
        for (int fi = 0; fi < F; ++fi) got.field[(size_t)fi].resize(want.field[(size_t)fi].size());
        got.batch.resize((size_t)N_cap);
        got.nptr.resize((size_t)G_cap + 1);
        got.eptr.resize((size_t)G_cap + 1);
        got.n_valid.resize(1);
        std::vector<gsn_loader_field> tab((size_t)F);
        std::vector<uint64_t> fill((size_t)F);
        for (int fi = 0; fi < F; ++fi) {
            const HostField &f = fields[(size_t)fi];
            gsn_loader_field &t = tab[(size_t)fi];
            std::memset(&t, 0, sizeof t);
            t.src = f.data.data();
            t.row_ptr = rp[f.cls].data();
            t.dst_rows = cap[f.cls];
            t.dst = t.dst_rows ? got.field[(size_t)fi].data() : nullptr;
            t.row_bytes = f.row_bytes;
            t.elem_bytes = f.elem_bytes;
            t.ptr_class = f.cls;
            t.kind = f.kind;
            t.inc_class = 0;
            t.flags = f.flags;
            t.src_stride = rp[1][G];
            t.dst_stride = E_cap;
            fill[(size_t)fi] = f.fill;
        }
        const int64_t n_pairs = (int64_t)F * G_cap;
        auto unit = [&](int64_t pair, int lane) {
            int field;
            int64_t slot;
            ld_pair_of(pair, G_cap, &field, &slot);
            lp_run_pair(tab[(size_t)field], fill[(size_t)field], pad, order.data(), plan.data(), G, first, slot, lane, got.batch.data(), got.nptr.data(),
                        got.eptr.data(), got.n_valid.data());
        };
        const Bytes want_flat = want.flat();
        for (int round = 0; round < 2; ++round) {      // every pair, every lane -- in an order no launch would promise
            got.poison(round ? 0x5A : 0xA5);
            for (int64_t pair = n_pairs - 1; pair >= 0; --pair)
                for (int lane = LD_WAVE - 1; lane >= 0; --lane) unit(pair, lane);
            const Bytes g = got.flat();
            CHECK(g.size() == want_flat.size(), "output sizes");
            CHECK(g == want_flat, "G %" PRId64 " bs %" PRId64 " batch %" PRId64 " poison %d: outputs differ", G, bs, b, round);
            for (int fi = 0; fi < F; ++fi)
                CHECK(got.field[(size_t)fi] == want.field[(size_t)fi], "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": field %d differs", G, bs, b, fi);
            CHECK(got.batch == want.batch && got.nptr == want.nptr && got.eptr == want.eptr && got.n_valid == want.n_valid, "batch vector, pointers or n_valid differ");
        }
        if (count_writers) {
            std::vector<int> writers(want_flat.size(), 0);
            for (int64_t pair = 0; pair < n_pairs; ++pair)
                for (int lane = 0; lane < LD_WAVE; ++lane) {
                    got.poison(0xA5);
                    unit(pair, lane);
                    const Bytes a = got.flat();
                    got.poison(0x5A);
                    unit(pair, lane);
                    const Bytes c = got.flat();
                    for (size_t i = 0; i < a.size(); ++i) writers[i] += a[i] != 0xA5 || c[i] != 0x5A;      // (a written byte differs from one poison at least)
                }
            size_t bad = 0;
            for (size_t i = 0; i < writers.size(); ++i) bad += writers[i] != 1;
            CHECK(bad == 0, "G %" PRId64 " bs %" PRId64 " batch %" PRId64 ": %zu of %zu bytes do not have exactly one writer", G, bs, b, bad, writers.size());
        }
    }
}

// capacities a batch misses by exactly one row, and the arithmetic beyond 2^32 (no memory behind it)
static void fit_and_big_offsets() {
    gsn_loader_pad p = {3, 7, 10, 12, 10 + 4 + 5, 12 + 3, 4, 6};      // S = 4, r_n = 5, r_e = 3
    CHECK(lp_fits(p), "fits");
    const int64_t want_v[5] = {10, 14, 17, 18, 19}, want_e[5] = {12, 15, 15, 15, 15};
    for (int k = 0; k <= 4; ++k) CHECK(lp_node_start(p, k) == want_v[k] && lp_edge_start(p, k) == want_e[k], "starts of pad graph %d", k);
    p.node_capacity = 10 + 4 - 1;
    CHECK(!lp_fits(p), "one vertex short: the last pad slot would be empty");
    p.node_capacity = 10 + 4;
    CHECK(lp_fits(p) && lp_node_start(p, 4) == 14, "every pad graph one vertex");
    p.edge_capacity = 11;
    CHECK(!lp_fits(p), "one edge column short");
    p.edge_capacity = 12 + 4 * 6 + 1;
    CHECK(!lp_fits(p), "more spare columns than the pad graphs hold");
    p.edge_capacity = 12 + 4 * 6;
    p.node_capacity = 10 + 4 + 4 * 3 + 1;
    CHECK(!lp_fits(p), "more spare vertices than the pad graphs hold");
    p.node_capacity -= 1;
    CHECK(lp_fits(p) && lp_node_start(p, 4) == p.node_capacity && lp_edge_start(p, 4) == p.edge_capacity, "filled to the brim");
    p.n_real = 7;
    CHECK(!lp_fits(p), "no pad slot");

    const int64_t big = (int64_t)1 << 33;
    gsn_loader_pad q = {5, 5 + 4 * big, 3 * big + 1, 7 * big + 2, 0, 0, 6, 3};
    const int64_t S = 4 * big;
    q.node_capacity = q.n_real_nodes + S + (2 * big + 3);      // r_n = 2^34 + 3: pad graphs 0 .. ceil(r_n / 5) - 1 are larger than one vertex
    q.edge_capacity = q.n_real_edges + 9 * big + 1;            // r_e = 9 * 2^33 + 1
    CHECK(lp_fits(q), "fits, beyond 2^32");
    const int64_t k1 = big / 4, k2 = 3 * big + 5;
    CHECK(lp_node_start(q, k1) == q.n_real_nodes + k1 + 5 * k1, "vertex start in the full chunks");
    CHECK(lp_node_start(q, k2) == q.n_real_nodes + k2 + 2 * big + 3, "vertex start behind the spare vertices");
    CHECK(lp_node_start(q, S) == q.node_capacity && lp_edge_start(q, S) == q.edge_capacity, "ends are the capacities");
    CHECK(lp_edge_start(q, k1) == q.n_real_edges + 3 * k1 && lp_edge_start(q, k2) == q.n_real_edges + 9 * big + 1, "edge starts");
    const int64_t kb = (2 * big + 3) / 5;                      // the pad graph that takes the remainder
    CHECK(lp_node_start(q, kb + 1) - lp_node_start(q, kb) == 1 + (2 * big + 3) % 5, "the remainder's pad graph");
    const uintptr_t base = (uintptr_t)1 << 45;
    const uintptr_t addr = base + (uintptr_t)lp_node_start(q, k2) * 20u;      // a 20-byte row
    CHECK(addr - base == (uintptr_t)20 * (uintptr_t)(3 * big + 1 + 3 * big + 5 + 2 * big + 3) && (uint64_t)(addr - base) > ((uint64_t)1 << 39), "byte address on a fake base");
    int field;
    int64_t slot;
    ld_pair_of(2 * q.graph_slots + k2, q.graph_slots, &field, &slot);
    CHECK(field == 2 && slot == k2, "pair of a batch of 2^35 slots");
}

int main() {
    run_case(1, 1, 1, -1, false, false, true);
    run_case(5, 7, 2, -1, false, false, true);       // G < B
    run_case(13, 4, 3, -1, false, false, true);      // last batch of one graph
    run_case(9, 4, 4, -1, true, false, true);        // every graph a single vertex
    run_case(9, 4, 5, -1, false, true, true);        // no edges at all: edge fields of no rows
    run_case(40, 7, 6, 17, false, false, false);     // a 300-vertex / 700-column graph: many passes of a wave
    run_case(40, 40, 7, 0, false, false, false);
    run_case(300, 300, 8, -1, true, false, false);   // more than 256 slots
    run_case(131, 32, 9, 64, false, false, false);
    fit_and_big_offsets();
    if (failures) {
        std::fprintf(stderr, "padded harness: %d failures\n", failures);
        return 1;
    }
    std::printf("padded harness ok\n");
    return 0;
}
