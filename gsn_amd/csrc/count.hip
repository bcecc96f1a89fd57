// HP-1 counting kernel for gfx950 (MI355X) + its C-ABI launcher gsn_count_hip.
//
// One workgroup = one graph.  The graph lives in LDS for the whole kernel:
//   * adjacency bit matrix A[n][W] (W = ceil(n/64) 64-bit words per row), built from the edge_index columns with
//     LDS atomic-or (self loops dropped, parallel edges merged -> the simple undirected graph graph-tool matches on);
//     directed plans (main.py --directed, vertex mode): A holds the out-neighbour rows and a second matrix the in-neighbour rows,
//   * edge mode: the column endpoints (u8), a CSR rank  slot(u,v) = rowstart[u] + popcount(A[u] & below(v))  and
//     last[slot] = highest column holding (u,v)  ("last duplicate wins", utils_graph_processing.py:142-144),
//   * the packed plan table, a lane-interleaved candidate stack, and (if it fits) a staging copy of the output rows.
// Work is a pool of tasks (output column, output row); lanes pull tasks with a wave-aggregated LDS atomic
// (ballot + mbcnt prefix) so that lanes whose search finished early are refilled immediately -- rooted searches have
// wildly different lengths.  Every (row, column) cell is produced by exactly one lane: no atomics on the counts, no
// global atomics, deterministic.  Edge mode with undirected orbit classes: rows (u,v) and (v,u) are equal, the u < v row
// searches and writes both.  HBM traffic = read edge_index once (16 B/column) + write the int64 rows once.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "count_core.h"
#include "count_plan.h"

namespace gsn {

// The side arguments are read from the kernel-argument segment where they are used (scalar loads through a laundered pointer), not held in
// scalar registers from the kernel's entry: the molecule instantiation runs at its register bound (amdgpu_waves_per_eu).
typedef const SideArgs __attribute__((address_space(4))) *side_ptr_t;
__device__ __forceinline__ side_ptr_t side_late() {
    typedef const unsigned char __attribute__((address_space(4))) *kptr_t;
    kptr_t k = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return (side_ptr_t)(k + offsetof(CountArgs, side));
}
// The same for the whole argument block: the cycle instantiation's body reads every field where it uses it (a scalar load from the
// kernel-argument segment) -- held from the kernel's entry, the ~110 argument words were most of its scalar spills.
typedef const CountArgs __attribute__((address_space(4))) *args_ptr_t;
__device__ __forceinline__ args_ptr_t args_late() {
    typedef const unsigned char __attribute__((address_space(4))) *kptr_t;
    kptr_t k = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return (args_ptr_t)k;
}
__device__ __forceinline__ int side_byte(const unsigned w0, const unsigned w1, const int c) { return (int)(((c < 4 ? w0 : w1) >> (8 * (c & 3))) & 0xffu); }

// One side workgroup: the graphs g_lo .. g_hi - 1 (those of the SIDE_EVERY counting workgroups dispatched right in front of it), taken in
// chunks of consecutive graphs that fit the launch's LDS together.  A chunk is a disjoint union -- consecutive vertex ids, consecutive
// columns, no column between two graphs -- so ONE stable counting sort by target sorts all its graphs (what csr_graphs_kernel does per
// graph in a launch of its own; GSN_sparse.py:140-143).  Per chunk: (A) every global load -- targets, sources, vertex codes, edge codes --
// in batches of four per lane, results into LDS; (B) histogram, scan, placement, order restore in LDS; (C) every global store: seg_ptr,
// perm / sorted targets / sorted sources, the node pack rows (four lanes per 64-byte row; what gsn_one_hot_pack16_hip writes,
// utils_graph_learning.py:170-187), the edge codes' columns of the edge pack.  Loads and stores are kept apart because gfx9 counts them in one
// counter: a load issued behind a store waits for the store's acknowledgement too.  Statuses stay with the counting workgroups (they test every
// column's endpoints against their graph); a code outside its classes ORs 1 into *code_status.
// FL: the launch-uniform flags as a type (CycAny / CycKeys, in front of count_body).  With CycKeys the side outputs are the headline step's
// and nothing else: CSR with sorted targets and sources, ONE node code column as key bytes, ONE edge code column in the key words, global
// vertex ids, no row pack -- the arms of every other form are not compiled in (count_plan.cpp: choose_kernel sends every other launch to CycAny).
struct CycAny { static constexpr bool KEYS = false; };
struct CycKeys { static constexpr bool KEYS = true; };
template <int T, class FL = CycAny>
__device__ __forceinline__ void side_block(const CountArgs &a, unsigned char *smem, const int g_lo, const int g_hi) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    constexpr bool KEYS = FL::KEYS;
    const side_ptr_t sd = side_late();
    const int tid = threadIdx.x;
    const bool do_csr = KEYS || (a.side_mask & 1) != 0, do_np = KEYS || (a.side_mask & 2) != 0, do_ec = KEYS || (a.side_mask & 4) != 0;
    const bool ids_global = KEYS || a.ids_are_global != 0;
    // the code status is this launch's.  The first side workgroup clears it -- an atomic, so that the clear and the ORs below meet
    // at the same place whichever XCD issues them -- as its first memory operation.  ASSUMPTION, by timing and not by a dependency: no other
    // workgroup ORs before that clear lands.  An OR comes behind the workgroup's pointer reads and the loads of its codes (part (C): also
    // behind three barriers and the sort; the plain loops of a graph that does not fit LDS: behind the code load alone), and workgroups are
    // handed out in grid order, round-robin over the XCDs, and the first side workgroup is the fifth of the grid.  The
    // alternative that needs no assumption, a memset on the stream in front of the launch, is one more node in the captured step.
    if (g_lo == 0 && tid == 0 && sd->code_status) atomicExch(sd->code_status, 0);
    const int64_t *trow = sd->csr_row ? a.dst : a.src, *orow = sd->csr_row ? a.src : a.dst;
    auto need = [&](int64_t n, int64_t E) { return (n + 1) * 8 + n * 4 + E * 7 + 16; };
    if (do_csr) {
        // the ends of seg_ptr: vertices in front of the first graph (none in a collated batch) and the closing entries behind the last
        if (g_lo == 0) for (int64_t v = tid; v < a.node_ptr[0]; v += T) sd->csr_seg[v] = 0;
        if (g_hi == a.n_graphs) for (int64_t v = a.node_ptr[g_hi] + tid; v <= sd->tot_nodes; v += T) sd->csr_seg[v] = (int32_t)sd->tot_edges;
    }
    int g = g_lo;
    while (g < g_hi) {
        const int64_t n0 = a.node_ptr[g], e0 = a.edge_ptr[g];
        int g2 = g + 1;
        int64_t n64 = a.node_ptr[g2] - n0, E64 = a.edge_ptr[g2] - e0;
        const bool fits = n64 >= 0 && E64 >= 0 && n64 < 65535 && E64 < 65535 && need(n64, E64) <= a.lds_bytes;
        if (fits && ids_global)
            while (g2 < g_hi) {                          // (graph-local ids: one graph per chunk -- the offset of a column depends on its graph)
                const int64_t n2 = a.node_ptr[g2 + 1] - n0, E2 = a.edge_ptr[g2 + 1] - e0;
                if (n2 < n64 || E2 < E64 || n2 >= 65535 || E2 >= 65535 || need(n2, E2) > a.lds_bytes) break;
                n64 = n2; E64 = E2; ++g2;
            }
        g = g2;
        if (!fits) {
            // a graph beyond what the launch's LDS sorts (the counting workgroup reports it: GSN_ST_TOO_LARGE): its vertices own no columns, its
            // columns map to themselves (as csr_graphs_kernel); its rows of the packs are encoded by the plain loops
            if (n64 < 0 || E64 < 0) continue;
            if (do_csr) {
                for (int64_t v = tid; v < n64; v += T) sd->csr_seg[n0 + v] = (int32_t)e0;
                for (int64_t e = tid; e < E64; e += T) {
                    sd->csr_perm[e0 + e] = (int32_t)(e0 + e);
                    if (sd->csr_tgt) sd->csr_tgt[e0 + e] = (int32_t)n0;
                    if (sd->csr_oth) sd->csr_oth[e0 + e] = (int32_t)n0;
                }
            }
            // the compact outputs of such a graph, by the plain loops as well: every column names the graph's first vertex at both ends
            auto key_of = [&](int64_t v) {
                const unsigned w0 = sd->ncode_ptr_w[0], w1 = sd->ncode_ptr_w[1];
                unsigned key = 0;
                for (int c = 0; c < sd->ncode_cols; ++c) {
                    int64_t x = sd->ncode[v * sd->ncode_cols + c];
                    const int ncls = side_byte(w0, w1, c + 1) - side_byte(w0, w1, c);
                    if (sd->ncode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                    key = key * ((sd->nkey_radix_w >> (8 * c)) & 0xffu) + ((x >= 0 && x < ncls) ? (unsigned)x : (unsigned)ncls);
                }
                return key;
            };
            if (do_np && sd->nkey) for (int64_t v = tid; v < n64; v += T) sd->nkey[n0 + v] = (uint8_t)key_of(n0 + v);
            if (do_csr && sd->ekeys && n64 > 0) {
                const unsigned w0 = sd->ecode_ptr_w[0], w1 = sd->ecode_ptr_w[1];
                const unsigned k0 = do_np ? key_of(n0) : 0u;
                for (int64_t r = tid; r < E64; r += T) {
                    unsigned hot = 0;
                    for (int c = 0; do_ec && c < sd->ecode_cols; ++c) {
                        int64_t x = sd->ecode[(e0 + r) * sd->ecode_cols + c];
                        const int lo = side_byte(w0, w1, c), ncls = side_byte(w0, w1, c + 1) - lo;
                        if (sd->ecode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                        if (x >= 0 && x < ncls) hot |= 1u << (lo - sd->ecode_col0 + (int)x);
                        else if (sd->code_status && !sd->epack) atomicOr(sd->code_status, 1);
                    }
                    sd->ekeys[e0 + r] = k0 | (k0 << 8) | (hot << 16);
                }
            }
            if (do_np) {
                const unsigned w0 = sd->ncode_ptr_w[0], w1 = sd->ncode_ptr_w[1];
                for (int64_t i = tid; i < 4 * n64; i += T) {
                    if (!sd->npack && (i & 3)) continue;     // (no pack: the pass only raises the code status)
                    const int64_t v = i >> 2;
                    const int q = (int)(i & 3);
                    unsigned m = 0x80000000u;
                    for (int c = 0; c < sd->ncode_cols; ++c) {
                        int64_t x = sd->ncode[(n0 + v) * sd->ncode_cols + c];
                        const int lo = side_byte(w0, w1, c), ncls = side_byte(w0, w1, c + 1) - lo;
                        if (sd->ncode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                        if (x >= 0 && x < ncls) m |= 1u << (lo + (int)x);
                        else if (sd->code_status && q == 0) atomicOr(sd->code_status, 1);
                    }
                    const unsigned hot = m >> (8 * q);
                    auto word = [&](int kk) { return ((hot >> kk) & 1u ? 0x3c00u : 0u) | ((hot >> (kk + 1)) & 1u ? 0x3c000000u : 0u); };
                    if (sd->npack) *reinterpret_cast<u4v *>(sd->npack + (n0 + v) * 32 + 8 * q) = u4v{word(0), word(2), word(4), word(6)};
                }
            }
            if (do_ec && sd->epack) {
                const unsigned w0 = sd->ecode_ptr_w[0], w1 = sd->ecode_ptr_w[1];
                const int q0 = sd->ecode_col0 >> 2;
                for (int64_t i = tid; i < E64 * (4 - q0); i += T) {
                    const int64_t r = i / (4 - q0);
                    const int q = q0 + (int)(i - r * (4 - q0));
                    unsigned hot = 0;
                    for (int c = 0; c < sd->ecode_cols; ++c) {
                        int64_t x = sd->ecode[(e0 + r) * sd->ecode_cols + c];
                        const int lo = side_byte(w0, w1, c), ncls = side_byte(w0, w1, c + 1) - lo;
                        if (sd->ecode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                        if (x >= 0 && x < ncls) hot |= 1u << (lo + (int)x);
                        else if (sd->code_status && q == q0) atomicOr(sd->code_status, 1);
                    }
                    hot >>= 4 * q;
                    uint2 o;
                    o.x = ((hot & 1u) ? 0x3c00u : 0u) | ((hot & 2u) ? 0x3c000000u : 0u);
                    o.y = ((hot & 4u) ? 0x3c00u : 0u) | ((hot & 8u) ? 0x3c000000u : 0u);
                    *reinterpret_cast<uint2 *>(sd->epack + (e0 + r) * 16 + 4 * q) = o;
                }
            }
            continue;
        }
        const int n = (int)n64, E = (int)E64;
        int *cstart = reinterpret_cast<int *>(smem);
        int *ccur = cstart + (n + 1);
        unsigned *nmask = reinterpret_cast<unsigned *>(ccur + (n + 1));   // hot pack columns of the vertex as a bit mask; with SideArgs::nkey its dictionary row instead
        uint16_t *tloc = reinterpret_cast<uint16_t *>(nmask + n);
        uint16_t *oloc = tloc + E;
        uint16_t *pl = oloc + E;
        unsigned char *ecls = reinterpret_cast<unsigned char *>(pl + E);      // bit mask of the edge codes' classes over pack columns ecode_col0 .. +7
        __syncthreads();                                 // (the chunk before this one has left LDS)
        for (int v = tid; v <= n; v += T) cstart[v] = 0;
        __syncthreads();
        // ---- (A) loads: four per lane in flight --------------------------------------------------------------------------
        const int64_t off = ids_global ? n0 : 0;         // (graph-local ids: the chunk is one graph)
        bool bad_code = false;
        if (do_csr)
            for (int c0 = 0; c0 < E; c0 += 4 * T) {
                int64_t tq[4], oq[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int c = c0 + j * T + tid; tq[j] = c < E ? trow[e0 + c] : off; oq[j] = c < E ? orow[e0 + c] : off; }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + j * T + tid;
                    if (c < E) {
                        uint32_t td, od;                 // (a column that leaves its graph: the counting workgroup reports it)
                        const int tl = endpoint_local(tq[j], off, (uint32_t)n, td) ? (int)td : 0, ol = endpoint_local(oq[j], off, (uint32_t)n, od) ? (int)od : 0;
                        tloc[c] = (uint16_t)tl; oloc[c] = (uint16_t)ol;
                        atomicAdd(&cstart[tl], 1);
                    }
                }
            }
        if (do_np) {
            const unsigned w0 = sd->ncode_ptr_w[0], w1 = sd->ncode_ptr_w[1];
            const int nc = KEYS ? 1 : sd->ncode_cols;
            const bool as_key = KEYS || sd->nkey != nullptr;
            for (int v0 = 0; v0 < n; v0 += 4 * T) {
                if (nc == 1) {
                    int64_t xq[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const int v = v0 + j * T + tid; xq[j] = v < n ? sd->ncode[n0 + v] : 0; }
                    const int ncls = side_byte(w0, w1, 1);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int v = v0 + j * T + tid;
                        int64_t x = xq[j];
                        if (sd->ncode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                        const bool ok = x >= 0 && x < ncls;
                        if (v < n) { nmask[v] = as_key ? (unsigned)(ok ? (int)x : ncls) : 0x80000000u | (ok ? 1u << (int)x : 0u); bad_code = bad_code || !ok; }
                    }
                } else {
                    for (int j = 0; j < 4; ++j) {
                        const int v = v0 + j * T + tid;
                        if (v >= n) break;
                        unsigned m = 0x80000000u, key = 0;
                        for (int c = 0; c < nc; ++c) {
                            int64_t x = sd->ncode[(n0 + v) * nc + c];
                            const int lo = side_byte(w0, w1, c), ncls = side_byte(w0, w1, c + 1) - lo;
                            if (sd->ncode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                            const bool ok = x >= 0 && x < ncls;
                            if (ok) m |= 1u << (lo + (int)x); else bad_code = true;
                            key = key * ((sd->nkey_radix_w >> (8 * c)) & 0xffu) + (ok ? (unsigned)x : (unsigned)ncls);
                        }
                        nmask[v] = as_key ? key : m;
                    }
                }
            }
        }
        if (do_ec) {
            const unsigned w0 = sd->ecode_ptr_w[0], w1 = sd->ecode_ptr_w[1];
            const int nc = KEYS ? 1 : sd->ecode_cols, c00 = sd->ecode_col0;
            for (int r0 = 0; r0 < E; r0 += 4 * T) {
                if (nc == 1) {
                    int64_t xq[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const int r = r0 + j * T + tid; xq[j] = r < E ? sd->ecode[e0 + r] : 0; }
                    const int ncls = side_byte(w0, w1, 1) - c00;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = r0 + j * T + tid;
                        int64_t x = xq[j];
                        if (sd->ecode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                        const bool ok = x >= 0 && x < ncls;
                        if (r < E) { ecls[r] = ok ? (unsigned char)(1u << (int)x) : (unsigned char)0; bad_code = bad_code || !ok; }
                    }
                } else {
                    for (int j = 0; j < 4; ++j) {
                        const int r = r0 + j * T + tid;
                        if (r >= E) break;
                        unsigned m = 0;
                        for (int c = 0; c < nc; ++c) {
                            int64_t x = sd->ecode[(e0 + r) * nc + c];
                            const int lo = side_byte(w0, w1, c) - c00, ncls = side_byte(w0, w1, c + 1) - c00 - lo;
                            if (sd->ecode_clamp) x = x < 0 ? 0 : (x >= ncls ? ncls - 1 : x);
                            if (x >= 0 && x < ncls) m |= 1u << (lo + (int)x); else bad_code = true;
                        }
                        ecls[r] = (unsigned char)m;
                    }
                }
            }
        }
        __syncthreads();
        // ---- (B) the sort, in LDS ----------------------------------------------------------------------------------------
        if (do_csr) {
            if (tid < 64) {                              // exclusive scan of the n + 1 counters, 64 at a time (start[n] becomes E)
                int carry = 0;
                for (int base = 0; base <= n; base += 64) {
                    const int v = base + tid;
                    const int cnt = v <= n ? cstart[v] : 0;
                    int incl = cnt;
                    if constexpr (KEYS && T == 64) {     // (one wave, every lane active: the six DPP adds of count_body's phase 2)
                        incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);      // row_shr:1
                        incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);      // row_shr:2
                        incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);      // row_shr:4
                        incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);      // row_shr:8
                        incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
                        incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
                    } else {
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int t = __shfl_up(incl, o);
                        if (tid >= o) incl += t;
                    }
                    }
                    const int ex = carry + incl - cnt;
                    if (v <= n) { cstart[v] = ex; ccur[v] = ex; }
                    if constexpr (KEYS && T == 64) carry += __builtin_amdgcn_readlane(incl, 63);
                    else carry += __shfl(incl, 63);
                }
            }
            __syncthreads();
            for (int c = tid; c < E; c += T) pl[atomicAdd(&ccur[tloc[c]], 1)] = (uint16_t)c;
            __syncthreads();
            for (int v = tid; v < n; v += T) {          // column order inside every segment (the cursor hands out slots in arbitrary order)
                const int lo = cstart[v], hi = cstart[v + 1];
                for (int i = lo + 1; i < hi; ++i) {
                    const uint16_t x = pl[i];
                    int j = i - 1;
                    while (j >= lo && pl[j] > x) { pl[j + 1] = pl[j]; --j; }
                    pl[j + 1] = x;
                }
            }
            __syncthreads();
        }
        // ---- (C) stores --------------------------------------------------------------------------------------------------
        if (bad_code && sd->code_status) atomicOr(sd->code_status, 1);
        if (do_csr) {
            for (int v = tid; v < n; v += T) sd->csr_seg[n0 + v] = (int32_t)(e0 + cstart[v]);
            for (int i = tid; i < E; i += T) {
                const int le = pl[i];
                const int tl = tloc[le], ol = oloc[le];  // (read once: the sorted endpoints and the key word share them)
                sd->csr_perm[e0 + i] = (int32_t)(e0 + le);
                if (KEYS || sd->csr_tgt) sd->csr_tgt[e0 + i] = (int32_t)(n0 + tl);
                if (KEYS || sd->csr_oth) sd->csr_oth[e0 + i] = (int32_t)(n0 + ol);
                if (KEYS || sd->ekeys)
                    sd->ekeys[e0 + i] = (do_np ? nmask[tl] | (nmask[ol] << 8) : 0u) | (do_ec ? (unsigned)ecls[le] << 16 : 0u);
            }
        }
        if (do_np && (KEYS || sd->nkey)) for (int v = tid; v < n; v += T) sd->nkey[n0 + v] = (uint8_t)nmask[v];
        if (!KEYS && do_np && sd->npack)
            for (int i = tid; i < 4 * n; i += T) {
                const int v = i >> 2, q = i & 3;
                const unsigned hot = nmask[v] >> (8 * q);
                auto word = [&](int kk) { return ((hot >> kk) & 1u ? 0x3c00u : 0u) | ((hot >> (kk + 1)) & 1u ? 0x3c000000u : 0u); };
                *reinterpret_cast<u4v *>(sd->npack + (n0 + v) * 32 + 8 * q) = u4v{word(0), word(2), word(4), word(6)};
            }
        if (!KEYS && do_ec && sd->epack) {
            const int q0 = sd->ecode_col0 >> 2, nq = 4 - q0;      // the 4-column groups from ecode_col0 to the end of the row
            for (int i = tid; i < E * nq; i += T) {
                const int r = nq == 1 ? i : i / nq;
                const int qq = i - r * nq;
                const unsigned hot = (unsigned)ecls[r] >> (4 * qq);
                uint2 o;
                o.x = ((hot & 1u) ? 0x3c00u : 0u) | ((hot & 2u) ? 0x3c000000u : 0u);
                o.y = ((hot & 4u) ? 0x3c00u : 0u) | ((hot & 8u) ? 0x3c000000u : 0u);
                *reinterpret_cast<uint2 *>(sd->epack + (e0 + r) * 16 + 4 * (q0 + qq)) = o;
            }
        }
    }
}

// diagnostic build (-DCOUNT_PROF, scripts/rr_variant.sh with RR_VARIANT_SRC=count): cycles of thread 0 per phase, summed over the workgroups;
// with -DCOUNT_PROF_STEP as well: the arms inside lane_step (count_core.h: Lane::prof -- 24 more registers per lane: for the large-graph
// instantiations, it distorts the molecule ones)
#ifdef COUNT_PROF
__device__ unsigned long long *g_count_prof;   // [items][8], set by the launcher
__device__ unsigned long long *g_count_prof2;  // [12] wave-level sums over the launch: the arms inside lane_step (count_core.h: Lane::prof)
#define COUNT_T(I) do { __syncthreads(); if (threadIdx.x == 0 && g_count_prof) { const unsigned long long t_now = __builtin_amdgcn_s_memtime(); g_count_prof[(size_t)blockIdx.x * 16 + (I)] = t_now - t_prev; t_prev = t_now; } } while (0)
#else
#define COUNT_T(I)
#endif

// One pass of a workgroup over `ng` consecutive graphs g .. g + ng - 1 taken as ONE graph, their disjoint union (ng = 2 only for plans
// whose patterns are connected: an image of a connected pattern lies inside one component, so every rooted count of the union is the
// count in the root's own graph; vertex ids of the second graph follow the first's, rows and columns are contiguous in the batch
// anyway).  Two ZINC-sized graphs fill the 64 lanes of the wave that had one before: the set-up phases (adjacency, cores, distance
// tables, edge ranks: latency of dependent LDS round trips, half of a workgroup's life) are paid once per pair, and the task pool
// keeps 64 lanes busy twice as long.  report = false (a pair): nothing is reported, a pair that does not fit or holds an error
// returns 1 and the caller redoes its graphs one by one.
// MOL: the launch's invariants of the molecule datasets' identifier pass as compile-time constants -- edge mode with undirected orbit
// classes (symmetric rows), four output columns, one workgroup per pair of graphs (no split), encoded rows staged as class
// indices -- instead of ~12 launch arguments that are tested in every arm of the pool and held in scalar registers
// through the whole kernel (106 of them + spills before).  The planner selects it when all of that holds (count_plan.cpp: count_molecule_route).
// CYC = L > 0 (with MOL): every column is a non-induced cycle of length <= L -- no plan table, candidate stack or distance tables in LDS,
// and the task pool is one bitset path walk per searching row (count_core.h: cycle_walk) that yields the row's four cells at once.
// FL (CYC only): the flags that are the same for every workgroup of a launch, as a type.  CycAny tests them where they are used (scalar
// loads and branches in every workgroup); CycKeys is the headline step's combination (gsn_count_encode_keys_side_hip on staged rows),
// selected by the launcher when all of it holds: int64 rows staged in LDS as 16-bit counts, class indices taken from those counts, the
// identifier masks the only encoded form (no fp32 rows, no fp16 pack), global vertex ids, a grid with side workgroups, status words zeroed
// by their own workgroups.  Same body, the other arms are not compiled in.  (The types stand in front of side_block, which takes them too.)
template <int W, int T, bool DIR, bool TAIL, bool MOL, int CYC = 0, class FL = CycAny, class Args = CountArgs>
__device__ __forceinline__ int count_body(const Args &a, unsigned char *smem, const int item, const int part, const int g, const int ng, const bool report) {
    constexpr bool KEYS = CYC > 0 && FL::KEYS;
#ifdef COUNT_PROF
    unsigned long long t_prev = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();                                    // (a pass before this one has finished with LDS)
    uint64_t *A = reinterpret_cast<uint64_t *>(smem);
    uint64_t *valid = reinterpret_cast<uint64_t *>(smem + a.off_valid);
    uint64_t *stack = reinterpret_cast<uint64_t *>(smem + a.off_stack) - (size_t)a.stack_skip * W * T;   // (frame l at stack + l W T: see the launcher)
    uint32_t *plan = reinterpret_cast<uint32_t *>(smem + a.off_plan);
    typedef typename std::conditional<(W <= 4), uint8_t, uint16_t>::type vid_t;   // column endpoints
    vid_t *eu = reinterpret_cast<vid_t *>(smem + a.off_eu);
    vid_t *ev = reinterpret_cast<vid_t *>(smem + a.off_ev);
    // (prefix sums of the distinct-neighbour degrees: one-word graphs -- at most 64 x 63 pairs -- keep them as 16-bit values: 128 bytes of
    //  a molecule pair's 6.9 KiB, the difference between 23 and 24 workgroups per CU)
    typedef typename std::conditional<(W == 1), uint16_t, int>::type rs_t;
    rs_t *rowstart = reinterpret_cast<rs_t *>(smem + a.off_rowstart);
    int *last = reinterpret_cast<int *>(smem + a.off_last);
    // (column tables as 16-bit values: a workgroup whose per-column state fits LDS has far fewer than 65535 columns; 0xffff = none)
    uint16_t *prim = reinterpret_cast<uint16_t *>(smem + a.off_prim);
    uint16_t *revof = reinterpret_cast<uint16_t *>(smem + a.off_revof);
    uint16_t *out_lds = reinterpret_cast<uint16_t *>(smem + a.off_out);   // staged counts as 16-bit values; 0xffff = this cell went to HBM by itself
    int *misc = reinterpret_cast<int *>(smem + a.off_misc);  // [0] next task  [1] n_active  [2] status
    uint64_t *balls = (!CYC && a.off_ball >= 0) ? reinterpret_cast<uint64_t *>(smem + a.off_ball) : nullptr;
    uint64_t *cores = reinterpret_cast<uint64_t *>(smem + a.off_core);   // [CORE_MAX + 1][W]
    uint64_t *degp = (TAIL && a.off_degp >= 0) ? reinterpret_cast<uint64_t *>(smem + a.off_degp) : nullptr;     // (TAIL = false: none of this exists)
    uint64_t *A_in = DIR ? reinterpret_cast<uint64_t *>(smem + a.off_ain) : nullptr;
    const int *enc = reinterpret_cast<const int *>(smem + a.off_enc);   // [2 * n_cols] (encoded output only)

    int tid_v = threadIdx.x;
    // (CYC: the lane id is opaque per pass, so that 64-bit lane offsets of the output loops are made where they are used and not held
    //  -- hoisted out of the kernel's pass loop -- across the whole body: the last two registers above the bound)
    if constexpr (CYC > 0) asm volatile("" : "+v"(tid_v));
    const int tid = tid_v;
    (void)item;
    const int64_t n0 = a.node_ptr[g], e0 = a.edge_ptr[g];
    const int64_t n64 = a.node_ptr[g + ng] - n0, E64 = a.edge_ptr[g + ng] - e0;
    const int64_t nA64 = a.node_ptr[g + 1] - n0, EA64 = a.edge_ptr[g + 1] - e0;      // the first graph's share (ng = 1: everything)
    const bool edge_mode = MOL || a.mode == GSN_MODE_EDGE;
    const int64_t rows64 = edge_mode ? E64 : n64;
    const int64_t row0 = edge_mode ? e0 : n0;
    const int n_cols = MOL ? 4 : a.n_cols;
    const bool a_stage_out = KEYS || a.stage_out != 0, a_sym = MOL || a.sym != 0, a_enc = MOL || a.enc_out != nullptr, a_enc_stage = MOL || a.enc_stage != 0;
    const bool a_enc_from_counts = KEYS || a.enc_from_counts != 0;
    const int a_split = MOL ? 1 : a.split;

    // CYC: the zeros of an error path (a graph beyond the declared sizes, a bad index), a row per thread and trip: the same bytes as the
    // flat loops of the other instantiations without their 64-bit quotients, whose expansion was this instantiation's register peak
    auto zero_rows_cyc = [&](const int64_t nrows, const bool pack_always) {
        if constexpr (KEYS) {                           // (the int64 rows and the masks are all there is)
            (void)pack_always;
            for (int64_t r = tid; r < nrows; r += T) {
                for (int c = 0; c < 4; ++c) a.out[(row0 + r) * 4 + c] = 0;
                a.idmask[row0 + r] = 0;
            }
            return;
        }
        const bool z32 = a.enc_out && !a.enc_no32, z16 = a.enc16 && (pack_always || a.enc_no32);
        for (int64_t r = tid; r < nrows; r += T) {
            if (a.out) for (int c = 0; c < 4; ++c) a.out[(row0 + r) * 4 + c] = 0;
            if (z32) for (int k = 0; k < a.enc_width; ++k) a.enc_out[(row0 + r) * a.enc_width + k] = 0.f;
            if (z16) for (int k = 0; k < a.enc_width; ++k) a.enc16[(row0 + r) * a.enc16_stride + a.enc16_col0 + k] = 0;
            if (!DIR && args_late()->idmask) args_late()->idmask[row0 + r] = 0;
        }
    };
    if (ng > 1 && (n64 > a.n_cap || E64 > a.e_cap || n64 > W * 64)) return 1;
    if (ng == 1 && (n64 > a.n_decl || E64 > a.e_decl || n64 > W * 64)) {
        // caller under-declared max_nodes / max_edges: report, leave zeros
        if (part == 0) {
            if constexpr (CYC > 0) zero_rows_cyc(rows64, true);
            else {
            if (a.out) for (int64_t i = tid; i < rows64 * n_cols; i += T) a.out[row0 * n_cols + i] = 0;
            if (a.enc_out && !a.enc_no32) for (int64_t i = tid; i < rows64 * a.enc_width; i += T) a.enc_out[row0 * a.enc_width + i] = 0.f;
            if (a.enc16) for (int64_t i = tid; i < rows64 * a.enc_width; i += T) a.enc16[(row0 + i / a.enc_width) * a.enc16_stride + a.enc16_col0 + i % a.enc_width] = 0;
            if (!DIR && args_late()->idmask) for (int64_t i = tid; i < rows64; i += T) args_late()->idmask[row0 + i] = 0;
            }
            if (tid == 0) atomicMax(&a.status[g], (int)GSN_ST_TOO_LARGE);
        }
        return 0;
    }
    const int n = (int)n64, E = (int)E64, rows = (int)rows64;
    const int nA = (int)nA64, EA = (int)EA64;

    // one finished cell (row, column) = cnt: the int64 row (staged or direct), the staged class index or the encoded floats
    auto emit_cell = [&](int row, int col, uint64_t cnt) {
        if (a_stage_out) {
            // two bytes per staged cell (eight cost a ZINC pair 5.6 KiB: more than its LDS budget, so every cell went to HBM by itself from
            // inside the pool -- 12.5 M scattered 8-byte stores per 65 536 molecules); the rare count that does not fit goes out directly
            if (cnt < 0xffffull) out_lds[row * n_cols + col] = (uint16_t)cnt;
            else { out_lds[row * n_cols + col] = (uint16_t)0xffff; a.out[(row0 + row) * n_cols + col] = (int64_t)cnt; }
        }
        else if (a.out) a.out[(row0 + row) * n_cols + col] = (int64_t)cnt;
        if (a_enc) {
            const int *enc_t = reinterpret_cast<const int *>(smem + a.off_enc);
            const int eo = enc_t[2 * col], ncls = enc_t[2 * col + 1];
            uint64_t v = cnt;
            if (a.enc_clamp && v >= (uint64_t)ncls) v = (uint64_t)(ncls - 1);
            if (a_enc_stage) {
                if (!a_enc_from_counts) (smem + a.off_encst)[row * n_cols + col] = v < (uint64_t)ncls ? (unsigned char)v : (unsigned char)0xff;
            } else {
                float *d0 = a.enc_out + (row0 + row) * a.enc_width + eo;
                for (int j = 0; j < ncls; ++j) d0[j] = (uint64_t)j == v ? 1.f : 0.f;
            }
        }
    };

    // CYC: the four cells of one row at once -- the staged 16-bit counts as ONE 8-byte LDS store, the class bytes (only without staged
    // counts) as one word.  The path is the molecule one (staged cells, staged class indices, no direct float rows), so none of emit_cell's
    // other arms exist here; the class counts are read from the kernel arguments, wave-uniform, not from the LDS table.  32-bit counts (count_core.h:
    // CycleAcc) are widened at the int64 store only.
    auto emit_row = [&](const int row, const uint32_t c0, const uint32_t c1, const uint32_t c2, const uint32_t c3) {
        if (a_stage_out) {
            auto lo16 = [](const uint32_t c) { return c < 0xffffu ? c : 0xffffu; };
            *reinterpret_cast<uint2 *>(out_lds + 4 * row) = uint2{lo16(c0) | (lo16(c1) << 16), lo16(c2) | (lo16(c3) << 16)};
            if (((c0 | c1 | c2 | c3) >> 16) || c0 == 0xffffu || c1 == 0xffffu || c2 == 0xffffu || c3 == 0xffffu) {      // (rare: a count that does not fit goes out directly)
                int64_t *d = a.out + (row0 + row) * 4;
                if (c0 >= 0xffffu) d[0] = (int64_t)c0;
                if (c1 >= 0xffffu) d[1] = (int64_t)c1;
                if (c2 >= 0xffffu) d[2] = (int64_t)c2;
                if (c3 >= 0xffffu) d[3] = (int64_t)c3;
            }
        } else if (a.out) {
            int64_t *d = a.out + (row0 + row) * 4;
            d[0] = (int64_t)c0; d[1] = (int64_t)c1; d[2] = (int64_t)c2; d[3] = (int64_t)c3;
        }
        if (!a_enc_from_counts) {
            const bool clamp = a.enc_clamp != 0;
            auto cls = [&](const uint32_t c, const uint32_t ncls) { return c < ncls ? c : (clamp ? ncls - 1u : 0xffu); };
            *reinterpret_cast<uint32_t *>(smem + a.off_encst + 4 * row) =
                cls(c0, a.enc_n[0]) | (cls(c1, a.enc_n[1]) << 8) | (cls(c2, a.enc_n[2]) << 16) | (cls(c3, a.enc_n[3]) << 24);
        }
    };

    // ---- phase 0: clear LDS state, copy the plan table ------------------------------------------------------------
    typedef unsigned lds16_t __attribute__((ext_vector_type(4)));      // CYC: every cleared array starts and ends on 16 bytes (count_plan.cpp: lds_layout)
    if constexpr (CYC > 0) {
        for (int i = tid; i < (n + 1) / 2; i += T) reinterpret_cast<lds16_t *>(A)[i] = lds16_t{0u, 0u, 0u, 0u};
    } else
    for (int i = tid; i < n * W; i += T) A[i] = 0ull;
    if (DIR)
        for (int i = tid; i < n * W; i += T) A_in[i] = 0ull;
    if (!CYC)
        for (int i = tid; i < a.plan_words; i += T) plan[i] = a.plan[i];
    if constexpr (CYC > 0) {                            // (the same table from four wave-uniform reads: no per-lane index into the arguments)
        const int e0 = a.enc_n[0], e1 = a.enc_n[1], e2 = a.enc_n[2], e3 = a.enc_n[3];
        if (tid < 4) {
            reinterpret_cast<int *>(smem + a.off_enc)[2 * tid] = (tid > 0 ? e0 : 0) + (tid > 1 ? e1 : 0) + (tid > 2 ? e2 : 0);
            reinterpret_cast<int *>(smem + a.off_enc)[2 * tid + 1] = tid == 0 ? e0 : (tid == 1 ? e1 : (tid == 2 ? e2 : e3));
        }
    } else
    if (a_enc)                                          // (first float, n_classes) per column
        for (int c = tid; c < n_cols; c += T) {
            int o = 0;
            for (int x = 0; x < c; ++x) o += a.enc_n[x];
            reinterpret_cast<int *>(smem + a.off_enc)[2 * c] = o;
            reinterpret_cast<int *>(smem + a.off_enc)[2 * c + 1] = a.enc_n[c];
        }
    if constexpr (CYC > 0) {
        if (tid < 2) reinterpret_cast<lds16_t *>(misc)[tid] = lds16_t{0u, 0u, 0u, 0u};
    } else
    if (tid < 8) misc[tid] = 0;
    // staged outputs start at zero: rows that carry nothing (self loops, earlier duplicates) and rows whose roots lie outside every plan's core
    // then need no cell-by-cell zeros from the one wave that ranks the columns (8 LDS stores per such row: 7 k of a molecule pair's 60 k cycles)
    const bool bulk_zero = edge_mode && a_stage_out && (!a_enc || a_enc_stage);
    if constexpr (CYC > 0) {                            // (two staged rows, or four rows' class bytes, per 16-byte store: one trip for a ZINC pair)
        if (bulk_zero) {
            for (int i = tid; i < (rows + 1) / 2; i += T) reinterpret_cast<lds16_t *>(out_lds)[i] = lds16_t{0u, 0u, 0u, 0u};
            if (!a_enc_from_counts)
                for (int i = tid; i < (rows + 3) / 4; i += T) reinterpret_cast<lds16_t *>(smem + a.off_encst)[i] = lds16_t{0u, 0u, 0u, 0u};
        }
    } else
    if (bulk_zero) {
        uint32_t *z = reinterpret_cast<uint32_t *>(out_lds);
        for (int i = tid; i < (rows * n_cols + 1) / 2; i += T) z[i] = 0u;
        if (a_enc && !a_enc_from_counts) {
            unsigned char *zb = smem + a.off_encst;
            for (int i = tid; i < rows * n_cols; i += T) zb[i] = 0;      // (count 0 = class 0)
        }
    }
    __syncthreads();

    COUNT_T(0);
    // ---- phase 1: adjacency bit matrix from the columns -----------------------------------------------------------
    // CYC (one wave): no LDS atomic per column for the flag and the vertex count.  A column with a bad index raises its lane's flag, read
    // with one ballot behind the loop; the vertex counts misc[1] / misc[5] are not kept at all: they bound the set of vertices that exist,
    // and this path reads that set only to start the 2-core, which lies inside the vertices with a neighbour whatever the largest id is.
    // Its endpoint loads: the graph's first column as a scalar base, the lane's column as a 32-bit byte offset.
    bool bad_lane = false;
    if constexpr (CYC > 0) {
        // CYC: an endpoint is tested against its graph's range by count_core.h's endpoint_local -- one 64-bit subtraction of the range's first
        // id (global ids: n0, n0 + nA for the second graph; graph-local ids: 0 for both), then 32-bit tests; its id inside the pair is the
        // difference plus the second graph's nA.
        const uint32_t wA = endpoint_width(0, nA), wB = endpoint_width(nA, n);
        const bool ids_global = KEYS || a.ids_are_global != 0;
        for (int c = tid; c < E; c += T) {
            const bool second = c >= EA;                // (a column of the pair's second graph: its vertices are nA .. n - 1)
            const uint32_t cb = (uint32_t)c * 8u;
            const int64_t ur = *reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(a.src + e0) + cb);
            const int64_t vr = *reinterpret_cast<const int64_t *>(reinterpret_cast<const char *>(a.dst + e0) + cb);
            const int64_t base = ids_global ? (second ? n0 + nA : n0) : 0;
            const uint32_t width = second ? wB : wA, first = second ? (uint32_t)nA : 0u;
            uint32_t ud, vd;
            const bool u_ok = endpoint_local(ur, base, width, ud), v_ok = endpoint_local(vr, base, width, vd);
            if (!(u_ok && v_ok)) { bad_lane = true; eu[c] = 0; ev[c] = 0; continue; }
            const int u = (int)(first + ud), v = (int)(first + vd);
            eu[c] = (vid_t)u; ev[c] = (vid_t)v;
            if (u != v) {
                atomicOr(reinterpret_cast<unsigned long long *>(&A[u]), 1ull << v);
                atomicOr(reinterpret_cast<unsigned long long *>(&A[v]), 1ull << u);
            }
        }
    } else
    for (int c = tid; c < E; c += T) {
        const bool second = c >= EA;                    // (a column of the pair's second graph: its vertices are nA .. n - 1)
        const int64_t off = a.ids_are_global ? n0 : (second ? -(int64_t)nA : 0);
        const int64_t u64 = a.src[e0 + c] - off, v64 = a.dst[e0 + c] - off;
        const int64_t lo = second ? nA : 0, hi = second ? n : nA;
        if (u64 < lo || v64 < lo || u64 >= hi || v64 >= hi) {
            atomicMax(&misc[2], (int)GSN_ST_BAD_INDEX);
            if (edge_mode) { eu[c] = 0; ev[c] = 0; }
            continue;
        }
        const int u = (int)u64, v = (int)v64;
        if (edge_mode) { eu[c] = (vid_t)u; ev[c] = (vid_t)v; }
        atomicMax(&misc[second ? 5 : 1], (u > v ? u : v) + 1);  // graph-tool creates vertices 0..max id, self-loop columns included
        if (u != v) {
            atomicOr(reinterpret_cast<unsigned long long *>(&A[u * W + (v >> 6)]), 1ull << (v & 63));
            atomicOr(reinterpret_cast<unsigned long long *>(&(DIR ? A_in : A)[v * W + (u >> 6)]), 1ull << (u & 63));
        }
    }
    __syncthreads();
    COUNT_T(1);
    uint64_t core2 = 0;                                  // CYC: the 2-core, the only core its plans name -- a wave-uniform register, never in LDS
    bool cyc_bad = false;                                // CYC: some column of the pass has an endpoint outside its graph
    if constexpr (CYC > 0) {
        cyc_bad = __ballot(bad_lane) != 0ull;
        const uint64_t arow = tid < n ? A[tid] : 0ull;
        uint64_t cur = __ballot(arow != 0ull);           // (the peeling may start from the vertices with a neighbour: no other vertex is in a 2-core)
        for (;;) {                                       // (the ballot peeling below, d = 2)
            const uint64_t nxt = __ballot(((cur >> tid) & 1ull) && popc64(arow & cur) >= 2);
            if (nxt == cur) break;
            cur = nxt;
        }
        core2 = cur;
    } else {
    // the vertices that exist: 0 .. largest id of the first graph, nA .. largest id of the second
    if (tid < W) valid[tid] = below_word(misc[1], tid) | (below_word(misc[5], tid) & ~below_word(nA, tid));
    // d-cores: every image of a pattern with minimum degree d lies in the d-core of the graph (its >= d pattern neighbours
    // are images too), so the plan's candidate universe is that core instead of all vertices -- on molecules the 2-core
    // (ring systems and what connects them) is a fraction of the graph and rooted searches from the rest end at once.
    __syncthreads();
    for (int d = 0; d <= CORE_MAX; ++d) {
        if (tid < W) cores[d * W + tid] = valid[tid];
    }
    __syncthreads();
    for (int d = 1; d <= CORE_MAX; ++d) {
        if (!((a.core_mask >> d) & 1)) continue;
        uint64_t *core = cores + d * W;
        if (W == 1 && T == 64) {                    // one wave, one vertex per lane: peel with ballots, no LDS round trips
            uint64_t cur = core[0];
            for (;;) {
                const bool in = (cur >> tid) & 1ull;
                const bool keep = in && tid < n && popc64(A[tid] & cur) >= d;
                const uint64_t nxt = __ballot(keep);
                if (nxt == cur) break;
                cur = nxt;
            }
            __syncthreads();
            if (tid == 0) core[0] = cur;
        } else {
            for (;;) {                               // Jacobi peeling: decide on a snapshot, then remove
                __syncthreads();
                if (tid == 0) misc[3] = 0;
                __syncthreads();
                uint32_t dropm = 0;                  // vertices tid + i*T, i < 12 (n <= 768, T >= 64)
                for (int v = tid, i = 0; v < n; v += T, ++i) {
                    const bool in = (core[v >> 6] >> (v & 63)) & 1ull;
                    if (in && !core_keeps<W>(A, core, v, d)) dropm |= 1u << i;
                }
                __syncthreads();
                for (int v = tid, i = 0; v < n; v += T, ++i)
                    if ((dropm >> i) & 1u) atomicAnd(reinterpret_cast<unsigned long long *>(&core[v >> 6]), ~(1ull << (v & 63)));
                if (dropm) misc[3] = 1;
                __syncthreads();
                if (misc[3] == 0) break;
            }
        }
    }
    __syncthreads();
    // degree bit planes of the cores that hold a chain-tail plan (count_core.h: tail_pairs, mode 3)
    if (TAIL && degp) {
        for (int i = tid; i < (CORE_MAX + 1) * DEG_PLANES * W; i += T) degp[i] = 0ull;
        __syncthreads();
        for (int d = 0; d <= CORE_MAX; ++d) {
            if (!((a.degp_mask >> d) & 1)) continue;
            for (int v = tid; v < n; v += T)
                deg_planes_vertex<W>(A, cores + d * W, v, degp + d * DEG_PLANES * W,
                                     [](uint64_t *wp, uint64_t bit) { atomicOr(reinterpret_cast<unsigned long long *>(wp), (unsigned long long)bit); });
        }
        __syncthreads();
    }
    }
    COUNT_T(2);
    // distance pruning tables: vertices within 2 / 3 hops (count_core.h, candidates())
    if (balls) {
        for (int v = tid; v < n; v += T) ball_expand<W>(A, nullptr, v, balls);
        __syncthreads();
        for (int v = tid; v < n; v += T) ball_expand<W>(A, balls, v, balls + a.n_cap * W);
    }

    COUNT_T(3);
    // ---- phase 2 (edge mode): CSR rank of every directed pair, last-duplicate-wins column, the rows that search ---------
    if (edge_mode) {
        int n_slots;                             // slots of the CSR rank = the sum of the degrees (wave-uniform; CYC: from the scan's last lane)
        if (W == 1 && T == 64) {                 // one wave, n <= 64: the row starts are a wave prefix sum of the degrees
            const int d = tid < n ? popc64(A[tid]) : 0;
            int incl = d;
            if constexpr (CYC > 0) {
                // CYC: the scan as six adds with DPP operands (shifts inside a row of 16 lanes, then lane 15 / lane 31 broadcast to the rows behind;
                // a lane without a source adds the `old` operand, 0) instead of six LDS permutes with their address and select instructions.
                // All 64 lanes are active here.
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);      // row_shr:1
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);      // row_shr:2
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);      // row_shr:4
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);      // row_shr:8
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
                incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
            } else {
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (tid >= o) incl += t;
            }
            }
            if (tid <= n) rowstart[tid] = (rs_t)(incl - d);
            if (tid == 63 && n == 64) rowstart[64] = (rs_t)incl;
            if constexpr (CYC > 0) n_slots = __builtin_amdgcn_readlane(incl, 63);      // (lanes from n on add nothing: the total)
            else n_slots = 0;
        } else {
            for (int u = tid; u <= n; u += T) {
                int s = 0;
                for (int x = 0; x < u; ++x) {
#pragma unroll
                    for (int w = 0; w < W; ++w) s += popc64(A[x * W + w]);
                }
                rowstart[u] = (rs_t)s;
            }
            n_slots = 0;
        }
        // last[] is addressed by SLOT, not by column: a graph has two slots per undirected pair, which is more than its columns where pairs
        // come in one direction only.  Every slot in use is cleared (cleared up to E only, the slots beyond held whatever the pass before
        // left there: a stale column id made a live column lose its atomicMax, and rows of graphs with one-way pairs came out zero now and
        // then), and every slot lies inside last[]: the planner sizes it for a single graph's slots (count_plan.cpp: last_cap >= 2 e_decl or
        // n_decl (n_decl - 1)), and a pair with more slots than that is redone graph by graph.
        if constexpr (!(CYC > 0)) {                      // (the total is rowstart[n]: behind a barrier where more than one wave wrote the row starts)
            __syncthreads();
            n_slots = (int)rowstart[n];
        }
        if (ng > 1 && n_slots > a.last_cap) return 1;
        for (int i = tid; i < (n_slots > E ? n_slots : E); i += T) last[i] = -1;
        __syncthreads();
        if constexpr (CYC > 0) {
            // CYC: the column's own slot AND the slot of its reverse pair in this one visit, both staged as 16-bit values -- the own slot
            // where revof[c] will stand, the reverse slot in prim[c] (the compaction below writes prim[k] only for k <= c, behind the trip's
            // reads) -- so that the pass below reads last[] twice and ranks nothing again.
            for (int c = tid; c < E; c += T) {
                const int u = eu[c], v = ev[c];
                if (u == v) continue;
                const int r = rowstart[u] + popc64(A[u] & ((1ull << v) - 1ull)), rr = rowstart[v] + popc64(A[v] & ((1ull << u) - 1ull));
                revof[c] = (uint16_t)r; prim[c] = (uint16_t)rr;
                atomicMax(&last[r], c);
            }
        } else
        for (int c = tid; c < E; c += T) {
            const int u = eu[c], v = ev[c];
            if (u == v) continue;
            int r = rowstart[u];
#pragma unroll
            for (int w = 0; w < W; ++w) r += popc64(A[u * W + w] & below_word(v, w));
            revof[c] = (uint16_t)r;              // (its slot, until the pass below replaces it)
            atomicMax(&last[r], c);
        }
        __syncthreads();
        // Per column, once (not per task): is it the column that carries the counts of its pair (the last duplicate,
        // utils_graph_processing.py:142-144), which column carries the reverse pair, and does it search at all?  Undirected orbit
        // classes: every map that puts a pattern edge (a,b) on (u,v) puts (b,a), same class, on (v,u), so the two rows are equal
        // -- the u < v row searches and writes both.  Rows that carry nothing (self loops, earlier duplicates) get their zeros
        // here.  The searching rows are compacted IN COLUMN ORDER by one wave: every workgroup of a split graph enumerates the
        // same task list.
        if (tid < 64) {
            int n_prim = 0;
            for (int c0 = 0; c0 < E; c0 += 64) {
                const int c = c0 + tid;
                bool primary = false;
                if (c < E) {
                    const int u = eu[c], v = ev[c];
                    bool live = false;
                    int rev = -1;
                    if (u != v) {
                        live = last[revof[c]] == c;
                        int rr;
                        if constexpr (CYC > 0) rr = prim[c];      // (staged by the visit above)
                        else {
                        rr = rowstart[v];
#pragma unroll
                        for (int w = 0; w < W; ++w) rr += popc64(A[v * W + w] & below_word(u, w));
                        }
                        rev = last[rr];
                    }
                    revof[c] = rev < 0 ? (uint16_t)0xffffu : (uint16_t)rev;
                    primary = live && !(a_sym && rev >= 0 && u > v);
                    if (!live && part == 0 && !bulk_zero) {
                        if constexpr (CYC > 0) emit_row(c, 0u, 0u, 0u, 0u);
                        else
                        for (int col = 0; col < n_cols; ++col) emit_cell(c, col, 0ull);
                    }
#ifndef COUNT_NO_CORE_FILTER
                    if (primary) {
                        // A root outside the WEAKEST core any plan of the launch lives in is the image of nothing (cores are nested: it is outside
                        // every plan's core; lane_begin would find that out one task at a time -- a pull, a begin and a finish per cell).  Its
                        // cells, and those of the reverse row it would have written, are zero here and the row never enters the pool: on
                        // molecules (cycle plans: the 2-core = ring systems and what connects them) more than half of the rows.
                        bool in_core;
                        if constexpr (CYC > 0) in_core = ((core2 >> u) & (core2 >> v) & 1ull) != 0;
                        else {
                            const uint64_t *cm = cores + (__ffs(a.core_mask | (1 << CORE_MAX)) - 1) * W;
                            in_core = (((cm[u >> 6] >> (u & 63)) & (cm[v >> 6] >> (v & 63))) & 1ull) != 0;
                        }
                        if (!in_core) {
                            primary = false;
                            if (part == 0 && !bulk_zero) {
                                if constexpr (CYC > 0) {
                                    emit_row(c, 0u, 0u, 0u, 0u);
                                    if (rev >= 0) emit_row(rev, 0u, 0u, 0u, 0u);
                                } else
                                for (int col = 0; col < n_cols; ++col) {
                                    emit_cell(c, col, 0ull);
                                    if (a_sym && rev >= 0) emit_cell(rev, col, 0ull);
                                }
                            }
                        }
                    }
#endif
                }
                const uint64_t pm = __ballot(primary);
                if (primary) prim[n_prim + __popcll(pm & ((1ull << tid) - 1ull))] = (uint16_t)c;
                n_prim += __popcll(pm);
            }
            if (tid == 0) misc[3] = n_prim;
        }
    }
    __syncthreads();
    if (CYC > 0 ? cyc_bad : misc[2] != 0) {  // bad index: zeros + status
        if (!report) return 1;
        if (part == 0) {
            if constexpr (CYC > 0) zero_rows_cyc(rows, false);
            else {
            if (a.out) for (int i = tid; i < rows * n_cols; i += T) a.out[row0 * n_cols + i] = 0;
            if (a.enc_out && !a.enc_no32) for (int i = tid; i < rows * a.enc_width; i += T) a.enc_out[row0 * a.enc_width + i] = 0.f;
            if (a.enc16 && a.enc_no32) for (int i = tid; i < rows * a.enc_width; i += T) a.enc16[(row0 + i / a.enc_width) * a.enc16_stride + a.enc16_col0 + i % a.enc_width] = 0;
            if (!DIR && args_late()->idmask) for (int i = tid; i < rows; i += T) args_late()->idmask[row0 + i] = 0;
            }
            if (tid == 0) atomicMax(&a.status[g], CYC > 0 ? (int)GSN_ST_BAD_INDEX : misc[2]);
        }
        return 0;
    }

    COUNT_T(4);
#ifdef COUNT_PROF
    unsigned prof_iters = 0, prof_lanes = 0;          // pool loop trips of the wave, lanes inside a rooted search summed over the trips
    unsigned prof_arm[4] = {0, 0, 0, 0};              // cycles of the wave in the pull / begin / step / finish arm
#define COUNT_ARM(I, T0) do { prof_arm[I] += (unsigned)(__builtin_amdgcn_s_memtime() - (T0)); } while (0)
#define COUNT_ARM_T0() __builtin_amdgcn_s_memtime()
#else
#define COUNT_ARM(I, T0)
#define COUNT_ARM_T0() 0ull
#endif
    if constexpr (CYC > 0) {
        // ---- phase 3 (cycle columns): one path walk per searching row, a row per lane; the walk's counts are the row's four cells and
        // those of its mirror row.  Inner vertices are pruned with the 2-core, the core the cycle plans name (and the one phase 2
        // filtered the roots with).
        static_assert(W == 1 && MOL, "the cycle walk is the molecule instantiation's: one-word adjacency rows, four columns");
        const int n_div = misc[3];                         // rows that run walks
        // the four columns' lengths are wave-uniform: decoded once, each cell is one select chain on 32-bit counters (count_core.h: CycleAcc)
        typedef typename CycleAcc<CYC>::type acc_t;
        static_assert(sizeof(acc_t) == 4, "emit_row takes 32-bit counts");
        const int j0 = (int)(a.cyc_len & 0xffu) - 3, j1 = (int)((a.cyc_len >> 8) & 0xffu) - 3, j2 = (int)((a.cyc_len >> 16) & 0xffu) - 3, j3 = (int)(a.cyc_len >> 24) - 3;
        for (int i = tid; i < n_div; i += T) {
#ifdef COUNT_PROF
            prof_iters += 1; prof_lanes += (unsigned)__popcll(__ballot(1));      // passes of the wave, rows walked per pass
#endif
            const unsigned long long t0 = COUNT_ARM_T0();
            (void)t0;
            const int row = prim[i];
            acc_t cnt[CYC - 2];
            cycle_walk<CYC>(A, eu[row], ev[row], core2, cnt);
            COUNT_ARM(2, t0);
            const unsigned long long t0f = COUNT_ARM_T0();
            (void)t0f;
            const int rev = revof[row] == 0xffffu ? -1 : (int)revof[row];
            auto pick = [&](const int j) {
                acc_t c = 0;
#pragma unroll
                for (int q = 0; q < CYC - 2; ++q) c = j == q ? cnt[q] : c;
                return c;
            };
            const acc_t c0 = pick(j0), c1 = pick(j1), c2 = pick(j2), c3 = pick(j3);
            emit_row(row, c0, c1, c2, c3);
            if (rev >= 0) emit_row(rev, c0, c1, c2, c3);
            else if ((c0 | c1 | c2 | c3) != 0) atomicMax(&misc[2], (int)GSN_ST_KEYERROR);
            COUNT_ARM(3, t0f);
        }
    } else {
        // ---- phase 3: task pool -- (column, row) cells, pulled by lanes as they go idle --------------------------------
        // this workgroup takes the tasks  part, part + split, part + 2*split, ...  (strided, so the heavy columns of a
        // pattern family are spread over all the workgroups of a graph); n_tasks = how many of them
        const int n_div = edge_mode ? misc[3] : rows;            // rows that run searches
        const int n_tasks_all = n_div * n_cols;
        const int n_tasks = n_tasks_all > part ? (n_tasks_all - part + a_split - 1) / a_split : 0;
        const float div_rcp = n_div > 0 ? 1.0f / (float)n_div : 0.f;
        const bool div_float = n_tasks_all < (1 << 22);        // task index exact in fp32: quotient by one multiply + one correction
        const uint32_t *col_ptr = plan + PLAN_HEADER_WORDS;
        const uint32_t *col_order = col_ptr + n_cols + 1;
        const uint32_t *plans = plan + a.plans_off;
        const int lane = tid & 63;
        const uint64_t lane_lt = (1ull << lane) - 1ull;

        Lane<W> s;
#ifdef COUNT_PROF_STEP
        for (int q = 0; q < 12; ++q) s.prof[q] = 0;
#endif
        s.l = -1; s.cnt = 0; s.k = 0; s.nfix = 0; s.fvec = fv_roots<W>(0, 0); s.plan = plans;
        s.balls = balls; s.ball_n = a.n_cap; s.degp = nullptr; s.loop = 0;
        if (TAIL) { s.degp = degp; s.loop = a.tail_loop; }
#pragma unroll
        for (int w = 0; w < W; ++w) s.used.w[w] = 0ull;
        bool has_task = false, exhausted = false;
        int t_row = 0, t_col = 0, p_i = 0, p_e = 0;
        FVec<W> roots = fv_roots<W>(0, 0);
        bool rev_missing = false;
        int mirror_row = -1;
        const uint64_t *lane_valid = valid;     // candidate universe of the lane's current plan (a core of the graph)

        // The loop is a state machine per lane (pull a cell, begin a plan, one search step, finish the cell) and a wave executes every arm
        // some lane is in: on molecules a trip is ~350 instructions of which the step arm is ~100, and the whole pool is ~9 trips of ~4 000
        // cycles (profiles/r05_count_phase_profile.txt) -- dependent LDS round trips, not arithmetic.  So (i) a cell that ends inside a begin
        // or a step is finished in the SAME trip (its own arm behind them), and (ii) idle lanes are refilled in batches: the pull arm (an LDS
        // atomic, the task decode, five dependent table reads) runs when GSN_PULL_BATCH lanes wait or when no lane is inside a search, not
        // in every trip for the one lane that happened to finish.
        for (;;) {
            const bool need = !has_task && !exhausted;
            uint64_t m = __ballot(need);
            if (m && __popcll(m) < a.pull_batch && __ballot(has_task) != 0ull) m = 0ull;
            const unsigned long long arm_t0 = COUNT_ARM_T0();
            if (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&misc[0], __popcll(m));
                base = __shfl(base, leader);
                if (need) {
                    const int t = base + __popcll(m & lane_lt);
                    if (t < n_tasks) {
                        const int tt = part + t * a_split;
                        int t_idx;
                        if (div_float) {
                            t_col = (int)((float)tt * div_rcp);
                            t_idx = tt - t_col * n_div;
                            if (t_idx < 0) { --t_col; t_idx += n_div; }
                            if (t_idx >= n_div) { ++t_col; t_idx -= n_div; }
                        } else {
                            t_col = tt / n_div;
                            t_idx = tt - t_col * n_div;
                        }
                        // columns in the plan compiler's order of falling estimated cost: the lanes that go idle at the end of the pool
                        // should be left with the short searches, not with the long ones
                        t_col = (int)col_order[t_col];
                        has_task = true;
                        s.cnt = 0; s.l = -1;
                        p_i = (int)col_ptr[t_col]; p_e = (int)col_ptr[t_col + 1];
                        rev_missing = false;
                        mirror_row = -1;
                        if (edge_mode) {
                            t_row = prim[t_idx];
                            const int rev = revof[t_row] == 0xffffu ? -1 : (int)revof[t_row];
                            rev_missing = rev < 0;
                            if (a_sym && rev >= 0) mirror_row = rev;
                            roots = fv_roots<W>(eu[t_row], ev[t_row]);
                        } else {
                            t_row = t_idx;
                            if (!((valid[t_row >> 6] >> (t_row & 63)) & 1ull)) p_i = p_e;  // vertex beyond the largest id: not a vertex of the matched graph
                            roots = fv_roots<W>(t_row, 0);
                        }
                    } else {
                        exhausted = true;
                    }
                }
            }
            if (m) COUNT_ARM(0, arm_t0);
            if (__ballot(has_task) == 0ull) break;
#ifdef COUNT_PROF
            prof_iters += 1; prof_lanes += (unsigned)__popcll(__ballot(has_task && s.l >= 0));
#endif
            if (has_task) {
                if (s.l < 0) {
                    if (p_i < p_e) {
                        const unsigned long long t0 = COUNT_ARM_T0();
                        const uint32_t *pl = plans + p_i * (DIR ? PLAN_STRIDE_DIRECTED : PLAN_STRIDE_WORDS);
                        lane_valid = cores + plan_core(pl) * W;
                        lane_begin<W, DIR, TAIL>(s, pl, roots, A, lane_valid, stack, T, tid, A_in);
                        ++p_i;
                        COUNT_ARM(1, t0);
                    }
                } else {
                    const unsigned long long t0 = COUNT_ARM_T0();
                    lane_step<W, DIR, TAIL>(s, A, lane_valid, stack, T, tid, A_in);
                    COUNT_ARM(2, t0);
#ifdef COUNT_PROF_STEP
                    s.prof[9] += 1; s.prof[10] += (unsigned long long)__popcll(__ballot(1));      // lane_step visits / active lanes
#endif
                }
                const unsigned long long t0f = COUNT_ARM_T0();
                if (s.l < 0 && p_i >= p_e) {
                    // cell finished (its last plan ended in this trip's begin or step, or it had none)
                    emit_cell(t_row, t_col, s.cnt);
                    if (mirror_row >= 0) emit_cell(mirror_row, t_col, s.cnt);
                    if (edge_mode && rev_missing && s.cnt != 0) atomicMax(&misc[2], (int)GSN_ST_KEYERROR);
                    has_task = false;
                    COUNT_ARM(3, t0f);
                }
            }
        }
#ifdef COUNT_PROF_STEP
        if ((threadIdx.x & 63) == 0 && g_count_prof2) for (int q = 0; q < 12; ++q) atomicAdd(&g_count_prof2[q], s.prof[q]);
#endif
    }
    __syncthreads();

    COUNT_T(5);
#ifdef COUNT_PROF
    if (threadIdx.x == 0 && g_count_prof) { g_count_prof[(size_t)blockIdx.x * 16 + 7] = ((unsigned long long)prof_iters << 32) | prof_lanes; for (int q = 0; q < 4; ++q) g_count_prof[(size_t)blockIdx.x * 16 + 8 + q] = prof_arm[q]; }
#endif
    // ---- phases 4 and 4' of the headline combination (CycKeys) as ONE loop, a row per lane and trip: the row's four staged counts are one
    // 8-byte LDS read; the int64 row leaves as two 16-byte stores (32 contiguous bytes per lane, 2 KiB per wave) and the 2-byte identifier
    // mask is made from the same registers (count_core.h: cyc_row_store, cyc_row_mask).  Addresses: the graph's first row as a scalar base,
    // the lane's row as a 32-bit byte offset.  An int64 base that is not 16-byte aligned takes 8-byte stores (row0 * 32 keeps the base's
    // alignment: wave-uniform).
    if constexpr (KEYS) {
        char *orow = reinterpret_cast<char *>(a.out + row0 * 4), *mrow = reinterpret_cast<char *>(a.idmask + row0);
        const bool wide = (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
        const uint32_t ncls_w = (uint32_t)a.enc_n[0] | ((uint32_t)a.enc_n[1] << 8) | ((uint32_t)a.enc_n[2] << 16) | ((uint32_t)a.enc_n[3] << 24);
        const bool clamp = a.enc_clamp != 0;
        const int col0 = a.enc16_col0;
        // The int64 rows leave through a buffer resource over this pass's rows (scalar base, the lane's byte offset, the second half of a row
        // as the instruction's immediate: no 64-bit vector add per trip; a store past the pass's last row would be dropped by the hardware).
        // The rare row with a cell that went out by itself takes count_core.h's cell-by-cell arm through a pointer.
        typedef unsigned st16_t __attribute__((ext_vector_type(4)));
        typedef unsigned st8_t __attribute__((ext_vector_type(2)));
        const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(orow, 0, rows * 32, 0x00020000);
        const __amdgpu_buffer_rsrc_t mrs = __builtin_amdgcn_make_buffer_rsrc(mrow, 0, rows * 2, 0x00020000);      // (the masks of the same rows)
        for (int r = tid; r < rows; r += T) {
            const uint2 q = *reinterpret_cast<const uint2 *>(out_lds + 4 * r);
            const int ob = r * 32;
            if (cyc_row_has_direct(q.x, q.y)) cyc_row_store(reinterpret_cast<int64_t *>(orow + (uint32_t)ob), q.x, q.y, wide);
            else if (wide) {
                __builtin_amdgcn_raw_buffer_store_b128(st16_t{q.x & 0xffffu, 0u, q.x >> 16, 0u}, ors, ob, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(st16_t{q.y & 0xffffu, 0u, q.y >> 16, 0u}, ors, ob + 16, 0, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b64(st8_t{q.x & 0xffffu, 0u}, ors, ob, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(st8_t{q.x >> 16, 0u}, ors, ob + 8, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(st8_t{q.y & 0xffffu, 0u}, ors, ob + 16, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(st8_t{q.y >> 16, 0u}, ors, ob + 24, 0, 0);
            }
            __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(cyc_row_mask(q.x, q.y, ncls_w, clamp) << col0), mrs, r * 2, 0, 0);
        }
    }
    // ---- phase 4: coalesced write of the staged rows --------------------------------------------------------------
    if (!KEYS && a_stage_out) {   // (only with split == 1)
        int64_t *dst = a.out + row0 * n_cols;
        for (int i = tid; i < rows * n_cols; i += T) {
            const uint16_t v = out_lds[i];
            if (v != (uint16_t)0xffff) dst[i] = (int64_t)v;
        }
    }
    // ---- phase 4': encoded rows from the staged class indices, one float per thread and trip, consecutive addresses ----------
    if (!KEYS && a_enc && a_enc_stage) {
        const unsigned char *est = smem + a.off_encst;
        // class index of cell (r, c): the staged byte, or from the staged 16-bit count (0xffff = a count of 65 535 and more: the last class
        // when clamped, none otherwise -- class counts fit a byte here)
        auto cls_from_count = [&](unsigned v, int c) -> int {
            const int ncls = enc[2 * c + 1];
            if (a.enc_clamp) return (int)v >= ncls ? ncls - 1 : (int)v;
            return (int)v < ncls ? (int)v : 0xff;
        };
        float *dst = a.enc_out + row0 * a.enc_width;
        const int total = rows * a.enc_width;
        const bool pack_ok = !a.enc16 || (((a.enc16_stride | a.enc16_col0) & 3) == 0 && (reinterpret_cast<uintptr_t>(a.enc16) & 7) == 0);
        if ((MOL || n_cols == 4) && (a.enc_width & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && pack_ok) {
            // four identifier columns (the cycle / clique families of the reference's configurations): a thread owns a row, reads
            // its four class indices as one word and writes the row as float4s
            int hot0 = enc[0], hot1 = enc[2], hot2 = enc[4], hot3 = enc[6];
            for (int r = tid; r < rows; r += T) {
                int c0, c1, c2, c3;
                if (a_enc_from_counts) {
                    const uint2 q = *reinterpret_cast<const uint2 *>(out_lds + 4 * r);
                    c0 = cls_from_count(q.x & 0xffffu, 0); c1 = cls_from_count(q.x >> 16, 1);
                    c2 = cls_from_count(q.y & 0xffffu, 2); c3 = cls_from_count(q.y >> 16, 3);
                } else {
                    const unsigned cw = *reinterpret_cast<const unsigned *>(est + 4 * r);
                    c0 = (int)(cw & 0xffu); c1 = (int)((cw >> 8) & 0xffu); c2 = (int)((cw >> 16) & 0xffu); c3 = (int)(cw >> 24);
                }
                const int h0 = c0 == 0xff ? -1 : hot0 + c0, h1 = c1 == 0xff ? -1 : hot1 + c1;
                const int h2 = c2 == 0xff ? -1 : hot2 + c2, h3 = c3 == 0xff ? -1 : hot3 + c3;
                float4 *d4 = reinterpret_cast<float4 *>(dst + r * a.enc_width);
                if (!a.enc_no32)
                for (int k = 0; k < a.enc_width; k += 4) {
                    float4 o;
                    o.x = (h0 == k || h1 == k || h2 == k || h3 == k) ? 1.f : 0.f;
                    o.y = (h0 == k + 1 || h1 == k + 1 || h2 == k + 1 || h3 == k + 1) ? 1.f : 0.f;
                    o.z = (h0 == k + 2 || h1 == k + 2 || h2 == k + 2 || h3 == k + 2) ? 1.f : 0.f;
                    o.w = (h0 == k + 3 || h1 == k + 3 || h2 == k + 3 || h3 == k + 3) ? 1.f : 0.f;
                    d4[k >> 2] = o;
                }
                if (a.enc16) {                          // the same row as fp16 (1.0 = 0x3c00) into the pack's column range, 8 bytes per store
                    uint2 *p2 = reinterpret_cast<uint2 *>(a.enc16 + (row0 + r) * a.enc16_stride + a.enc16_col0);
                    for (int k = 0; k < a.enc_width; k += 4) {
                        uint2 o;
                        o.x = ((h0 == k || h1 == k || h2 == k || h3 == k) ? 0x3c00u : 0u) | ((h0 == k + 1 || h1 == k + 1 || h2 == k + 1 || h3 == k + 1) ? 0x3c000000u : 0u);
                        o.y = ((h0 == k + 2 || h1 == k + 2 || h2 == k + 2 || h3 == k + 2) ? 0x3c00u : 0u) | ((h0 == k + 3 || h1 == k + 3 || h2 == k + 3 || h3 == k + 3) ? 0x3c000000u : 0u);
                        p2[k >> 2] = o;
                    }
                }
                // the row's hot pack columns as a bit mask (2 bytes instead of the 8 enc_width / 4 above)
                if (!DIR && args_late()->idmask)
                    args_late()->idmask[row0 + r] = (uint16_t)(((h0 < 0 ? 0u : 1u << h0) | (h1 < 0 ? 0u : 1u << h1) | (h2 < 0 ? 0u : 1u << h2) | (h3 < 0 ? 0u : 1u << h3)) << a.enc16_col0);
            }
        } else {
        // column c owns floats enc[2c] .. enc[2c] + enc[2c + 1] of a row; the table is short: a linear scan per float
        if (!a.enc_no32 || a.enc16)
        for (int i = tid; i < total; i += T) {
            const int r = i / a.enc_width;              // (exact: the reciprocal multiply was off by one for wide encodings, e.g. width 1000 from row 6100 on; this loop is bound by its stores)
            const int j = i - r * a.enc_width;
            int c = 0;
            while (c + 1 < n_cols && enc[2 * (c + 1)] <= j) ++c;
            const int k = j - enc[2 * c];
            const int cls = a_enc_from_counts ? cls_from_count(out_lds[r * n_cols + c], c) : (int)est[r * n_cols + c];
            const bool hot = k < enc[2 * c + 1] && cls == k;
            if (!a.enc_no32) dst[i] = hot ? 1.f : 0.f;
            if (a.enc16) a.enc16[(row0 + r) * a.enc16_stride + a.enc16_col0 + j] = hot ? (uint16_t)0x3c00 : (uint16_t)0;
        }
        if (!DIR && args_late()->idmask)                                   // the same rows as bit masks, a row per thread
            for (int r = tid; r < rows; r += T) {
                unsigned m = 0;
                for (int c = 0; c < n_cols; ++c) {
                    const int cls = a_enc_from_counts ? cls_from_count(out_lds[r * n_cols + c], c) : (int)est[r * n_cols + c];
                    if (cls < enc[2 * c + 1]) m |= 1u << (enc[2 * c] + cls);
                }
                args_late()->idmask[row0 + r] = (uint16_t)(m << a.enc16_col0);
            }
        }
    }
    COUNT_T(6);
    if (misc[2] != 0) {
        if (!report) return 1;
        if (tid == 0) atomicMax(&a.status[g], misc[2]);   // status[] starts at zero: zeroed by this workgroup (zero_status) or by the launcher
    }
    return 0;
}

// (Measured and dropped: amdgpu_waves_per_eu(6 / 7) on the molecule instantiation spills 72 / 104 bytes per lane for 1.4 / 2 % on the kernel
//  and 0.5 % on the step; even a bound of 5 -- no tighter than what the allocator picks by itself -- changed its choices: 94 registers and
//  36 bytes of scratch instead of 83 and none, +3 % kernel time.  No occupancy attribute.)
// Register bound of the two-word instantiations (graphs of 65 .. 128 vertices: BASELINE config 5, ER G(128,1000)).  Left to itself the
// allocator takes 136 registers = 3 waves per SIMD for a kernel that is bound by the latency of dependent LDS reads at 0.30 lane activity
// (profiles/r06_count_er128_phase.txt); bounded to 80 (6 waves) it spills 188 bytes per lane and the launch is still 22 % faster:
// 43.6 k -> 53.5 k graphs/s at 2 048 graphs per launch (4 waves 50.0 k, 5: 52.9 k, 8: 52.4 k; scripts/gpu/r6_er_ab.sh).  The molecule
// instantiation has its own bound (COUNT_MOL_WAVES); the wider ones (W >= 4) are left alone: no BASELINE config runs them.
#ifndef COUNT_W2_WAVES
#define COUNT_W2_WAVES 6
#endif
#ifndef COUNT_W1_WAVES
#define COUNT_W1_WAVES 1
#endif
#ifndef COUNT_W4_WAVES
#define COUNT_W4_WAVES 1
#endif
// Register bound of the cycle instantiation (CYC > 0): one-wave workgroups of dependent LDS round trips, a ZINC pair in ~4 KiB of LDS -- 32
// workgroups fit a CU, so the register file decides how many are resident.  8 waves per SIMD = 64 registers: it takes 55, no spill, no
// scratch (profiles/count_resources_after.txt; 95 registers = 5 waves before).  What brought it there is marked "CYC:" in count_body
// -- error-path zeros without 64-bit quotients, arguments read where they are used, whole-row staging from 32-bit counters,
// the 2-core in a register, the lane id opaque per pass; side_block, which shares the kernel, fits the bound as it is.
// At eight waves the SIMD's vector issue is what is full (profiles/count_cycle_instruction_diet.txt), so the instantiation is also kept
// short: both flag types, CycAny and CycKeys, stay at 55 registers without scratch (profiles/count_resources_diet.txt).
#ifndef COUNT_CYC_WAVES
#define COUNT_CYC_WAVES 8
#endif
template <int W, int T, bool DIR, bool TAIL, bool MOL = false, int CYC = 0, class FL = CycAny>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(CYC > 0 ? COUNT_CYC_WAVES : DIR ? 1 : (W == 1 ? COUNT_W1_WAVES : (W == 2 ? COUNT_W2_WAVES : (W == 4 ? COUNT_W4_WAVES : 1))))))
void count_kernel(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool KEYS = CYC > 0 && FL::KEYS;           // (the headline launch: side workgroups, pairs, status words zeroed here -- count_plan.cpp: choose_kernel)
    int bid = (int)blockIdx.x;
    if (KEYS || a.side_mask) {                           // (launches with side workgroups: one workgroup per item, no graph list)
        const int grp = bid / (SIDE_EVERY + 1), j = bid - grp * (SIDE_EVERY + 1);
        if (j == SIDE_EVERY) {
            const int i0 = grp * SIDE_EVERY, i1 = i0 + SIDE_EVERY < a.n_items ? i0 + SIDE_EVERY : a.n_items;
            const int per = (MOL || a.pair) ? 2 : 1;
            side_block<T, FL>(a, smem, per * i0, per * i1 < a.n_graphs ? per * i1 : a.n_graphs);
            return;
        }
        bid = grp * SIDE_EVERY + j;
        if (bid >= a.n_items) return;
    }
    const int item = MOL ? bid : bid / a.split, part = MOL ? 0 : bid - item * a.split;
    // one call site (the body is inlined once): pass 0 = the graph, or the pair 2 i, 2 i + 1 as one; passes 1, 2 = the pair's graphs one by
    // one when it did not fit or held an error
    const int g0 = (MOL || a.pair) ? 2 * item : (a.graph_ids ? a.graph_ids[item] : item);
    const bool two = (MOL || a.pair) && g0 + 1 < a.n_graphs;
    if ((KEYS || a.zero_status) && threadIdx.x == 0) {   // (the thread that raises them later: same address, program order)
        a.status[g0] = 0;
        if (two) a.status[g0 + 1] = 0;
    }
    for (int pass = 0; pass < 3; ++pass) {
        const int g = pass == 2 ? g0 + 1 : g0;
        const int ng = (pass == 0 && two) ? 2 : 1;
        int rc;
        if constexpr (CYC > 0) rc = count_body<W, T, DIR, TAIL, MOL, CYC, FL>(*args_late(), smem, item, 0, g, ng, ng == 1);      // (the body reads every field where it uses it)
        else rc = count_body<W, T, DIR, TAIL, MOL, CYC>(a, smem, item, (MOL || a.pair) ? 0 : part, g, ng, ng == 1);
        if (!two || (pass == 0 && rc == 0)) break;
    }
}

// the molecule instantiation as its own kernel: its register bound is set apart from the generic instantiations
#ifndef COUNT_MOL_WAVES
#define COUNT_MOL_WAVES 6
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(COUNT_MOL_WAVES))) void count_kernel_mol(CountArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int item = (int)blockIdx.x;
    if (a.side_mask) {
        const int grp = item / (SIDE_EVERY + 1), j = item - grp * (SIDE_EVERY + 1);
        if (j == SIDE_EVERY) {
            const int i0 = grp * SIDE_EVERY, i1 = i0 + SIDE_EVERY < a.n_items ? i0 + SIDE_EVERY : a.n_items;
            side_block<64>(a, smem, 2 * i0, 2 * i1 < a.n_graphs ? 2 * i1 : a.n_graphs);
            return;
        }
        item = grp * SIDE_EVERY + j;
        if (item >= a.n_items) return;
    }
    const int g0 = 2 * item;
    const bool two = g0 + 1 < a.n_graphs;
    if (a.zero_status && threadIdx.x == 0) {
        a.status[g0] = 0;
        if (two) a.status[g0 + 1] = 0;
    }
    for (int pass = 0; pass < 3; ++pass) {
        const int g = pass == 2 ? g0 + 1 : g0;
        const int ng = (pass == 0 && two) ? 2 : 1;
        const int rc = count_body<1, 64, false, false, true>(a, smem, item, 0, g, ng, ng == 1);
        if (!two || (pass == 0 && rc == 0)) break;
    }
}

__global__ void status_zero_kernel(const int32_t *graph_ids, int n, int32_t *status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) status[graph_ids[i]] = 0;
}

template <int W, int T, bool DIR, bool TAIL, bool MOL = false, int CYC = 0, class FL = CycAny>
static int launch_d(CountArgs &a, int n_items, size_t lds, hipStream_t stream) {
    // (the size varies per call: no once-per-device flag; no label: the error names the byte count)
    if (int rc = lds_limit(nullptr, {kernel_ptr(&count_kernel<W, T, DIR, TAIL, MOL, CYC, FL>)}, nullptr, (int)lds)) return rc;
    hipLaunchKernelGGL((count_kernel<W, T, DIR, TAIL, MOL, CYC, FL>), dim3((unsigned)n_items), dim3(T), lds, stream, a);
    if (int rc = launch_check("count_kernel launch")) return rc;
#ifdef COUNT_PROF
    {
        (void)hipStreamSynchronize(stream);
        static EveryNth show{16};
        if (show()) {
            unsigned long long *buf = nullptr;
            (void)hipMalloc(&buf, (size_t)n_items * 128);
            (void)hipMemset(buf, 0, (size_t)n_items * 128);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_count_prof), &buf, sizeof(buf));
            unsigned long long *buf2 = buf + (size_t)n_items * 16 - 16;      // (the last item's slots 16..: its own row is read first)
            (void)hipMalloc(&buf2, 128); (void)hipMemset(buf2, 0, 128);
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_count_prof2), &buf2, sizeof(buf2));
            hipLaunchKernelGGL((count_kernel<W, T, DIR, TAIL, MOL, CYC, FL>), dim3((unsigned)n_items), dim3(T), lds, stream, a);
            (void)hipStreamSynchronize(stream);
            unsigned long long *h = new unsigned long long[(size_t)n_items * 16];
            (void)hipMemcpy(h, buf, (size_t)n_items * 128, hipMemcpyDeviceToHost);
            double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            double it_sum = 0, ln_sum = 0, arm[4] = {0, 0, 0, 0};
            for (int i = 0; i < n_items; ++i) {
                for (int q = 0; q < 7; ++q) s[q] += (double)h[(size_t)i * 16 + q];
                it_sum += (double)(h[(size_t)i * 16 + 7] >> 32); ln_sum += (double)(h[(size_t)i * 16 + 7] & 0xffffffffull);
                for (int q = 0; q < 4; ++q) arm[q] += (double)h[(size_t)i * 16 + 8 + q];
            }
            fprintf(stderr, "countprof pool: %.1f loop trips per workgroup (wave 0), %.1f lanes of 64 inside a search per trip; cycles per workgroup in the arms: pull %.0f begin %.0f step %.0f finish %.0f\n",
                    it_sum / n_items, it_sum > 0 ? ln_sum / it_sum : 0.0, arm[0] / n_items, arm[1] / n_items, arm[2] / n_items, arm[3] / n_items);
            fprintf(stderr, "countprof W %d T %d cycle walk %d items %d: cycles per workgroup: clear+plan %.0f adjacency %.0f cores %.0f balls %.0f edge ranks %.0f task pool %.0f write %.0f\n", W, T, CYC, n_items,
                    s[0] / n_items, s[1] / n_items, s[2] / n_items, s[3] / n_items, s[4] / n_items, s[5] / n_items, s[6] / n_items);
            delete[] h;
            {
                unsigned long long p2[16];
                (void)hipMemcpy(p2, buf2, 96, hipMemcpyDeviceToHost);
                fprintf(stderr, "countprof step arms (summed over the launch's waves): tail_loop %.3g cycles in %.3g visits, %.1f lanes per visit, %.1f iterations per lane, %.1f = the longest lane's per visit | "
                                "tail_pairs %.3g cycles in %.3g visits, %.1f lanes per visit | lane_step %.3g visits, %.1f lanes per visit\n",
                        (double)p2[0], (double)p2[1], p2[1] ? (double)p2[2] / p2[1] : 0.0, p2[2] ? (double)p2[3] / p2[2] : 0.0, p2[1] ? (double)p2[4] / p2[1] : 0.0,
                        (double)p2[5], (double)p2[6], p2[6] ? (double)p2[7] / p2[6] : 0.0, (double)p2[9], p2[9] ? (double)p2[10] / p2[9] : 0.0);
                unsigned long long *nul2 = nullptr;
                (void)hipMemcpyToSymbol(HIP_SYMBOL(g_count_prof2), &nul2, sizeof(nul2));
                (void)hipFree(buf2);
            }
            unsigned long long *nul = nullptr;
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_count_prof), &nul, sizeof(nul));
            (void)hipFree(buf);
        }
    }
#endif
    return GSN_OK;
}
static int launch_mol(CountArgs &a, int n_items, size_t lds, hipStream_t stream) {
    if (int rc = lds_limit(nullptr, {kernel_ptr(&count_kernel_mol)}, nullptr, (int)lds)) return rc;
    hipLaunchKernelGGL(count_kernel_mol, dim3((unsigned)n_items), dim3(64), lds, stream, a);
    return launch_check("count_kernel_mol launch");
}

constexpr int kernel_key(int W, int T, CountKernel k) { return (W * 1024 + T) * 8 + (int)k; }

// The instantiations of the library, one per plan (count_plan.cpp: choose_kernel): one-word graphs have all four of directed x tail, and at
// 64 threads the molecule and cycle kernels; wider graphs always run with the tails.
static int dispatch(CountLaunchPlan &p, hipStream_t st) {
    CountArgs &a = p.args;
    const int n = p.grid;
    const size_t lds = (size_t)p.lds_bytes;
    switch (kernel_key(p.W, p.T, p.kernel)) {
        case kernel_key(1, 64, DIRECTED_TAIL): return launch_d<1, 64, true, true>(a, n, lds, st);
        case kernel_key(1, 64, DIRECTED): return launch_d<1, 64, true, false>(a, n, lds, st);
        case kernel_key(1, 64, CYCLE_KEYS): return launch_d<1, 64, false, false, true, 6, CycKeys>(a, n, lds, st);
        case kernel_key(1, 64, CYCLE_ANY): return launch_d<1, 64, false, false, true, 6>(a, n, lds, st);
        case kernel_key(1, 64, CountKernel::MOL): return launch_mol(a, n, lds, st);
        case kernel_key(1, 64, GENERIC_TAIL): return launch_d<1, 64, false, true>(a, n, lds, st);
        case kernel_key(1, 64, GENERIC): return launch_d<1, 64, false, false>(a, n, lds, st);
        case kernel_key(1, 256, DIRECTED_TAIL): return launch_d<1, 256, true, true>(a, n, lds, st);
        case kernel_key(1, 256, DIRECTED): return launch_d<1, 256, true, false>(a, n, lds, st);
        case kernel_key(1, 256, GENERIC_TAIL): return launch_d<1, 256, false, true>(a, n, lds, st);
        case kernel_key(1, 256, GENERIC): return launch_d<1, 256, false, false>(a, n, lds, st);
        case kernel_key(2, 64, DIRECTED_TAIL): return launch_d<2, 64, true, true>(a, n, lds, st);
        case kernel_key(2, 64, GENERIC_TAIL): return launch_d<2, 64, false, true>(a, n, lds, st);
        case kernel_key(2, 256, DIRECTED_TAIL): return launch_d<2, 256, true, true>(a, n, lds, st);
        case kernel_key(2, 256, GENERIC_TAIL): return launch_d<2, 256, false, true>(a, n, lds, st);
        case kernel_key(4, 64, DIRECTED_TAIL): return launch_d<4, 64, true, true>(a, n, lds, st);
        case kernel_key(4, 64, GENERIC_TAIL): return launch_d<4, 64, false, true>(a, n, lds, st);
        case kernel_key(4, 256, DIRECTED_TAIL): return launch_d<4, 256, true, true>(a, n, lds, st);
        case kernel_key(4, 256, GENERIC_TAIL): return launch_d<4, 256, false, true>(a, n, lds, st);
        case kernel_key(8, 64, DIRECTED_TAIL): return launch_d<8, 64, true, true>(a, n, lds, st);
        case kernel_key(8, 64, GENERIC_TAIL): return launch_d<8, 64, false, true>(a, n, lds, st);
        case kernel_key(12, 64, DIRECTED_TAIL): return launch_d<12, 64, true, true>(a, n, lds, st);
        case kernel_key(12, 64, GENERIC_TAIL): return launch_d<12, 64, false, true>(a, n, lds, st);
    }
    return set_error(GSN_E_UNSUPPORTED, "gsn_count_hip: no count_kernel<%d,%d> of kind %d in this build", p.W, p.T, (int)p.kernel);
}

}  // namespace gsn

using namespace gsn;

// Plan (count_plan.cpp: every decision, on the host), status words, trace, dispatch.
static int count_launch(const CountRequest &rq, void *stream) {
    CountSwitches sw = CountSwitches::read();
#ifdef COUNT_PROF       // (the phase profile is read from the generic instantiation, or from the cycle one; here, where the profiling build's define is seen)
    sw.cycle = sw_on(SW_COUNT_CYCLE, true);
    sw.mol = false;
#endif
    CountLaunchPlan p;
    if (int rc = count_plan(rq, sw, &p)) return rc;
    if (p.grid == 0) return GSN_OK;
    const CountArgs &a = p.args;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (p.memset_status) {
        hipError_t e = rq.graph_ids ? hipSuccess : hipMemsetAsync(rq.status, 0, sizeof(int32_t) * (size_t)rq.n_graphs, st);
        if (rq.graph_ids) hipLaunchKernelGGL(status_zero_kernel, dim3((unsigned)((rq.n_items + 255) / 256)), dim3(256), 0, st, rq.graph_ids, (int)rq.n_items, rq.status);
        if (e != hipSuccess) return set_error(GSN_E_HIP, "hipMemsetAsync(status): %s", hipGetErrorString(e));
    }
    trace("gsn count: count_kernel<%d,%d> workgroups %d pair %d split %d lds %d\n", p.W, p.T, p.grid, a.pair, a.split, p.lds_bytes);
    if (p.W == 1 && p.T == 64 && a.off_ain < 0) {
        const bool tail = a.any_tail != 0 || a.tail_loop != 0;
        trace("gsn count: molecule instantiation %d cycle walk %d (tail %d mode %d sym %d cols %d pair %d split %d stage %d out %d enc %d enc_stage %d ids %d)\n", (int)count_molecule_route(a, sw),
                    (int)(a.cyc_len != 0), (int)tail, a.mode, a.sym, a.n_cols, a.pair, a.split, a.stage_out, a.out != nullptr, a.enc_out != nullptr, a.enc_stage, a.graph_ids != nullptr);
        if (a.cyc_len) trace("gsn count: cycle flags %s\n", p.kernel == CYCLE_KEYS ? "CycKeys" : "CycAny");
    }
    return dispatch(p, st);
}

// the identifier columns pack_col0 .. of a pack row: inside the row (the widths as far as the arguments can be read; the planner validates them)
static int pack_columns_check(const char *entry, const CountRequest &rq) {
    const int64_t pack_stride = rq.enc16_stride;
    int64_t w = 0;
    if (rq.n_classes && rq.plan_host && rq.plan_words >= PLAN_HEADER_WORDS) for (uint32_t c = 0; c < rq.plan_host[4] && c < GSN_ENC_MAX_COLS; ++c) w += rq.n_classes[c];
    if (pack_stride <= 0 || pack_stride > 0x7fffffff || rq.enc16_col0 < 0 || rq.enc16_col0 + w > pack_stride)
        return set_error(GSN_E_INVALID, "%s: columns %lld .. %lld outside a pack row of %lld", entry, (long long)rq.enc16_col0, (long long)(rq.enc16_col0 + w), (long long)pack_stride);
    return GSN_OK;
}

extern "C" int gsn_count_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                             const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                             int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                             int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status, void *stream) {
    if (!out) return set_error(GSN_E_INVALID, "gsn_count_hip: null pointer argument");
    CountRequest rq;
    rq.plan_host = plan_host; rq.plan_dev = plan_dev; rq.plan_words = plan_words; rq.n_graphs = n_graphs; rq.node_ptr = node_ptr; rq.edge_ptr = edge_ptr;
    rq.edge_index = edge_index; rq.edge_row_stride = edge_row_stride; rq.ids_are_global = ids_are_global; rq.max_nodes = max_nodes; rq.max_edges = max_edges;
    rq.out = out; rq.status = status;
    rq.graph_ids = graph_ids; rq.n_items = n_items;
    return count_launch(rq, stream);
}

extern "C" int gsn_count_encode_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                    const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                    int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                                    int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status,
                                    const int32_t *n_classes, int clamp, float *enc_out, void *stream) {
    if (!enc_out) return set_error(GSN_E_INVALID, "gsn_count_encode_hip: enc_out is null");
    CountRequest rq;
    rq.plan_host = plan_host; rq.plan_dev = plan_dev; rq.plan_words = plan_words; rq.n_graphs = n_graphs; rq.node_ptr = node_ptr; rq.edge_ptr = edge_ptr;
    rq.edge_index = edge_index; rq.edge_row_stride = edge_row_stride; rq.ids_are_global = ids_are_global; rq.max_nodes = max_nodes; rq.max_edges = max_edges;
    rq.out = out; rq.status = status;
    rq.graph_ids = graph_ids; rq.n_items = n_items;
    rq.n_classes = n_classes; rq.enc_clamp = clamp; rq.enc_out = enc_out;
    return count_launch(rq, stream);
}

extern "C" int gsn_count_encode_pack16_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                           const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                           int64_t edge_row_stride, int ids_are_global, const int32_t *graph_ids, int64_t n_items,
                                           int64_t max_nodes, int64_t max_edges, int64_t *out, int32_t *status,
                                           const int32_t *n_classes, int clamp, float *enc_out, uint16_t *pack, int64_t pack_stride,
                                           int64_t pack_col0, void *stream) {
    if (!pack) return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_hip: pack is null");
    CountRequest rq;
    rq.plan_host = plan_host; rq.plan_dev = plan_dev; rq.plan_words = plan_words; rq.n_graphs = n_graphs; rq.node_ptr = node_ptr; rq.edge_ptr = edge_ptr;
    rq.edge_index = edge_index; rq.edge_row_stride = edge_row_stride; rq.ids_are_global = ids_are_global; rq.max_nodes = max_nodes; rq.max_edges = max_edges;
    rq.out = out; rq.status = status;
    rq.graph_ids = graph_ids; rq.n_items = n_items;
    // enc_out == NULL (r05): the pack columns are the only form of the encoded rows -- the fp32 one-hot rows (48 bytes per row of four 3-class
    // columns) are not written at all; the kernel takes the same path with a placeholder address it never stores to
    rq.enc_no32 = enc_out ? 0 : 1;
    rq.n_classes = n_classes; rq.enc_clamp = clamp; rq.enc_out = enc_out ? enc_out : reinterpret_cast<float *>(pack);
    rq.enc16 = pack; rq.enc16_stride = pack_stride; rq.enc16_col0 = pack_col0;
    if (int rc = pack_columns_check("gsn_count_encode_pack16_hip", rq)) return rc;
    return count_launch(rq, stream);
}

extern "C" int gsn_count_encode_pack16_side_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                                const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                                int64_t edge_row_stride, int ids_are_global, int64_t max_nodes, int64_t max_edges, int64_t *out,
                                                int32_t *status, const int32_t *n_classes, int clamp, uint16_t *pack, int64_t pack_stride,
                                                int64_t pack_col0, const gsn_count_side *side, void *stream) {
    if (!side) return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: side is null");
    if (!out) return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: the int64 counts are always written (out is null)");
    CountRequest rq;
    rq.plan_host = plan_host; rq.plan_dev = plan_dev; rq.plan_words = plan_words; rq.n_graphs = n_graphs; rq.node_ptr = node_ptr; rq.edge_ptr = edge_ptr;
    rq.edge_index = edge_index; rq.edge_row_stride = edge_row_stride; rq.ids_are_global = ids_are_global; rq.max_nodes = max_nodes; rq.max_edges = max_edges;
    rq.out = out; rq.status = status;
    rq.n_items = n_graphs; rq.side = side;
    if (!pack) return count_launch(rq, stream);     // (no identifier pack: plain counts + the CSR / node pack; edge codes need the pack and are refused by the planner)
    rq.n_classes = n_classes; rq.enc_clamp = clamp; rq.enc_out = reinterpret_cast<float *>(pack); rq.enc_no32 = 1;
    rq.enc16 = pack; rq.enc16_stride = pack_stride; rq.enc16_col0 = pack_col0;
    if (int rc = pack_columns_check("gsn_count_encode_pack16_side_hip", rq)) return rc;
    return count_launch(rq, stream);
}

extern "C" int gsn_count_encode_keys_side_hip(const uint32_t *plan_host, const uint32_t *plan_dev, int64_t plan_words, int64_t n_graphs,
                                              const int64_t *node_ptr, const int64_t *edge_ptr, const int64_t *edge_index,
                                              int64_t edge_row_stride, int ids_are_global, int64_t max_nodes, int64_t max_edges, int64_t *out,
                                              int32_t *status, const int32_t *n_classes, int clamp, int64_t pack_col0, const gsn_count_side *side,
                                              const gsn_count_keys *keys, void *stream) {
    if (!side || !keys || !keys->idmask) return set_error(GSN_E_INVALID, "gsn_count_encode_keys_side_hip: side / keys / keys->idmask is null");
    if (!out) return set_error(GSN_E_INVALID, "gsn_count_encode_keys_side_hip: the int64 counts are always written (out is null)");
    CountRequest rq;
    rq.plan_host = plan_host; rq.plan_dev = plan_dev; rq.plan_words = plan_words; rq.n_graphs = n_graphs; rq.node_ptr = node_ptr; rq.edge_ptr = edge_ptr;
    rq.edge_index = edge_index; rq.edge_row_stride = edge_row_stride; rq.ids_are_global = ids_are_global; rq.max_nodes = max_nodes; rq.max_edges = max_edges;
    rq.out = out; rq.status = status;
    rq.n_items = n_graphs; rq.side = side; rq.keys = keys;
    // (no fp32 rows and no pack: the identifier masks are the only form of the encoded rows; enc_out is a placeholder that is never written)
    rq.n_classes = n_classes; rq.enc_clamp = clamp; rq.enc_out = reinterpret_cast<float *>(keys->idmask); rq.enc_no32 = 1;
    rq.enc16_stride = 16; rq.enc16_col0 = pack_col0;
    return count_launch(rq, stream);
}
