// Arithmetic of the PADDED batch collate (gsn_loader_collate_padded_hip in loader.hip), shared with the host-side logic harness used ONLY by
// tests (tests/padded_harness.cpp compiles this header with g++; it is not a product fallback).
//
// A padded batch has fixed capacities: N_cap vertices, E_cap edge columns, G_cap graph slots.  Slots [0, b) hold the real graphs, laid out
// as loader_core.h lays out an unpadded batch; the S = G_cap - b slots behind them hold PAD GRAPHS that use up what is left:
//   r_n = N_cap - N_r - S spare vertices beyond the one every pad graph has, r_e = E_cap - E_r spare edge columns;
//   pad graph k has 1 + min(n_chunk - 1, max(0, r_n - k (n_chunk - 1))) vertices and min(e_chunk, max(0, r_e - k e_chunk)) edge columns,
// so it begins at vertex N_r + k + min(r_n, k (n_chunk - 1)) and at column E_r + min(r_e, k e_chunk): closed forms, no scan.  Its edge column
// t is the self loop of its vertex t mod v; its rows of every other field are the field's fill word.  Every offset is int64.
#pragma once

#include "loader_core.h"

namespace gsn {

LD_HD int64_t lp_min(int64_t a, int64_t b) { return a < b ? a : b; }

LD_HD int64_t lp_pad_slots(const gsn_loader_pad &p) { return p.graph_slots - p.n_real; }
LD_HD int64_t lp_spare_nodes(const gsn_loader_pad &p) { return p.node_capacity - p.n_real_nodes - lp_pad_slots(p); }
LD_HD int64_t lp_spare_edges(const gsn_loader_pad &p) { return p.edge_capacity - p.n_real_edges; }

// the batch fits its capacities and the pad slots can take up every spare row (lp_node_start(S) == N_cap, lp_edge_start(S) == E_cap)
LD_HD bool lp_fits(const gsn_loader_pad &p) {
    if (p.n_real < 1 || p.n_real >= p.graph_slots || p.n_real_nodes < 0 || p.n_real_edges < 0 || p.n_chunk < 2 || p.e_chunk < 1) return false;
    const int64_t S = lp_pad_slots(p), rn = lp_spare_nodes(p), re = lp_spare_edges(p);
    if (rn < 0 || re < 0) return false;
    // (divisions: S * chunk could pass 2^63 with capacities that are themselves in range)
    return (rn + p.n_chunk - 2) / (p.n_chunk - 1) <= S && (re + p.e_chunk - 1) / p.e_chunk <= S;
}

// first vertex / edge column of pad graph k; k = S gives the capacities
LD_HD int64_t lp_node_start(const gsn_loader_pad &p, int64_t k) {
    const int64_t rn = lp_spare_nodes(p), c = p.n_chunk - 1;
    return p.n_real_nodes + k + (k >= (rn + c - 1) / c ? rn : k * c);
}
LD_HD int64_t lp_edge_start(const gsn_loader_pad &p, int64_t k) {
    const int64_t re = lp_spare_edges(p), c = p.e_chunk;
    return p.n_real_edges + (k >= (re + c - 1) / c ? re : k * c);
}

template <class T> LD_HD void lp_fill_lane(T *dst, int64_t n, T value, int lane) {
    for (int64_t i = lane; i < n; i += LD_WAVE) dst[i] = value;
}
// columns [0, n) of one row of a pad graph's edge_index: column t names vertex v0 + t mod nv (t mod nv kept by addition: one division per lane)
LD_HD void lp_loop_lane(int64_t *dst, int64_t n, int64_t v0, int64_t nv, int lane) {
    int64_t m = lane % nv;
    const int64_t step = LD_WAVE % nv;
    for (int64_t i = lane; i < n; i += LD_WAVE) {
        dst[i] = v0 + m;
        m += step;
        if (m >= nv) m -= nv;
    }
}

// What lane `lane` of the wave that owns (field f, pad slot) does: the slot's rows of the field, and for the vertex field (`x`) / the
// edge_index field the slot's batch_vec entries and pointer entry -- the last slot also the closing pointer entry.
LD_HD void lp_run_pad(const gsn_loader_field &f, uint64_t fill, const gsn_loader_pad &p, int64_t slot, int lane, int64_t *batch_vec,
                      int64_t *node_ptr_out, int64_t *edge_ptr_out) {
    const int64_t k = slot - p.n_real;
    const int64_t v0 = lp_node_start(p, k), nv = lp_node_start(p, k + 1) - v0;
    const int64_t e0 = lp_edge_start(p, k), ne = lp_edge_start(p, k + 1) - e0;
    const bool last = slot == p.graph_slots - 1;
    if (f.kind == GSN_LOADER_EDGE_INDEX) {
        if (ne > 0 && f.dst_rows > 0) {
            int64_t *dst = static_cast<int64_t *>(f.dst);
            for (int r = 0; r < 2; ++r) lp_loop_lane(dst + (int64_t)r * f.dst_stride + e0, ne, v0, nv, lane);
        }
        if (edge_ptr_out && lane == 0) {
            edge_ptr_out[slot] = e0;
            if (last) edge_ptr_out[p.graph_slots] = e0 + ne;
        }
        return;
    }
    int64_t r0 = v0, nr = nv;
    if (f.flags & GSN_LOADER_F_PAD_GRAPH) { r0 = slot; nr = 1; }
    else if (f.flags & GSN_LOADER_F_PAD_EDGES) { r0 = e0; nr = ne; }
    const int64_t n = nr * ld_row_elems(f.row_bytes, f.elem_bytes), d0 = r0 * ld_row_elems(f.row_bytes, f.elem_bytes);
    if (n > 0 && f.dst_rows > 0) {
        if (f.elem_bytes == 8) lp_fill_lane(static_cast<uint64_t *>(f.dst) + d0, n, fill, lane);
        else lp_fill_lane(static_cast<uint32_t *>(f.dst) + d0, n, (uint32_t)fill, lane);
    }
    if (f.flags & GSN_LOADER_F_NODES) {
        if (batch_vec) ld_fill_lane(batch_vec + v0, nv, slot, lane);
        if (node_ptr_out && lane == 0) {
            node_ptr_out[slot] = v0;
            if (last) node_ptr_out[p.graph_slots] = v0 + nv;
        }
    }
}

// One (field, slot) pair of a padded batch.  Real slots are ld_run_pair's (told a batch of G_cap slots: the closing pointer entries belong
// to the last PAD slot, and there always is one); n_valid belongs to slot 0 of the vertex field.  With lp_fits and fields whose dst_rows
// are the capacities, every byte of every output has exactly one writer.
LD_HD void lp_run_pair(const gsn_loader_field &f, uint64_t fill, const gsn_loader_pad &p, const int64_t *order, const int64_t *plan, int64_t stride,
                       int64_t first, int64_t slot, int lane, int64_t *batch_vec, int64_t *node_ptr_out, int64_t *edge_ptr_out, int64_t *n_valid) {
    if (slot < p.n_real) ld_run_pair(f, order, plan, stride, first, p.graph_slots, slot, lane, batch_vec, node_ptr_out, edge_ptr_out);
    else lp_run_pad(f, fill, p, slot, lane, batch_vec, node_ptr_out, edge_ptr_out);
    if ((f.flags & GSN_LOADER_F_NODES) && slot == 0 && lane == 0 && n_valid) *n_valid = p.n_real;
}

}  // namespace gsn
