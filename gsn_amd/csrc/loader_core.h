// Address arithmetic of the batch collate, shared between the HIP kernel (loader.hip) and a host-side logic harness used ONLY by tests
// (tests/loader_harness.cpp compiles this header with g++; it is not a product fallback):
//   * which (field, slot) a pair number stands for,
//   * a slot's source segment and destination row (row pointer, epoch order, epoch plan),
//   * the element range a lane walks and the offsets of the two rows of an edge_index segment,
//   * the increment of an edge_index segment,
// and the per-lane routine that moves one pair with them.  Every offset is int64: a field of a large dataset passes 2^32 bytes.
#pragma once

#include <stdint.h>

#include "../../include/gsn_abi.h"

#if defined(__HIPCC__)
#define LD_HD __host__ __device__ __forceinline__
#else
#define LD_HD inline
#endif

namespace gsn {

constexpr int LD_WAVE = 64;                    // lanes that share a pair
constexpr int LD_WAVES_PER_BLOCK = 4;

// pairs are numbered field-major: consecutive waves take consecutive slots of ONE field, so their destinations are adjacent
LD_HD void ld_pair_of(int64_t pair, int64_t batch, int *field, int64_t *slot) {
    *field = (int)(pair / batch);
    *slot = pair - (int64_t)(*field) * batch;
}

LD_HD int64_t ld_plan_at(const int64_t *plan, int64_t stride, int cls, int64_t pos) { return plan[(int64_t)cls * stride + pos]; }

struct LdSeg {
    int64_t src_row;      // first row of the graph in the field's storage
    int64_t n_rows;
    int64_t dst_row;      // first row of the graph in the batch's output
};

LD_HD LdSeg ld_segment(const int64_t *row_ptr, const int64_t *order, const int64_t *plan, int64_t stride, int cls, int64_t pos) {
    const int64_t g = order[pos];
    LdSeg s;
    s.src_row = row_ptr[g];
    s.n_rows = row_ptr[g + 1] - s.src_row;
    s.dst_row = ld_plan_at(plan, stride, cls, pos);
    return s;
}

// the segment lies inside a destination of dst_rows rows (a loader's own tables always do: see gsn_abi.h)
LD_HD bool ld_fits(const LdSeg &s, int64_t dst_rows) { return s.n_rows >= 0 && s.dst_row >= 0 && s.n_rows <= dst_rows - s.dst_row; }

// GSN_LOADER_COPY, in units of elem_bytes: [src_elem, src_elem + n_elems) -> [dst_elem, ..)
LD_HD int64_t ld_row_elems(int64_t row_bytes, int elem_bytes) { return row_bytes / elem_bytes; }
LD_HD int64_t ld_copy_elems(const LdSeg &s, int64_t row_bytes, int elem_bytes) { return s.n_rows * ld_row_elems(row_bytes, elem_bytes); }
LD_HD int64_t ld_copy_src_elem(const LdSeg &s, int64_t row_bytes, int elem_bytes) { return s.src_row * ld_row_elems(row_bytes, elem_bytes); }
LD_HD int64_t ld_copy_dst_elem(const LdSeg &s, int64_t row_bytes, int elem_bytes) { return s.dst_row * ld_row_elems(row_bytes, elem_bytes); }

// GSN_LOADER_EDGE_INDEX: row r (0: sources, 1: targets) of the segment, in int64 elements
LD_HD int64_t ld_edge_src_elem(const LdSeg &s, int r, int64_t src_stride) { return (int64_t)r * src_stride + s.src_row; }
LD_HD int64_t ld_edge_dst_elem(const LdSeg &s, int r, int64_t dst_stride) { return (int64_t)r * dst_stride + s.dst_row; }

// elements lane, lane + LD_WAVE, .. of [0, n): consecutive lanes touch consecutive elements
template <class T> LD_HD void ld_copy_lane(const T *src, T *dst, int64_t n, int lane) {
    for (int64_t i = lane; i < n; i += LD_WAVE) dst[i] = src[i];
}
LD_HD void ld_add_lane(const int64_t *src, int64_t *dst, int64_t n, int64_t inc, int lane) {
    for (int64_t i = lane; i < n; i += LD_WAVE) dst[i] = src[i] + inc;
}
LD_HD void ld_fill_lane(int64_t *dst, int64_t n, int64_t value, int lane) {
    for (int64_t i = lane; i < n; i += LD_WAVE) dst[i] = value;
}

// What lane `lane` of the wave that owns (field f, slot) does.  Every byte of every output has one writer: the rows of a slot belong to its
// pair, pointer entry `slot` to the pair of the vertex / edge_index field, entry `batch` to that field's last slot.
LD_HD void ld_run_pair(const gsn_loader_field &f, const int64_t *order, const int64_t *plan, int64_t stride, int64_t first, int64_t batch,
                       int64_t slot, int lane, int64_t *batch_vec, int64_t *node_ptr_out, int64_t *edge_ptr_out) {
    const int64_t pos = first + slot;
    const LdSeg s = ld_segment(f.row_ptr, order, plan, stride, f.ptr_class, pos);
    const bool move = f.dst_rows > 0 && ld_fits(s, f.dst_rows);
    int64_t *ptr_out = nullptr;
    if (f.kind == GSN_LOADER_EDGE_INDEX) {
        ptr_out = edge_ptr_out;
        if (move) {
            const int64_t inc = ld_plan_at(plan, stride, f.inc_class, pos);
            const int64_t *src = static_cast<const int64_t *>(f.src);
            int64_t *dst = static_cast<int64_t *>(f.dst);
            for (int r = 0; r < 2; ++r)
                ld_add_lane(src + ld_edge_src_elem(s, r, f.src_stride), dst + ld_edge_dst_elem(s, r, f.dst_stride), s.n_rows, inc, lane);
        }
    } else {
        if (move) {
            const int64_t n = ld_copy_elems(s, f.row_bytes, f.elem_bytes);
            const int64_t so = ld_copy_src_elem(s, f.row_bytes, f.elem_bytes), d0 = ld_copy_dst_elem(s, f.row_bytes, f.elem_bytes);
            if (f.elem_bytes == 8)
                ld_copy_lane(static_cast<const uint64_t *>(f.src) + so, static_cast<uint64_t *>(f.dst) + d0, n, lane);
            else
                ld_copy_lane(static_cast<const uint32_t *>(f.src) + so, static_cast<uint32_t *>(f.dst) + d0, n, lane);
        }
        if (f.flags & GSN_LOADER_F_NODES) {
            ptr_out = node_ptr_out;
            if (move && batch_vec) ld_fill_lane(batch_vec + s.dst_row, s.n_rows, slot, lane);
        }
    }
    if (ptr_out && lane == 0) {
        ptr_out[slot] = s.dst_row;
        if (slot == batch - 1) ptr_out[batch] = s.dst_row + s.n_rows;
    }
}

}  // namespace gsn
