// The kernel-argument block of the counting kernels (count.hip), as plain C++ (no HIP include): the launch planner (count_plan.cpp) fills
// it on the host, tests/count_plan_harness.cpp reads it back without a GPU, and the kernels read it from the kernel-argument segment.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gsn {

constexpr int GSN_ENC_MAX_COLS = 64;

// What gsn_count_encode_pack16_side_hip adds to a counting launch (r06): the target-sorted CSR of the batch's columns, the node pack from
// integer node codes, the edge codes' one-hot columns of the edge pack.  They are made by SIDE WORKGROUPS of the same launch (count.hip:
// side_block), every (SIDE_EVERY + 1)-th workgroup of the grid; the counting workgroups run count_body exactly as without them.
// gsn_count_encode_keys_side_hip: the same launch leaving COMPACT outputs in place of the packs -- a key byte per vertex and a key word per sorted
// column from the side workgroups, a 16-bit mask of the identifier classes per column from the counting workgroups (include/gsn_abi.h: gsn_count_keys).
struct SideArgs {
    int32_t *csr_seg, *csr_perm, *csr_tgt, *csr_oth;   // csr_seg == null: no CSR
    int64_t tot_nodes, tot_edges;
    const int64_t *ncode;      // node codes [tot_nodes][ncode_cols] or null
    uint16_t *npack;           // fp16 [tot_nodes][32]
    const int64_t *ecode;      // edge codes [tot_edges][ecode_cols] or null
    uint16_t *epack;           // fp16 [tot_edges][16]: columns ecode_col0 .. 15 are written
    int32_t *code_status;      // or null
    int csr_row;               // the row of edge_index that is the aggregation target
    int ncode_cols, ncode_clamp, ecode_cols, ecode_clamp, ecode_col0;
    unsigned ncode_ptr_w[2], ecode_ptr_w[2];    // first pack column of every code column's classes, one BYTE per column + the end (prefix sums; the
                                                // edge codes' start at ecode_col0) -- as words: byte-sized kernel arguments are vector loads on gfx9
    // compact outputs (gsn_count_encode_keys_side_hip): what layer 0 reads in place of the two packs
    uint8_t *nkey;             // [tot_nodes] or null: row of the vertex in the node dictionary = the mixed-radix number of its code digits, column 0
                               // most significant; without clamp every column has one digit more, "none" (a code outside its classes: zero segment)
    uint32_t *ekeys;           // [tot_edges] or null, target-sorted order: nkey[target] | nkey[other] << 8 | edge-code class mask << 16
    unsigned nkey_radix_w;     // digits per node code column, one byte per column
};
#ifndef GSN_SIDE_EVERY
#define GSN_SIDE_EVERY 4
#endif
constexpr int SIDE_EVERY = GSN_SIDE_EVERY;  // counting workgroups per side workgroup (A/B: 2: +0.0xx, 8: see profiles/r06_count_side_ab.txt; at 8 waves per SIMD 8 loses 0.017 ms: profiles/count_cycle_occupancy.txt)

struct CountArgs {
    const uint32_t *plan;      // device
    int plan_words;
    int mode, n_cols, n_plans, plans_off, kmax;
    const int64_t *node_ptr, *edge_ptr, *src, *dst;
    int ids_are_global;
    const int32_t *graph_ids;  // or null
    int n_cap, e_cap;          // LDS capacities (rows of A, columns)
    int last_cap;              // entries of last[] (edge mode): the slots of the CSR rank a workgroup may address, >= e_cap
    int n_decl, e_decl;        // the caller's max_nodes / max_edges: a single graph beyond them is reported (GSN_ST_TOO_LARGE)
    int stack_skip;            // frames of the candidate stack that are never addressed (the smallest n_fixed of the plans)
    int pair;                  // 1: a workgroup takes the graphs 2 i, 2 i + 1 -- as ONE graph, their disjoint union, when that fits n_cap / e_cap
    int n_graphs;
    int stage_out;             // 1: output rows staged in LDS then written coalesced
    int sym;                   // edge mode with undirected orbit classes: rows (u,v) and (v,u) are equal -> search once
    int split;                 // workgroups per graph (each takes a contiguous slice of the (column,row) task space)
    int64_t *out;
    int32_t *status;
    // LDS byte offsets
    int off_valid, off_stack, off_plan, off_eu, off_ev, off_rowstart, off_last, off_out, off_misc;
    int off_prim, off_revof;   // edge mode: the rows that run searches, in column order; per column the last column of the reverse pair
    int off_ball;              // distance-pruning tables (radius 2, radius 3: n_cap rows each) or -1
    int off_degp;              // degree bit planes of the cores, [CORE_MAX + 1][DEG_PLANES][W] words (plans with a chain tail), or -1
    int degp_mask;             // bit d: some chain-tail plan lives in the d-core
    int any_tail;              // some plan ends in a closed form (plan_tail != 0)
    int tail_loop;             // graphs of <= 64 vertices: the last two levels in the tight loop too (dense graphs; GSN_COUNT_TAIL_LOOP)
    int off_core;              // d-cores of the graph, d = 0 .. CORE_MAX (W words each)
    int core_mask;             // bit d: some plan needs the d-core
    int off_ain;               // directed plans: the in-neighbour bit matrix
    int stride;                // words per plan (plan_stride)
    int pull_batch;            // idle lanes that wait before the pool's pull arm runs (1: every trip; GSN_PULL_BATCH)
    int zero_status;           // 1: a workgroup owns its graphs' status words (no split, no graph list) and zeroes them itself -- no memset launch in front
    // fused identifier encoding (gsn_count_encode_hip): column c of a finished cell also / instead leaves as n_classes[c] floats
    // with a single 1 (utils_graph_learning.one_hot_encoder, :170-187) -- the int64 round trip through HBM and the one-hot launch go
    unsigned short enc_n[GSN_ENC_MAX_COLS];   // n_classes per output column (blocks in column order)
    float *enc_out;            // [rows_total][enc_width] or null
    int enc_width, enc_clamp, off_enc;
    int enc_stage;             // 1: cells leave their class index in an LDS byte array, the rows are expanded and written coalesced at the end
    int off_encst;             // that array: [rows_cap][n_cols] bytes, 0xff = no class (count out of range, unclamped)
    int enc_from_counts;       // 1: no byte array -- the staged 16-bit counts (stage_out) give the class indices at the end (LDS per workgroup: occupancy)
    uint16_t *enc16;           // the same rows as fp16 into a column range of an exact row pack (gsn_count_encode_pack16_hip), or null; staged rows only
    int enc_no32;              // 1: the fp16 pack columns are the ONLY form of the encoded rows (enc_out is a placeholder that is never written)
    int enc16_stride, enc16_col0;
    int side_mask;             // bit 0: CSR, bit 1: node pack, bit 2: edge codes; != 0: the grid holds side workgroups
    int n_items;               // counting work items of the launch (graphs, or pairs of graphs)
    int lds_bytes;             // dynamic LDS of the launch (a side workgroup sorts as many graphs at a time as fit there)
    unsigned cyc_len;          // cycle instantiation: the cycle length of output column c in byte c (count_core.h: cycle_plan_lengths)
    uint16_t *idmask;          // [rows_total] or null: bit enc16_col0 + (first column of c's classes) + class of every column c of a row -- the hot pack
                               // columns of the row as a bit mask, from the staged class indices (phase 4')
    SideArgs side;
};
// the kernels find `side` by its offset in the kernel-argument segment (count.hip: side_late); host and device compile must agree on both
static_assert(sizeof(CountArgs) == 592 && offsetof(CountArgs, side) == 440, "CountArgs layout changed: host and device read the same bytes");

}  // namespace gsn
