// The counting launch planner (count_plan.h): host arithmetic only.
#include "count_plan.h"

#include "count_core.h"

namespace gsn {

CountSwitches CountSwitches::read() {
    CountSwitches s;
    const int pull_env = sw_int(SW_PULL_BATCH, 8);
    s.pull_batch = pull_env < 1 ? 1 : (pull_env > 64 ? 64 : pull_env);
    s.pair = sw_on(SW_COUNT_PAIR, true);
    s.tail_loop = sw_int(SW_COUNT_TAIL_LOOP, -1);
    s.mol = sw_on(SW_COUNT_MOL, true);
    s.cycle = sw_on(SW_COUNT_CYCLE, true) && s.mol;
    const int64_t split_target_env = sw_int64(SW_COUNT_SPLIT_TARGET, 0);
    s.split_target = split_target_env > 0 ? split_target_env : 2048;
    s.enc_bytes = sw_present(SW_COUNT_ENC_BYTES);     // (A/B: keep the byte array beside staged counts)
    return s;
}

namespace {

inline int align_up(int x, int a) { return (x + a - 1) / a * a; }

// The plan under construction: the steps in the order count_plan runs them, and what they hand to each other.
struct Planner {
    const CountRequest &rq;
    const CountSwitches &sw;
    CountLaunchPlan &p;
    CountArgs &a;
    int64_t n_items = 0;
    int64_t max_nodes = 0, max_edges = 0;      // the caller's capacities; from route_size on, of what a workgroup holds: a graph, or the union of two
    int64_t rows_cap = 0, rows_cap_u = 0;      // output rows of a graph by the caller's capacities / of what a workgroup holds
    int64_t enc_width = 0;
    bool enc_bytes = true;                     // every class index fits a byte (0xff = none)
    bool directed = false, edge_mode = false, pair = false, cyc = false;
    int W = 0, T = 0;
    int o = 0;                                 // running end of the LDS layout
    const uint32_t *plan_word(int i) const { return rq.plan_host + a.plans_off + (int64_t)i * a.stride; }

    int validate_request();
    int fill_request();
    int side_node_codes();
    int side_edge_codes();
    int side_and_keys();
    void route_size();
    void route_tails();
    int lds_layout();
    void staging_and_split();
    int check_layout();
    void size_grid();
    CountKernel choose_kernel() const;
};

// The request: a narrow plan table, the pointers every launch needs, graphs of at most 768 vertices.  n_items <= 0 is not an error:
// the plan's grid stays 0.
int Planner::validate_request() {
    if (rq.plan_host && rq.plan_words >= PLAN_HEADER_WORDS && rq.plan_host[0] == PLAN_MAGIC_WIDE) return set_error(GSN_E_UNSUPPORTED, GSN_WIDE_PLAN_REFUSAL);
    if (!rq.plan_host || !rq.plan_dev || rq.plan_words < PLAN_HEADER_WORDS || rq.plan_host[0] != PLAN_MAGIC)
        return set_error(GSN_E_INVALID, "gsn_count_hip: not a plan table (build it with gsn_count_plan_build)");
    if (!rq.node_ptr || !rq.edge_ptr || (!rq.out && !rq.enc_out) || !rq.status) return set_error(GSN_E_INVALID, "gsn_count_hip: null pointer argument");
    if (rq.enc_out && !rq.n_classes) return set_error(GSN_E_INVALID, "gsn_count_encode_hip: n_classes is null");
    n_items = rq.graph_ids ? rq.n_items : rq.n_graphs;
    if (n_items <= 0) return GSN_OK;
    if (rq.max_nodes > 768)
        return set_error(GSN_E_UNSUPPORTED, "graphs with more than 768 vertices (%lld) are outside this build", (long long)rq.max_nodes);
    max_nodes = rq.max_nodes < 1 ? 1 : rq.max_nodes;
    max_edges = rq.max_edges < 0 ? 0 : rq.max_edges;
    return GSN_OK;
}

// The plan table's header and the request's pointers into the argument block; the widths of the encoded rows.
int Planner::fill_request() {
    const uint32_t *plan_host = rq.plan_host;
    a.plan = rq.plan_dev; a.plan_words = (int)rq.plan_words;
    a.mode = (int)plan_host[1]; a.n_plans = (int)plan_host[3]; a.n_cols = (int)plan_host[4]; a.kmax = (int)plan_host[5];
    a.plans_off = (int)plan_host[7];
    a.sym = (a.mode == GSN_MODE_EDGE && (plan_host[6] & 1u) == 0) ? 1 : 0;
    directed = (plan_host[6] & 2u) != 0;
    edge_mode = a.mode == GSN_MODE_EDGE;
    a.stride = plan_stride(plan_host[6]);
    a.pull_batch = sw.pull_batch;
    if (directed && a.mode != GSN_MODE_VERTEX) return set_error(GSN_E_UNSUPPORTED, "gsn_count_hip: directed plans are vertex-mode plans");
    a.node_ptr = rq.node_ptr; a.edge_ptr = rq.edge_ptr;
    a.src = rq.edge_index; a.dst = rq.edge_index ? rq.edge_index + rq.edge_row_stride : nullptr;
    a.ids_are_global = rq.ids_are_global; a.graph_ids = rq.graph_ids;
    a.out = rq.out; a.status = rq.status;
    a.enc_out = rq.enc_out; a.enc_width = 0; a.enc_clamp = rq.enc_clamp;
    if (rq.enc_out) {
        if (a.n_cols > GSN_ENC_MAX_COLS)
            return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_hip: %d output columns; the fused encoding handles <= %d", a.n_cols, GSN_ENC_MAX_COLS);
        for (int c = 0; c < a.n_cols; ++c) {
            if (rq.n_classes[c] < 1 || rq.n_classes[c] > 65535) return set_error(GSN_E_INVALID, "gsn_count_encode_hip: n_classes[%d] = %d", c, rq.n_classes[c]);
            a.enc_n[c] = (unsigned short)rq.n_classes[c];
            enc_width += rq.n_classes[c];
            enc_bytes = enc_bytes && rq.n_classes[c] <= 255;
        }
        a.enc_width = (int)enc_width;
    }
    if (max_edges > 0 && !rq.edge_index) return set_error(GSN_E_INVALID, "gsn_count_hip: edge_index is null");
    return GSN_OK;
}

// Side outputs, node codes: the first pack column of every code column's classes as prefix-sum bytes, and the radices of the node keys.
int Planner::side_node_codes() {
    const gsn_count_side *side = rq.side;
    const bool nk = rq.keys && rq.keys->nkey;          // (the node keys may stand in for the node pack)
    if ((side->node_pack ? (reinterpret_cast<uintptr_t>(side->node_pack) & 15) != 0 : !nk) || side->node_code_cols < 1 || side->node_code_cols > 4)
        return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: node pack (16-byte aligned) and 1..4 node code columns");
    int col = 0;
    int64_t dict_rows = 1;
    for (int c = 0; c < side->node_code_cols; ++c) {
        if (side->node_n_classes[c] < 1) return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: node_n_classes[%d] < 1", c);
        a.side.ncode_ptr_w[c >> 2] |= (unsigned)col << (8 * (c & 3)); col += side->node_n_classes[c];
        if (col > 28) return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: more than 28 encoded node columns");
        const int radix = side->node_n_classes[c] + (side->node_clamp ? 0 : 1);
        a.side.nkey_radix_w |= (unsigned)radix << (8 * c); dict_rows *= radix;
    }
    if (nk && dict_rows > 256)
        return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_keys_side_hip: a node dictionary of %lld rows (one byte per key: <= 256)", (long long)dict_rows);
    if (nk && side->node_pack)
        return set_error(GSN_E_INVALID, "gsn_count_encode_keys_side_hip: node keys stand in for the node pack (side->node_pack must be NULL)");
    a.side.nkey = nk ? rq.keys->nkey : nullptr;
    a.side.ncode_ptr_w[side->node_code_cols >> 2] |= (unsigned)col << (8 * (side->node_code_cols & 3));
    a.side_mask |= 2;
    a.side.ncode = side->node_codes; a.side.npack = side->node_pack; a.side.ncode_cols = side->node_code_cols; a.side.ncode_clamp = side->node_clamp ? 1 : 0;
    return GSN_OK;
}

// Side outputs, edge codes: at most 8 classes in a multiple-of-4 column behind the identifier columns of a 16-column edge pack (or of
// the edge keys, which stand in for it).
int Planner::side_edge_codes() {
    const gsn_count_side *side = rq.side;
    if ((rq.enc16 ? (rq.enc16_stride != 16 || (reinterpret_cast<uintptr_t>(rq.enc16) & 15)) : !(rq.keys && rq.keys->ekeys)) || side->edge_code_cols < 1 || side->edge_code_cols > 4)
        return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: edge codes need a 16-column, 16-byte-aligned edge pack and 1..4 code columns");
    if (side->edge_col0 < 0 || (side->edge_col0 & 3) || side->edge_col0 < rq.enc16_col0 + enc_width)
        return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: edge_col0 %d must be a multiple of 4 behind the identifier columns (%lld .. %lld)",
                         side->edge_col0, (long long)rq.enc16_col0, (long long)(rq.enc16_col0 + enc_width));
    int col = side->edge_col0;
    for (int c = 0; c < side->edge_code_cols; ++c) {
        if (side->edge_n_classes[c] < 1) return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: edge_n_classes[%d] < 1", c);
        a.side.ecode_ptr_w[c >> 2] |= (unsigned)col << (8 * (c & 3)); col += side->edge_n_classes[c];
    }
    a.side.ecode_ptr_w[side->edge_code_cols >> 2] |= (unsigned)col << (8 * (side->edge_code_cols & 3));
    if (col > 16 || col - side->edge_col0 > 8)
        return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: %d edge code classes at column %d (<= 8, inside the 16 columns)", col - side->edge_col0, side->edge_col0);
    a.side_mask |= 4;
    a.side.ecode = side->edge_codes; a.side.epack = rq.enc16; a.side.ecode_cols = side->edge_code_cols; a.side.ecode_clamp = side->edge_clamp ? 1 : 0;
    a.side.ecode_col0 = side->edge_col0;
    return GSN_OK;
}

// Side outputs (gsn_count_encode_pack16_side_hip) and compact outputs (gsn_count_encode_keys_side_hip): validated and packed here; the
// grid gets its side workgroups in size_grid.
int Planner::side_and_keys() {
    const gsn_count_side *side = rq.side;
    const gsn_count_keys *keys = rq.keys;
    if (side) {
        if (rq.graph_ids) return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_pack16_side_hip: a graph list (the side outputs cover every graph of the batch)");
        if (side->seg_ptr) {
            if ((max_edges > 0 && !side->perm) || side->n_nodes < 0 || side->n_edges < 0 || side->n_nodes >= ((int64_t)1 << 31) - 1 || side->n_edges >= (int64_t)1 << 31)
                return set_error(GSN_E_INVALID, "gsn_count_encode_pack16_side_hip: CSR outputs / totals");
            a.side_mask |= 1;
            a.side.csr_seg = side->seg_ptr; a.side.csr_perm = side->perm; a.side.csr_tgt = side->sorted_target; a.side.csr_oth = side->sorted_other;
        }
        a.side.csr_row = side->csr_row ? 1 : 0; a.side.tot_nodes = side->n_nodes; a.side.tot_edges = side->n_edges;
        if (side->node_codes) if (int rc = side_node_codes()) return rc;
        if (side->edge_codes) if (int rc = side_edge_codes()) return rc;
        a.side.code_status = side->code_status;
        if (keys && keys->ekeys) {
            if (!(a.side_mask & 1) || !side->sorted_target || !side->sorted_other)
                return set_error(GSN_E_INVALID, "gsn_count_encode_keys_side_hip: the edge keys are written with the CSR arrays (seg_ptr, perm, sorted_target, sorted_other)");
            a.side.ekeys = keys->ekeys;
        }
    }
    if (keys && keys->idmask) {
        if (directed) return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_keys_side_hip: directed plans (their instantiations carry no identifier masks)");
        if (!rq.enc_out || rq.enc16_col0 < 0 || rq.enc16_col0 + enc_width > 16)
            return set_error(GSN_E_INVALID, "gsn_count_encode_keys_side_hip: the identifier masks hold pack columns %lld .. %lld (<= 16) of an encoded launch", (long long)rq.enc16_col0,
                             (long long)(rq.enc16_col0 + enc_width));
        a.idmask = keys->idmask;
    }
    return GSN_OK;
}

// Word class W, block size T, and pairing.
void Planner::route_size() {
    W = max_nodes <= 64 ? 1 : (max_nodes <= 128 ? 2 : (max_nodes <= 256 ? 4 : (max_nodes <= 512 ? 8 : 12)));
    rows_cap = edge_mode ? max_edges : max_nodes;
    // large graphs (W > 4: 16-bit vertex ids, adjacency up to 72 KiB) keep one wave per workgroup so that the candidate
    // stack stays small; their parallelism comes from `split` workgroups per graph
    T = (rows_cap * a.n_cols <= 512 || W > 4) ? 64 : 256;
    a.n_decl = (int)max_nodes; a.e_decl = (int)max_edges;
    a.n_graphs = (int)rq.n_graphs;
    // Two consecutive graphs per workgroup, as one graph (count_body): whole batches of small graphs whose plans hold connected patterns
    // only (every enumerated level of every plan has an adjacency constraint); GSN_COUNT_PAIR=0 switches it off.
    const int64_t tasks_cap1 = rows_cap * a.n_cols;
    pair = !rq.graph_ids && rq.n_graphs >= 2 && W == 1 && T == 64 && !(n_items < 2048 && tasks_cap1 >= 1024);
    if (pair && !sw.pair) pair = false;
    for (int i = 0; pair && i < a.n_plans; ++i) {
        const uint32_t *w = plan_word(i);
        const int k = (int)(w[0] & 0xffu), nfix = (int)((w[0] >> 8) & 0xffu);
        for (int l = nfix; l < k; ++l) {
            const uint32_t adj = (w[2 + l] & 0xffu) | (directed ? (w[PLAN_STRIDE_WORDS + l] & 0xffu) : 0u);
            if (adj == 0) pair = false;
        }
    }
    a.pair = pair ? 1 : 0;
    if (pair) {
        max_nodes = 2 * max_nodes < 64 ? 2 * max_nodes : 64;
        max_edges = 2 * max_edges;
    }
    rows_cap_u = edge_mode ? max_edges : max_nodes;      // (of what a workgroup holds: a graph, or the union of two)
    a.n_cap = (int)max_nodes; a.e_cap = (int)max_edges;
}

// Closed-form tails, the tail loop and the cycle walk.
void Planner::route_tails() {
    // degree planes only when a plan ends in a chain (patterns.cpp: plan_tail_mode == 3): cycles, cliques -- the molecule workloads -- do not
    a.off_degp = -1; a.degp_mask = 0; a.any_tail = 0;
    for (int i = 0; i < a.n_plans; ++i) {
        const uint32_t *w = plan_word(i);
        if (plan_tail(w)) a.any_tail = 1;
        if (plan_tail(w) == 3) a.degp_mask |= 1 << plan_core(w);
    }
    // one-word graphs: the tight loop over the images of level k - 2 pays where those sets are long -- dense graphs (average degree >= 8 by
    // the caller's capacities: clique-rich ego networks 1.81 -> 0.96 ms per 1000, 12-regular n = 25 +5 %), not molecules (ZINC 0.073 ->
    // 0.082 ms with it).  GSN_COUNT_TAIL_LOOP=0 / 1 forces it off / on.
    a.tail_loop = 0;
    if (W == 1) a.tail_loop = sw.tail_loop >= 0 ? (sw.tail_loop != 0) : ((int64_t)a.e_decl >= 8 * (int64_t)a.n_decl);     // (the caller's capacities, before pairing)
    // Cycle columns (count_core.h: cycle_plan_lengths / cycle_walk): a launch that meets the molecule instantiation's conditions
    // (count_molecule_route) and whose four columns are all non-induced cycles of length <= 6 counts by path walks -- no candidate stack, plan
    // table or distance tables in its LDS.  Longer cycles (7, 8) keep the interpreter.  GSN_COUNT_CYCLE=0 sends such a launch down the interpreter.
    a.cyc_len = 0;
    if (W == 1 && T == 64 && pair && edge_mode && a.sym && !directed && a.n_cols == 4 && rq.enc_out && enc_bytes && !a.any_tail && !a.tail_loop) {
        uint8_t len[4];
        const int lmax = sw.cycle ? cycle_plan_lengths(rq.plan_host, rq.plan_words, len, 4) : 0;
        if (lmax >= 3 && lmax <= 6) a.cyc_len = (unsigned)len[0] | ((unsigned)len[1] << 8) | ((unsigned)len[2] << 16) | ((unsigned)len[3] << 24);
    }
    cyc = a.cyc_len != 0;
}

// The LDS layout up to the output rows: adjacency, candidate stack, plan table, the edge-mode column tables, cores, distance tables, degree planes.
int Planner::lds_layout() {
    o = align_up((int)max_nodes * W * 8, 16);
    a.off_ain = -1;
    if (directed) { a.off_ain = o; o += align_up((int)max_nodes * W * 8, 16); }
    a.off_valid = o; o += align_up(W * 8, 16);
    // candidate stack: one frame per enumerated level below the last (levels n_fixed .. k - 2; .. k - 3 for W >= 2); the frames of the root levels are
    // never touched, so the array starts at the smallest n_fixed of the plans (stack_skip frames in front of it do not exist)
    int nfix_min = 255;
    for (int i = 0; i < a.n_plans; ++i) { const int nf = (int)((plan_word(i)[0] >> 8) & 0xffu); nfix_min = nf < nfix_min ? nf : nfix_min; }
    if (nfix_min > a.kmax - 1 || a.n_plans == 0) nfix_min = 0;
    a.stack_skip = nfix_min;
    // (W >= 2: levels k - 2 and k - 1 never get a frame -- count_core.h counts them in closed form or in tail_loop)
    const int last_frame = W >= 2 ? a.kmax - 2 : a.kmax - 1;
    const int depth = last_frame - nfix_min > 1 ? last_frame - nfix_min : 1;
    a.off_stack = o; o += cyc ? 0 : depth * W * T * 8;
    a.off_plan = o; o += cyc ? 0 : align_up((int)rq.plan_words * 4, 16);
    const int vid_bytes = W > 4 ? 2 : 1;
    a.off_eu = o; o += edge_mode ? align_up((int)max_edges * vid_bytes, 16) : 0;
    a.off_ev = o; o += edge_mode ? align_up((int)max_edges * vid_bytes, 16) : 0;
    a.off_rowstart = o; o += edge_mode ? align_up(((int)max_nodes + 1) * (W == 1 ? 2 : 4), 16) : 0;
    // last[] holds one entry per SLOT of the CSR rank (two per undirected pair): a single graph has at most min(2 e_decl, n_decl (n_decl - 1)) of
    // them, which a pair's 2 e_decl columns already cover; a pair with more is redone graph by graph (count_body, phase 2)
    {
        const int64_t one = 2 * (int64_t)a.e_decl < (int64_t)a.n_decl * (a.n_decl - 1) ? 2 * (int64_t)a.e_decl : (int64_t)a.n_decl * (a.n_decl - 1);
        a.last_cap = (int)(one > max_edges ? one : max_edges);
    }
    a.off_last = o; o += edge_mode ? align_up(a.last_cap * 4, 16) : 0;
    if (edge_mode && max_edges >= 65535) return set_error(GSN_E_UNSUPPORTED, "gsn_count_hip: %lld columns per workgroup (16-bit column tables; LDS ends far earlier)", (long long)max_edges);
    a.off_prim = o; o += edge_mode ? align_up((int)max_edges * 2, 16) : 0;
    a.off_revof = o; o += edge_mode ? align_up((int)max_edges * 2, 16) : 0;
    a.off_misc = o; o += 32;
    a.off_enc = o; o += rq.enc_out ? align_up(2 * a.n_cols * 4, 16) : 0;
    a.off_core = o; o += align_up((CORE_MAX + 1) * W * 8, 16);
    a.core_mask = 0;
    for (int i = 0; i < a.n_plans; ++i) a.core_mask |= 1 << plan_core(plan_word(i));
    // pruning tables only for graphs of <= 64 vertices (molecules): on larger, denser targets the balls are (nearly)
    // everything and the extra AND per step costs more than it saves (measured: ER G(128,1000) +8 %)
    a.off_ball = -1;
    if (W == 1 && a.kmax >= 4 && !directed && !cyc) { a.off_ball = o; o += align_up(2 * (int)max_nodes * W * 8, 16); }
    if (a.degp_mask) { a.off_degp = o; o += align_up((CORE_MAX + 1) * DEG_PLANES * W * 8, 16); }
    a.off_out = o;
    return GSN_OK;
}

// Staged output rows, the split of few heavy graphs over several workgroups, and the form the encoded rows leave in.
void Planner::staging_and_split() {
    const int64_t stage_bytes = align_up((int)(rows_cap_u * a.n_cols * 2 < ((int64_t)1 << 28) ? rows_cap_u * a.n_cols * 2 : ((int64_t)1 << 28)), 16);      // (16-bit staged counts)
    // Stage the output rows in LDS (coalesced final write) only while that keeps the workgroup small: the search is
    // latency-bound on dependent LDS reads, so heavy graphs want as many co-resident workgroups per CU as possible
    // (>= 8 waves per SIMD) and write their cells straight to HBM instead.
    const int64_t lds_budget = (T == 64 ? (pair ? 160 * 1024 / 16 : 160 * 1024 / 32) : 160 * 1024 / 8);
    a.stage_out = (rq.out && o + stage_bytes <= lds_budget) ? 1 : 0;
    // few heavy graphs: several workgroups per graph so that every CU gets >= 8 of them
    a.split = 1;
    const int64_t tasks_cap = rows_cap * a.n_cols;
    if (!pair && n_items < sw.split_target && tasks_cap >= 1024) {
        int64_t sp = (sw.split_target + n_items - 1) / n_items;
        if (sp > 32) sp = 32;
        if (sp > tasks_cap / 256) sp = tasks_cap / 256;
        if (sp > 1) { a.split = (int)sp; a.stage_out = 0; }
    }
    if (a.stage_out) o += (int)stage_bytes;
    // class indices of the encoded rows: staged whenever one workgroup owns the whole graph and the indices fit a byte; else
    // every cell writes its floats itself
    a.enc_stage = 0; a.off_encst = o; a.enc_from_counts = 0;
    a.enc16 = rq.enc16; a.enc16_stride = (int)rq.enc16_stride; a.enc16_col0 = (int)rq.enc16_col0;
    a.enc_no32 = ((rq.enc16 || a.idmask) && rq.enc_no32) ? 1 : 0;
    if (rq.enc_out && a.split == 1 && enc_bytes && rows_cap_u * enc_width < (int64_t)1 << 24 && o + rows_cap_u * a.n_cols <= 150 * 1024) {
        a.enc_stage = 1;
        if (a.stage_out && !sw.enc_bytes) a.enc_from_counts = 1;      // the staged 16-bit counts hold what the class indices need: no second array
        else o += align_up((int)(rows_cap_u * a.n_cols), 16);         // (16-byte aligned: with four columns a row's indices are read as one word)
    }
}

// What the layout must still hold (a side workgroup's sort) and what the chosen modes rule out.
int Planner::check_layout() {
    if (a.side_mask) {
        if (a.split != 1)
            return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_pack16_side_hip: this launch splits a graph over %d workgroups (few heavy graphs): the side workgroups ride a "
                                                "one-workgroup-per-item grid; use gsn_csr_build_graphs_hip / gsn_one_hot_pack16_hip", a.split);
        // a side workgroup sorts a graph of the declared sizes in the launch's LDS (several at a time where they fit)
        const int64_t need = ((int64_t)a.n_decl + 1) * 8 + (int64_t)a.n_decl * 4 + (int64_t)a.e_decl * 7 + 16;
        if (a.n_decl >= 65535 || a.e_decl >= 65535 || need > 160 * 1024)
            return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_pack16_side_hip: graphs of %d vertices / %d columns do not sort in LDS (%lld B)", a.n_decl, a.e_decl, (long long)need);
        if (need > o) o = align_up((int)need, 16);
    }
    if (o > 160 * 1024) return set_error(GSN_E_UNSUPPORTED, "graph too large for LDS (%d B needed)", o);
    // (a pair of one-word graphs of <= 128 columns each: a few KiB, class indices in a byte -- always staged)
    if (cyc && !(a.enc_stage && a.split == 1)) return set_error(GSN_E_UNSUPPORTED, "gsn_count_hip: cycle launch without staged class indices (%d B of LDS)", o);
    if (a.idmask && !a.enc_stage)
        return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_keys_side_hip: the identifier masks are written from the staged class indices (one workgroup per graph, n_classes <= 255)");
    if (rq.enc16 && !a.enc_stage)
        return set_error(GSN_E_UNSUPPORTED, "gsn_count_encode_pack16_hip: the fp16 rows are written from the staged class indices (one workgroup per graph, "
                                            "n_classes <= 255); pack the fp32 rows with gsn_pack16_rows_hip instead");
    return GSN_OK;
}

// Status words and the grid.
void Planner::size_grid() {
    // per-graph status words start at OK; workgroups raise them with atomicMax.  One workgroup per graph (or pair) and every graph taken:
    // the workgroup zeroes its own words -- the memset was a 6 us launch (+ the gap behind it) in front of every counting launch
    a.zero_status = (!rq.graph_ids && a.split == 1) ? 1 : 0;
    p.memset_status = !a.zero_status;
    int items = pair ? (int)((rq.n_graphs + 1) / 2) : (int)n_items * a.split;
    a.n_items = items; a.lds_bytes = o;
    if (a.side_mask) items = (items + SIDE_EVERY - 1) / SIDE_EVERY * (SIDE_EVERY + 1);      // every (SIDE_EVERY + 1)-th workgroup is a side workgroup
    p.W = W; p.T = T; p.grid = items; p.lds_bytes = o;
}

// The instantiation.  TAIL: the one with the closed forms / the tight loop of the last two levels (count_core.h) -- graphs above 64 vertices
// (always: no second instantiation to compile), or a plan that ends in a closed form; the molecule workloads with cycle / clique patterns
// run the instantiation without them.
CountKernel Planner::choose_kernel() const {
    const bool tail = W >= 2 || a.any_tail != 0 || a.tail_loop != 0;
    if (a.off_ain >= 0) return tail ? DIRECTED_TAIL : DIRECTED;
    if (W == 1 && T == 64) {
        // every column a cycle of length <= 6 (route_tails: the launch's LDS was laid out for it): the walk
        if (a.cyc_len) {
            // (the headline step's flag combination as compile-time constants: count_body, CycKeys)
            // -- and the launch-uniform rest of it: global vertex ids, pairs, status words zeroed by their workgroups, and side workgroups that
            // leave the CSR with both sorted endpoint arrays, one node code column as key bytes and one edge code column in the key words
            // (side_block<T, CycKeys>).  Anything else is CycAny's.
            const SideArgs &sd = a.side;
            const bool side_keys = a.side_mask == 7 && sd.csr_tgt && sd.csr_oth && sd.nkey && sd.ekeys && !sd.npack && !sd.epack && sd.ncode_cols == 1 && sd.ecode_cols == 1;
            const bool keys = a.out && a.stage_out && a.enc_stage && a.enc_from_counts && a.enc_no32 && !a.enc16 && a.idmask && a.split == 1 &&
                              a.ids_are_global && a.pair && a.zero_status && side_keys;
            return keys ? CYCLE_KEYS : CYCLE_ANY;
        }
        if (count_molecule_route(a, sw)) return MOL;
    }
    return tail ? GENERIC_TAIL : GENERIC;
}

}  // namespace

bool count_molecule_route(const CountArgs &a, const CountSwitches &sw) {
    const bool tail = a.any_tail != 0 || a.tail_loop != 0;
    return sw.mol && !tail && a.mode == GSN_MODE_EDGE && a.sym && a.n_cols == 4 && a.pair && a.split == 1 && a.enc_out && a.enc_stage && !a.graph_ids;
}

int count_plan(const CountRequest &rq, const CountSwitches &sw, CountLaunchPlan *plan) {
    *plan = CountLaunchPlan{};
    Planner s{rq, sw, *plan, plan->args};
    if (int rc = s.validate_request()) return rc;
    if (s.n_items <= 0) return GSN_OK;
    if (int rc = s.fill_request()) return rc;
    if (int rc = s.side_and_keys()) return rc;
    s.route_size();
    s.route_tails();
    if (int rc = s.lds_layout()) return rc;
    s.staging_and_split();
    if (int rc = s.check_layout()) return rc;
    s.size_grid();
    plan->kernel = s.choose_kernel();
    return GSN_OK;
}

}  // namespace gsn
