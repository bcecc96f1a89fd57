// TEST-ONLY harness (not product code, never shipped in libgsn_hip.so).
// Compiles the counting launch planner (gsn_amd/csrc/count_plan.cpp) for the HOST and runs one request through it: the request arrives as
// flat integers (pointers as made-up addresses that are never followed), the plan leaves the same way.  set_error and the switch readers
// are the harness's own: the refusal's text is kept for the caller, and the switches come from the case, not from the environment.
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../gsn_amd/csrc/count_plan.cpp"

// request integers (addresses for pointers; 0 = null), in the order of CountRequest
#define RQ_FIELDS(X) X(plan_dev) X(plan_words) X(n_graphs) X(node_ptr) X(edge_ptr) X(edge_index) X(edge_row_stride) X(ids_are_global) X(graph_ids) \
    X(n_items) X(max_nodes) X(max_edges) X(out) X(status) X(enc_clamp) X(enc_out) X(enc16) X(enc16_stride) X(enc16_col0) X(enc_no32)
// gsn_count_side, in its order
#define SIDE_FIELDS(X) X(csr_row) X(seg_ptr) X(perm) X(sorted_target) X(sorted_other) X(n_nodes) X(n_edges) X(node_codes) X(node_code_cols) \
    X(node_n_classes0) X(node_n_classes1) X(node_n_classes2) X(node_n_classes3) X(node_clamp) X(node_pack) X(edge_codes) X(edge_code_cols) \
    X(edge_n_classes0) X(edge_n_classes1) X(edge_n_classes2) X(edge_n_classes3) X(edge_clamp) X(edge_col0) X(code_status)
#define KEYS_FIELDS(X) X(nkey) X(ekeys) X(idmask)
// the switches a case may set, in this order (texts, null = unset)
#define SW_FIELDS(X) X(PULL_BATCH) X(COUNT_PAIR) X(COUNT_TAIL_LOOP) X(COUNT_CYCLE) X(COUNT_MOL) X(COUNT_SPLIT_TARGET) X(COUNT_ENC_BYTES)

// every field of CountArgs and SideArgs; enc_n[] and the byte words follow as arrays
#define ARG_INTS(X) X(plan_words) X(mode) X(n_cols) X(n_plans) X(plans_off) X(kmax) X(ids_are_global) X(n_cap) X(e_cap) X(last_cap) X(n_decl) X(e_decl) \
    X(stack_skip) X(pair) X(n_graphs) X(stage_out) X(sym) X(split) X(off_valid) X(off_stack) X(off_plan) X(off_eu) X(off_ev) X(off_rowstart) X(off_last) \
    X(off_out) X(off_misc) X(off_prim) X(off_revof) X(off_ball) X(off_degp) X(degp_mask) X(any_tail) X(tail_loop) X(off_core) X(core_mask) X(off_ain) \
    X(stride) X(pull_batch) X(zero_status) X(enc_width) X(enc_clamp) X(off_enc) X(enc_stage) X(off_encst) X(enc_from_counts) X(enc_no32) X(enc16_stride) \
    X(enc16_col0) X(side_mask) X(n_items) X(lds_bytes) X(cyc_len)
#define ARG_PTRS(X) X(plan) X(node_ptr) X(edge_ptr) X(src) X(dst) X(graph_ids) X(out) X(status) X(enc_out) X(enc16) X(idmask)
#define SIDEARG_INTS(X) X(tot_nodes) X(tot_edges) X(csr_row) X(ncode_cols) X(ncode_clamp) X(ecode_cols) X(ecode_clamp) X(ecode_col0) X(nkey_radix_w)
#define SIDEARG_PTRS(X) X(csr_seg) X(csr_perm) X(csr_tgt) X(csr_oth) X(ncode) X(npack) X(ecode) X(epack) X(code_status) X(nkey) X(ekeys)

#define AS_ENUM_RQ(n) RQ_##n,
#define AS_ENUM_SIDE(n) SD_##n,
#define AS_ENUM_KEYS(n) KY_##n,
#define AS_ENUM_SW(n) HS_##n,
enum { RQ_FIELDS(AS_ENUM_RQ) RQ_COUNT };
enum { SIDE_FIELDS(AS_ENUM_SIDE) SD_COUNT };
enum { KEYS_FIELDS(AS_ENUM_KEYS) KY_COUNT };
enum { SW_FIELDS(AS_ENUM_SW) HS_COUNT };

static std::string g_error;
static const char *const *g_switch_text = nullptr;

namespace gsn {
int set_error(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_error = buf;
    return code;
}
// the readers' rules of switches.h, over the case's texts
const char *sw_str(Switch s) {
#define AS_CASE_SW(n) if (s == SW_##n) return g_switch_text[HS_##n];
    SW_FIELDS(AS_CASE_SW)
    abort();            // a switch the planner is not known to read
}
int sw_int(Switch s, int dflt) { const char *t = sw_str(s); return t ? atoi(t) : dflt; }
int64_t sw_int64(Switch s, int64_t dflt) { const char *t = sw_str(s); return t ? atoll(t) : dflt; }
bool sw_on(Switch s, bool dflt) { const char *t = sw_str(s); return t ? atoi(t) != 0 : dflt; }
bool sw_present(Switch s) { return sw_str(s) != nullptr; }
}  // namespace gsn
using namespace gsn;

template <class T> static T *as_ptr(int64_t address) { return reinterpret_cast<T *>(static_cast<uintptr_t>(address)); }
template <class T> static int64_t as_int(T *p) { return static_cast<int64_t>(reinterpret_cast<uintptr_t>(p)); }

#define AS_NAME(n) #n ","
extern "C" const char *count_plan_harness_request_fields() { return RQ_FIELDS(AS_NAME) ""; }
extern "C" const char *count_plan_harness_side_fields() { return SIDE_FIELDS(AS_NAME) ""; }
extern "C" const char *count_plan_harness_keys_fields() { return KEYS_FIELDS(AS_NAME) ""; }
extern "C" const char *count_plan_harness_switch_fields() { return SW_FIELDS(AS_NAME) ""; }
#define AS_SIDE_NAME(n) "side." #n ","
extern "C" const char *count_plan_harness_int_fields() {
    return "W,T,kernel,grid,lds_bytes,memset_status," ARG_INTS(AS_NAME) SIDEARG_INTS(AS_SIDE_NAME)
           "side.ncode_ptr_w0,side.ncode_ptr_w1,side.ecode_ptr_w0,side.ecode_ptr_w1,";       // then enc_n[0 .. GSN_ENC_MAX_COLS)
}
extern "C" const char *count_plan_harness_pointer_fields() { return ARG_PTRS(AS_NAME) SIDEARG_PTRS(AS_SIDE_NAME) ""; }
extern "C" const char *count_plan_harness_error() { return g_error.c_str(); }

// plan_host: the table or null.  side, keys: SD_COUNT / KY_COUNT integers or null.  Returns count_plan's status; on GSN_OK ints[] and
// pointers[] hold the plan in the order of the two field lists (ints[]: enc_n[] behind them).
extern "C" int count_plan_harness_run(const uint32_t *plan_host, const int64_t *rq, const int32_t *n_classes, const int64_t *side, const int64_t *keys,
                                      const char *const *switch_text, int64_t *ints, int64_t *pointers) {
    g_error.clear();
    g_switch_text = switch_text;
    gsn_count_side sd{};
    if (side) {
        sd.csr_row = (int)side[SD_csr_row];
        sd.seg_ptr = as_ptr<int32_t>(side[SD_seg_ptr]); sd.perm = as_ptr<int32_t>(side[SD_perm]);
        sd.sorted_target = as_ptr<int32_t>(side[SD_sorted_target]); sd.sorted_other = as_ptr<int32_t>(side[SD_sorted_other]);
        sd.n_nodes = side[SD_n_nodes]; sd.n_edges = side[SD_n_edges];
        sd.node_codes = as_ptr<const int64_t>(side[SD_node_codes]); sd.node_code_cols = (int)side[SD_node_code_cols];
        for (int c = 0; c < 4; ++c) { sd.node_n_classes[c] = (int)side[SD_node_n_classes0 + c]; sd.edge_n_classes[c] = (int)side[SD_edge_n_classes0 + c]; }
        sd.node_clamp = (int)side[SD_node_clamp]; sd.node_pack = as_ptr<uint16_t>(side[SD_node_pack]);
        sd.edge_codes = as_ptr<const int64_t>(side[SD_edge_codes]); sd.edge_code_cols = (int)side[SD_edge_code_cols];
        sd.edge_clamp = (int)side[SD_edge_clamp]; sd.edge_col0 = (int)side[SD_edge_col0]; sd.code_status = as_ptr<int32_t>(side[SD_code_status]);
    }
    gsn_count_keys ky{};
    if (keys) { ky.nkey = as_ptr<uint8_t>(keys[KY_nkey]); ky.ekeys = as_ptr<uint32_t>(keys[KY_ekeys]); ky.idmask = as_ptr<uint16_t>(keys[KY_idmask]); }
    CountRequest r;
    r.plan_host = plan_host; r.plan_dev = as_ptr<const uint32_t>(rq[RQ_plan_dev]); r.plan_words = rq[RQ_plan_words]; r.n_graphs = rq[RQ_n_graphs];
    r.node_ptr = as_ptr<const int64_t>(rq[RQ_node_ptr]); r.edge_ptr = as_ptr<const int64_t>(rq[RQ_edge_ptr]);
    r.edge_index = as_ptr<const int64_t>(rq[RQ_edge_index]); r.edge_row_stride = rq[RQ_edge_row_stride];
    r.ids_are_global = (int)rq[RQ_ids_are_global]; r.graph_ids = as_ptr<const int32_t>(rq[RQ_graph_ids]); r.n_items = rq[RQ_n_items];
    r.max_nodes = rq[RQ_max_nodes]; r.max_edges = rq[RQ_max_edges]; r.out = as_ptr<int64_t>(rq[RQ_out]); r.status = as_ptr<int32_t>(rq[RQ_status]);
    r.n_classes = n_classes; r.enc_clamp = (int)rq[RQ_enc_clamp]; r.enc_out = as_ptr<float>(rq[RQ_enc_out]);
    r.enc16 = as_ptr<uint16_t>(rq[RQ_enc16]); r.enc16_stride = rq[RQ_enc16_stride]; r.enc16_col0 = rq[RQ_enc16_col0]; r.enc_no32 = (int)rq[RQ_enc_no32];
    r.side = side ? &sd : nullptr; r.keys = keys ? &ky : nullptr;

    CountLaunchPlan p;
    const int rc = count_plan(r, CountSwitches::read(), &p);
    if (rc != GSN_OK) return rc;
    const CountArgs &a = p.args;
    int64_t *o = ints;
    *o++ = p.W; *o++ = p.T; *o++ = (int64_t)p.kernel; *o++ = p.grid; *o++ = p.lds_bytes; *o++ = p.memset_status ? 1 : 0;
#define PUT_INT(n) *o++ = (int64_t)a.n;
#define PUT_SIDE_INT(n) *o++ = (int64_t)a.side.n;
    ARG_INTS(PUT_INT) SIDEARG_INTS(PUT_SIDE_INT)
    *o++ = a.side.ncode_ptr_w[0]; *o++ = a.side.ncode_ptr_w[1]; *o++ = a.side.ecode_ptr_w[0]; *o++ = a.side.ecode_ptr_w[1];
    for (int c = 0; c < GSN_ENC_MAX_COLS; ++c) *o++ = a.enc_n[c];
    o = pointers;
#define PUT_PTR(n) *o++ = as_int(a.n);
#define PUT_SIDE_PTR(n) *o++ = as_int(a.side.n);
    ARG_PTRS(PUT_PTR) SIDEARG_PTRS(PUT_SIDE_PTR)
    return GSN_OK;
}
