// Error reporting, version and device discovery for libgsn_hip.so (C ABI: gsn_last_error, gsn_version, gsn_device_count).
#include <hip/hip_runtime.h>

#include <cstring>

#include "gsn_internal.h"
#include "layer_rr.h"

namespace gsn {

static thread_local char g_err[512] = "";

int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace gsn

extern "C" const char *gsn_last_error(void) { return gsn::g_err; }

extern "C" int gsn_version(void) { return GSN_ABI_VERSION; }

extern "C" int gsn_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int good = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
    }
    return good;
}

// 0 when `stream` is not being captured into a graph, else the capture's id (unique per capture sequence, hipStreamGetCaptureInfo).
// The host side keys its zero-initialised scratch arenas on it: a buffer whose fill was recorded into one capture must not be
// handed out in another capture or in eager execution (the fill would not run there).
extern "C" int64_t gsn_stream_capture_id(void *stream) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(reinterpret_cast<hipStream_t>(stream), &st, &id) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (st == hipStreamCaptureStatusNone) return 0;
    return (int64_t)(id ? id : 1);
}

namespace gsn {
int current_device() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    return dev;
}

int lds_limit(DeviceOnce *once, std::initializer_list<const void *> kernels, const char *label, int bytes) {
    const int dev = once ? current_device() : -1;
    if (once && once->done(dev)) return GSN_OK;
    char sized[32];
    if (!label) { snprintf(sized, sizeof(sized), "%d B LDS", bytes); label = sized; }
    for (const void *k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return set_error(GSN_E_HIP, "hipFuncSetAttribute(%s): %s", label, hipGetErrorString(e));
    }
    if (once) once->mark(dev);
    return GSN_OK;
}

int launch_check(const char *label_fmt, ...) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return GSN_OK;
    char label[256];
    va_list ap;
    va_start(ap, label_fmt);
    vsnprintf(label, sizeof(label), label_fmt, ap);
    va_end(ap);
    return set_error(GSN_E_HIP, "%s: %s", label, hipGetErrorString(e));
}

void trace(const char *fmt, ...) {
    if (!sw_present(SW_CHAIN_TRACE)) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

ProfCounters::ProfCounters(size_t n, void *stream) {
    n_ = n;
    if (n == 0 || hipMalloc(&dev_, n * sizeof(unsigned long long)) != hipSuccess) { dev_ = nullptr; return; }
    (void)hipMemsetAsync(dev_, 0, n * sizeof(unsigned long long), reinterpret_cast<hipStream_t>(stream));
}
ProfCounters::~ProfCounters() { if (dev_) (void)hipFree(dev_); }
std::vector<unsigned long long> ProfCounters::fetch(void *stream) {
    std::vector<unsigned long long> h(n_, 0ull);
    (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
    if (dev_) {
        (void)hipMemcpy(h.data(), dev_, n_ * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        (void)hipFree(dev_);
        dev_ = nullptr;
    }
    return h;
}
}  // namespace gsn

// HP-1 + HP-2 in one host call (include/gsn_abi.h: gsn_count_layer_step_hip): the counting launch with its side outputs, then layer 0 on the packs
extern "C" int gsn_count_layer_step_hip(const gsn_count_call *c, const gsn_layer_pack16_call *l, void *event_between, void *stream) {
    if (!c || !l) return gsn::set_error(GSN_E_INVALID, "gsn_count_layer_step_hip: null call struct");
    const int rc = gsn_count_encode_pack16_side_hip(c->plan_host, c->plan_dev, c->plan_words, c->n_graphs, c->node_ptr, c->edge_ptr, c->edge_index,
                                                    c->edge_row_stride, c->ids_are_global, c->max_nodes, c->max_edges, c->out, c->status, c->n_classes,
                                                    c->clamp, c->pack, c->pack_stride, c->pack_col0, c->side, stream);
    if (rc != GSN_OK) return rc;
    if (event_between && hipEventRecord(reinterpret_cast<hipEvent_t>(event_between), reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
        return gsn::set_error(GSN_E_HIP, "gsn_count_layer_step_hip: hipEventRecord(event_between)");
    return gsn_layer_fused_fwd_pack16_hip(l->n_nodes, l->n_edges, l->seg_ptr, l->edge, l->x, l->d_x, l->node0, l->node1, l->prepared, l->pack,
                                          l->edge_rows, l->out, stream);
}

// The same step on code keys (include/gsn_abi.h: gsn_count_layer_step_keys_hip): the counting launch leaves the CSR and the compact keys, layer 0
// gathers its operand rows from the node dictionary and the byte table through them -- no row pack is written or read
extern "C" int gsn_count_layer_step_keys_hip(const gsn_count_call *c, const gsn_layer_pack16_call *l, const gsn_count_keys *keys, const uint16_t *node_dict,
                                             int64_t dict_rows, void *event_between, void *stream) {
    return gsn_count_layer_step_tabs_hip(c, l, keys, node_dict, dict_rows, nullptr, event_between, stream);
}

// ... and with the x_i tables of gsn_layer_key_tables_hip (`tabs`, may be null): the edge stage starts from a table row per edge row
extern "C" int gsn_count_layer_step_tabs_hip(const gsn_count_call *c, const gsn_layer_pack16_call *l, const gsn_count_keys *keys, const uint16_t *node_dict,
                                             int64_t dict_rows, const float *tabs, void *event_between, void *stream) {
    if (!c || !l || !keys || !c->side) return gsn::set_error(GSN_E_INVALID, "gsn_count_layer_step_keys_hip: null call struct / keys / side");
    if (!keys->nkey || !keys->ekeys || !keys->idmask || !node_dict) return gsn::set_error(GSN_E_INVALID, "gsn_count_layer_step_keys_hip: null key array / node dictionary");
    if (!c->side->node_codes || !c->side->edge_codes) return gsn::set_error(GSN_E_INVALID, "gsn_count_layer_step_keys_hip: node and edge codes are both needed");
    if (!gsn_layer_fused_pack16_supported(l->edge, l->d_x, l->node0, l->node1))
        return gsn::set_error(GSN_E_UNSUPPORTED, "gsn_count_layer_step_keys_hip: shape outside the packed-row layer kernel");
    if (!l->seg_ptr || !l->out || !l->prepared || (reinterpret_cast<uintptr_t>(l->prepared) & 15) || l->n_nodes <= 0 || l->n_nodes > (int64_t)2000000000 ||
        l->n_edges > (int64_t)2000000000)
        return gsn::set_error(GSN_E_INVALID, "gsn_count_layer_step_keys_hip: null seg_ptr / out / prepared (16-byte aligned), or sizes outside 32-bit row arithmetic");
    // the layer reads the key arrays in the order of the CSR this launch writes
    if (l->edge->n_blocks < 3 || l->edge->blocks[0].idx32 != c->side->sorted_target || l->edge->blocks[1].idx32 != c->side->sorted_other ||
        l->edge->blocks[2].idx32 != c->side->perm || l->seg_ptr != c->side->seg_ptr || l->n_edges != c->side->n_edges || l->n_nodes != c->side->n_nodes)
        return gsn::set_error(GSN_E_INVALID, "gsn_count_layer_step_keys_hip: the layer's seg_ptr / block indices must be the counting launch's CSR arrays");
    int rc = gsn_count_encode_keys_side_hip(c->plan_host, c->plan_dev, c->plan_words, c->n_graphs, c->node_ptr, c->edge_ptr, c->edge_index, c->edge_row_stride,
                                            c->ids_are_global, c->max_nodes, c->max_edges, c->out, c->status, c->n_classes, c->clamp, c->pack_col0, c->side, keys, stream);
    if (rc != GSN_OK) return rc;
    if (event_between && hipEventRecord(reinterpret_cast<hipEvent_t>(event_between), reinterpret_cast<hipStream_t>(stream)) != hipSuccess)
        return gsn::set_error(GSN_E_HIP, "gsn_count_layer_step_keys_hip: hipEventRecord(event_between)");
    const gsn::RpKeys k{keys->ekeys, keys->nkey, keys->idmask, node_dict, dict_rows, c->side->edge_col0, tabs};
    rc = gsn::rp_forward(l->n_nodes, l->n_edges, l->seg_ptr, l->edge, l->x, l->d_x, l->node0, l->node1, l->prepared, nullptr, l->edge_rows, l->out,
                         reinterpret_cast<hipStream_t>(stream), &k);
    if (rc == 1) return gsn::set_error(GSN_E_UNSUPPORTED, "gsn_count_layer_step_keys_hip: key arrays beyond 2 GiB (32-bit buffer offsets)");
    return rc;
}
