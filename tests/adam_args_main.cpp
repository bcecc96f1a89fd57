// Stand-alone host program: the argument checks of gsn_adam_step_hip (csrc/optim.hip), for a run under the host sanitizers
// (tests/test_optim_cpu.py builds it with -Xarch_host -fsanitize=address,undefined).  Every call returns before anything touches a device.
// Linked with optim.hip alone: the three helpers of abi.cpp that the entry uses are restated below (abi.cpp pulls in every other kernel file).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../gsn_amd/csrc/gsn_internal.h"

static char last_error[512];

namespace gsn {
int set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
    return code;
}
int launch_check(const char *, ...) { return GSN_OK; }
}  // namespace gsn

extern "C" const char *gsn_last_error(void) { return last_error; }

static int failures = 0;

static void expect(const char *what, int got, int want, const char *needle) {
    const char *msg = gsn_last_error();
    const bool ok = got == want && (!needle || (msg && std::strstr(msg, needle)));
    if (!ok) {
        std::printf("FAIL %s: returned %d (want %d), message '%s'\n", what, got, want, msg ? msg : "");
        ++failures;
    }
}

int main() {
    int64_t tensors[GSN_ADAM_TENSOR_WORDS] = {0, 0, 0, 0, 0, 0};
    int32_t chunks[2] = {0, 0};
    double groups[GSN_ADAM_GROUP_DOUBLES] = {1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.0, 0.0};
    float m[4] = {0}, v[4] = {0}, steps[1] = {0};
    unsigned done = 0;
    expect("n_tensors < 0", gsn_adam_step_hip(-1, tensors, 0, chunks, 1, groups, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "negative");
    expect("n_groups < 0", gsn_adam_step_hip(1, tensors, 0, chunks, -1, groups, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "negative");
    expect("n_chunks < 0", gsn_adam_step_hip(1, tensors, -1, chunks, 1, groups, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "negative");
    expect("null tensor table", gsn_adam_step_hip(1, nullptr, 0, chunks, 1, groups, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "null");
    expect("null chunk table", gsn_adam_step_hip(1, tensors, 0, nullptr, 1, groups, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "null");
    expect("null group records", gsn_adam_step_hip(1, tensors, 0, chunks, 1, nullptr, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "null");
    expect("null exp_avg", gsn_adam_step_hip(1, tensors, 0, chunks, 1, groups, nullptr, v, steps, &done, 0, nullptr), GSN_E_INVALID, "null");
    expect("null exp_avg_sq", gsn_adam_step_hip(1, tensors, 0, chunks, 1, groups, m, nullptr, steps, &done, 0, nullptr), GSN_E_INVALID, "null");
    expect("null steps", gsn_adam_step_hip(1, tensors, 0, chunks, 1, groups, m, v, nullptr, &done, 0, nullptr), GSN_E_INVALID, "null");
    expect("null done word", gsn_adam_step_hip(1, tensors, 0, chunks, 1, groups, m, v, steps, nullptr, 0, nullptr), GSN_E_INVALID, "null");
    expect("2^31 elements", gsn_adam_step_hip(1, tensors, 1, chunks, 1, groups, m, v, steps, &done, (int64_t)1 << 31, nullptr), GSN_E_UNSUPPORTED,
           "2^31 - 1");
    expect("2^31 - 1 elements, no chunk", gsn_adam_step_hip(1, tensors, 0, chunks, 1, groups, m, v, steps, &done, ((int64_t)1 << 31) - 1, nullptr), GSN_OK,
           nullptr);
    expect("2^31 chunks", gsn_adam_step_hip(1, tensors, (int64_t)1 << 31, chunks, 1, groups, m, v, steps, &done, 4, nullptr), GSN_E_UNSUPPORTED, "chunks");
    expect("no chunk: nothing launched", gsn_adam_step_hip(0, tensors, 0, chunks, 0, groups, m, v, steps, &done, 0, nullptr), GSN_OK, nullptr);
    expect("chunks without tensors", gsn_adam_step_hip(0, tensors, 1, chunks, 1, groups, m, v, steps, &done, 0, nullptr), GSN_E_INVALID, "without");
    if (done != 0 || steps[0] != 0.0f) {
        std::printf("FAIL: a refused call wrote to its arguments\n");
        ++failures;
    }
    std::printf(failures ? "adam argument checks: %d FAILED\n" : "adam argument checks: all refused or accepted as documented (%d failures)\n", failures);
    return failures ? 1 : 0;
}
