// TEST-ONLY logic harness (not product code, never shipped in libgsn_hip.so).
// Compiles the row helpers of the cycle launch's output loop (gsn_amd/csrc/count_core.h: cyc_row_has_direct, cyc_row_store, cyc_row_mask)
// for the HOST: the 0xffff cell ("this count went to memory by itself") cannot occur in a real cycle launch, so its arm is checked here.
#include <cstdarg>
#include <cstdio>

#include "../gsn_amd/csrc/count_core.h"

namespace gsn {
int set_error(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr);
    return code;
}
}

extern "C" int cycle_rows_has_direct(uint32_t lo, uint32_t hi) { return gsn::cyc_row_has_direct(lo, hi) ? 1 : 0; }
// d: the int64 row (16-byte aligned when wide != 0)
extern "C" void cycle_rows_store(int64_t *d, uint32_t lo, uint32_t hi, int wide) { gsn::cyc_row_store(d, lo, hi, wide != 0); }
extern "C" uint32_t cycle_rows_mask(uint32_t lo, uint32_t hi, uint32_t ncls_w, int clamp) { return gsn::cyc_row_mask(lo, hi, ncls_w, clamp != 0); }
