// TEST-ONLY program (not product code, never shipped in libgsn_hip.so): the HOST build of the counting kernel's endpoint test
// (gsn_amd/csrc/count_core.h: endpoint_local / endpoint_width -- one 64-bit subtraction, the high word against zero, one unsigned 32-bit
// compare) against the plain 64-bit comparison  lo <= x < hi.  Prints one line per combination, "lo hi x inside offset", and exits with 1
// when the two disagree anywhere.  tests/test_endpoint_check_cpu.py builds it with -fsanitize=address,undefined and checks the lines again
// in Python integers.
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../gsn_amd/csrc/count_core.h"

namespace gsn {
int set_error(int code, const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr);
    return code;
}
}

int main() {
    const int64_t bounds[4] = {0, 1, 37, 64};
    int wrong = 0, n = 0;
    for (const int64_t lo : bounds)
        for (const int64_t hi : bounds) {
            const int64_t xs[11] = {INT64_MIN, -1, 0, lo - 1, lo, hi - 1, hi, (int64_t)1 << 31, (int64_t)1 << 32, ((int64_t)1 << 32) + lo, INT64_MAX};
            for (const int64_t x : xs) {
                uint32_t d = 0;
                const bool got = gsn::endpoint_local(x, lo, gsn::endpoint_width(lo, hi), d);
                const bool want = x >= lo && x < hi;
                if (got != want || (want && (int64_t)d != x - lo)) {
                    ++wrong;
                    fprintf(stderr, "lo %lld hi %lld x %lld: helper %d (offset %u), 64-bit comparison %d\n", (long long)lo, (long long)hi, (long long)x, (int)got, d, (int)want);
                }
                printf("%lld %lld %lld %d %u\n", (long long)lo, (long long)hi, (long long)x, (int)got, got ? d : 0u);
                ++n;
            }
        }
    fprintf(stderr, "endpoint_check_harness: %d combinations, %d wrong\n", n, wrong);
    return wrong ? 1 : 0;
}
