// Test-only host program over gsn_amd/csrc/dropout_core.h (the header the HIP kernels of csrc/dropout.hip draw their masks with): built with
// g++ and the address / undefined-behaviour sanitizers by tests/test_dropout_cpu.py and run as a process.  It checks the two known answers
// of Philox4x32-10 and prints, for every (seed, calls, e, thr) quadruple of its command line (hexadecimal, 64 / 64 / 64 / 32 bits), the line
// "seed calls e thr keep word": the Python test compares them with its numpy referee.  Not a product fallback.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../gsn_amd/csrc/dropout_core.h"

using namespace gsn;

static int known_answer(const uint32_t (&c)[4], const uint32_t (&k)[2], const uint32_t (&want)[4]) {
    const DrWords r = dr_philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
    for (int i = 0; i < 4; ++i)
        if (r.w[i] != want[i]) {
            std::fprintf(stderr, "known answer: word %d is %08x, expected %08x\n", i, r.w[i], want[i]);
            return 1;
        }
    return 0;
}

int main(int argc, char **argv) {
    if (known_answer({0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u})) return 1;
    if (known_answer({0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
                     {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}))
        return 1;
    if ((argc - 1) % 4 != 0) {
        std::fprintf(stderr, "usage: dropout_harness [seed calls e thr]... (hexadecimal)\n");
        return 2;
    }
    std::printf("dropout harness ok: known answers, %d cases\n", (argc - 1) / 4);
    for (int i = 1; i + 3 < argc; i += 4) {
        const uint64_t seed = std::strtoull(argv[i], nullptr, 16), calls = std::strtoull(argv[i + 1], nullptr, 16);
        const uint64_t e = std::strtoull(argv[i + 2], nullptr, 16);
        const uint32_t thr = (uint32_t)std::strtoull(argv[i + 3], nullptr, 16);
        const uint32_t word = dr_group_words(seed, calls, e >> 2).w[e & 3u];
        if (dr_keep(seed, calls, e, thr) != dr_keep_word(word, thr)) return 3;
        std::printf("%" PRIx64 " %" PRIx64 " %" PRIx64 " %x %d %08x\n", seed, calls, e, thr, dr_keep(seed, calls, e, thr) ? 1 : 0, word);
    }
    return 0;
}
