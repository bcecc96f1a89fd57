// Stand-alone check of the switch table and its readers (gsn_amd/csrc/switches.h): built with the host compiler together with
// switches.cpp and run by tests/test_abi_cpu.py.  Prints one line per failed check; the exit status is the number of failures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../gsn_amd/csrc/switches.h"

using namespace gsn;

static int g_failed = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { ++g_failed; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static void set(Switch s, const char *text) {
    if (text) setenv(switch_row(s).name, text, 1);
    else unsetenv(switch_row(s).name);
}

int main() {
    // ---- the table: unique names that start with GSN_, a description each, the trace switch read at every call
    std::set<std::string> names;
    for (int i = 0; i < SW_COUNT; ++i) {
        const SwitchRow &r = switch_row((Switch)i);
        CHECK(r.name && strncmp(r.name, "GSN_", 4) == 0 && strlen(r.name) > 4);
        CHECK(names.insert(r.name).second);
        CHECK(r.life == ONCE || r.life == LIVE);
        CHECK(r.what && r.what[0]);
        unsetenv(r.name);                                   // (whatever the caller's environment holds)
    }
    CHECK((int)names.size() == SW_COUNT);
    CHECK(switch_row(SW_CHAIN_TRACE).life == LIVE);
    CHECK(strcmp(switch_row(SW_CHAIN_TRACE).name, "GSN_CHAIN_TRACE") == 0);
    CHECK(strcmp(switch_row(SW_SEG_PRIO).name, "GSN_SEG_PRIO") == 0);

    // ---- every reader kind on LIVE rows: unset gives the site's default, then "0", "1", "" and "7"
    const Switch I = SW_CHAIN_DBG, L = SW_CHAIN_PERCU, B = SW_SEG_VEC4, P = SW_L16_NOVEC, S = SW_PROP_CP;
    CHECK(switch_row(I).life == LIVE && switch_row(L).life == LIVE && switch_row(B).life == LIVE && switch_row(P).life == LIVE &&
          switch_row(S).life == LIVE);
    CHECK(sw_int(I, 3) == 3 && sw_int(I, -1) == -1);       // (the default is the site's: two sites, two defaults)
    CHECK(sw_int64(L, (int64_t)1 << 40) == (int64_t)1 << 40);
    CHECK(sw_on(B, true) && !sw_on(B, false));
    CHECK(!sw_present(P));
    CHECK(sw_str(S) == nullptr);
    struct { const char *text; int as_int; bool as_on; } cases[] = {{"0", 0, false}, {"1", 1, true}, {"", 0, false}, {"7", 7, true}};
    for (const auto &c : cases) {
        for (Switch s : {I, L, B, P, S}) set(s, c.text);
        CHECK(sw_int(I, 3) == c.as_int);
        CHECK(sw_int64(L, 3) == (int64_t)c.as_int);
        CHECK(sw_on(B, true) == c.as_on && sw_on(B, false) == c.as_on);
        CHECK(sw_present(P));                               // set to anything, "0" and "" included
        CHECK(sw_str(S) && strcmp(sw_str(S), c.text) == 0);
    }
    set(L, "1099511627776");
    CHECK(sw_int64(L, 0) == (int64_t)1 << 40);
    set(S, "16,2,256");
    CHECK(strcmp(sw_str(S), "16,2,256") == 0);

    // ---- LIVE follows setenv / unsetenv between two reads
    set(I, "5");
    CHECK(sw_int(I, 0) == 5);
    set(I, "6");
    CHECK(sw_int(I, 0) == 6);
    set(I, nullptr);
    CHECK(sw_int(I, 0) == 0);
    set(SW_CHAIN_TRACE, "1");
    CHECK(sw_present(SW_CHAIN_TRACE));
    set(SW_CHAIN_TRACE, nullptr);
    CHECK(!sw_present(SW_CHAIN_TRACE));
    set(SW_CHAIN_TRACE, "0");
    CHECK(sw_present(SW_CHAIN_TRACE));                      // "present" is the trace switch's one rule
    set(SW_CHAIN_TRACE, nullptr);

    // ---- ONCE keeps the first read of the process, whichever reader asks later
    CHECK(switch_row(SW_FUSED_PRIO).life == ONCE && switch_row(SW_FUSED_W).life == ONCE && switch_row(SW_EMBED_NOVEC4).life == ONCE &&
          switch_row(SW_WGRAD_FP32).life == ONCE);
    set(SW_FUSED_PRIO, "5");
    CHECK(sw_int(SW_FUSED_PRIO, 1) == 5);
    set(SW_FUSED_PRIO, "9");
    CHECK(sw_int(SW_FUSED_PRIO, 1) == 5);
    set(SW_FUSED_PRIO, nullptr);
    CHECK(sw_int(SW_FUSED_PRIO, 1) == 5 && sw_on(SW_FUSED_PRIO, false) && strcmp(sw_str(SW_FUSED_PRIO), "5") == 0);
    CHECK(sw_int(SW_FUSED_W, 1) == 1);                      // first read while unset: the default, for good
    set(SW_FUSED_W, "0");
    CHECK(sw_int(SW_FUSED_W, 1) == 1 && sw_int(SW_FUSED_W, 4) == 4 && !sw_present(SW_FUSED_W));
    set(SW_EMBED_NOVEC4, "0");
    CHECK(sw_present(SW_EMBED_NOVEC4));
    set(SW_EMBED_NOVEC4, nullptr);
    CHECK(sw_present(SW_EMBED_NOVEC4));
    set(SW_WGRAD_FP32, "1");
    CHECK(sw_on(SW_WGRAD_FP32, false));
    set(SW_WGRAD_FP32, "0");
    CHECK(sw_on(SW_WGRAD_FP32, false));

    if (g_failed) fprintf(stderr, "%d check(s) failed\n", g_failed);
    else printf("switches ok: %d rows\n", (int)SW_COUNT);
    return g_failed;
}
