// The readers of the switch table (switches.h): the only getenv of the library.
#include "switches.h"

#include <cstdlib>
#include <mutex>
#include <string>

namespace gsn {

static const SwitchRow g_rows[SW_COUNT] = {
#define GSN_SWITCH_ROW(id, life, what) {"GSN_" #id, life, what},
    GSN_SWITCH_TABLE(GSN_SWITCH_ROW)
#undef GSN_SWITCH_ROW
};

const SwitchRow &switch_row(Switch s) { return g_rows[s]; }

namespace {
struct Latch {   // the first read of a ONCE switch
    std::once_flag once;
    bool set = false;
    std::string text;
};
Latch g_latch[SW_COUNT];
}  // namespace

const char *sw_str(Switch s) {
    const SwitchRow &r = g_rows[s];
    if (r.life == LIVE) return getenv(r.name);
    Latch &l = g_latch[s];
    std::call_once(l.once, [&] {
        if (const char *e = getenv(r.name)) { l.text = e; l.set = true; }
    });
    return l.set ? l.text.c_str() : nullptr;
}

int sw_int(Switch s, int dflt) { const char *e = sw_str(s); return e ? atoi(e) : dflt; }
int64_t sw_int64(Switch s, int64_t dflt) { const char *e = sw_str(s); return e ? (int64_t)atoll(e) : dflt; }
bool sw_on(Switch s, bool dflt) { const char *e = sw_str(s); return e ? atoi(e) != 0 : dflt; }
bool sw_present(Switch s) { return sw_str(s) != nullptr; }

}  // namespace gsn
