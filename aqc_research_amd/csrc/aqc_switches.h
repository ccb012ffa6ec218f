// The run-time switches (include/aqc_switches.def) on the C side: the only file of the library that reads the environment.
// A workspace reads its `create` switches once (read_switches, at the top of aqc_ws_create) and keeps them in aqc_ws::sw; the `call`
// switches are read where they are used (switch_now).  Host only, no HIP.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace aqc {

// the one parsing rule: unset or empty means the default, anything else is strtol base 10 / strtod (seconds: <= 0 means the default too)
inline const char* env_text(const char* name) {
    const char* v = getenv(name);
    return (v && *v) ? v : nullptr;
}
inline int64_t switch_int(const char* name, int64_t dflt) {
    const char* v = env_text(name);
    return v ? (int64_t)strtol(v, nullptr, 10) : dflt;
}
inline double switch_seconds(const char* name, double dflt) {
    const char* v = env_text(name);
    const double s = v ? strtod(v, nullptr) : 0.0;
    return s > 0.0 ? s : dflt;
}

// ---- the listing: every line of the table, the Python-only ones included ----
struct SwitchInfo { const char *name, *dflt, *when, *reader, *doc; };
#define AQC_SWITCH(NAME, field, dflt, when, reader, doc) {#NAME, #dflt, #when, #reader, doc},
constexpr SwitchInfo kSwitchTable[] = {
#include "../../include/aqc_switches.def"
};
#undef AQC_SWITCH
constexpr int kNumSwitches = (int)(sizeof(kSwitchTable) / sizeof(kSwitchTable[0]));

// ---- create switches: one member each, initialised to its default ----
#define AQC_SW_create_c(NAME, field, dflt) int64_t field = dflt;
#define AQC_SW_call_c(NAME, field, dflt)
#define AQC_SW_import_python(NAME, field, dflt)
#define AQC_SW_call_python(NAME, field, dflt)
#define AQC_SWITCH(NAME, field, dflt, when, reader, doc) AQC_SW_##when##_##reader(NAME, field, dflt)
struct Switches {
#include "../../include/aqc_switches.def"
    // the value a workspace was created with, by the switch's name; false: not a create switch of the C side
    bool get(const char* name, int64_t* value) const {
#undef AQC_SW_create_c
#define AQC_SW_create_c(NAME, field, dflt) if (!strcmp(name, #NAME)) { *value = field; return true; }
#include "../../include/aqc_switches.def"
        return false;
    }
};
inline Switches read_switches() {
    Switches s;
#undef AQC_SW_create_c
#define AQC_SW_create_c(NAME, field, dflt) s.field = switch_int(#NAME, dflt);
#include "../../include/aqc_switches.def"
    if (!env_text("AQC_KERNEL_FAMILY") && s.kernel_v2 >= 0) s.kernel_family = s.kernel_v2 + 1;   // the older spelling; a set AQC_KERNEL_FAMILY wins
    return s;
}
#undef AQC_SWITCH
#undef AQC_SW_create_c
#undef AQC_SW_call_c
#undef AQC_SW_import_python
#undef AQC_SW_call_python

// ---- call switches, by name: read now; the default is the table's ----
inline const SwitchInfo& call_switch(const char* name) {
    for (const SwitchInfo& e : kSwitchTable)
        if (!strcmp(e.name, name) && !strcmp(e.when, "call") && !strcmp(e.reader, "c")) return e;
    fprintf(stderr, "aqc_hip: %s is not a call switch of include/aqc_switches.def\n", name);
    abort();
}
inline int64_t switch_now(const char* name) { return switch_int(name, (int64_t)strtol(call_switch(name).dflt, nullptr, 10)); }
inline double switch_now_seconds(const char* name) { return switch_seconds(name, strtod(call_switch(name).dflt, nullptr)); }

}  // namespace aqc
