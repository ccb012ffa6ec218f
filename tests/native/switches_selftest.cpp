// Self-test of the run-time switches (csrc/aqc_switches.h over include/aqc_switches.def): defaults, the one parsing rule, the older
// spelling of the kernel family, the seconds, the listing.  Built with ASan + UBSan by tests/test_native_sanitizers.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "../../aqc_research_amd/csrc/aqc_switches.h"

using namespace aqc;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static void clear_all() {
    for (const SwitchInfo& e : kSwitchTable) unsetenv(e.name);
}
static void set(const char* name, const char* value) { setenv(name, value, 1); }

int main() {
    // ---- the listing: 44 lines, no name twice, every line complete ----
    std::set<std::string> names;
    int create_c = 0;
    for (const SwitchInfo& e : kSwitchTable) {
        CHECK(names.insert(e.name).second);
        CHECK(std::string(e.name).rfind("AQC_", 0) == 0);
        const std::string when = e.when, reader = e.reader;
        CHECK(when == "import" || when == "create" || when == "call");
        CHECK(reader == "c" || reader == "python");
        CHECK(e.dflt[0] != 0 && e.doc[0] != 0);
        create_c += when == "create" && reader == "c";
    }
    CHECK(kNumSwitches == 44 && (int)names.size() == kNumSwitches);

    // ---- defaults when unset: the member initialisers, read_switches and the table agree ----
    clear_all();
    const Switches fresh;
    Switches s = read_switches();
    int seen = 0;
    for (const SwitchInfo& e : kSwitchTable) {
        int64_t a = 0, b = 0;
        if (!s.get(e.name, &a)) continue;
        ++seen;
        CHECK(fresh.get(e.name, &b) && a == b);
        CHECK(a == strtol(e.dflt, nullptr, 10));
        CHECK(std::string(e.when) == "create" && std::string(e.reader) == "c");
    }
    CHECK(seen == create_c && seen == 32);
    CHECK(s.kernel_family == 0 && s.kernel_v2 == -1 && s.graph == 1 && s.sweep_grid == 0 && s.apply_persist == 2);
    CHECK(s.projected_vdag_min_elems == (1 << 24) && s.sparse_min_items == 512 && s.projected_fused_qb == 2 && s.skip_zero_w == 0);
    int64_t v = 0;
    CHECK(!s.get("AQC_CD_CHAIN", &v) && !s.get("AQC_HIP_LIB", &v) && !s.get("AQC_NO_SUCH_SWITCH", &v));
    CHECK(switch_now("AQC_CD_CHAIN") == 0 && switch_now("AQC_SVD_BLOCKED") == 1 && switch_now("AQC_SVD_DEBUG") == 0 && switch_now("AQC_DEVICE") == 0);
    CHECK(switch_now_seconds("AQC_COMM_TIMEOUT_S") == 300.0 && switch_now_seconds("AQC_COMM_INIT_TIMEOUT_S") == 180.0);

    // ---- defaults when empty ----
    for (const SwitchInfo& e : kSwitchTable) set(e.name, "");
    s = read_switches();
    for (const SwitchInfo& e : kSwitchTable) {
        int64_t a = 0, b = 0;
        if (s.get(e.name, &a)) CHECK(fresh.get(e.name, &b) && a == b);
    }
    CHECK(switch_now("AQC_SVD_BLOCKED") == 1 && switch_now("AQC_CD_CHAIN") == 0);
    CHECK(switch_now_seconds("AQC_COMM_TIMEOUT_S") == 300.0);

    // ---- values: negative, 64-bit, trailing garbage, no digits at all ----
    clear_all();
    set("AQC_GRAPH", "0");
    set("AQC_SWEEP_GRID", "-5");
    set("AQC_PROJECTED_VDAG_MIN_ELEMS", "4294967296");
    set("AQC_SPARSE_MIN_ITEMS", "3x");
    set("AQC_LOW_BITS", " 2");
    set("AQC_THREADS", "abc");
    s = read_switches();
    CHECK(s.graph == 0 && s.sweep_grid == -5 && s.projected_vdag_min_elems == 4294967296ll && s.sparse_min_items == 3);
    CHECK(s.low_bits == 2 && s.threads == 0);
    CHECK(s.get("AQC_PROJECTED_VDAG_MIN_ELEMS", &v) && v == 4294967296ll);
    CHECK(s.lazy_z == 1 && s.projected == 1);   // (the others keep their defaults)
    set("AQC_CD_CHAIN", "2");
    CHECK(switch_now("AQC_CD_CHAIN") == 2);     // any non-zero value takes the wide route
    set("AQC_CD_CHAIN", "0");
    CHECK(switch_now("AQC_CD_CHAIN") == 0);
    set("AQC_SVD_BLOCKED", "0");
    CHECK(switch_now("AQC_SVD_BLOCKED") == 0);
    set("AQC_DEVICE", "3");
    CHECK(switch_now("AQC_DEVICE") == 3);

    // ---- the older spelling of the kernel family; a set AQC_KERNEL_FAMILY wins ----
    clear_all();
    set("AQC_KERNEL_V2", "1");
    CHECK(read_switches().kernel_family == 2);
    set("AQC_KERNEL_V2", "0");
    CHECK(read_switches().kernel_family == 1);
    set("AQC_KERNEL_FAMILY", "3");
    CHECK(read_switches().kernel_family == 3);
    set("AQC_KERNEL_FAMILY", "");               // empty counts as unset: the older spelling again
    CHECK(read_switches().kernel_family == 1);
    set("AQC_KERNEL_V2", "-1");
    CHECK(read_switches().kernel_family == 0);

    // ---- seconds: fractional; <= 0 and text fall back to the default ----
    set("AQC_COMM_TIMEOUT_S", "0.25");
    CHECK(switch_now_seconds("AQC_COMM_TIMEOUT_S") == 0.25);
    set("AQC_COMM_TIMEOUT_S", "0");
    CHECK(switch_now_seconds("AQC_COMM_TIMEOUT_S") == 300.0);
    set("AQC_COMM_TIMEOUT_S", "-3");
    CHECK(switch_now_seconds("AQC_COMM_TIMEOUT_S") == 300.0);
    set("AQC_COMM_TIMEOUT_S", "soon");
    CHECK(switch_now_seconds("AQC_COMM_TIMEOUT_S") == 300.0);
    set("AQC_COMM_INIT_TIMEOUT_S", "1.5e1");
    CHECK(switch_now_seconds("AQC_COMM_INIT_TIMEOUT_S") == 15.0);

    printf("switches: %d in the table, %d read at creation, %d failures\n", kNumSwitches, seen, failures);
    return failures ? 1 : 0;
}
