// Host build of csrc/aqc_cd_rule.h (tests/test_cd_host.py, under ASan + UBSan).
//   cd_rule_selftest delta inv_d2n kind gr gi pr pi [kind gr gi pr pi ...] : the step of every tuple, as hex of the double's bits
//   cd_rule_selftest close fobj_thr dtheta_thr maxiter f1 d1 [f2 d2 ...]   : the close rule fed sweep by sweep (objective, max |dtheta|)
//       while the lane runs; per sweep "nit best_f(hex) status improved", then the profile's nit entries (hex) on one line
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_cd_rule.h"

static uint64_t bits_of(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char** argv) {
    if (argc >= 8 && !strcmp(argv[1], "delta") && (argc - 3) % 5 == 0) {
        const double inv_d2n = strtod(argv[2], nullptr);
        for (int i = 3; i < argc; i += 5) {
            double dt = 0;
            aqc::cd_delta(atoi(argv[i]), strtod(argv[i + 1], nullptr), strtod(argv[i + 2], nullptr), strtod(argv[i + 3], nullptr),
                          strtod(argv[i + 4], nullptr), inv_d2n, dt);
            printf("%016" PRIx64 "\n", bits_of(dt));
        }
        return 0;
    }
    if (argc >= 7 && !strcmp(argv[1], "close") && (argc - 5) % 2 == 0) {
        const double fobj_thr = strtod(argv[2], nullptr), dtheta_thr = strtod(argv[3], nullptr);
        const int maxiter = atoi(argv[4]);
        if (maxiter < 1) return 2;
        std::vector<double> profile(maxiter, 0.0);   // exactly maxiter entries: a write past the last sweep is ASan's to find
        int nit = 0, status = aqc::kCdRunning;
        double best = HUGE_VAL;
        for (int i = 5; i < argc && status == aqc::kCdRunning; i += 2) {
            const bool improved = aqc::cd_close(strtod(argv[i], nullptr), strtod(argv[i + 1], nullptr), fobj_thr, dtheta_thr, maxiter,
                                                profile.data(), nit, best, status);
            printf("%d %016" PRIx64 " %d %d\n", nit, bits_of(best), status, improved ? 1 : 0);
        }
        for (int i = 0; i < nit; ++i) printf("%016" PRIx64 "%c", bits_of(profile[i]), i + 1 < nit ? ' ' : '\n');
        return 0;
    }
    fprintf(stderr, "usage: cd_rule_selftest delta inv_d2n (kind gr gi pr pi)... | close fobj_thr dtheta_thr maxiter (fobj dtheta)...\n");
    return 2;
}
