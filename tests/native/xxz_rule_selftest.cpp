// Stand-alone driver of csrc/aqc_xxz_rule.h for tests/test_xxz_host.py (g++ -std=c++17 under ASan + UBSan; no HIP).
//   xxz_rule_selftest mul      stdin: n delta, then 2^n (re im) pairs     stdout: H psi by the header's rule in a plain host loop
//   xxz_rule_selftest bessel   stdin: x                                   stdout: K, then J_0 .. J_K(x)
//   xxz_rule_selftest coef     stdin: x (signed)                          stdout: K, then c_0 .. c_K as (re im) pairs
// Doubles travel as hex bit patterns.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_xxz_rule.h"

static bool read_f64(double& v) {
    uint64_t bits;
    if (scanf("%" SCNx64, &bits) != 1) return false;
    memcpy(&v, &bits, sizeof v);
    return true;
}

static void print_f64(double v) {
    uint64_t bits;
    memcpy(&bits, &v, sizeof v);
    printf("%016" PRIx64 "\n", bits);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "mul")) {
        int n;
        double delta;
        if (scanf("%d", &n) != 1 || n < aqc::kXxzMinQubits || n > 20 || !read_f64(delta)) return 2;
        const uint64_t dim = (uint64_t)1 << n;
        std::vector<double> psi(2 * dim), out(2 * dim);
        for (double& v : psi)
            if (!read_f64(v)) return 2;
        for (uint64_t s = 0; s < dim; ++s) {
            const uint64_t a = aqc::xxz_anti(s, n);
            double sr = 0.0, si = 0.0;
            for (int i = 0; i + 1 < n; ++i)
                if ((a >> i) & 1) {
                    const uint64_t p = aqc::xxz_partner(s, i);
                    if (p >= dim) return 3;
                    sr += psi[2 * p]; si += psi[2 * p + 1];
                }
            const double d = aqc::xxz_diag(a, n, delta);
            out[2 * s] = d * psi[2 * s] - 0.5 * sr;
            out[2 * s + 1] = d * psi[2 * s + 1] - 0.5 * si;
        }
        for (double v : out) print_f64(v);
        return 0;
    }
    const bool coef = !strcmp(argv[1], "coef");
    if (!coef && strcmp(argv[1], "bessel")) return 2;
    double x;
    if (!read_f64(x)) return 2;
    std::vector<double> J;
    const int K = aqc::xxz_series(x < 0 ? -x : x, J);
    printf("%d\n", K);
    if (K < 0) return 0;
    if ((int)J.size() != K + 1) return 3;
    for (int k = 0; k <= K; ++k) {
        if (!coef) { print_f64(J[k]); continue; }
        double re, im;
        aqc::xxz_coefficient(k, J[k], x < 0, re, im);
        print_f64(re);
        print_f64(im);
    }
    return 0;
}
