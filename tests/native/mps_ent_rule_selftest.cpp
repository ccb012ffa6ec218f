// Self-test of csrc/aqc_mps_ent_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_ent_rule.py): the Householder
// R of tall, square and wide matrices held to R^H R = M^H M, zero columns and the zero matrix, the mapping of the stacked rows onto the
// planes, the route, the factor offsets, the chunks of the SVD batch and the rank rule on hand-worked spectra.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_ent_rule.h"

using namespace aqc;
typedef std::complex<double> cd;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, in (-1, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 4503599627370496.0 - 1.0;
}

// max |R^H R - M^H M| and |M|_F^2 of the R factor the rule leaves of m; also checks that everything below the diagonal is exactly zero
static double gram_defect(int rows, int cols, const std::vector<cd>& m, double* fro2) {
    std::vector<cd> r(m);
    mps_ent_householder_r(rows, cols, r.data());
    for (int i = 1; i < rows; ++i)
        for (int c = 0; c < i && c < cols; ++c) CHECK(r[(size_t)i * cols + c] == cd(0.0, 0.0));
    *fro2 = 0.0;
    for (const cd& x : m) *fro2 += std::norm(x);
    const int k = mps_ent_r_rows(rows, cols);
    double worst = 0.0;
    for (int a = 0; a < cols; ++a)
        for (int b = 0; b < cols; ++b) {
            cd want = 0.0, got = 0.0;
            for (int i = 0; i < rows; ++i) want += std::conj(m[(size_t)i * cols + a]) * m[(size_t)i * cols + b];
            for (int i = 0; i < k; ++i) got += std::conj(r[(size_t)i * cols + a]) * r[(size_t)i * cols + b];
            const double d = std::abs(want - got);
            worst = d > worst ? d : worst;
        }
    return worst;
}

int main() {
    const double eps = 2.220446049250313e-16;
    {   // R^H R = M^H M within 64 eps |M|_F^2: tall, square, wide; a zero column; the zero matrix
        const int shapes[][2] = {{2, 2}, {10, 7}, {128, 64}, {2, 5}, {1, 3}, {6, 6}};
        for (const auto& sh : shapes) {
            const int rows = sh[0], cols = sh[1];
            std::vector<cd> m((size_t)rows * cols);
            for (cd& x : m) x = cd(uniform(), uniform());
            double fro2 = 0.0;
            double d = gram_defect(rows, cols, m, &fro2);
            std::printf("%3d x %2d: max |R^H R - M^H M| = %.3g (|M|_F^2 = %.3g)\n", rows, cols, d, fro2);
            CHECK(d <= 64.0 * eps * fro2);
            if (cols > 1) {   // column 1 exactly zero: its reflection is skipped
                for (int i = 0; i < rows; ++i) m[(size_t)i * cols + 1] = 0.0;
                d = gram_defect(rows, cols, m, &fro2);
                CHECK(d <= 64.0 * eps * fro2);
            }
            for (int i = 0; i < rows; ++i) m[(size_t)i * cols] = 0.0;   // and column 0
            d = gram_defect(rows, cols, m, &fro2);
            CHECK(d <= 64.0 * eps * fro2);
            std::fill(m.begin(), m.end(), cd(0.0, 0.0));
            d = gram_defect(rows, cols, m, &fro2);
            CHECK(d == 0.0 && fro2 == 0.0);
            std::vector<cd> r(m);
            mps_ent_householder_r(rows, cols, r.data());
            for (const cd& x : r) CHECK(x == cd(0.0, 0.0));
        }
        // a rank-1 matrix: R has one non-zero row to rounding
        std::vector<cd> m(12 * 5);
        for (int i = 0; i < 12; ++i)
            for (int c = 0; c < 5; ++c) m[(size_t)i * 5 + c] = cd(i + 1.0, 0.5 * i) * cd(c - 2.0, 1.0);
        double fro2 = 0.0;
        CHECK(gram_defect(12, 5, m, &fro2) <= 64.0 * eps * fro2);
        // the reflection itself: H x = alpha e_0 with |alpha| = |x|
        const MpsEntReflection h = mps_ent_reflection(3.0, 4.0, 25.0 + 144.0);
        CHECK(std::abs(std::abs(cd(h.alphar, h.alphai)) - 13.0) < 1e-14 && std::abs(cd(h.alphar, h.alphai) + cd(3.0, 4.0) * (13.0 / 5.0)) < 1e-14);
        CHECK(std::abs(h.tau - 2.0 / (std::norm(cd(h.v0r, h.v0i)) + 144.0)) < 1e-17);
        const MpsEntReflection z = mps_ent_reflection(0.0, 0.0, 4.0);   // a zero leading entry: phase 1
        CHECK(z.v0r == 2.0 && z.v0i == 0.0 && z.alphar == -2.0 && z.alphai == 0.0);
    }
    {   // the stacked rows, the reflections and the rows of R
        for (int chi = 1; chi <= 64; chi += 7)
            for (int r = 0; r < 2 * chi; ++r) {
                const MpsEntRow at = mps_ent_stacked_row(r, chi);
                CHECK(at.plane == (r < chi ? 0 : 1) && at.row == (r < chi ? r : r - chi) && at.row >= 0 && at.row < chi);
            }
        CHECK(mps_ent_stacked_row(0, 1).plane == 0 && mps_ent_stacked_row(1, 1).plane == 1 && mps_ent_stacked_row(1, 1).row == 0);
        CHECK(mps_ent_stacked_row(63, 64).plane == 0 && mps_ent_stacked_row(64, 64).plane == 1 && mps_ent_stacked_row(127, 64).row == 63);
        CHECK(mps_ent_reflections(2, 2) == 1 && mps_ent_reflections(10, 7) == 7 && mps_ent_reflections(128, 64) == 64 && mps_ent_reflections(2, 5) == 1);
        CHECK(mps_ent_reflections(1, 3) == 0 && mps_ent_r_rows(2, 5) == 2 && mps_ent_r_rows(10, 7) == 7 && mps_ent_r_rows(6, 6) == 6);
    }
    {   // route, offsets, chunks
        static_assert(kMpsEntFusedCap <= 64, "the chain kernel keeps the stacked matrix in four 64-row planes");
        std::vector<int> a = {1, 2, 4, 64, 64, 7, 1}, b = {1, 2, 65, 2, 1}, one = {1, 1};
        CHECK(mps_ent_route(6, a.data()) == kMpsEntFused && mps_max_bond(6, a.data()) == 64);
        CHECK(mps_ent_route(4, b.data()) == kMpsEntCanonical && mps_ent_route(1, one.data()) == kMpsEntFused);
        CHECK(mps_ent_method_ok(0) && mps_ent_method_ok(1) && mps_ent_method_ok(2) && !mps_ent_method_ok(3) && !mps_ent_method_ok(-1));
        CHECK(mps_ent_cuts(1) == 0 && mps_ent_cuts(2) == 1 && mps_ent_cuts(40) == 39);
        const std::vector<size_t> off = mps_ent_factor_offsets(6, a.data());
        CHECK(off.size() == 7 && off[1] == 0 && off[2] == 4 && off[3] == 20 && off[4] == 20 + 4096 && off[6] == 20 + 2 * 4096 + 49);
        CHECK(mps_ent_factor_offsets(1, one.data()).back() == 0);
        CHECK(mps_ent_chunk(64, 496, (size_t)256 << 20) == 496 && mps_ent_chunk(64, 5000, (size_t)256 << 20) == 819);
        CHECK(mps_ent_chunk(64, 120, (size_t)1 << 20) == 3 && mps_ent_chunk(64, 120, 1) == 1 && mps_ent_chunk(1, 7, 1000) == 7);
    }
    {   // the rank rule, worked by hand
        int k = -1;
        double d = -1.0;
        const double s1[] = {1.0, 0.5, 0.1, 1e-3, 1e-15, 0.0};
        CHECK(mps_rank_rule(6, s1, 0.0, 0, &k, &d) && k == 4 && d == 0.0);                       // the floor alone
        CHECK(mps_rank_rule(6, s1, 0.0, 2, &k, &d) && k == 2 && d == 0.0);                       // the cap
        CHECK(mps_rank_rule(6, s1, 2e-6, 0, &k, &d) && k == 3 && d == 1e-3 * 1e-3);              // 1e-6 < 2e-6 goes, 1e-6 + 1e-2 stays
        CHECK(mps_rank_rule(6, s1, 1e-6, 0, &k, &d) && k == 4 && d == 0.0);                      // strictly below: 1e-6 < 1e-6 is false
        CHECK(mps_rank_rule(6, s1, 0.02, 0, &k, &d) && k == 2 && d == 1e-3 * 1e-3 + 0.1 * 0.1);  // 1e-6 + 1e-2 < 0.02; + 0.25 is not
        CHECK(mps_rank_rule(6, s1, 100.0, 0, &k, &d) && k == 1);                                 // the last value always stays
        CHECK(mps_rank_rule(6, s1, 0.02, 3, &k, &d) && k == 2 && d == 0.1 * 0.1);                // the cap first, then the tail
        const double s2[] = {2.0, 2.1e-14, 1.9e-14};
        CHECK(mps_rank_rule(3, s2, 0.0, 0, &k, &d) && k == 2);                                   // the floor is 1e-14 s_max = 2e-14
        const double s3[] = {5.0};
        CHECK(mps_rank_rule(1, s3, 1.0, 7, &k, &d) && k == 1 && d == 0.0);
        const double zero[] = {0.0, 0.0}, nan[] = {std::nan(""), 1.0}, inf[] = {HUGE_VAL, 1.0};
        k = 77;
        CHECK(!mps_rank_rule(2, zero, 0.0, 0, &k, &d) && !mps_rank_rule(2, nan, 0.0, 0, &k, &d) && !mps_rank_rule(2, inf, 0.0, 0, &k, &d) && k == 77);
    }
    std::printf("mps_ent_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
