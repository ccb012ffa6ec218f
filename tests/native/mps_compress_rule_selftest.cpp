// Self-test of csrc/aqc_mps_compress_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_compress_rule.py): the
// decision of a cut in its host-and-device form against mps_rank_rule on 200 random spectra (values under the floor, caps and tails
// among them) and on spectra that must be refused, one step of the rule on a 6 x 3 and a 2 x 5 stacked matrix against a direct
// computation, the route, the offsets and the chunks.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_compress_rule.h"

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

// rows x k with orthonormal columns (modified Gram-Schmidt, twice)
static std::vector<cd> orthonormal(int rows, int k) {
    std::vector<cd> u((size_t)rows * k);
    for (cd& x : u) x = cd(uniform(), uniform());
    for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j < k; ++j) {
            for (int p = 0; p < j; ++p) {
                cd dot = 0.0;
                for (int i = 0; i < rows; ++i) dot += std::conj(u[(size_t)i * k + p]) * u[(size_t)i * k + j];
                for (int i = 0; i < rows; ++i) u[(size_t)i * k + j] -= dot * u[(size_t)i * k + p];
            }
            double nrm = 0.0;
            for (int i = 0; i < rows; ++i) nrm += std::norm(u[(size_t)i * k + j]);
            nrm = std::sqrt(nrm);
            for (int i = 0; i < rows; ++i) u[(size_t)i * k + j] /= nrm;
        }
    return u;
}

// one step on a rows x cols stacked matrix M = U X (so that U U^H M = M) with the given spectrum, against a direct computation
static void step_case(int rows, int cols, const std::vector<double>& s, double thr, int cap, int want_rank) {
    const double eps = 2.220446049250313e-16;
    const int count = std::min(rows, cols), rq = rows / 2;
    CHECK((int)s.size() == count);
    const std::vector<cd> u = orthonormal(rows, count);
    std::vector<cd> x((size_t)count * cols), m((size_t)rows * cols, cd(0.0, 0.0));
    for (cd& v : x) v = cd(uniform(), uniform());
    for (int i = 0; i < rows; ++i)
        for (int c = 0; c < cols; ++c)
            for (int j = 0; j < count; ++j) m[(size_t)i * cols + c] += u[(size_t)i * count + j] * x[(size_t)j * cols + c];
    std::vector<double> lam_left(rq);
    for (int l = 0; l < rq; ++l) lam_left[l] = 0.25 + 0.5 * (l + 1);
    const MpsCompressStep st = mps_compress_step(rows, cols, m.data(), u.data(), count, s.data(), lam_left.data(), thr, cap);
    CHECK(st.d.ok == 1 && st.d.rank == want_rank);
    const int r = st.d.rank;
    double total = 0.0, kept = 0.0;
    for (int j = count - 1; j >= 0; --j) { total += s[j] * s[j]; if (j < r) kept += s[j] * s[j]; }   // (the other order of summation)
    CHECK(std::fabs(st.d.total - total) <= 8 * eps * total && std::fabs(st.d.kept - kept) <= 8 * eps * total);
    const double rescale = std::sqrt(total / kept);
    CHECK(std::fabs(st.d.rescale - rescale) <= 8 * eps * rescale);
    CHECK((int)st.lam.size() == r && (int)st.site.size() == rows * r && (int)st.carry.size() == r * cols);
    double worst = 0.0;
    for (int j = 0; j < r; ++j) worst = std::max(worst, std::fabs(st.lam[j] - rescale * s[j]));
    for (int a = 0; a < 2; ++a)
        for (int l = 0; l < rq; ++l)
            for (int j = 0; j < r; ++j) {
                const cd want = u[(size_t)(a * rq + l) * count + j] * (rescale * s[j]) / lam_left[l];
                worst = std::max(worst, std::abs(st.site[((size_t)a * rq + l) * r + j] - want));
            }
    // the carry: U[:, :r] (carry / rescale) is the projection of M on the kept columns; with every column kept it is M itself
    for (int i = 0; i < rows; ++i)
        for (int c = 0; c < cols; ++c) {
            cd got = 0.0, want = 0.0;
            for (int j = 0; j < r; ++j) got += u[(size_t)i * count + j] * st.carry[(size_t)j * cols + c] / rescale;
            for (int j = 0; j < r; ++j) want += u[(size_t)i * count + j] * x[(size_t)j * cols + c];
            worst = std::max(worst, std::abs(got - want));
            if (r == count) worst = std::max(worst, std::abs(got - m[(size_t)i * cols + c]));
        }
    std::printf("step %d x %d, rank %d of %d: max deviation %.3g\n", rows, cols, r, count, worst);
    CHECK(worst <= 256 * eps);
    // without a vector on the left the divisor is 1
    const MpsCompressStep first = mps_compress_step(rows, cols, m.data(), u.data(), count, s.data(), nullptr, thr, cap);
    CHECK(first.d.rank == r && std::abs(first.site[0] - u[0] * first.lam[0]) <= 8 * eps);
}

int main() {
    {   // the decision against mps_rank_rule: the same rank and the same tail weight, bit for bit
        int taken = 0, floors = 0, caps = 0, tails = 0;
        for (int trial = 0; taken < 200 && trial < 4000; ++trial) {
            const int size = 1 + (int)(19.5 * (uniform() + 1.0));
            std::vector<double> s(size);
            for (double& v : s) v = std::fabs(uniform()) * std::pow(10.0, -4.5 * (uniform() + 1.0));
            std::sort(s.begin(), s.end(), [](double a, double b) { return a > b; });
            const bool under = uniform() < -0.4;
            if (under)
                for (int j = size / 2; j < size; ++j) s[j] *= 1e-16;
            const double thr = uniform() < -0.5 ? 0.0 : std::pow(10.0, -7.0 * (uniform() + 1.0));
            const int cap = uniform() < 0.0 ? 0 : 1 + (int)(19.5 * (uniform() + 1.0));
            if (!(s[0] > 0.0)) continue;
            int rank = -1;
            double dropped = -1.0;
            CHECK(mps_rank_rule(size, s.data(), thr, cap, &rank, &dropped));
            const MpsCompressDecision d = mps_compress_decide(size, s.data(), thr, cap);
            CHECK(d.ok == 1 && d.rank == rank && d.tail == dropped);
            double total = 0.0, kept = 0.0;
            for (int j = 0; j < size; ++j) total += s[j] * s[j];
            for (int j = 0; j < rank; ++j) kept += s[j] * s[j];
            CHECK(d.total == total && d.kept == kept && d.rescale == std::sqrt(total / kept) && std::fabs((d.total - d.kept) - d.tail) <= 8 * 2.220446049250313e-16 * total + (cap > 0 || under ? total : 0.0));   // (the tail alone when neither floor nor cap took anything)
            int above = 0;
            for (int j = 0; j < size; ++j) above = s[j] > kMpsRankFloor * s[0] ? j + 1 : above;
            floors += above < size;
            caps += cap > 0 && cap < above;
            tails += dropped > 0.0;
            ++taken;
        }
        std::printf("decisions: %d spectra, %d with values under the floor, %d cut by max_bond, %d with a tail dropped\n", taken, floors, caps, tails);
        CHECK(taken == 200 && floors >= 20 && caps >= 20 && tails >= 20);
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        const double bad[][2] = {{0.0, 0.0}, {nan, 1.0}, {inf, 1.0}, {-1.0, -2.0}};
        for (const auto& s : bad) {
            int rank = 7;
            double dropped = 7.0;
            CHECK(!mps_rank_rule(2, s, 0.0, 0, &rank, &dropped) && rank == 7 && dropped == 7.0);
            CHECK(mps_compress_decide(2, s, 0.0, 0).ok == 0);
        }
        const double hand[6] = {1.0, 0.5, 0.1, 1e-3, 1e-15, 0.0};
        CHECK(mps_compress_decide(6, hand, 0.0, 0).rank == 4 && mps_compress_decide(6, hand, 0.0, 0).tail == 0.0);
        const MpsCompressDecision d = mps_compress_decide(6, hand, 0.02, 3);
        CHECK(d.rank == 2 && d.tail == 0.1 * 0.1 && std::fabs((d.total - d.kept) - (0.01 + 1e-6 + 1e-30)) <= 1e-15);
        CHECK(mps_compress_site_factor(3.0, 1.5) == 2.0);
    }
    {   // the index of a packed site element, shared by host and device, against the % form: every element for r = 1 .. 5, rk = 1 .. 2 r
        int checked = 0;
        for (int r = 1; r <= 5; ++r)
            for (int rk = 1; rk <= 2 * r; ++rk)
                for (int e = 0; e < 2 * r * rk; ++e, ++checked) {
                    const MpsCompressSiteIndex at = mps_compress_site_index(e, r, rk);
                    CHECK(at.row == e / rk && at.j == e % rk && at.l == (e / rk) % r && at.row * rk + at.j == e && at.row < 2 * r);
                }
        std::printf("site index: %d elements\n", checked);
        CHECK(checked == 2 * (1 * 3 + 2 * 10 + 3 * 21 + 4 * 36 + 5 * 55));
    }
    // one step: a tall stacked matrix (three values, one dropped by the threshold; all kept) and a wide one (two values; capped to one)
    step_case(6, 3, {2.0, 0.5, 0.01}, 1e-3, 0, 2);
    step_case(6, 3, {2.0, 0.5, 0.01}, 0.0, 0, 3);
    step_case(2, 5, {1.5, 0.25}, 0.0, 0, 2);
    step_case(2, 5, {1.5, 0.25}, 0.0, 1, 1);
    {   // a zero spectrum fails the step and leaves nothing
        const std::vector<cd> u = orthonormal(2, 2), m(10, cd(0.0, 0.0));
        const double zero[2] = {0.0, 0.0};
        const MpsCompressStep st = mps_compress_step(2, 5, m.data(), u.data(), 2, zero, nullptr, 0.0, 0);
        CHECK(st.d.ok == 0 && st.lam.empty() && st.site.empty() && st.carry.empty());
    }
    {   // route, offsets, chunks
        const int small[] = {1, 2, 64, 64, 2, 1}, large[] = {1, 2, 65, 2, 1}, one[] = {1, 1};
        CHECK(mps_compress_route(5, small) == kMpsEntFused && mps_compress_route(4, large) == kMpsEntCanonical && mps_compress_route(1, one) == kMpsEntFused);
        const int dims[] = {1, 2, 3, 2, 1};
        const std::vector<size_t> so = mps_site_offsets(4, dims), lo = mps_compress_lam_offsets(4, dims);
        CHECK(so.size() == 5 && so[0] == 0 && so[1] == 4 && so[2] == 16 && so[3] == 28 && so[4] == 32);
        CHECK(lo.size() == 4 && lo[0] == 0 && lo[1] == 2 && lo[2] == 5 && lo[3] == 7);
        CHECK(mps_compress_lam_offsets(1, one).size() == 1 && mps_site_offsets(1, one)[1] == 2);
        const size_t budget = (size_t)256 << 20;
        CHECK(mps_compress_chunk(64, 16, budget) == 16 && mps_compress_chunk(64, 100000, budget) == 512 && mps_compress_chunk(1, 5, 1) == 1);
        CHECK((size_t)mps_compress_chunk(64, 100000, budget) * 8 * 16 * 64 * 64 <= budget);
    }
    std::printf("mps_compress_rule selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
