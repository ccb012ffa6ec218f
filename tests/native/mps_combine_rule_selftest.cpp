// Self-test of csrc/aqc_mps_combine_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_combine_rule.py): the
// summed bonds, block offsets and site offsets, the route at the cap, the checks of a term table, and the assembled sites of
// mps_combine_site contracted to the dense vector against sum_k c_k psi_k for n = 1 .. 5 with 1 .. 4 terms (a state listed twice among
// them); every element of a site is written, the blocks off the diagonal are exact zeros.
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_combine_rule.h"

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

struct State {
    std::vector<int> dims;
    std::vector<std::vector<cd>> sites;
};
static State random_state(const std::vector<int>& dims) {
    State st;
    st.dims = dims;
    const int n = (int)dims.size() - 1;
    for (int q = 0; q < n; ++q) {
        st.sites.emplace_back((size_t)2 * dims[q] * dims[q + 1]);
        for (cd& x : st.sites.back()) x = cd(uniform(), uniform());
    }
    return st;
}
// psi(b) at index sum_q b_q 2^q
static std::vector<cd> dense(int n, const int* dims, const std::vector<std::vector<cd>>& sites) {
    std::vector<cd> psi((size_t)1 << n);
    for (size_t b = 0; b < psi.size(); ++b) {
        std::vector<cd> row(1, cd(1.0, 0.0));
        for (int q = 0; q < n; ++q) {
            const int s = (int)(b >> q) & 1, r = dims[q], c = dims[q + 1];
            std::vector<cd> next(c, cd(0.0, 0.0));
            for (int i = 0; i < r; ++i)
                for (int j = 0; j < c; ++j) next[j] += row[i] * sites[q][((size_t)s * r + i) * c + j];
            row.swap(next);
        }
        psi[b] = row[0];
    }
    return psi;
}

static void sum_case(const std::vector<State>& pool, const std::vector<int>& terms) {
    const int n = (int)pool[0].dims.size() - 1, K = (int)terms.size();
    std::vector<int> dims;
    std::vector<cd> coeffs(K);
    for (int k = 0; k < K; ++k) {
        dims.insert(dims.end(), pool[terms[k]].dims.begin(), pool[terms[k]].dims.end());
        coeffs[k] = cd(uniform(), uniform());
    }
    const std::vector<int> sum = mps_combine_dims(n, K, dims.data());
    const std::vector<int> off = mps_combine_block_offsets(n, K, dims.data());
    const std::vector<size_t> site_off = mps_combine_site_offsets(n, K, dims.data());
    CHECK(sum[0] == 1 && sum[n] == 1 && (int)off.size() == (K + 1) * (n + 1) && (int)site_off.size() == n + 1);
    int widest = 1;
    for (int q = 0; q <= n; ++q) {
        CHECK(off[(size_t)K * (n + 1) + q] == sum[q]);
        widest = sum[q] > widest ? sum[q] : widest;
        if (q < n) CHECK(site_off[q + 1] - site_off[q] == (size_t)2 * sum[q] * sum[q + 1]);
        for (int k = 0; k < K; ++k) {
            const int width = off[(size_t)(k + 1) * (n + 1) + q] - off[(size_t)k * (n + 1) + q];
            if (q > 0 && q < n) CHECK(width == pool[terms[k]].dims[q]);
            else CHECK(off[(size_t)k * (n + 1) + q] == 0);
        }
    }
    CHECK(mps_combine_max_bond(n, K, dims.data()) == widest);
    std::vector<std::vector<cd>> assembled(n);
    for (int q = 0; q < n; ++q) {
        std::vector<const cd*> sites(K);
        for (int k = 0; k < K; ++k) sites[k] = pool[terms[k]].sites[q].data();
        assembled[q].assign(3, cd(std::numeric_limits<double>::quiet_NaN(), 0.0));   // (every element must be set)
        mps_combine_site(n, K, dims.data(), q, sites.data(), coeffs.data(), assembled[q]);
        CHECK(assembled[q].size() == site_off[q + 1] - site_off[q]);
        size_t zeros = 0, want_zeros = (size_t)2 * sum[q] * sum[q + 1];
        for (const cd& x : assembled[q]) {
            CHECK(std::isfinite(x.real()) && std::isfinite(x.imag()));
            if (x == cd(0.0, 0.0)) ++zeros;
        }
        for (int k = 0; k < K; ++k) want_zeros -= pool[terms[k]].sites[q].size();
        if (n > 1) CHECK(zeros == want_zeros);   // (random entries are never zero)
    }
    const std::vector<cd> got = dense(n, sum.data(), assembled);
    std::vector<cd> want(got.size(), cd(0.0, 0.0));
    double scale = 0.0;
    for (int k = 0; k < K; ++k) {
        const std::vector<cd> psi = dense(n, pool[terms[k]].dims.data(), pool[terms[k]].sites);
        double nrm = 0.0;
        for (size_t b = 0; b < psi.size(); ++b) { want[b] += coeffs[k] * psi[b]; nrm += std::norm(psi[b]); }
        scale += std::abs(coeffs[k]) * std::sqrt(nrm);
    }
    double err = 0.0;
    for (size_t b = 0; b < got.size(); ++b) err = std::fmax(err, std::abs(got[b] - want[b]));
    CHECK(err <= 1e-13 * scale);
}

int main() {
    // sums of states
    const std::vector<std::vector<std::vector<int>>> profiles = {
        {{1, 1}, {1, 1}, {1, 1}},
        {{1, 2, 1}, {1, 1, 1}, {1, 2, 1}},
        {{1, 2, 2, 1}, {1, 1, 2, 1}, {1, 2, 1, 1}},
        {{1, 2, 3, 2, 1}, {1, 1, 1, 1, 1}, {1, 2, 4, 2, 1}, {1, 2, 2, 2, 1}},
        {{1, 2, 4, 3, 2, 1}, {1, 2, 3, 4, 2, 1}, {1, 1, 1, 1, 1, 1}},
    };
    for (const auto& set : profiles) {
        std::vector<State> pool;
        for (const auto& dims : set) pool.push_back(random_state(dims));
        sum_case(pool, {0});
        sum_case(pool, {0, 1});
        sum_case(pool, {2, 0, 1});
        sum_case(pool, {1, 1});
        sum_case(pool, {0, 2, 0, 1});
    }
    {   // the route at the cap: 4 x 16 = 64 fused, one more canonical; the sum of many bonds does not wrap
        std::vector<int> d;
        for (int k = 0; k < 5; ++k) for (int v : {1, 2, k < 4 ? 16 : 1, 2, 1}) d.push_back(v);
        CHECK(mps_combine_route(4, 4, d.data()) == kMpsEntFused && mps_combine_max_bond(4, 4, d.data()) == 64);
        CHECK(mps_combine_route(4, 5, d.data()) == kMpsEntCanonical && mps_combine_max_bond(4, 5, d.data()) == 65);
        CHECK(mps_combine_route(1, 5, d.data()) == kMpsEntFused);
        const int big[6] = {1, 2147483647, 1, 1, 2147483647, 1};
        CHECK(mps_combine_max_bond(2, 2, big) == 2 * 2147483647ll && mps_combine_route(2, 2, big) == kMpsEntCanonical);
    }
    {   // term tables
        const int off_ok[4] = {0, 1, 3, 6}, st_ok[6] = {0, 1, 2, 0, 0, 2};
        CHECK(mps_combine_check_terms(3, 3, off_ok, st_ok) == 0);
        const int off_first[4] = {1, 2, 3, 6};
        CHECK(mps_combine_check_terms(3, 3, off_first, st_ok) == 1);
        const int off_empty[4] = {0, 1, 1, 6}, off_back[4] = {0, 3, 2, 6};
        CHECK(mps_combine_check_terms(3, 3, off_empty, st_ok) == 2 && mps_combine_check_terms(3, 3, off_back, st_ok) == 2);
        const int st_high[6] = {0, 1, 3, 0, 0, 2}, st_neg[6] = {0, 1, 2, 0, -1, 2};
        CHECK(mps_combine_check_terms(3, 3, off_ok, st_high) == 3 && mps_combine_check_terms(3, 3, off_ok, st_neg) == 3);
        CHECK(mps_combine_check_terms(4, 3, off_ok, st_high) == 0);
    }
    {   // owners at the block borders
        const int dims[10] = {1, 3, 2, 4, 1, 1, 2, 5, 1, 1};
        const std::vector<int> off = mps_combine_block_offsets(4, 2, dims);
        CHECK(mps_combine_owner(2, 4, off.data(), 1, 2) == 0 && mps_combine_owner(2, 4, off.data(), 1, 3) == 1 && mps_combine_owner(2, 4, off.data(), 1, 4) == 1);
        CHECK(mps_combine_owner(2, 4, off.data(), 2, 0) == 0 && mps_combine_owner(2, 4, off.data(), 2, 6) == 1);
        const MpsCombineSource off_diag = mps_combine_source(4, 2, off.data(), 1, (size_t)0 * 7 + 2);   // row 0 (term 0), column 2 (term 1)
        CHECK(off_diag.term == -1);
        const MpsCombineSource second = mps_combine_source(4, 2, off.data(), 1, (size_t)5 * 7 * 1 + 4 * 7 + 6);   // s = 1, row 4, column 6
        CHECK(second.term == 1 && second.elem == (size_t)(1 * 2 + 1) * 5 + 4);
    }
    std::printf("mps_combine_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
