// Self-test of csrc/aqc_mps_opsum_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_opsum_rule.py): the
// product bonds in 64 bits, the route at the cap, the checks of a term table and of an operator's packed layout, and the assembled
// sites of mps_opsum_site -- every element of every site against a brute-force loop over (term, a, b, i, j, s), written once, exact
// zeros elsewhere -- contracted to the dense vector against sum_t c_t O_t psi_t for n = 1 .. 5: an identity term next to an operator
// term, an operator bond of 1 inside a wider operator, a state and an operator listed twice.
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_opsum_rule.h"

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

struct Chain {   // a state (site q: 2 dims[q] dims[q+1] elements) or an operator (site q: 4 dims[q] dims[q+1])
    std::vector<int> dims;
    std::vector<std::vector<cd>> sites;
};
static Chain random_chain(const std::vector<int>& dims, int phys) {
    Chain c;
    c.dims = dims;
    for (size_t q = 0; q + 1 < dims.size(); ++q) {
        c.sites.emplace_back((size_t)phys * dims[q] * dims[q + 1]);
        for (cd& x : c.sites.back()) x = cd(uniform(), uniform());
    }
    return c;
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
// (O psi)(b_out) = sum_{b_in} O(b_out, b_in) psi(b_in), O as the product of its D x D matrices
static std::vector<cd> apply_dense(int n, const Chain& op, const std::vector<cd>& psi) {
    std::vector<cd> out(psi.size(), cd(0.0, 0.0));
    for (size_t bo = 0; bo < psi.size(); ++bo)
        for (size_t bi = 0; bi < psi.size(); ++bi) {
            std::vector<cd> row(1, cd(1.0, 0.0));
            for (int q = 0; q < n; ++q) {
                const int so = (int)(bo >> q) & 1, si = (int)(bi >> q) & 1, r = op.dims[q], c = op.dims[q + 1];
                std::vector<cd> next(c, cd(0.0, 0.0));
                for (int a = 0; a < r; ++a)
                    for (int b = 0; b < c; ++b) next[b] += row[a] * op.sites[q][((size_t)a * c + b) * 4 + 2 * so + si];
                row.swap(next);
            }
            out[bo] += row[0] * psi[bi];
        }
    return out;
}

struct Term { int state, op; };   // op -1: none

static void sum_case(const std::vector<Chain>& states, const std::vector<Chain>& ops, const std::vector<Term>& terms) {
    const int n = (int)states[0].dims.size() - 1, K = (int)terms.size();
    std::vector<int> sdims, odims, widths((size_t)K * (n + 1));
    std::vector<cd> coeffs(K);
    for (int k = 0; k < K; ++k) {
        const std::vector<int>& sd = states[terms[k].state].dims;
        sdims.insert(sdims.end(), sd.begin(), sd.end());
        if (terms[k].op >= 0) odims.insert(odims.end(), ops[terms[k].op].dims.begin(), ops[terms[k].op].dims.end());
        else odims.insert(odims.end(), n + 1, 1);
        coeffs[k] = cd(uniform(), uniform());
        std::vector<long long> wide(n + 1);
        CHECK(mps_opsum_term_dims(n, sd.data(), terms[k].op >= 0 ? ops[terms[k].op].dims.data() : nullptr, wide.data(), widths.data() + (size_t)k * (n + 1)));
        for (int q = 0; q <= n; ++q) CHECK(wide[q] == (long long)sd[q] * odims[(size_t)k * (n + 1) + q] && widths[(size_t)k * (n + 1) + q] == wide[q]);
    }
    const std::vector<int> sum = mps_combine_dims(n, K, widths.data());
    const std::vector<int> off = mps_combine_block_offsets(n, K, widths.data());
    const std::vector<size_t> site_off = mps_combine_site_offsets(n, K, widths.data());
    CHECK(mps_opsum_max_bond(n, K, sdims.data(), odims.data()) == mps_combine_max_bond(n, K, widths.data()));
    std::vector<std::vector<cd>> assembled(n);
    for (int q = 0; q < n; ++q) {
        std::vector<const cd*> sites(K), w(K);
        for (int k = 0; k < K; ++k) {
            sites[k] = states[terms[k].state].sites[q].data();
            w[k] = terms[k].op >= 0 ? ops[terms[k].op].sites[q].data() : nullptr;
        }
        assembled[q].assign(3, cd(std::numeric_limits<double>::quiet_NaN(), 0.0));   // (every element must be set)
        mps_opsum_site(n, K, sdims.data(), odims.data(), q, sites.data(), w.data(), coeffs.data(), assembled[q]);
        CHECK(assembled[q].size() == site_off[q + 1] - site_off[q]);
        // the brute-force statement: every (term, s, a, i, b, j) lands on one element, once; the rest are exact zeros
        std::vector<cd> want(assembled[q].size(), cd(0.0, 0.0));
        std::vector<int> hits(assembled[q].size(), 0);
        for (int k = 0; k < K; ++k) {
            const int* sd = sdims.data() + (size_t)k * (n + 1);
            const int* od = odims.data() + (size_t)k * (n + 1);
            const int r0 = q > 0 ? off[(size_t)k * (n + 1) + q] : 0, c0 = q + 1 < n ? off[(size_t)k * (n + 1) + q + 1] : 0;
            for (int s = 0; s < 2; ++s)
                for (int a = 0; a < od[q]; ++a)
                    for (int i = 0; i < sd[q]; ++i)
                        for (int b = 0; b < od[q + 1]; ++b)
                            for (int j = 0; j < sd[q + 1]; ++j) {
                                const cd t0 = sites[k][((size_t)0 * sd[q] + i) * sd[q + 1] + j], t1 = sites[k][((size_t)1 * sd[q] + i) * sd[q + 1] + j];
                                cd v = s ? t1 : t0;
                                if (w[k]) v = w[k][((size_t)a * od[q + 1] + b) * 4 + 2 * s] * t0 + w[k][((size_t)a * od[q + 1] + b) * 4 + 2 * s + 1] * t1;
                                if (n == 1) { want[s] += coeffs[k] * v; hits[s] = 1; continue; }
                                if (q == 0) v = coeffs[k] * v;
                                const size_t e = ((size_t)s * sum[q] + r0 + a * sd[q] + i) * sum[q + 1] + c0 + b * sd[q + 1] + j;
                                CHECK(e < want.size());
                                if (e < want.size()) { want[e] = v; ++hits[e]; }
                            }
        }
        size_t zeros = 0, unhit = 0;
        for (size_t e = 0; e < want.size(); ++e) {
            CHECK(hits[e] <= 1);
            CHECK(std::isfinite(assembled[q][e].real()) && std::isfinite(assembled[q][e].imag()));
            if (n == 1) CHECK(std::abs(assembled[q][e] - want[e]) <= 1e-14 * K);
            else CHECK(assembled[q][e] == want[e]);                     // the same two products in the same order: the same bits
            if (!hits[e]) { ++unhit; if (assembled[q][e] == cd(0.0, 0.0)) ++zeros; }
        }
        CHECK(zeros == unhit);
    }
    const std::vector<cd> got = dense(n, sum.data(), assembled);
    std::vector<cd> want(got.size(), cd(0.0, 0.0));
    double scale = 0.0;
    for (int k = 0; k < K; ++k) {
        std::vector<cd> psi = dense(n, states[terms[k].state].dims.data(), states[terms[k].state].sites);
        double onorm = 1.0, nrm = 0.0;
        for (const cd& x : psi) nrm += std::norm(x);
        if (terms[k].op >= 0) {
            psi = apply_dense(n, ops[terms[k].op], psi);
            for (const auto& site : ops[terms[k].op].sites) {   // (a bound of |O|_2: the product of the sites' Frobenius norms)
                double f = 0.0;
                for (const cd& x : site) f += std::norm(x);
                onorm *= std::sqrt(f);
            }
        }
        for (size_t b = 0; b < psi.size(); ++b) want[b] += coeffs[k] * psi[b];
        scale += std::abs(coeffs[k]) * onorm * std::sqrt(nrm);
    }
    double err = 0.0;
    for (size_t b = 0; b < got.size(); ++b) err = std::fmax(err, std::abs(got[b] - want[b]));
    CHECK(err <= 1e-13 * scale);
}

int main() {
    struct Set { std::vector<std::vector<int>> states, ops; };
    const std::vector<Set> sets = {
        {{{1, 1}, {1, 1}}, {{1, 1}, {1, 1}}},                                                              // n = 1
        {{{1, 2, 1}, {1, 1, 1}}, {{1, 2, 1}, {1, 1, 1}}},                                                  // n = 2
        {{{1, 2, 2, 1}, {1, 1, 2, 1}}, {{1, 2, 1, 1}, {1, 3, 2, 1}}},                                      // D_2 = 1 inside
        {{{1, 2, 3, 2, 1}, {1, 1, 1, 1, 1}}, {{1, 3, 1, 3, 1}, {1, 2, 4, 2, 1}}},                          // D_2 = 1 between bonds of 3
        {{{1, 2, 4, 3, 2, 1}, {1, 2, 3, 4, 2, 1}}, {{1, 5, 5, 5, 5, 1}, {1, 1, 1, 1, 1, 1}}},
    };
    for (const Set& set : sets) {
        std::vector<Chain> states, ops;
        for (const auto& d : set.states) states.push_back(random_chain(d, 2));
        for (const auto& d : set.ops) ops.push_back(random_chain(d, 4));
        sum_case(states, ops, {{0, 0}});
        sum_case(states, ops, {{0, -1}});
        sum_case(states, ops, {{0, 0}, {0, -1}});                 // an identity term next to an operator term: (O - E) psi
        sum_case(states, ops, {{1, -1}, {0, 1}, {1, 0}});
        sum_case(states, ops, {{0, 0}, {0, 0}});                  // the same state and operator twice
        sum_case(states, ops, {{0, 1}, {1, -1}, {0, -1}, {1, 1}});
    }
    {   // product bonds and the route: 5 x 12 = 60 fused, 5 x 13 = 65 canonical, 64 x 1 fused; 64-bit before any comparison
        const int s12[5] = {1, 2, 12, 2, 1}, s13[5] = {1, 2, 13, 2, 1}, s64[5] = {1, 2, 64, 2, 1}, d5[5] = {1, 5, 5, 5, 1}, d1[5] = {1, 1, 1, 1, 1};
        CHECK(mps_opsum_max_bond(4, 1, s12, d5) == 60 && mps_opsum_route(4, 1, s12, d5) == kMpsEntFused);
        CHECK(mps_opsum_max_bond(4, 1, s13, d5) == 65 && mps_opsum_route(4, 1, s13, d5) == kMpsEntCanonical);
        CHECK(mps_opsum_route(4, 1, s64, d1) == kMpsEntFused && mps_opsum_route(4, 1, s64, nullptr) == kMpsEntFused);
        const int two_s[10] = {1, 2, 12, 2, 1, 1, 2, 4, 2, 1}, two_d[10] = {1, 5, 5, 5, 1, 1, 1, 1, 1, 1};
        CHECK(mps_opsum_max_bond(4, 2, two_s, two_d) == 64 && mps_opsum_route(4, 2, two_s, two_d) == kMpsEntFused);
        const int one_s[4] = {1, 1, 1, 1}, one_d[4] = {1, 1, 1, 1};
        CHECK(mps_opsum_route(1, 2, one_s, one_d) == kMpsEntFused);
        const int big_s[3] = {1, 2147483647, 1}, big_d[3] = {1, 2147483647, 1};
        CHECK(mps_opsum_max_bond(2, 1, big_s, big_d) == 2147483647ll * 2147483647ll && mps_opsum_route(2, 1, big_s, big_d) == kMpsEntCanonical);
        long long wide[3];
        int narrow[3];
        CHECK(!mps_opsum_term_dims(2, big_s, big_d, wide, narrow) && wide[1] == 2147483647ll * 2147483647ll && wide[0] == 1 && wide[2] == 1);
        const int many[9] = {1, 2147483647, 1, 1, 2147483647, 1, 1, 2147483647, 1};
        CHECK(mps_opsum_max_bond(2, 2, many, many) == 2 * (2147483647ll * 2147483647ll));
        CHECK(mps_opsum_max_bond(2, 3, many, many) == 9223372036854775807ll);   // (three of them pass 2^63: saturates instead of wrapping)
        const int fits_s[3] = {1, 65536, 1}, fits_d[3] = {1, 32767, 1};
        CHECK(mps_opsum_term_dims(2, fits_s, fits_d, wide, narrow) && narrow[1] == 65536 * 32767);
    }
    {   // term tables
        const int off_ok[4] = {0, 1, 3, 6}, st_ok[6] = {0, 1, 2, 0, 0, 2}, op_ok[6] = {-1, 0, 1, -1, 1, 0};
        CHECK(mps_opsum_check_terms(3, 2, 3, off_ok, st_ok, op_ok) == 0);
        const int off_first[4] = {1, 2, 3, 6}, off_empty[4] = {0, 1, 1, 6}, st_high[6] = {0, 1, 3, 0, 0, 2};
        CHECK(mps_opsum_check_terms(3, 2, 3, off_first, st_ok, op_ok) == 1 && mps_opsum_check_terms(3, 2, 3, off_empty, st_ok, op_ok) == 2);
        CHECK(mps_opsum_check_terms(3, 2, 3, off_ok, st_high, op_ok) == 3);
        const int op_high[6] = {-1, 0, 2, -1, 1, 0}, op_low[6] = {-1, 0, 1, -2, 1, 0};
        CHECK(mps_opsum_check_terms(3, 2, 3, off_ok, st_ok, op_high) == 4 && mps_opsum_check_terms(3, 2, 3, off_ok, st_ok, op_low) == 4);
        CHECK(mps_opsum_check_terms(3, 3, 3, off_ok, st_ok, op_high) == 0);
        const int none[6] = {-1, -1, -1, -1, -1, -1};
        CHECK(mps_opsum_check_terms(3, 0, 3, off_ok, st_ok, none) == 0 && mps_opsum_check_terms(3, 0, 3, off_ok, st_ok, op_ok) == 4);
    }
    {   // the packed layout of an operator
        const int d[5] = {1, 5, 2, 5, 1};
        const std::vector<long long> off = mps_opsum_op_offsets(4, d, 7);
        CHECK(off.size() == 5 && off[0] == 7 && off[1] == 27 && off[2] == 67 && off[3] == 107 && off[4] == 127);
        CHECK(mps_opsum_check_op(4, d, off.data()) == 0);
        const int open_l[5] = {2, 5, 2, 5, 1}, open_r[5] = {1, 5, 2, 5, 3}, zero[5] = {1, 5, 0, 5, 1};
        CHECK(mps_opsum_check_op(4, open_l, off.data()) == 1 && mps_opsum_check_op(4, open_r, off.data()) == 1 && mps_opsum_check_op(4, zero, off.data()) == 1);
        std::vector<long long> loose = off;
        loose[2] += 1;
        CHECK(mps_opsum_check_op(4, d, loose.data()) == 2);
        const std::vector<long long> neg = mps_opsum_op_offsets(4, d, -1);
        CHECK(mps_opsum_check_op(4, d, neg.data()) == 2);
        CHECK(mps_opsum_check_op(3, d, off.data()) == 1);   // the dims of an operator on 4 qubits read as one on 3: D_3 = 5 is no edge
    }
    {   // sources at the borders of a block: term 0 has D = (1, 2, 1, 1) on chi = (1, 2, 3, 1), term 1 no operator on chi = (1, 2, 2, 1)
        const int widths[8] = {1, 4, 3, 1, 1, 2, 2, 1}, chi[8] = {1, 2, 3, 1, 1, 2, 2, 1}, has_op[2] = {0, -1};
        const std::vector<int> off = mps_combine_block_offsets(3, 2, widths);
        // site 1 is [2][6][5]; row 3 = (a = 1, i = 1) of term 0, column 2 = (b = 0, j = 2); s = 1
        const MpsOpsumSource in = mps_opsum_source(3, 2, off.data(), chi, has_op, 1, (size_t)1 * 30 + 3 * 5 + 2);
        CHECK(in.term == 0 && in.kind == kMpsOpsumProduct && in.a == 1 && in.b == 0 && in.s == 1 && in.x0 == 1 * 3 + 2 && in.x1 == 6 + 1 * 3 + 2);
        const MpsOpsumSource zero = mps_opsum_source(3, 2, off.data(), chi, has_op, 1, (size_t)3 * 5 + 3);        // row of term 0, column of term 1
        CHECK(zero.kind == kMpsOpsumZero && zero.term == -1);
        const MpsOpsumSource copy = mps_opsum_source(3, 2, off.data(), chi, has_op, 1, (size_t)1 * 30 + 5 * 5 + 4);   // s = 1, row 5, column 4
        CHECK(copy.term == 1 && copy.kind == kMpsOpsumCopy && copy.x0 == (size_t)(1 * 2 + 1) * 2 + 1);
        // site 0 is [2][1][6]: column 5 is j = 1 of term 1; site 2 is [2][5][1]: row 2 = (a = 0, i = 2) of term 0
        const MpsOpsumSource first = mps_opsum_source(3, 2, off.data(), chi, has_op, 0, (size_t)5);
        CHECK(first.term == 1 && first.kind == kMpsOpsumCopy && first.x0 == 1);
        const MpsOpsumSource edge = mps_opsum_source(3, 2, off.data(), chi, has_op, 0, (size_t)1 * 6 + 3);            // s = 1, (b = 1, j = 1) of term 0
        CHECK(edge.term == 0 && edge.kind == kMpsOpsumProduct && edge.a == 0 && edge.b == 1 && edge.s == 1 && edge.x0 == 1 && edge.x1 == 3);
        const MpsOpsumSource last = mps_opsum_source(3, 2, off.data(), chi, has_op, 2, (size_t)2);
        CHECK(last.term == 0 && last.kind == kMpsOpsumProduct && last.a == 0 && last.b == 0 && last.s == 0 && last.x0 == 2 && last.x1 == 5);
    }
    std::printf("mps_opsum_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
