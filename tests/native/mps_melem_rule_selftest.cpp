// Self-test of csrc/aqc_mps_melem_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_melem_rule.py): the route
// at both caps, the list of entries of an operator site (order, first marks, masks, what counts as a zero), the scratch sizes in 64
// bits with their saturation, the group size, and the walk of mps_melem_value against conj(phi) . O . psi of the dense vectors for
// n = 1 .. 5: rectangular bra and ket, an operator with zeros, an operator bond of 1 inside, the identity.
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_melem_rule.h"

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
    std::vector<const cd*> ptrs() const {
        std::vector<const cd*> p;
        for (const auto& s : sites) p.push_back(s.data());
        return p;
    }
};
static Chain random_chain(const std::vector<int>& dims, int phys, double zeros = 0.0) {
    Chain c;
    c.dims = dims;
    for (size_t q = 0; q + 1 < dims.size(); ++q) {
        c.sites.emplace_back((size_t)phys * dims[q] * dims[q + 1]);
        for (cd& x : c.sites.back()) x = std::fabs(uniform()) < zeros ? cd(0.0, 0.0) : cd(uniform(), uniform());
    }
    return c;
}
// psi(b) at index sum_q b_q 2^q
static std::vector<cd> dense(const Chain& c) {
    const int n = (int)c.sites.size();
    std::vector<cd> psi((size_t)1 << n);
    for (size_t b = 0; b < psi.size(); ++b) {
        std::vector<cd> row(1, cd(1.0, 0.0));
        for (int q = 0; q < n; ++q) {
            const int s = (int)(b >> q) & 1, r = c.dims[q], w = c.dims[q + 1];
            std::vector<cd> next(w, cd(0.0, 0.0));
            for (int i = 0; i < r; ++i)
                for (int j = 0; j < w; ++j) next[j] += row[i] * c.sites[q][((size_t)s * r + i) * w + j];
            row.swap(next);
        }
        psi[b] = row[0];
    }
    return psi;
}
// O(b_out, b_in) as the product of its D x D matrices
static cd op_element(const Chain& op, size_t bo, size_t bi) {
    const int n = (int)op.sites.size();
    std::vector<cd> row(1, cd(1.0, 0.0));
    for (int q = 0; q < n; ++q) {
        const int so = (int)(bo >> q) & 1, si = (int)(bi >> q) & 1, r = op.dims[q], w = op.dims[q + 1];
        std::vector<cd> next(w, cd(0.0, 0.0));
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < w; ++j) next[j] += row[i] * op.sites[q][(((size_t)i * w + j) * 2 + so) * 2 + si];
        row.swap(next);
    }
    return row[0];
}

static void check_walk(const std::vector<int>& bd, const std::vector<int>& kd, const std::vector<int>& od, double zeros) {
    const int n = (int)kd.size() - 1;
    const Chain bra = random_chain(bd, 2), ket = random_chain(kd, 2), op = random_chain(od.empty() ? std::vector<int>(n + 1, 1) : od, 4, zeros);
    const std::vector<cd> phi = dense(bra), psi = dense(ket);
    cd want(0.0, 0.0);
    double scale = 0.0;
    for (size_t bo = 0; bo < phi.size(); ++bo)
        for (size_t bi = 0; bi < psi.size(); ++bi) {
            const cd o = od.empty() ? cd(bo == bi ? 1.0 : 0.0, 0.0) : op_element(op, bo, bi);
            want += std::conj(phi[bo]) * o * psi[bi];
            scale += std::abs(phi[bo]) * std::abs(o) * std::abs(psi[bi]);
        }
    const std::vector<const cd*> bp = bra.ptrs(), kp = ket.ptrs(), opp = op.ptrs();
    const cd got = mps_melem_value(n, bd.data(), kd.data(), od.empty() ? nullptr : od.data(), bp.data(), kp.data(), od.empty() ? nullptr : opp.data());
    CHECK(std::abs(got - want) <= 1e-13 * (scale + 1.0));
}

int main() {
    // methods and routes
    CHECK(mps_melem_method_ok(0) && mps_melem_method_ok(1) && mps_melem_method_ok(2) && !mps_melem_method_ok(3) && !mps_melem_method_ok(-1));
    {
        const int k64[] = {1, 2, 64, 2, 1}, k65[] = {1, 2, 65, 2, 1}, b[] = {1, 2, 3, 2, 1}, o32[] = {1, 4, 32, 4, 1}, o33[] = {1, 4, 33, 4, 1};
        CHECK(mps_melem_route(4, nullptr, k64, nullptr) == kMpsMelemFused);
        CHECK(mps_melem_route(4, nullptr, k65, nullptr) == kMpsMelemGemm);
        CHECK(mps_melem_route(4, b, k64, o32) == kMpsMelemFused);
        CHECK(mps_melem_route(4, k65, b, o32) == kMpsMelemGemm);
        CHECK(mps_melem_route(4, b, k64, o33) == kMpsMelemGemm);
        CHECK(mps_melem_max_bond(4, b, k64) == 64 && mps_melem_max_bond(4, k65, b) == 65 && mps_melem_max_op_bond(4, o33) == 33);
        CHECK(mps_melem_max_op_bond(4, nullptr) == 1);
        const int one[] = {1, 1};
        CHECK(mps_melem_route(1, nullptr, one, nullptr) == kMpsMelemFused && mps_melem_route(1, one, one, one) == kMpsMelemFused);
    }
    // entries: order a, s', b, s; exact zeros of either sign skipped, a NaN kept; first marks and masks
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::vector<double> w(2 * 4 * 2 * 3, 0.0);   // dl = 2, dr = 3
        auto at = [&](int a, int b, int s, int sp) -> double* { return w.data() + 2 * ((((size_t)a * 3 + b) * 2 + s) * 2 + sp); };
        at(0, 0, 0, 0)[0] = 1.0;
        at(0, 0, 0, 1)[1] = -2.0;
        at(1, 0, 0, 0)[0] = 3.0;
        at(0, 2, 1, 1)[0] = nan;
        at(1, 1, 0, 1)[0] = -0.0; at(1, 1, 0, 1)[1] = -0.0;   // a zero
        at(1, 2, 0, 0)[0] = 0.0; at(1, 2, 0, 0)[1] = 5e-324;   // no zero
        std::vector<MpsMelemEntry> ent;
        std::vector<int> mask;
        mps_melem_entries(2, 3, w.data(), ent, mask);
        CHECK(ent.size() == 5 && mask.size() == 3 && mask[0] == 1 && mask[1] == 0 && mask[2] == 3);
        const int want[5][5] = {{0, 0, 0, 0, 1}, {0, 1, 0, 0, 0}, {0, 1, 2, 1, 1}, {1, 0, 0, 0, 0}, {1, 0, 2, 0, 1}};
        for (size_t e = 0; e < ent.size() && e < 5; ++e)
            CHECK(ent[e].a == want[e][0] && ent[e].sp == want[e][1] && ent[e].b == want[e][2] && ent[e].s == want[e][3] && ent[e].first == want[e][4]);
        CHECK(ent.size() == 5 && ent[1].wi == -2.0 && std::isnan(ent[2].wr) && ent[4].wi == 5e-324);
        ent.clear();
        mps_melem_entries(7, 9, nullptr, ent, mask);   // the identity: D = 1 whatever is said
        CHECK(ent.size() == 2 && mask.size() == 1 && mask[0] == 3 && ent[0].sp == 0 && ent[0].s == 0 && ent[1].sp == 1 && ent[1].s == 1);
        CHECK(ent.size() == 2 && ent[0].first == 1 && ent[1].first == 1 && ent[0].wr == 1.0 && ent[1].wr == 1.0 && ent[0].wi == 0.0);
    }
    // scratch: 256 XXZ jobs at bond 64 fit the budget together; 64-bit sizes; saturation
    {
        std::vector<int> k(33, 64), o(33, 5);
        k[0] = k[32] = o[0] = o[32] = 1;
        CHECK(mps_melem_e_elems(32, nullptr, k.data(), o.data()) == (size_t)5 * 64 * 64);
        CHECK(mps_melem_g_elems(32, nullptr, k.data(), o.data()) == (size_t)10 * 64 * 64);
        CHECK(mps_melem_f_elems(32, nullptr, k.data(), o.data()) == (size_t)10 * 64 * 64);
        const size_t job = mps_melem_job_elems(32, nullptr, k.data(), o.data(), false);
        CHECK(job == (size_t)20 * 64 * 64 && mps_melem_job_elems(32, nullptr, k.data(), o.data(), true) == (size_t)30 * 64 * 64);
        CHECK(mps_melem_group_size(job, 256, kMpsMelemBudget) == 256 && mps_melem_group_size(job, 100000, kMpsMelemBudget) == 409);
        CHECK(mps_melem_group_size(job, 5, 1) == 1 && mps_melem_group_size(1, 100000, kMpsMelemBudget) == kMpsMelemGroupMax);
        CHECK(mps_melem_group_size(0, 7, kMpsMelemBudget) == 7);
        const int b3[] = {1, 3, 1}, k3[] = {1, 5, 1}, o3[] = {1, 2, 1};
        CHECK(mps_melem_e_elems(2, b3, k3, o3) == 30 && mps_melem_g_elems(2, b3, k3, o3) == 20 && mps_melem_f_elems(2, b3, k3, o3) == 12);
        CHECK(mps_melem_e_elems(2, b3, k3, nullptr) == 15 && mps_melem_g_elems(2, b3, k3, nullptr) == 10);
        const int big[] = {1, 100000, 1}, obig[] = {1, 3000, 1};
        CHECK(mps_melem_e_elems(2, nullptr, big, obig) == (size_t)3000 * 100000 * 100000);            // 3e13: beyond 32 bits
        CHECK(mps_melem_g_elems(2, nullptr, big, obig) == (size_t)2 * 3000 * 100000);
        const int huge[] = {1, 2147483647, 1};
        CHECK(mps_melem_e_elems(2, huge, huge, huge) == ~(size_t)0);                                    // 2^93 saturates
        CHECK(mps_melem_job_elems(2, huge, huge, huge, true) == ~(size_t)0 && mps_melem_group_size(~(size_t)0, 9, kMpsMelemBudget) == 1);
        CHECK(mps_melem_sat_add(~(size_t)0 - 1, 1) == ~(size_t)0 && mps_melem_sat_add(~(size_t)0 - 1, 2) == ~(size_t)0 && mps_melem_sat_mul(0, ~(size_t)0) == 0);
    }
    // the walk against the dense vectors
    check_walk({1, 1}, {1, 1}, {1, 1}, 0.0);
    check_walk({1, 1}, {1, 1}, {}, 0.0);
    check_walk({1, 2, 1}, {1, 1, 1}, {1, 2, 1}, 0.0);
    check_walk({1, 2, 3, 1}, {1, 2, 2, 1}, {1, 3, 2, 1}, 0.0);
    check_walk({1, 2, 3, 1}, {1, 2, 2, 1}, {1, 3, 2, 1}, 0.6);       // many zeros: F, G and whole E matrices skipped
    check_walk({1, 2, 3, 2, 1}, {1, 2, 4, 2, 1}, {1, 2, 1, 3, 1}, 0.3);   // an operator bond of 1 inside
    check_walk({1, 2, 3, 2, 1}, {1, 2, 4, 2, 1}, {}, 0.0);          // the identity
    check_walk({1, 2, 4, 3, 2, 1}, {1, 2, 3, 4, 2, 1}, {1, 4, 5, 4, 2, 1}, 0.8);
    check_walk({1, 2, 4, 3, 2, 1}, {1, 2, 3, 4, 2, 1}, {1, 4, 5, 4, 2, 1}, 1.1);   // the zero operator
    std::printf("mps_melem_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
