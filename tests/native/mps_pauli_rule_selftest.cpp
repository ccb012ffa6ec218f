// Self-test of csrc/aqc_mps_pauli_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_pauli_rule.py): the
// supports of strings, the route rule over both states' bonds at the fused cap, the letter table held to the 2 x 2 Pauli matrices (and
// the turn that applies a phase without a multiplication), the check of letters and the grouping of jobs.
#include <complex>
#include <cstdio>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_pauli_rule.h"

using namespace aqc;
typedef std::complex<double> cd;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

int main() {
    {   // supports
        struct Case { std::vector<uint8_t> s; int first, last; };
        const std::vector<Case> cases = {
            {{0}, 0, 0}, {{3}, 0, 0}, {{0, 0, 0, 0}, 0, 0}, {{0, 0, 0, 2}, 3, 3}, {{1, 0, 0, 0}, 0, 0}, {{0, 1, 0, 3, 0}, 1, 3},
            {{2, 2, 2, 2, 2}, 0, 4}, {{0, 0, 3, 0, 0, 0}, 2, 2}, {{3, 0, 0, 0, 0, 1}, 0, 5}};
        for (const Case& c : cases) {
            int32_t first = -7, last = -7;
            mps_pauli_support((int)c.s.size(), c.s.data(), &first, &last);
            CHECK(first == c.first && last == c.last);
            CHECK(mps_pauli_bad_letter(c.s.data(), c.s.size()) == -1);
        }
        const std::vector<uint8_t> bad = {0, 3, 4, 1, 255};
        CHECK(mps_pauli_bad_letter(bad.data(), bad.size()) == 2);
        CHECK(mps_pauli_bad_letter(bad.data(), 2) == -1);
        CHECK(mps_pauli_bad_letter(bad.data() + 3, 2) == 1);
    }
    {   // the route rule at the cap, over both states
        static_assert(kMpsPauliFusedCap <= 64, "the fused kernel keeps M in two 64 x 64 complex planes");
        std::vector<int> ket = {1, 2, 4, 64, 64, 7, 1}, bra = {1, 2, 3, 5, 64, 2, 1};
        CHECK(mps_pauli_route(6, nullptr, ket.data()) == kMpsPauliFused && mps_pauli_max_bond(6, nullptr, ket.data()) == 64);
        CHECK(mps_pauli_route(6, bra.data(), ket.data()) == kMpsPauliFused);
        bra[3] = 65;
        CHECK(mps_pauli_route(6, bra.data(), ket.data()) == kMpsPauliGemm && mps_pauli_max_bond(6, bra.data(), ket.data()) == 65);
        CHECK(mps_pauli_route(6, nullptr, ket.data()) == kMpsPauliFused);   // the bra is not looked at when it is the ket
        CHECK(mps_pauli_route(6, ket.data(), bra.data()) == kMpsPauliGemm);
        bra[3] = 5;
        ket[4] = 65;
        CHECK(mps_pauli_route(6, bra.data(), ket.data()) == kMpsPauliGemm && mps_pauli_route(6, nullptr, ket.data()) == kMpsPauliGemm);
        const std::vector<int> ones(2, 1);
        CHECK(mps_pauli_route(1, nullptr, ones.data()) == kMpsPauliFused);
        CHECK(mps_pauli_method_ok(0) && mps_pauli_method_ok(1) && mps_pauli_method_ok(2) && !mps_pauli_method_ok(3) && !mps_pauli_method_ok(-1));
    }
    {   // the letters: P[c ^ f][c] = ph(c) = i^turns and every other entry of the column is 0
        const cd I(0, 1);
        const cd pauli[4][2][2] = {{{1, 0}, {0, 1}}, {{0, 1}, {1, 0}}, {{0, -I}, {I, 0}}, {{1, 0}, {0, -1}}};
        const cd power[4] = {1, I, -1, -I};
        for (int letter = 0; letter < 4; ++letter)
            for (int c = 0; c < 2; ++c) {
                const int f = mps_pauli_flip(letter), k = mps_pauli_turns(letter, c);
                CHECK((f == 0 || f == 1) && k >= 0 && k < 4);
                CHECK(pauli[letter][c ^ f][c] == power[k]);
                CHECK(pauli[letter][c ^ f ^ 1][c] == cd(0, 0));
            }
        for (int k = 0; k < 4; ++k) {   // the turn is the product with i^k, exactly
            double re, im;
            mps_pauli_turn(k, 0.75, -2.5, re, im);
            CHECK(cd(re, im) == power[k] * cd(0.75, -2.5));
        }
    }
    {   // scratch of the gemm route and its groups: at least one job, never more than there are, within the budget when it can
        const std::vector<int> ket = {1, 2, 3, 5, 2, 1}, bra = {1, 2, 4, 4, 2, 1};
        CHECK(mps_pauli_m_elems(5, nullptr, ket.data()) == 25 && mps_pauli_f_elems(5, nullptr, ket.data()) == 2 * 3 * 5);
        CHECK(mps_pauli_m_elems(5, bra.data(), ket.data()) == 20 && mps_pauli_f_elems(5, bra.data(), ket.data()) == 2 * 4 * 5);
        CHECK(mps_pauli_job_elems(5, bra.data(), ket.data()) == 60);
        CHECK(mps_pauli_group_size(60, 7, 1) == 1);
        CHECK(mps_pauli_group_size(60, 7, 3 * 16 * 60) == 3);
        CHECK(mps_pauli_group_size(60, 7, 3 * 16 * 60 + 100) == 3);
        CHECK(mps_pauli_group_size(60, 7, (size_t)1 << 30) == 7);
        CHECK(mps_pauli_group_size(1, 1 << 20, (size_t)1 << 30) == kMpsPauliGroupMax);
        CHECK(mps_pauli_group_size(60, 1, 0) == 1);
    }
    std::printf("mps_pauli_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
