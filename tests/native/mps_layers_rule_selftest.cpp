// Self-test of csrc/aqc_mps_layers_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_layers_rule.py): routing
// against route_pair, the routed, folded and layered program against the program applied in its own order on a dense vector of n = 5
// qubits (long-range pairs both ways round, a qubit that no 2-qubit op touches, 1-qubit ops before, between and after the last 2-qubit
// op on their qubit), the bounds, the route and the chunks.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_layers_rule.h"

using namespace aqc;

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

// dense vectors: bit q of the index <-> qubit q
static void dense1(std::vector<cd>& psi, int q, const cd* g) {
    for (size_t i = 0; i < psi.size(); ++i) {
        if ((i >> q) & 1) continue;
        const size_t j = i | ((size_t)1 << q);
        const cd x = psi[i], y = psi[j];
        psi[i] = g[0] * x + g[1] * y;
        psi[j] = g[2] * x + g[3] * y;
    }
}
static void dense2(std::vector<cd>& psi, int a, int b, const cd* g) {   // index 2 bit_a + bit_b
    for (size_t i = 0; i < psi.size(); ++i) {
        if (((i >> a) & 1) || ((i >> b) & 1)) continue;
        size_t at[4];
        cd in[4];
        for (int k = 0; k < 4; ++k) { at[k] = i | ((size_t)(k >> 1) << a) | ((size_t)(k & 1) << b); in[k] = psi[at[k]]; }
        for (int r = 0; r < 4; ++r) {
            cd acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += g[4 * r + k] * in[k];
            psi[at[r]] = acc;
        }
    }
}

struct Op { int two, a, b; cd m[16]; };
static Op random_op(int two, int a, int b) {
    Op op{two, a, b, {}};
    for (int i = 0; i < (two ? 16 : 4); ++i) op.m[i] = cd(uniform(), uniform());
    return op;
}

static void program_case(int n, const std::vector<Op>& prog, int want_singles) {
    std::vector<cd> psi((size_t)1 << n), want;
    for (cd& x : psi) x = cd(uniform(), uniform());
    want = psi;
    for (const Op& op : prog) {
        if (op.two) dense2(want, op.a, op.b, op.m);
        else dense1(want, op.a, op.m);
    }
    std::vector<MpsLayersOp> ops;
    for (const Op& op : prog) ops.push_back({op.two, op.a, op.two ? op.b : op.a});
    const std::vector<MpsLayersRouted> routed = mps_layers_route_ops(ops);
    const MpsLayersPlan plan = mps_layers_plan(n, routed);
    static const double swap_gate[32] = {1, 0, 0, 0, 0, 0, 0, 0,  0, 0, 0, 0, 1, 0, 0, 0,  0, 0, 1, 0, 0, 0, 0, 0,  0, 0, 0, 0, 0, 0, 1, 0};
    std::vector<cd> mats(routed.size() * 16, cd(0.0, 0.0));
    for (size_t r = 0; r < routed.size(); ++r) {
        const Op& src = prog[routed[r].src];
        double* dst = reinterpret_cast<double*>(&mats[16 * r]);
        if (!routed[r].two) std::copy(src.m, src.m + 4, &mats[16 * r]);
        else if (routed[r].swap) std::copy(swap_gate, swap_gate + 32, dst);
        else permute_gate(reinterpret_cast<const double*>(src.m), routed[r].flip != 0, dst);
    }
    std::vector<cd> gates(std::max<size_t>(plan.gates.size(), 1) * 16), singles((size_t)4 * n);
    mps_layers_fold(plan, routed, mats.data(), gates.data(), singles.data());
    // layers: disjoint sites, every gate once, a gate never before one it depends on
    std::vector<int> seen(plan.gates.size(), 0), ready(n, 0);
    for (size_t l = 0; l < plan.layers.size(); ++l) {
        std::vector<int> used(n, 0);
        for (int g : plan.layers[l]) {
            const int q = plan.gates[g].q;
            CHECK(plan.gates[g].layer == (int)l && !used[q] && !used[q + 1] && q + 1 < n);
            used[q] = used[q + 1] = 1;
            ++seen[g];
        }
    }
    for (size_t g = 0; g < plan.gates.size(); ++g) {   // as soon as possible, in program order
        const int q = plan.gates[g].q, layer = std::max(ready[q], ready[q + 1]);
        CHECK(seen[g] == 1 && plan.gates[g].layer == layer);
        ready[q] = ready[q + 1] = layer + 1;
    }
    for (const std::vector<int>& layer : plan.layers)
        for (int g : layer) dense2(psi, plan.gates[g].q, plan.gates[g].q + 1, &gates[(size_t)16 * g]);
    int count = 0;
    for (int q = 0; q < n; ++q) {
        CHECK(plan.has_single[q] == 0 || plan.touched[q] == 0);
        if (plan.has_single[q]) { dense1(psi, q, &singles[4 * q]); ++count; }
        else CHECK(singles[4 * q] == cd(1.0, 0.0) && singles[4 * q + 1] == cd(0.0, 0.0) && singles[4 * q + 3] == cd(1.0, 0.0));
    }
    CHECK(count == want_singles);
    double err = 0.0, norm = 0.0;
    for (size_t i = 0; i < psi.size(); ++i) { err += std::norm(psi[i] - want[i]); norm += std::norm(want[i]); }
    std::printf("n = %d: %zu ops -> %zu routed -> %zu folded gates in %zu layers, %d singles, |layered - in order| / |psi| = %.3g\n", n, prog.size(), routed.size(),
                plan.gates.size(), plan.layers.size(), count, std::sqrt(err / norm));
    CHECK(std::sqrt(err) <= 1e-12 * std::sqrt(norm));
}

int main() {
    {   // routing against route_pair
        const int pairs[][2] = {{0, 3}, {4, 1}, {2, 3}, {3, 2}, {0, 4}};
        for (const auto& p : pairs) {
            const std::vector<RouteStep> want = route_pair(p[0], p[1]);
            const std::vector<MpsLayersRouted> got = mps_layers_route_ops({{1, p[0], p[1]}});
            CHECK(got.size() == want.size() && (int)got.size() == 2 * (std::abs(p[0] - p[1]) - 1) + 1);
            int gates = 0;
            for (size_t i = 0; i < got.size() && i < want.size(); ++i) {
                CHECK(got[i].two == 1 && got[i].q == want[i].q && got[i].swap == (want[i].swap ? 1 : 0) && got[i].flip == want[i].flip && got[i].src == 0);
                if (!got[i].swap) { ++gates; CHECK(got[i].q == std::min(p[0], p[1]) && got[i].flip == (p[0] > p[1] ? 1 : 0)); }
            }
            CHECK(gates == 1);
        }
        const std::vector<MpsLayersRouted> one = mps_layers_route_ops({{0, 2, 2}, {1, 1, 2}});
        CHECK(one.size() == 2 && one[0].two == 0 && one[0].q == 2 && one[1].two == 1 && one[1].q == 1 && one[1].src == 1);
    }
    // n = 5: every qubit touched; then qubit 4 touched by 1-qubit ops alone; 1-qubit ops only; an empty program
    program_case(5, {random_op(0, 0, 0), random_op(0, 2, 0), random_op(1, 0, 1), random_op(0, 1, 0), random_op(1, 2, 3), random_op(1, 0, 3), random_op(0, 3, 0),
                     random_op(0, 3, 0), random_op(1, 4, 1), random_op(0, 4, 0), random_op(1, 2, 1), random_op(0, 0, 0), random_op(0, 2, 0), random_op(1, 3, 4),
                     random_op(0, 4, 0), random_op(0, 1, 0)}, 0);
    program_case(5, {random_op(0, 4, 0), random_op(1, 0, 1), random_op(0, 1, 0), random_op(1, 3, 1), random_op(0, 4, 0), random_op(1, 2, 3), random_op(0, 0, 0),
                     random_op(1, 3, 0), random_op(0, 3, 0)}, 1);
    program_case(5, {random_op(0, 1, 0), random_op(0, 3, 0), random_op(0, 1, 0)}, 2);
    program_case(5, {}, 0);
    {   // bounds and route
        const std::vector<int> b6 = mps_layers_bounds(6, 0, nullptr), b6c = mps_layers_bounds(6, 3, nullptr), b16 = mps_layers_bounds(16, 0, nullptr);
        const int want6[] = {1, 2, 4, 8, 4, 2, 1}, want6c[] = {1, 2, 3, 3, 3, 2, 1};
        CHECK(std::equal(b6.begin(), b6.end(), want6) && std::equal(b6c.begin(), b6c.end(), want6c));
        CHECK(b16[8] == 64 && b16[6] == 64 && b16[5] == 32 && b16[16] == 1 && mps_layers_natural(16, 8, 0) == 256 && mps_layers_natural(16, 8, 100) == 100);
        CHECK(mps_layers_natural(100, 50, 0) == 1 << 20 && mps_layers_natural(100, 50, 7) == 7 && mps_layers_natural(100, 99, 7) == 2);
        const int hand[] = {1, 64, 64, 64, 1}, ragged[] = {1, 40, 64, 40, 1}, wide[] = {1, 2, 65, 2, 1};
        const std::vector<int> bh = mps_layers_bounds(4, 64, hand), br = mps_layers_bounds(4, 0, ragged), bw = mps_layers_bounds(4, 0, wide);
        CHECK(std::equal(bh.begin(), bh.end(), hand) && std::equal(br.begin(), br.end(), ragged) && bw[2] == 65);
        CHECK(mps_layers_route(4, hand, 64) == kMpsLayersFused && mps_layers_route(4, ragged, 0) == kMpsLayersFused && mps_layers_route(4, wide, 0) == kMpsLayersGatewise);
        CHECK(mps_layers_route(13, nullptr, 0) == kMpsLayersFused && mps_layers_route(14, nullptr, 0) == kMpsLayersGatewise);
        CHECK(mps_layers_route(32, nullptr, 64) == kMpsLayersFused && mps_layers_route(32, nullptr, 65) == kMpsLayersGatewise && mps_layers_route(32, nullptr, 1) == kMpsLayersFused);
        CHECK(mps_layers_ranks_fit(4, hand, ragged) && !mps_layers_ranks_fit(4, ragged, hand));
        CHECK(mps_layers_method_ok(0) && mps_layers_method_ok(1) && mps_layers_method_ok(2) && !mps_layers_method_ok(3) && !mps_layers_method_ok(-1));
    }
    {   // chunks: five stores of 2k x 2k complex numbers per matrix
        const size_t budget = kMpsCallBudget;
        CHECK(mps_layers_chunk(64, 16 * 16, budget) == 204 && (size_t)204 * 80 * 128 * 128 <= budget && (size_t)205 * 80 * 128 * 128 > budget);
        CHECK(mps_layers_chunk(8, 27, budget) == 27 && mps_layers_chunk(8, 27, 3 * 80 * 256 + 7) == 3 && mps_layers_chunk(8, 27, 80 * 256 + 7) == 1 && mps_layers_chunk(8, 27, 1) == 1);
        CHECK(mps_layers_chunk(1, (size_t)1 << 20, budget) == 1 << 16);
    }
    std::printf("mps_layers_rule selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
