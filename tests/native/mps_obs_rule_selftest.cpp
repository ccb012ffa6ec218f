// Self-test of csrc/aqc_mps_obs_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_obs_rule.py): the chain plan
// -- every pair served once from the right emission, chains that end at their farthest partner, transposed and duplicate pairs, refused
// lists --, the route rule at the fused cap, the table of the upper triangle, the placement of a transposed pair and the scratch sizes.
#include <cstdio>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_obs_rule.h"

using namespace aqc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static void check_plan(int n, const std::vector<int32_t>& pairs) {
    const int npairs = (int)pairs.size() / 2;
    MpsObsPlan plan;
    CHECK(mps_obs_plan(n, npairs, pairs.data(), plan));
    CHECK((int)plan.last.size() == n && (int)plan.pair_emit.size() == npairs && (int)plan.pair_transposed.size() == npairs);
    std::vector<int> farthest(n, -1);
    std::set<std::pair<int, int>> wanted;
    for (int p = 0; p < npairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1], lo = a < b ? a : b, hi = a < b ? b : a;
        farthest[lo] = hi > farthest[lo] ? hi : farthest[lo];
        wanted.insert({lo, hi});
        // every pair is served, by the emission of its own chain at its own site
        CHECK(plan.pair_emit[p] >= 0 && plan.pair_emit[p] < (int)plan.emits.size());
        const MpsObsEmit e = plan.emits[plan.pair_emit[p]];
        CHECK(e.chain == lo && e.site == hi);
        CHECK(plan.pair_transposed[p] == (a > b));
    }
    int chains = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(plan.last[i] == farthest[i]);   // chains end at the farthest partner, and only requested chains exist
        chains += farthest[i] >= 0;
    }
    CHECK(plan.nchains == chains);
    // every (chain, site) once, ordered by site and then by chain, and none that nobody asked for
    CHECK(plan.emits.size() == wanted.size());
    for (size_t k = 0; k < plan.emits.size(); ++k) {
        CHECK(wanted.count({plan.emits[k].chain, plan.emits[k].site}) == 1);
        CHECK(plan.emits[k].site <= plan.last[plan.emits[k].chain]);
        if (k) {
            const MpsObsEmit &x = plan.emits[k - 1], &y = plan.emits[k];
            CHECK(x.site < y.site || (x.site == y.site && x.chain < y.chain));
        }
    }
}

int main() {
    // all pairs, nearest neighbours, one long pair, transposed and duplicate pairs
    for (int n : {2, 3, 5, 13, 40}) {
        std::vector<int32_t> all, nn, rev;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) { all.push_back(i); all.push_back(j); rev.push_back(j); rev.push_back(i); }
        for (int i = 0; i + 1 < n; ++i) { nn.push_back(i); nn.push_back(i + 1); }
        check_plan(n, all);
        check_plan(n, rev);
        check_plan(n, nn);
        check_plan(n, {0, n - 1});
        check_plan(n, {n - 1, 0, 0, n - 1, n - 1, 0});
    }
    check_plan(13, {12, 0, 0, 12, 5, 6, 0, 12, 6, 5, 5, 6, 5, 9, 0, 3});
    {   // duplicates share an emission, a transposed pair shares it too and is flagged
        const std::vector<int32_t> pairs = {12, 0, 0, 12, 5, 6, 0, 12, 6, 5};
        MpsObsPlan plan;
        CHECK(mps_obs_plan(13, 5, pairs.data(), plan));
        CHECK(plan.emits.size() == 2 && plan.nchains == 2);
        CHECK(plan.pair_emit[0] == plan.pair_emit[1] && plan.pair_emit[1] == plan.pair_emit[3] && plan.pair_emit[2] == plan.pair_emit[4]);
        CHECK(plan.pair_transposed[0] == 1 && plan.pair_transposed[1] == 0 && plan.pair_transposed[4] == 1);
        CHECK(plan.last[0] == 12 && plan.last[5] == 6 && plan.last[6] == -1 && plan.last[12] == -1);
    }
    {   // refused lists
        MpsObsPlan plan;
        const int32_t same[2] = {2, 2}, high[2] = {0, 5}, low[2] = {-1, 2}, fine[2] = {0, 1};
        CHECK(!mps_obs_plan(5, 1, same, plan));
        CHECK(!mps_obs_plan(5, 1, high, plan));
        CHECK(!mps_obs_plan(5, 1, low, plan));
        CHECK(!mps_obs_plan(1, 1, fine, plan));
        CHECK(!mps_obs_plan(5, 1, nullptr, plan));
        CHECK(mps_obs_plan(2, 1, fine, plan) && plan.nchains == 1 && plan.last[0] == 1);
    }
    {   // the route rule at the cap
        static_assert(kMpsObsFusedCap <= 64, "the fused kernel keeps E in two 64 x 64 complex planes");
        std::vector<int> dims = {1, 2, 4, 64, 64, 7, 1};
        CHECK(mps_obs_route(6, dims.data()) == kMpsObsFused && mps_max_bond(6, dims.data()) == 64);
        dims[4] = 65;
        CHECK(mps_obs_route(6, dims.data()) == kMpsObsGemm);
        const std::vector<int> ones(14, 1);
        CHECK(mps_obs_route(13, ones.data()) == kMpsObsFused);
        dims[4] = kMpsObsFusedCap;
        dims[3] = kMpsObsFusedCap + 1;
        CHECK(mps_obs_route(6, dims.data()) == kMpsObsGemm);
    }
    {   // the upper triangle: ten different entries with row <= col, each from the components that hold its index values
        std::set<std::pair<int, int>> seen;
        for (int e = 0; e < kMpsObsUpper; ++e) {
            const MpsObsEntry en = mps_obs_upper(e);
            CHECK(en.row >= 0 && en.row <= en.col && en.col < 4);
            seen.insert({en.row, en.col});
            const int a = en.row & 1, c = en.row >> 1, b = en.col & 1, d = en.col >> 1;
            // E^{ab}: 00 -> 0, 01 -> 1, 11 -> 2, 10 -> the adjoint of 1;  K^{cd} likewise, and 10 never occurs in the upper triangle
            const int ecomp = a == b ? 2 * a : 1, kcomp = c == d ? 2 * c : 1;
            CHECK(en.ecomp == ecomp && en.kcomp == kcomp && en.eadj == (a == 1 && b == 0));
            CHECK(!(c == 1 && d == 0));
        }
        CHECK(seen.size() == (size_t)kMpsObsUpper);
    }
    {   // placement: transposed swaps the two index bits of rows and columns
        double m[32], out[32];
        for (int i = 0; i < 32; ++i) m[i] = i;
        mps_obs_place(m, 0, out);
        for (int i = 0; i < 32; ++i) CHECK(out[i] == m[i]);
        mps_obs_place(m, 1, out);
        const int sw[4] = {0, 2, 1, 3};
        for (int r = 0; r < 4; ++r)
            for (int s = 0; s < 4; ++s) CHECK(out[2 * (4 * r + s)] == m[2 * (4 * sw[r] + sw[s])] && out[2 * (4 * r + s) + 1] == m[2 * (4 * sw[r] + sw[s]) + 1]);
    }
    {   // scratch: offsets add up, a group holds at least one chain and stays within the budget when it can
        const std::vector<int> dims = {1, 2, 3, 5, 2, 1};
        const std::vector<size_t> off = mps_obs_env_offsets(5, dims.data());
        CHECK(off.size() == 7 && off[0] == 0 && off[1] == 1 && off[3] == 14 && off[5] == 43 && off[6] == 1 + 4 + 9 + 25 + 4 + 1);
        CHECK(mps_obs_slot_elems(5, dims.data()) == 25 && mps_obs_chain_elems(5, dims.data()) == 9 * 25);
        CHECK(mps_obs_group_size(5, dims.data(), 4, 1) == 1);
        CHECK(mps_obs_group_size(5, dims.data(), 4, 2 * 16 * 225) == 2);
        CHECK(mps_obs_group_size(5, dims.data(), 4, (size_t)1 << 30) == 4);
    }
    std::printf("mps_obs_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
