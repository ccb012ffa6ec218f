// Stand-alone self-test of csrc/aqc_backwalk.h (host only): the partial-R row of a mirrored sub-stage is the forward sub-stage it
// mirrors, for every split of a plan into stages, checked against a plan mirrored the way mirror_plan does it (stages reversed, the
// sub-stages of every stage reversed).  Prints "ok".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_backwalk.h"

using namespace aqc;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// every composition of `total` sub-stages into stages of at least one sub-stage
static void compositions(int total, std::vector<int>& cur, std::vector<std::vector<int>>& out) {
    if (total == 0) { out.push_back(cur); return; }
    for (int n = 1; n <= total; ++n) { cur.push_back(n); compositions(total - n, cur, out); cur.pop_back(); }
}

int main() {
    static_assert(backwalk_r_slot(11, 10) == 0 && backwalk_r_slot(11, 4) == 6 && backwalk_conj_sub(11, 4) == 6, "the headline plan: 7 + 4 sub-stages");
    for (int total = 1; total <= 9; ++total) {
        std::vector<std::vector<int>> splits;
        std::vector<int> cur;
        compositions(total, cur, splits);
        for (const std::vector<int>& stages : splits) {
            // forward plan: stage s holds the sub-stages [begin_s, begin_s + n_s); mirrored: the list of (forward ids) reversed as a whole
            std::vector<std::vector<int>> fwd;
            int id = 0;
            for (int n : stages) { fwd.emplace_back(); for (int i = 0; i < n; ++i) fwd.back().push_back(id++); }
            std::vector<std::vector<int>> mir = fwd;
            std::reverse(mir.begin(), mir.end());
            for (auto& st : mir) std::reverse(st.begin(), st.end());
            int m = 0, begin_last = 0;
            std::vector<bool> seen(total, false);
            for (size_t s = 0; s < mir.size(); ++s) {
                if (s + 1 == mir.size()) begin_last = m;
                for (int f : mir[s]) {
                    const int slot = backwalk_r_slot(total, m++);
                    CHECK(slot == f);
                    CHECK(slot >= 0 && slot < total && !seen[slot]);
                    if (slot >= 0 && slot < total) seen[slot] = true;
                }
            }
            // the mirrored plan's last stage is the forward plan's first: its rows are 0 .. n_0 - 1, walked from the top, and the first
            // one walked -- the forward stage's last sub-stage -- is the one the gradient walk conjugates
            CHECK(begin_last == total - stages[0]);
            CHECK(backwalk_conj_sub(total, begin_last) == stages[0] - 1);
            for (int j = 0; j < stages[0]; ++j) CHECK(backwalk_r_slot(total, begin_last + j) == stages[0] - 1 - j);
        }
    }
    for (int k = 0; k <= 16; ++k) CHECK(backwalk_tile(k) == (k == 8 || k == 9 || k == 10 || k == 12));
    if (fails) return 1;
    std::puts("ok");
    return 0;
}
