// Self-test of csrc/aqc_mps_states_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_states_rule.py): the table
// layout of the three calls that pack one held to the word arithmetic they used to write out by hand, with values written and read back
// through it; the distinct list; the one chunk rule against the two it replaced; the bond helpers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_compress_rule.h"
#include "../../aqc_research_amd/csrc/aqc_mps_ent_rule.h"
#include "../../aqc_research_amd/csrc/aqc_mps_states_rule.h"

using namespace aqc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// A table of `states` records in `layout`, whose sections hold `counts[s]` entries (ints where is_int[s]): every entry gets a value of
// its own through the packed offset, as a call packs it on the host, and is read back through the same layout's pointer offset, as a
// call forms its device pointers; a trailing guard word behind the table must stay untouched
static void write_and_read_back(const MpsTableLayout& layout, const std::vector<size_t>& counts, const std::vector<bool>& is_int, size_t states) {
    const unsigned long long guard = 0xA5A5A5A5A5A5A5A5ull;
    std::vector<unsigned long long> words(layout.per * states + 1, 0);
    words.back() = guard;
    for (size_t i = 0; i < states; ++i)
        for (size_t s = 0; s < counts.size(); ++s) {
            unsigned long long* at = words.data() + layout.word(i, (int)s);
            CHECK(((const char*)at - (const char*)words.data()) % 8 == 0);
            for (size_t k = 0; k < counts[s]; ++k) {
                if (is_int[s]) {
                    const int v = (int)(1000000 * i + 1000 * s + k + 1);
                    memcpy((char*)at + k * sizeof(int), &v, sizeof(int));
                } else {
                    const unsigned long long v = ((unsigned long long)(i + 1) << 40) | ((unsigned long long)(s + 1) << 20) | (k + 1);
                    memcpy(at + k, &v, 8);
                }
            }
        }
    for (size_t i = 0; i < states; ++i)
        for (size_t s = 0; s < counts.size(); ++s)
            for (size_t k = 0; k < counts[s]; ++k) {
                if (is_int[s]) {
                    const int* p = reinterpret_cast<const int*>(words.data() + layout.word(i, (int)s));
                    CHECK(p[k] == (int)(1000000 * i + 1000 * s + k + 1));
                } else {
                    const unsigned long long* p = words.data() + layout.word(i, (int)s);
                    CHECK(p[k] == (((unsigned long long)(i + 1) << 40) | ((unsigned long long)(s + 1) << 20) | (k + 1)));
                }
            }
    CHECK(words.back() == guard);
}

int main() {
    // ---- layout: the records of Schmidt spectra, compression and Pauli strings against their hand formulas
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)64}) {
        const MpsTableLayout ent({mps_table_words(n), mps_table_words(n + 1), mps_table_ints(n + 1)});
        CHECK(ent.per == n + (n + 1) + (n + 2) / 2);
        CHECK(ent.at.size() == 3 && ent.at[0] == 0 && ent.at[1] == n && ent.at[2] == 2 * n + 1);
        const MpsTableLayout cmp({mps_table_words(n), mps_table_words(n + 1), mps_table_words(n), mps_table_words(n), mps_table_ints(n + 1)});
        CHECK(cmp.per == n + (n + 1) + n + n + (n + 2) / 2);
        CHECK(cmp.at.size() == 5 && cmp.at[0] == 0 && cmp.at[1] == n && cmp.at[2] == 2 * n + 1 && cmp.at[3] == 3 * n + 1 && cmp.at[4] == 4 * n + 1);
        const MpsTableLayout pauli({mps_table_words(n), mps_table_words(n + 2), mps_table_words(n + 1), mps_table_ints(n + 1)});
        CHECK(pauli.per == n + (n + 2) + (n + 1) + (n + 2) / 2);
        CHECK(pauli.at.size() == 4 && pauli.at[0] == 0 && pauli.at[1] == n && pauli.at[2] == 2 * n + 2 && pauli.at[3] == 3 * n + 3);
        // the trailing int section of n + 1 entries fits (odd and even n), and the record of the next state starts behind it
        for (const MpsTableLayout* l : {&ent, &cmp, &pauli}) {
            CHECK(l->at.back() * 8 + (n + 1) * sizeof(int) <= l->per * 8);
            CHECK(l->per * 8 - (l->at.back() * 8 + (n + 1) * sizeof(int)) < 8);
            for (int s = 0; s < (int)l->at.size(); ++s) {
                CHECK(l->word(0, s) == l->at[s] && l->word(3, s) == 3 * l->per + l->at[s]);
                CHECK(l->word(1, 0) > l->word(0, s));
            }
        }
        write_and_read_back(ent, {n, n + 1, n + 1}, {false, false, true}, 3);
        write_and_read_back(cmp, {n, n + 1, n, n, n + 1}, {false, false, false, false, true}, 3);
        write_and_read_back(pauli, {n, n + 2, n + 1, n + 1}, {false, false, false, true}, 3);
    }
    {   // an int section in the middle is rounded up to whole words; an empty layout is empty
        const MpsTableLayout l({mps_table_ints(3), mps_table_words(2), mps_table_ints(0), mps_table_ints(1)});
        CHECK(l.at[0] == 0 && l.at[1] == 2 && l.at[2] == 4 && l.at[3] == 4 && l.per == 5);
        write_and_read_back(l, {3, 2, 0, 1}, {true, false, true, true}, 2);
        const MpsTableLayout none;
        CHECK(none.per == 0 && none.at.empty());
    }

    // ---- distinct list: first appearance, lane_state
    {
        int a = 0, b = 0, c = 0;   // three addresses, listed in an order that is not theirs
        const int* handles[5] = {&c, &a, &c, &b, &a};
        const MpsDistinct<const int*> d = mps_distinct(handles, 5);
        CHECK(d.items.size() == 3 && d.items[0] == &c && d.items[1] == &a && d.items[2] == &b);
        CHECK(d.lane_state == (std::vector<int>{0, 1, 0, 2, 1}));
        const int* abacb[5] = {&a, &b, &a, &c, &b};
        const MpsDistinct<const int*> e = mps_distinct(abacb, 5);
        CHECK(e.items == (std::vector<const int*>{&a, &b, &c}) && e.lane_state == (std::vector<int>{0, 1, 0, 2, 1}));
        const MpsDistinct<const int*> one = mps_distinct(handles, 1), none = mps_distinct(handles, 0);
        CHECK(one.items.size() == 1 && one.lane_state == std::vector<int>{0} && none.items.empty() && none.lane_state.empty());
    }

    // ---- chunk rule: the two callers' rules are the one rule at (k, k) and at (2k, k), with their caps
    for (int k : {1, 3, 64})
        for (size_t total : {(size_t)1, (size_t)7, (size_t)1000000})
            for (size_t budget : {(size_t)1, (size_t)1 << 20, (size_t)256 << 20}) {
                const int ent = mps_svd_chunk(k, k, total, budget, (size_t)1 << 20), cmp = mps_svd_chunk(2 * k, k, total, budget, (size_t)1 << 16);
                CHECK(ent == mps_ent_chunk(k, total, budget) && cmp == mps_compress_chunk(k, total, budget));
                // what the two rules were before they became calls of the one: 5 and 8 matrices of k x k complex numbers per item
                size_t ge = budget / ((size_t)5 * 16 * k * k), gc = budget / ((size_t)8 * 16 * k * k);
                ge = ge > total ? total : ge; ge = ge > ((size_t)1 << 20) ? (size_t)1 << 20 : ge; ge = ge < 1 ? 1 : ge;
                gc = gc > total ? total : gc; gc = gc > ((size_t)1 << 16) ? (size_t)1 << 16 : gc; gc = gc < 1 ? 1 : gc;
                CHECK((size_t)ent == ge && (size_t)cmp == gc);
            }
    CHECK(mps_svd_chunk(64, 64, 1000000, (size_t)256 << 20, (size_t)1 << 20) == 819 && mps_svd_chunk(128, 64, 1000000, (size_t)256 << 20, (size_t)1 << 16) == 512);
    CHECK(mps_svd_chunk(1, 1, 0, 1, 8) == 1 && mps_svd_chunk(0, 0, 5, 1, 8) == 5 && mps_svd_chunk(1, 1, 100, (size_t)1 << 20, 8) == 8);

    // ---- bonds
    {
        const int dims[5] = {1, 2, 3, 2, 1}, one[2] = {1, 1};
        CHECK(mps_max_bond(4, dims) == 3 && mps_max_bond(1, one) == 1);
        const std::vector<size_t> so = mps_site_offsets(4, dims);
        CHECK(so == (std::vector<size_t>{0, 4, 16, 28, 32}) && mps_site_offsets(1, one) == (std::vector<size_t>{0, 2}));
    }

    std::printf("mps_states_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
