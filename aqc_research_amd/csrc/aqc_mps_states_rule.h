// What the single-lane MPS calls (aqc_mps_obs_api.cpp, aqc_mps_sample_api.cpp, aqc_mps_pauli_api.cpp, aqc_mps_ent_api.cpp,
// aqc_mps_compress_api.cpp) share about their input states, HIP-free: the same text is compiled into the library and by a plain C++
// compiler (tests/native/mps_states_rule_selftest.cpp).  The host side that uses it is aqc_mps_call.h.
//   bonds     the largest bond dimension and the element offsets of the site tensors of a state
//   table     what the kernels read of every state of a call travels in ONE upload of 8-byte words, a record per state; the layout
//             gives the word offset of every section of a record, to the code that packs it and to the code that forms the device
//             pointers alike
//   distinct  a state listed many times in a call is read once: the distinct handles in order of first appearance
//   chunk     how many matrices of a batched SVD share its stores
#pragma once
#include <stddef.h>

#include <initializer_list>
#include <map>
#include <vector>

namespace aqc {

constexpr size_t kMpsCallBudget = (size_t)256 << 20;   // bytes of scratch that a call sizes its groups and chunks by

// dims: the n + 1 bond dimensions
inline int mps_max_bond(int n, const int* dims) {
    int m = 1;
    for (int q = 0; q <= n; ++q) m = dims[q] > m ? dims[q] : m;
    return m;
}
// element offset of site q ([2][dims[q]][dims[q+1]] complex) in the sites of one state packed back to back, n + 1 entries (the last =
// total)
inline std::vector<size_t> mps_site_offsets(int n, const int* dims) {
    std::vector<size_t> off(n + 1, 0);
    for (int q = 0; q < n; ++q) off[q + 1] = off[q] + (size_t)2 * dims[q] * dims[q + 1];
    return off;
}

// ---- the record of one state in a call's table: sections of 8-byte words (pointers, size_t) or of ints rounded up to whole words, in
// the order given; every section starts on a word
struct MpsTableSection { size_t count; bool ints; };
inline MpsTableSection mps_table_words(size_t count) { return {count, false}; }
inline MpsTableSection mps_table_ints(size_t count) { return {count, true}; }
struct MpsTableLayout {
    std::vector<size_t> at;   // word offset of every section in a record
    size_t per = 0;           // words of a record
    MpsTableLayout() = default;
    MpsTableLayout(std::initializer_list<MpsTableSection> sections) {
        for (const MpsTableSection& s : sections) {
            at.push_back(per);
            per += s.ints ? (s.count * sizeof(int) + 7) / 8 : s.count;
        }
    }
    size_t word(size_t state, int section) const { return state * per + at[section]; }
};

// ---- the distinct handles of a call in order of first appearance; lane_state[i] = the index of handles[i] among them
template <class H>
struct MpsDistinct {
    std::vector<H> items;
    std::vector<int> lane_state;
};
template <class H>
MpsDistinct<H> mps_distinct(const H* handles, size_t count) {
    MpsDistinct<H> d;
    std::map<H, int> seen;
    for (size_t i = 0; i < count; ++i) {
        auto it = seen.find(handles[i]);
        if (it == seen.end()) {
            it = seen.emplace(handles[i], (int)d.items.size()).first;
            d.items.push_back(handles[i]);
        }
        d.lane_state.push_back(it->second);
    }
    return d;
}

// ---- chunks of a batched SVD of rows x cols matrices: as many as keep its five stores (a, u, work: rows x cols; vh, vmat: cols x cols
// complex numbers each) within budget_bytes, at most `cap` and `total`, at least one
inline int mps_svd_chunk(int rows, int cols, size_t total, size_t budget_bytes, size_t cap) {
    const size_t per = (size_t)16 * (3 * (size_t)rows * (size_t)cols + 2 * (size_t)cols * (size_t)cols);
    size_t g = per ? budget_bytes / per : total;
    if (g > total) g = total;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace aqc
