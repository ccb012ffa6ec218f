// The rules of the pair density matrices of MPS states (aqc_mps_obs.hip, aqc_mps_obs_api.cpp), HIP-free: the same text is compiled into the
// library and by a plain C++ compiler (tests/native/mps_obs_rule_selftest.cpp); tests/mps_obs_ref.py states the result in NumPy.
//   state       psi(b) = T_0[b_0] T_1[b_1] ... T_{n-1}[b_{n-1}], site tensors [2][chi_q][chi_{q+1}], any gauge
//   convention  for the pair (i, j) the row index is value(i) + 2 value(j):  rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b)
//   L_0 = [1]   L_{q+1}[u][v] = sum_c sum_xy conj(T_q[c][x][u]) L_q[x][y] T_q[c][y][v]
//   R_n = [1]   R_q[x][y]     = sum_c sum_uv T_q[c][x][u] R_{q+1}[u][v] conj(T_q[c][y][v])
//   open  i     E^{ab}[u][v]  = sum_xy conj(T_i[b][x][u]) L_i[x][y] T_i[a][y][v]                     (E^{ba} = (E^{ab})^H)
//   step  q     E^{ab}[u][v] <- sum_c sum_xy conj(T_q[c][x][u]) E^{ab}[x][y] T_q[c][y][v]            (i < q < j)
//   close j     K^{cd}[y][x]  = sum_uv T_j[c][y][v] R_{j+1}[v][u] conj(T_j[d][x][u])                 (K^{dc} = (K^{cd})^H)
//   result      rho_(i,j)[a + 2c][b + 2d] = sum_xy E^{ab}[x][y] K^{cd}[y][x]
// Kept: the components 00, 01, 11 of E and of K (kMpsObsComps); the ten entries of the upper triangle follow from them
// (mps_obs_upper), the rest is mirrored, so a matrix is exactly Hermitian with an exactly real diagonal.
//   plan        all pairs with the same lower qubit i share chain i, which walks from i to its farthest partner and emits one matrix at
//               every requested j; a pair given as (j, i), j > i, is rho_(i,j) with its two index bits transposed; a pair that occurs
//               twice is served twice from the same emission.  The plan depends on n and the pair list only.
//   route       fused (one workgroup per chain component walks the chain inside one launch, E in LDS) when every bond dimension of the
//               state is <= kMpsObsFusedCap, else gemm (one batch of zgemm launches per site for all chains that cross it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "aqc_mps_states_rule.h"

namespace aqc {

enum { kMpsObsComps = 3, kMpsObsUpper = 10, kMpsObsFusedCap = 64 };
enum { kMpsObsByRule = 0, kMpsObsFused = 1, kMpsObsGemm = 2 };

// entry e of the upper triangle: row r <= column s of the 4 x 4, the component of E and of K it is summed from, and whether E enters as
// its adjoint (E^{10} = (E^{01})^H).  Components: 0 = 00, 1 = 01, 2 = 11.
struct MpsObsEntry { int row, col, ecomp, kcomp, eadj; };
inline MpsObsEntry mps_obs_upper(int e) {
    static const MpsObsEntry tab[kMpsObsUpper] = {
        {0, 0, 0, 0, 0}, {0, 1, 1, 0, 0}, {0, 2, 0, 1, 0}, {0, 3, 1, 1, 0}, {1, 1, 2, 0, 0},
        {1, 2, 1, 1, 1}, {1, 3, 2, 1, 0}, {2, 2, 0, 2, 0}, {2, 3, 1, 2, 0}, {3, 3, 2, 2, 0}};
    return tab[e];
}

struct MpsObsEmit { int chain, site; };   // one 4 x 4 matrix: chain `chain` (= the lower qubit) read at site `site` (= the higher one)
struct MpsObsPlan {
    std::vector<int> last;                 // [n] per start site the last site its chain walks to, -1: no chain starts there
    std::vector<MpsObsEmit> emits;         // ordered by site, then by chain; every (chain, site) once
    std::vector<int> pair_emit;            // per pair: index into emits
    std::vector<int> pair_transposed;      // per pair: 1 = given as (higher, lower)
    int nchains = 0;
};

// pairs [npairs][2]; false: n < 2, a qubit out of range or two equal qubits in a pair (the plan is then unspecified)
inline bool mps_obs_plan(int n, int npairs, const int32_t* pairs, MpsObsPlan& plan) {
    plan = MpsObsPlan();
    if (n < 2 || npairs < 0 || (npairs > 0 && !pairs)) return false;
    plan.last.assign(n, -1);
    plan.pair_emit.assign(npairs, -1);
    plan.pair_transposed.assign(npairs, 0);
    for (int p = 0; p < npairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= n || b < 0 || b >= n || a == b) return false;
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        plan.pair_transposed[p] = a > b;
        if (hi > plan.last[lo]) plan.last[lo] = hi;
    }
    for (int i = 0; i < n; ++i) plan.nchains += plan.last[i] >= 0;
    // emissions by site, then by chain: the order in which a walk over the sites meets them
    std::vector<std::vector<int>> at(n);   // per site the chains that emit there, ascending, once each
    for (int p = 0; p < npairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        std::vector<int>& v = at[hi];
        size_t k = 0;
        while (k < v.size() && v[k] < lo) ++k;
        if (k == v.size() || v[k] != lo) v.insert(v.begin() + k, lo);
    }
    std::vector<int> first(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        first[j + 1] = first[j] + (int)at[j].size();
        for (int c : at[j]) plan.emits.push_back(MpsObsEmit{c, j});
    }
    for (int p = 0; p < npairs; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const std::vector<int>& v = at[hi];
        size_t k = 0;
        while (v[k] != lo) ++k;
        plan.pair_emit[p] = first[hi] + (int)k;
    }
    return true;
}

inline int mps_obs_route(int n, const int* dims) { return mps_max_bond(n, dims) <= kMpsObsFusedCap ? kMpsObsFused : kMpsObsGemm; }

// the pair's matrix from its emission: out[r][s] = m[r][s], or with the two index bits of r and of s swapped (complex numbers as pairs)
inline void mps_obs_place(const double* m, int transposed, double* out) {
    for (int r = 0; r < 4; ++r)
        for (int s = 0; s < 4; ++s) {
            const int rr = transposed ? ((r & 1) << 1) | (r >> 1) : r, ss = transposed ? ((s & 1) << 1) | (s >> 1) : s;
            out[2 * (4 * r + s)] = m[2 * (4 * rr + ss)];
            out[2 * (4 * r + s) + 1] = m[2 * (4 * rr + ss) + 1];
        }
}

// ---- scratch of one state, in complex numbers
// the environments, packed back to back: element offset of L_q in the one buffer and of R_q in the other, q = 0 .. n, and (entry
// n + 1) the size of each buffer
inline std::vector<size_t> mps_obs_env_offsets(int n, const int* dims) {
    std::vector<size_t> off(n + 2, 0);
    for (int q = 0; q <= n; ++q) off[q + 1] = off[q] + (size_t)dims[q] * dims[q];
    return off;
}
// gemm route: a chain holds kMpsObsComps matrices E and, during a step, kMpsObsComps stacked products [E T_0; E T_1]
inline size_t mps_obs_slot_elems(int n, const int* dims) { const size_t m = (size_t)mps_max_bond(n, dims); return m * m; }
inline size_t mps_obs_chain_elems(int n, const int* dims) { return 3 * (size_t)kMpsObsComps * mps_obs_slot_elems(n, dims); }
// chains walked together (a group) so that their scratch stays below budget_bytes; at least one
inline int mps_obs_group_size(int n, const int* dims, int nchains, size_t budget_bytes) {
    const size_t per = 16 * mps_obs_chain_elems(n, dims);
    size_t g = per ? budget_bytes / per : (size_t)nchains;
    if (g < 1) g = 1;
    if (g > (size_t)nchains) g = (size_t)nchains;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace aqc
