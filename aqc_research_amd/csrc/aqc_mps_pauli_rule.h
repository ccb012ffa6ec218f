// The rules of Pauli strings between MPS states (aqc_mps_pauli.hip, aqc_mps_pauli_api.cpp), HIP-free: the same text is compiled into the
// library and by a plain C++ compiler (tests/native/mps_pauli_rule_selftest.cpp); tests/mps_pauli_ref.py states the result in NumPy.
// Notation of aqc_mps_obs_rule.h:
//   ket         psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], bonds chi_q; bra phi with site tensors B_q, bonds beta_q; both [2][left][right],
//               any gauge, neither modified
//   string      uint8 [n], 0, 1, 2, 3 = I, X, Y, Z; entry q acts on qubit q = site q = index bit q of the dense vector
//   letter      a flip f and two phases with P[c ^ f][c] = ph(c):   I: 0, 1, 1    X: 1, 1, 1    Y: 1, i, -i    Z: 0, 1, -1
//   walk        M_0 = [1]   M_{q+1}[u][v] = sum_c ph_q(c) sum_xy conj(B_q[c ^ f_q][x][u]) M_q[x][y] T_q[c][y][v]     (M_q: beta_q x chi_q)
//   result      <phi|P|psi> = M_n[0][0], no normalisation
//   dressed     M' = D^H [M T[0]; M T[1]] with D[c] = conj(ph(c)) B[c ^ f]: a site tensor is that stacked [2 left][right] matrix already
//   expectation (phi = psi) [i, j] = the string's first and last non-identity site (all identity: [0, 0]); the walk starts from L_i, runs
//               over the sites i .. j and closes as sum_uv M_{j+1}[u][v] R_{j+1}[v][u] with the L, R of aqc_mps_obs_rule.h
//   route       fused (one workgroup walks a whole string inside one launch, M in LDS) when every bond of bra and ket is
//               <= kMpsPauliFusedCap, else gemm (per site one batch of zgemm launches for all strings that cross it)
// Every sum runs in a fixed order that depends on the bond dimensions of the two states and on the string only.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace aqc {

enum { kMpsPauliByRule = 0, kMpsPauliFused = 1, kMpsPauliGemm = 2, kMpsPauliFusedCap = 64 };
enum { kMpsPauliI = 0, kMpsPauliX = 1, kMpsPauliY = 2, kMpsPauliZ = 3 };

inline bool mps_pauli_method_ok(int method) { return method == kMpsPauliByRule || method == kMpsPauliFused || method == kMpsPauliGemm; }

// the flip of a letter, and its phase ph(c) as quarter turns k: ph = i^k (0: 1, 1: i, 2: -1, 3: -i)
#if defined(__HIPCC__)
#define AQC_PAULI_HD __host__ __device__
#else
#define AQC_PAULI_HD
#endif
AQC_PAULI_HD inline int mps_pauli_flip(int letter) { return letter == kMpsPauliX || letter == kMpsPauliY; }
AQC_PAULI_HD inline int mps_pauli_turns(int letter, int c) { return letter == kMpsPauliY ? (c ? 3 : 1) : letter == kMpsPauliZ ? (c ? 2 : 0) : 0; }
// i^k (re, im) = ...: no multiplication, signs and a swap
AQC_PAULI_HD inline void mps_pauli_turn(int k, double re, double im, double& out_re, double& out_im) {
    out_re = k == 0 ? re : k == 1 ? -im : k == 2 ? -re : im;
    out_im = k == 0 ? im : k == 1 ? re : k == 2 ? -im : -re;
}
#undef AQC_PAULI_HD

// strings [nstrings][n]: the index of the first entry that is no letter, -1: none
inline int64_t mps_pauli_bad_letter(const uint8_t* strings, size_t count) {
    for (size_t k = 0; k < count; ++k)
        if (strings[k] > 3) return (int64_t)k;
    return -1;
}

// first and last non-identity site of one string; all identity: [0, 0]
inline void mps_pauli_support(int n, const uint8_t* s, int32_t* first, int32_t* last) {
    int i = -1, j = -1;
    for (int q = 0; q < n; ++q)
        if (s[q] != kMpsPauliI) { if (i < 0) i = q; j = q; }
    *first = i < 0 ? 0 : i;
    *last = j < 0 ? 0 : j;
}

// dims: the n + 1 bond dimensions of a state; bra_dims null: the ket's
inline int mps_pauli_max_bond(int n, const int* bra_dims, const int* ket_dims) {
    int m = 1;
    for (int q = 0; q <= n; ++q) {
        m = ket_dims[q] > m ? ket_dims[q] : m;
        if (bra_dims) m = bra_dims[q] > m ? bra_dims[q] : m;
    }
    return m;
}
inline int mps_pauli_route(int n, const int* bra_dims, const int* ket_dims) {
    return mps_pauli_max_bond(n, bra_dims, ket_dims) <= kMpsPauliFusedCap ? kMpsPauliFused : kMpsPauliGemm;
}

// ---- gemm route: a job (one string of one pair) holds M (beta x chi) and, during a step, the stacked product [M T_0; M T_1]
// (sizes in complex numbers: the largest M and the largest stacked product along the chain)
enum { kMpsPauliGroupMax = 32768 };   // a group is one grid dimension of a table launch
inline size_t mps_pauli_m_elems(int n, const int* bra_dims, const int* ket_dims) {
    size_t m = 1;
    for (int q = 0; q <= n; ++q) {
        const size_t e = (size_t)(bra_dims ? bra_dims[q] : ket_dims[q]) * (size_t)ket_dims[q];
        m = e > m ? e : m;
    }
    return m;
}
inline size_t mps_pauli_f_elems(int n, const int* bra_dims, const int* ket_dims) {
    size_t f = 1;
    for (int q = 0; q < n; ++q) {
        const size_t e = 2 * (size_t)(bra_dims ? bra_dims[q] : ket_dims[q]) * (size_t)ket_dims[q + 1];
        f = e > f ? e : f;
    }
    return f;
}
inline size_t mps_pauli_job_elems(int n, const int* bra_dims, const int* ket_dims) {
    return mps_pauli_m_elems(n, bra_dims, ket_dims) + mps_pauli_f_elems(n, bra_dims, ket_dims);
}
// jobs walked together (a group) so that their scratch stays below budget_bytes; at least one, at most kMpsPauliGroupMax
inline int mps_pauli_group_size(size_t job_elems, int njobs, size_t budget_bytes) {
    const size_t per = 16 * job_elems;
    size_t g = per ? budget_bytes / per : (size_t)njobs;
    if (g > (size_t)njobs) g = (size_t)njobs;
    if (g > (size_t)kMpsPauliGroupMax) g = (size_t)kMpsPauliGroupMax;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace aqc
