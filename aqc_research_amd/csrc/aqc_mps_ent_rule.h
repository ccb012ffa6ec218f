// The rules of the Schmidt spectra of MPS states (aqc_mps_ent.hip, aqc_mps_ent_api.cpp), HIP-free: the same text is compiled into the
// library and by a plain C++ compiler (tests/native/mps_ent_rule_selftest.cpp); tests/mps_ent_ref.py states the result in NumPy.
// Notation of aqc_mps_obs_rule.h: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], site tensors [2][chi_q][chi_{q+1}], any gauge.
//   left    C_0 = [1]   C_{q+1} = the R factor (chi_{q+1} x chi_{q+1}) of the stacked 2 chi_q x chi_{q+1} matrix [C_q T_q[0]; C_q T_q[1]];
//           rows beyond min(2 chi_q, chi_{q+1}) are zero.  C_q^H C_q = L_q, the left environment, which is never formed.
//   right   D_n = [1]   D_q = the R factor of [D_{q+1} T_q[0]^T; D_{q+1} T_q[1]^T]: the same step with the site read transposed.
//           D_q^H D_q = conj R_q.
//   cut q   (qubits 0 .. q-1 | q .. n-1, q = 1 .. n-1): the Schmidt values are the singular values of S_q = C_q D_q^T (chi_q x chi_q),
//           descending.  Nothing is normalised: sum_k s_k^2 = <psi|psi> at every cut.
//   R       by unpivoted Householder reflections, R only: column j takes its reflection from rows j .. of the stacked matrix, a column
//           that is zero there (or below 1e-150: mps_ent_reflects) is skipped, the last row needs none; no Q is kept.  Any R with R^H R = M^H M gives the same
//           singular values, so rank-deficient bonds need no special case.  (Eigenvalues of L_q R_q would square the condition number
//           and lose every value below about 1e-8 s_max.)
//   route   fused (one workgroup walks the whole chain of factors inside one launch, the stacked matrix in LDS; the cuts' SVDs in one
//           batch) when every bond is <= kMpsEntFusedCap, else canonical (the identity sweeps of the engine on a clone; the bond vectors
//           are the values, zero-padded to chi_q).
//   rank    the engine's rank decision on a descending spectrum (moved here from gate_adjacent, which calls it): the floor
//           kMpsRankFloor s_max, then max_bond, then the tail dropped while its weight stays below trunc_thr.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <complex>
#include <vector>

#include "aqc_mps_states_rule.h"

namespace aqc {

enum { kMpsEntFusedCap = 64 };
enum { kMpsEntByRule = 0, kMpsEntFused = 1, kMpsEntCanonical = 2 };
enum { kMpsEntConverged = 0, kMpsEntSweepLimit = 1, kMpsEntNonFinite = 2 };   // status of a cut (those of the batched SVD)
constexpr double kMpsRankFloor = 1e-14;

inline bool mps_ent_method_ok(int method) { return method == kMpsEntByRule || method == kMpsEntFused || method == kMpsEntCanonical; }
inline int mps_ent_route(int n, const int* dims) { return mps_max_bond(n, dims) <= kMpsEntFusedCap ? kMpsEntFused : kMpsEntCanonical; }
inline int mps_ent_cuts(int n) { return n > 1 ? n - 1 : 0; }
// the factors of one state, C_1 .. C_{n-1} (and in a second block of the same size D_1 .. D_{n-1}) packed back to back: element offset of
// the factor of bond q, q = 1 .. n - 1, and (entry n) the size of a block; entry 0 is unused
inline std::vector<size_t> mps_ent_factor_offsets(int n, const int* dims) {
    std::vector<size_t> off(n + 1, 0);
    for (int q = 1; q < n; ++q) off[q + 1] = off[q] + (size_t)dims[q] * dims[q];
    return off;
}

#if defined(__HIPCC__)
#define AQC_ENT_HD __host__ __device__
#else
#define AQC_ENT_HD
#endif
// ---- the stacked matrix of a step with chi_in rows per product: logical row r of [P_0; P_1] lives in the planes of the first product
// (plane 0) at row r when r < chi_in, else in those of the second (plane 1) at row r - chi_in
struct MpsEntRow { int plane, row; };
AQC_ENT_HD inline MpsEntRow mps_ent_stacked_row(int r, int chi_in) { return r < chi_in ? MpsEntRow{0, r} : MpsEntRow{1, r - chi_in}; }
// reflections of a rows x cols matrix: columns 0 .. min(rows - 1, cols) - 1
AQC_ENT_HD inline int mps_ent_reflections(int rows, int cols) { return rows - 1 < cols ? rows - 1 : cols; }
// rows of the R factor that can be non-zero
AQC_ENT_HD inline int mps_ent_r_rows(int rows, int cols) { return rows < cols ? rows : cols; }

// Whether a column with this sum of squares takes a reflection: not when it is zero, nor when it is so small (|x| < 1e-150: columns of
// deeply rank-deficient states) that tau below, 1 / (|x| (|x| + |x0|)), would overflow; a NaN reflects (and spreads).
AQC_ENT_HD inline bool mps_ent_reflects(double norm2) { return !(norm2 < 1e-300); }

// One reflection from the column x (its first entry x0, sum of squares norm2 > 0): H = 1 - tau v v^H with v = x + phase |x| e_0,
// H x = alpha e_0.  Stated on real numbers so that the device code takes the same operations.
struct MpsEntReflection { double v0r, v0i, alphar, alphai, tau; };
AQC_ENT_HD inline MpsEntReflection mps_ent_reflection(double x0r, double x0i, double norm2) {
    const double nrm = sqrt(norm2), ax = sqrt(x0r * x0r + x0i * x0i);
    const double pr = ax > 0.0 ? x0r / ax : 1.0, pi = ax > 0.0 ? x0i / ax : 0.0;
    MpsEntReflection h;
    h.v0r = x0r + pr * nrm; h.v0i = x0i + pi * nrm;
    h.alphar = -pr * nrm; h.alphai = -pi * nrm;
    h.tau = 1.0 / (nrm * (nrm + ax));   // 2 / (v^H v)
    return h;
}

#undef AQC_ENT_HD

// The R factor of the row-major rows x cols matrix m, in place: on return the upper triangle of the leading mps_ent_r_rows rows holds R,
// everything below the diagonal is zero.  The host statement of what mps_ent_chain_kernel does in LDS.
inline void mps_ent_householder_r(int rows, int cols, std::complex<double>* m) {
    typedef std::complex<double> cd;
    std::vector<cd> v(rows > 0 ? rows : 1);
    const int nref = mps_ent_reflections(rows, cols);
    for (int j = 0; j < nref; ++j) {
        double norm2 = 0.0;
        for (int r = j; r < rows; ++r) norm2 += std::norm(m[(size_t)r * cols + j]);
        if (!mps_ent_reflects(norm2)) continue;
        const cd x0 = m[(size_t)j * cols + j];
        const MpsEntReflection h = mps_ent_reflection(x0.real(), x0.imag(), norm2);
        v[0] = cd(h.v0r, h.v0i);
        for (int r = j + 1; r < rows; ++r) v[r - j] = m[(size_t)r * cols + j];
        for (int c = j + 1; c < cols; ++c) {
            cd w = 0.0;
            for (int r = j; r < rows; ++r) w += std::conj(v[r - j]) * m[(size_t)r * cols + c];
            w *= h.tau;
            for (int r = j; r < rows; ++r) m[(size_t)r * cols + c] -= v[r - j] * w;
        }
        m[(size_t)j * cols + j] = cd(h.alphar, h.alphai);
        for (int r = j + 1; r < rows; ++r) m[(size_t)r * cols + j] = 0.0;
    }
    for (int r = 1; r < rows; ++r)
        for (int c = 0; c < r && c < cols; ++c) m[(size_t)r * cols + c] = 0.0;   // (exact zeros already; rows past the reflections too)
}

// ---- chunks of the batched SVD: matrices of k x k whose five stores (a, u, vh, work, vmat) stay within budget_bytes; at least one
inline int mps_ent_chunk(int k, size_t total, size_t budget_bytes) { return mps_svd_chunk(k, k, total, budget_bytes, (size_t)1 << 20); }

// ---- the engine's rank decision on s[0 .. count), descending: false when s[0] is zero or not finite (rank and dropped untouched)
inline bool mps_rank_rule(int count, const double* s, double trunc_thr, int max_bond, int* rank, double* dropped) {
    const double smax = s[0];
    if (!(smax > 0.0) || !std::isfinite(smax)) return false;
    int k = 0;
    for (int j = 0; j < count; ++j)
        if (s[j] > kMpsRankFloor * smax) k = j + 1;              // drop numerically zero values (rank deficiency)
    if (max_bond > 0) k = k < max_bond ? k : max_bond;
    double d = 0.0;
    if (trunc_thr > 0.0) {                                       // discard the tail while its weight stays below the threshold
        while (k > 1 && d + s[k - 1] * s[k - 1] < trunc_thr) { d += s[k - 1] * s[k - 1]; --k; }
    }
    *rank = k;
    *dropped = d;
    return true;
}

}  // namespace aqc
