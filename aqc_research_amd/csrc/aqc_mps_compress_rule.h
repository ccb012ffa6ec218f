// The rules of MPS compression (aqc_mps_compress.hip, aqc_mps_compress_api.cpp), HIP-free: the same text is compiled into the library
// and by a plain C++ compiler (tests/native/mps_compress_rule_selftest.cpp); tests/mps_compress_ref.py states the result in NumPy.
// Notation of aqc_mps_ent_rule.h: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], site tensors [2][chi_q][chi_{q+1}], any gauge; D_q the right
// factors of that header (D_n = [1]).  The result is in the engine's gauge, T'_q = Gamma_q lambda'_q, every bond truncated left to right:
//   carry   W_0 = [1], r_0 = 1 (the new bond dimension on the left)
//   step q = 0 .. n - 2
//           M = [W_q T_q[0]; W_q T_q[1]]                      2 r_q x chi_{q+1}
//           B = M D_{q+1}^T = U Sigma V^H, Sigma descending: the Schmidt values of cut q + 1 of the current state (truncated on the
//           left, untouched on the right)
//           mps_compress_decide(Sigma): r_{q+1} by the engine's rank rule (floor, max_bond, tail: mps_rank_rule, the same operations
//           in the same order), total = sum of all squares, kept = sum of the kept ones, rescale = sqrt(total / kept) as gate_adjacent
//           lambda'_q = rescale Sigma[:r]
//           T'_q[s][l][j] = U[(s, l), j] lambda'_q[j] / lambda'_{q-1}[l]          (lambda'_{-1} = 1; mps_split_body in mode 0)
//           W_{q+1} = rescale U[:, :r]^H M                                        (no inverse of a factor anywhere)
//   last    T'_{n-1}[s][l] = (W_{n-1} T_{n-1}[s])[l] / lambda'_{n-2}[l]
//   weight  the cut drops total - kept (what gate_adjacent adds to the discarded weight: the tail of the rank rule, and whatever the floor
//           and max_bond took); the new state's discarded weight is the input's plus the sum over the cuts
//   failure a zero or non-finite spectrum (status 2) or an SVD at its sweep limit (status 1) fails the state at that cut, not the call;
//           the ranks of a failed state are 0 from that cut on
//   route   fused (every bond <= kMpsEntFusedCap: all states advance together, one workgroup per state in every launch, the rank
//           decisions on the device) else canonical (the engine's identity sweeps, then its truncating sweep, on a clone)
#pragma once
#include <float.h>

#include "aqc_mps_ent_rule.h"

namespace aqc {

enum { kMpsCompressOk = 0, kMpsCompressSweepLimit = 1, kMpsCompressNonFinite = 2 };   // status of a state

inline int mps_compress_route(int n, const int* dims) { return mps_ent_route(n, dims); }

// states per chunk of the sweep: the five stores of the batched SVD of 2k x k matrices (a, u, work: 2 k^2; vh, vmat: k^2 complex
// numbers each) stay within budget_bytes; at least one
inline int mps_compress_chunk(int k, size_t total, size_t budget_bytes) { return mps_svd_chunk(2 * k, k, total, budget_bytes, (size_t)1 << 16); }

// element offsets of the new site tensors (mps_site_offsets of aqc_mps_states_rule.h, n + 1 entries) and bond vectors (n entries) of one
// state, sized by the input's bond dimensions (a rank never exceeds the bond it replaces); the last entry is the total
inline std::vector<size_t> mps_compress_lam_offsets(int n, const int* dims) {
    std::vector<size_t> off(n > 0 ? n : 1, 0);
    for (int q = 0; q + 1 < n; ++q) off[q + 1] = off[q] + (size_t)dims[q + 1];
    return off;
}

#if defined(__HIPCC__)
#define AQC_CMP_HD __host__ __device__
#else
#define AQC_CMP_HD
#endif

// The decision of a cut on s[0 .. count), descending: mps_rank_rule (the same operations in the same order, so that host and device
// agree to the bit), then the weights and the rescaling of gate_adjacent.  ok = 0: s[0] is zero or not finite, nothing else is set.
struct MpsCompressDecision { int ok, rank; double tail, total, kept, rescale; };
AQC_CMP_HD inline MpsCompressDecision mps_compress_decide(int count, const double* s, double trunc_thr, int max_bond) {
    MpsCompressDecision d = {0, 0, 0.0, 0.0, 0.0, 1.0};
    const double smax = s[0];
    if (!(smax > 0.0) || !(smax <= DBL_MAX)) return d;
    int k = 0;
    for (int j = 0; j < count; ++j)
        if (s[j] > kMpsRankFloor * smax) k = j + 1;
    if (max_bond > 0) k = k < max_bond ? k : max_bond;
    double t = 0.0;
    if (trunc_thr > 0.0) {
        while (k > 1 && t + s[k - 1] * s[k - 1] < trunc_thr) { t += s[k - 1] * s[k - 1]; --k; }
    }
    double total = 0.0, kept = 0.0;
    for (int j = 0; j < count; ++j) total += s[j] * s[j];
    for (int j = 0; j < k; ++j) kept += s[j] * s[j];
    d.ok = 1; d.rank = k; d.tail = t; d.total = total; d.kept = kept;
    d.rescale = kept > 0.0 ? sqrt(total / kept) : 1.0;
    return d;
}
// the factor of U[(s, l), j] in T'_q[s][l][j]
AQC_CMP_HD inline double mps_compress_site_factor(double lam_new_j, double lam_left_l) { return lam_new_j / lam_left_l; }
// element e of T'_q packed [2][r][rk]: row (s, l) = s r + l of U, kept column j, left index l
struct MpsCompressSiteIndex { int row, j, l; };
AQC_CMP_HD inline MpsCompressSiteIndex mps_compress_site_index(int e, int r, int rk) {
    const int row = e / rk, j = e - row * rk, l = row < r ? row : row - r;
    return {row, j, l};
}

#undef AQC_CMP_HD

// One step of the rule after the SVD, on the host: m (rows = 2 r_q x cols) row-major, u (rows x ldu, the leading count = min(rows, cols)
// columns hold U), s the count values, lam_left the r_q values of the bond on the left (null: ones).  On success lam (rank), site
// ([2][r_q][rank]) and carry (rank x cols) are resized and filled.
struct MpsCompressStep {
    MpsCompressDecision d;
    std::vector<double> lam;
    std::vector<std::complex<double>> site, carry;
};
inline MpsCompressStep mps_compress_step(int rows, int cols, const std::complex<double>* m, const std::complex<double>* u, int ldu,
                                         const double* s, const double* lam_left, double trunc_thr, int max_bond) {
    typedef std::complex<double> cd;
    MpsCompressStep out;
    const int count = rows < cols ? rows : cols, rq = rows / 2;
    out.d = mps_compress_decide(count, s, trunc_thr, max_bond);
    if (!out.d.ok) return out;
    const int r = out.d.rank;
    out.lam.resize(r);
    for (int j = 0; j < r; ++j) out.lam[j] = out.d.rescale * s[j];
    out.site.resize((size_t)rows * r);
    for (int e = 0; e < rows * r; ++e) {
        const MpsCompressSiteIndex at = mps_compress_site_index(e, rq, r);
        out.site[e] = u[(size_t)at.row * ldu + at.j] * mps_compress_site_factor(out.lam[at.j], lam_left ? lam_left[at.l] : 1.0);
    }
    out.carry.assign((size_t)r * cols, cd(0.0, 0.0));
    for (int j = 0; j < r; ++j)
        for (int c = 0; c < cols; ++c) {
            cd acc = 0.0;
            for (int i = 0; i < rows; ++i) acc += std::conj(u[(size_t)i * ldu + j]) * m[(size_t)i * cols + c];
            out.carry[(size_t)j * cols + c] = out.d.rescale * acc;
        }
    return out;
}

}  // namespace aqc
