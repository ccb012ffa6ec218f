// The rules of linear combinations of MPS states (aqc_mps_combine.hip, aqc_mps_combine_api.cpp), HIP-free: the same text is compiled
// into the library and by a plain C++ compiler (tests/native/mps_combine_rule_selftest.cpp); tests/mps_combine_ref.py states the result
// in NumPy.  Notation of aqc_mps_ent_rule.h: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], site tensors [2][chi_q][chi_{q+1}], any gauge.
// Output j = sum_k c_k psi_k over its terms k = 0 .. K - 1 (states psi_k with sites T^k_q and bonds chi^k_q, complex c_k):
//   sum     the direct sum S with bonds Sigma_q = sum_k chi^k_q (0 < q < n), Sigma_0 = Sigma_n = 1
//           S_0[s]     = [c_0 T^0_0[s] | c_1 T^1_0[s] | ...]                  one row
//           S_q[s]     = diag(T^0_q[s], ..., T^{K-1}_q[s]), zero elsewhere    0 < q < n - 1
//           S_{n-1}[s] = the column stack of T^k_{n-1}[s]
//           n = 1: S_0[s] = sum_k c_k T^k_0[s], summed in the order of the terms
//   blocks  term k owns rows off[k][q] .. off[k+1][q] - 1 of bond q, off[k][q] = sum_{k' < k} chi^{k'}_q for 0 < q < n; at the two edge
//           bonds every term sits at 0 (they share the one row / column) and entry K is 1
//   result  compress(S, trunc_thr, max_bond) of aqc_mps_compress_rule.h: the engine's gauge, every bond cut left to right by
//           mps_compress_decide, the same statuses.  The result's discarded weight is what the cuts of this call dropped: the weights
//           the terms carry are not taken over.
//   errors  are relative to scale = sum_k |c_k| |psi_k|, not to the norm of the result: an exact cancellation is not detected, what is
//           left of it is rounding of that size.
//   route   fused (aqc_mps_compress.hip's sweep on the assembled sites) when every summed bond <= kMpsEntFusedCap, else canonical (S is
//           adopted as an engine state with unit bond vectors and takes compression's canonical route)
//   table   term_off [nout + 1] starts at 0 and grows by at least one term per output; term_state[t] indexes the call's states; the
//           coefficients need not be finite: a NaN coefficient fails its output (status 2), not the call
#pragma once
#include "aqc_mps_compress_rule.h"

namespace aqc {

// Sigma_0 .. Sigma_n of one output; dims: [nterms][n + 1], the bonds of its terms
inline std::vector<int> mps_combine_dims(int n, int nterms, const int* dims) {
    std::vector<int> sum(n + 1, 0);
    for (int k = 0; k < nterms; ++k)
        for (int q = 1; q < n; ++q) sum[q] += dims[(size_t)k * (n + 1) + q];
    sum[0] = sum[n] = 1;
    return sum;
}
// off[k][q], [nterms + 1][n + 1] row-major
inline std::vector<int> mps_combine_block_offsets(int n, int nterms, const int* dims) {
    std::vector<int> off((size_t)(nterms + 1) * (n + 1), 0);
    for (int k = 0; k < nterms; ++k)
        for (int q = 1; q < n; ++q) off[(size_t)(k + 1) * (n + 1) + q] = off[(size_t)k * (n + 1) + q] + dims[(size_t)k * (n + 1) + q];
    off[(size_t)nterms * (n + 1)] = off[(size_t)nterms * (n + 1) + n] = 1;
    return off;
}
// element offsets of the assembled sites of one output (n + 1 entries, the last = total)
inline std::vector<size_t> mps_combine_site_offsets(int n, int nterms, const int* dims) {
    const std::vector<int> sum = mps_combine_dims(n, nterms, dims);
    return mps_site_offsets(n, sum.data());
}
// largest summed bond: 64-bit, the sum of many bonds must not wrap before it is compared
inline long long mps_combine_max_bond(int n, int nterms, const int* dims) {
    long long m = 1;
    for (int q = 1; q < n; ++q) {
        long long s = 0;
        for (int k = 0; k < nterms; ++k) s += dims[(size_t)k * (n + 1) + q];
        m = s > m ? s : m;
    }
    return m;
}
inline int mps_combine_route(int n, int nterms, const int* dims) {
    return mps_combine_max_bond(n, nterms, dims) <= kMpsEntFusedCap ? kMpsEntFused : kMpsEntCanonical;
}
// a term table: 0 fine, else 1 term_off[0] != 0, 2 an output without terms (or term_off not monotone), 3 a state index out of range
inline int mps_combine_check_terms(int nstates, int nout, const int* term_off, const int* term_state) {
    if (term_off[0] != 0) return 1;
    for (int j = 0; j < nout; ++j)
        if (term_off[j + 1] <= term_off[j]) return 2;
    for (int t = 0; t < term_off[nout]; ++t)
        if (term_state[t] < 0 || term_state[t] >= nstates) return 3;
    return 0;
}

#if defined(__HIPCC__)
#define AQC_CMB_HD __host__ __device__
#else
#define AQC_CMB_HD
#endif
// the term that owns index i of bond q (0 < q < n): off[k][q] <= i < off[k+1][q]; a loop over the terms, nothing else
AQC_CMB_HD inline int mps_combine_owner(int nterms, int n, const int* off, int q, int i) {
    int k = 0;
    for (int t = 1; t < nterms; ++t)
        if (i >= off[(size_t)t * (n + 1) + q]) k = t;
    return k;
}
// Element e of assembled site q, packed [2][Sigma_q][Sigma_{q+1}]: the term and the element of its site that it copies (times the
// term's coefficient when q = 0), or term = -1 for a zero.  n >= 2
struct MpsCombineSource { int term; size_t elem; };
AQC_CMB_HD inline MpsCombineSource mps_combine_source(int n, int nterms, const int* off, int q, size_t e) {
    const int* end = off + (size_t)nterms * (n + 1);
    const int rows = end[q], cols = end[q + 1];
    const int s = (int)(e / ((size_t)rows * cols));
    const size_t in = e - (size_t)s * rows * cols;
    const int row = (int)(in / cols), col = (int)(in - (size_t)row * cols);
    const int kr = q > 0 ? mps_combine_owner(nterms, n, off, q, row) : -1;
    const int kc = q + 1 < n ? mps_combine_owner(nterms, n, off, q + 1, col) : -1;
    const int k = kr < 0 ? kc : kr;
    if (kr >= 0 && kc >= 0 && kr != kc) return {-1, 0};
    const int* mine = off + (size_t)k * (n + 1);
    const int r0 = q > 0 ? mine[q] : 0, c0 = q + 1 < n ? mine[q + 1] : 0;
    const int chi_l = q > 0 ? mine[n + 1 + q] - r0 : 1, chi_r = q + 1 < n ? mine[n + 1 + q + 1] - c0 : 1;
    return {k, ((size_t)s * chi_l + (row - r0)) * chi_r + (col - c0)};
}
#undef AQC_CMB_HD

// The host statement of one assembled site: sites[k] is T^k_q ([2][chi^k_q][chi^k_{q+1}]), dims [nterms][n + 1], coeffs [nterms];
// out is resized to 2 Sigma_q Sigma_{q+1} and every element set
inline void mps_combine_site(int n, int nterms, const int* dims, int q, const std::complex<double>* const* sites, const std::complex<double>* coeffs,
                             std::vector<std::complex<double>>& out) {
    typedef std::complex<double> cd;
    if (n == 1) {
        out.assign(2, cd(0.0, 0.0));
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < nterms; ++k) out[s] += coeffs[k] * sites[k][s];
        return;
    }
    const std::vector<int> off = mps_combine_block_offsets(n, nterms, dims);
    const int* end = off.data() + (size_t)nterms * (n + 1);
    out.resize((size_t)2 * end[q] * end[q + 1]);
    for (size_t e = 0; e < out.size(); ++e) {
        const MpsCombineSource src = mps_combine_source(n, nterms, off.data(), q, e);
        if (src.term < 0) out[e] = cd(0.0, 0.0);
        else out[e] = q == 0 ? coeffs[src.term] * sites[src.term][src.elem] : sites[src.term][src.elem];
    }
}

}  // namespace aqc
