// The rules of the conversion of dense vectors into MPS states (aqc_mps_fromvec.hip, aqc_mps_fromvec_api.cpp), HIP-free: the same text is
// compiled into the library and by a plain C++ compiler (tests/native/mps_fromvec_rule_selftest.cpp); tests/mps_fromvec_ref.py states
// the result in NumPy.  psi: 2^n amplitudes, index bit q is site q.  The result is in the engine's gauge, T'_q = Gamma_q lambda'_q, every
// bond cut left to right: the carry recursion of aqc_mps_compress_rule.h with the dense remainder in place of W_q T_q.
//   start   A_0 = psi read row-major as [2^(n-1)][2]: row = the bits above bit 0, column = bit 0; r_0 = 1
//   step q = 0 .. n - 2, r_q kept on the left: A_q is [N_r = 2^(n-1-q)][2 r_q] row-major, its column index s r_q + l, the order (s, l) of
//           mps_compress_step; M = A_q^T is the 2 r_q x N_r two-block matrix of that rule
//           R = the R factor of A_q (R only, by the reflections of aqc_mps_ent_rule.h; any R with R^H R = A_q^H A_q serves), taken
//           block by block: the first block of 64 rows of a part by itself, every other one stacked beneath the running R, in
//           mps_fromvec_parts(N_r) independent parts whose factors are folded four at a time in a fixed tree
//           R^T = U Sigma X^H (the leading min(2 r_q, N_r) columns of R^T: the other rows of R are exact zeros): U, Sigma are those of M
//           mps_compress_decide(Sigma, trunc_thr, max_bond): r_{q+1}, total, kept, rescale
//           lambda'_q = rescale Sigma[:r];  T'_q[s][l][j] = U[(s, l), j] lambda'_q[j] / lambda'_{q-1}[l]
//           A_{q+1} = Y = rescale A_q conj(U[:, :r]), row-major with row stride exactly r, then READ as [N_r / 2][2 r]: no transpose,
//           no data movement, the vector is never bit-reversed
//   last    T'_{n-1}[s][l] = A_{n-1}[0][s r + l] / lambda'_{n-2}[l]
//   weight  the sum over the cuts of total - kept
//   failure a zero or non-finite spectrum (status 2) or an SVD at its sweep limit (status 1) fails the lane at that site, not the call
//   route   fused (2 <= n <= 30 and every bond bound min(2^b, 2^(n-b), max_bond if > 0) <= kMpsFromVecCap) else host (the NumPy loop of
//           mps_operations.vector_to_canonical_mps).  The squared route (A^H A and its eigenvalues) loses every value below about
//           1e-8 s_max and is not taken anywhere.
#pragma once
#include <functional>

#include "aqc_mps_compress_rule.h"

namespace aqc {

enum { kMpsFromVecCap = 32 };                  // bonds of the fused route: [R; block] of 2 r <= 64 columns is the 128 x 64 of the four LDS planes
enum { kMpsFromVecMinQubits = 2, kMpsFromVecMaxQubits = 30 };
enum { kMpsFromVecByRule = 0, kMpsFromVecFused = 1, kMpsFromVecHost = 2 };
enum { kMpsFromVecBlockRows = 64, kMpsFromVecFanIn = 4, kMpsFromVecMaxParts = 256, kMpsFromVecProjectChunks = 16 };
constexpr size_t kMpsFromVecBudget = (size_t)8 << 30;   // bytes of the two ping-pong work buffers of a chunk of lanes

inline bool mps_fromvec_method_ok(int method) { return method == kMpsFromVecByRule || method == kMpsFromVecFused || method == kMpsFromVecHost; }

// the bound of bond b = 0 .. n: min(2^b, 2^(n-b), max_bond if > 0), saturated at 2^30
inline int mps_fromvec_bound(int n, int b, int max_bond) {
    const int e = b < n - b ? b : n - b;
    const int natural = e >= 30 ? 1 << 30 : 1 << (e < 0 ? 0 : e);
    return max_bond > 0 && max_bond < natural ? max_bond : natural;
}
inline int mps_fromvec_route(int n, int max_bond) {
    if (n < kMpsFromVecMinQubits || n > kMpsFromVecMaxQubits) return kMpsFromVecHost;
    return mps_fromvec_bound(n, n / 2, max_bond) <= kMpsFromVecCap ? kMpsFromVecFused : kMpsFromVecHost;
}

// the partial R factors of a matrix of `rows` rows: blocks of kMpsFromVecBlockRows rows, at least kMpsFromVecFanIn blocks per part where
// there are that many, at most kMpsFromVecMaxParts parts, no part empty.  A function of the row count alone.
inline size_t mps_fromvec_blocks(size_t rows) { return (rows + kMpsFromVecBlockRows - 1) / kMpsFromVecBlockRows; }
inline size_t mps_fromvec_blocks_per_part(size_t rows) {
    const size_t blocks = mps_fromvec_blocks(rows);
    size_t p0 = (blocks + kMpsFromVecFanIn - 1) / kMpsFromVecFanIn;
    if (p0 > kMpsFromVecMaxParts) p0 = kMpsFromVecMaxParts;
    if (p0 < 1) p0 = 1;
    const size_t per = (blocks + p0 - 1) / p0;
    return per ? per : 1;
}
inline int mps_fromvec_parts(size_t rows) {
    const size_t blocks = mps_fromvec_blocks(rows), per = mps_fromvec_blocks_per_part(rows);
    return blocks ? (int)((blocks + per - 1) / per) : 1;
}
// the tree: `parts` factors are folded kMpsFromVecFanIn at a time into this many
inline int mps_fromvec_fold(int parts) { return (parts + kMpsFromVecFanIn - 1) / kMpsFromVecFanIn; }

// lanes per chunk: the two work buffers of 2^n complex numbers per lane stay within budget_bytes; 0: not even one lane fits
inline size_t mps_fromvec_lane_bytes(int n) { return (size_t)2 * 16 * ((size_t)1 << n); }
inline int mps_fromvec_chunk(int n, size_t lanes, size_t budget_bytes) {
    size_t g = budget_bytes / mps_fromvec_lane_bytes(n);
    if (g > lanes) g = lanes;
    if (g > 65535) g = 65535;
    return (int)g;
}

// the bounds of the n + 1 bonds: what the stores of a lane's site tensors and bond vectors are sized by
inline std::vector<int> mps_fromvec_bounds(int n, int max_bond) {
    std::vector<int> b(n + 1);
    for (int q = 0; q <= n; ++q) b[q] = mps_fromvec_bound(n, q, max_bond);
    return b;
}

// R of the row-major rows x cols matrix a by the block recursion of the fused route: parts, blocks, tree.  Returns cols x cols, row-major
inline std::vector<std::complex<double>> mps_fromvec_r(size_t rows, int cols, const std::complex<double>* a) {
    typedef std::complex<double> cd;
    const size_t c = (size_t)cols, per = mps_fromvec_blocks_per_part(rows), blocks = mps_fromvec_blocks(rows);
    auto fold = [&](const cd* src, size_t src_rows, size_t height, size_t first, size_t last) {   // blocks [first, last) of `height` rows
        std::vector<cd> st((c + height) * c), r(c * c, cd(0.0, 0.0));
        for (size_t b = first; b < last; ++b) {
            const size_t row0 = b * height, h = std::min(height, src_rows - row0), top = b == first ? 0 : c;   // the first block by itself
            std::fill(st.begin(), st.end(), cd(0.0, 0.0));
            std::copy(r.begin(), r.begin() + top * c, st.begin());
            std::copy(src + row0 * c, src + (row0 + h) * c, st.begin() + top * c);
            mps_ent_householder_r((int)(top + h), cols, st.data());
            std::fill(r.begin(), r.end(), cd(0.0, 0.0));
            std::copy(st.begin(), st.begin() + std::min(top + h, c) * c, r.begin());
        }
        return r;
    };
    int parts = mps_fromvec_parts(rows);
    std::vector<cd> fac((size_t)parts * c * c);
    for (int p = 0; p < parts; ++p) {
        const std::vector<cd> r = fold(a, rows, kMpsFromVecBlockRows, p * per, std::min(blocks, (p + 1) * per));
        std::copy(r.begin(), r.end(), fac.begin() + (size_t)p * c * c);
    }
    while (parts > 1) {
        const int next = mps_fromvec_fold(parts);
        std::vector<cd> out((size_t)next * c * c);
        for (int p = 0; p < next; ++p) {
            const std::vector<cd> r = fold(fac.data(), (size_t)parts * c, c, (size_t)p * kMpsFromVecFanIn, std::min<size_t>(parts, (size_t)(p + 1) * kMpsFromVecFanIn));
            std::copy(r.begin(), r.end(), out.begin() + (size_t)p * c * c);
        }
        fac.swap(out);
        parts = next;
    }
    return fac;
}

// The whole conversion on the host.  svd(rows, cols, a row-major, u [rows][count], s [count]) with count = min(rows, cols), s descending.
struct MpsFromVec {
    int status = kMpsCompressOk, failed_at = -1;
    double discarded = 0.0;
    std::vector<int> bonds;                               // n + 1
    std::vector<double> dropped;                          // n - 1
    std::vector<std::vector<double>> lam;                 // n - 1
    std::vector<std::vector<std::complex<double>>> site;  // n, [2][bonds[q]][bonds[q+1]]
};
typedef std::function<void(int rows, int cols, const std::complex<double>* a, std::complex<double>* u, double* s)> MpsFromVecSvd;
inline MpsFromVec mps_fromvec_convert(int n, const std::complex<double>* psi, double trunc_thr, int max_bond, const MpsFromVecSvd& svd) {
    typedef std::complex<double> cd;
    MpsFromVec out;
    out.bonds.assign(n + 1, 0);
    out.bonds[0] = 1;
    out.dropped.assign(n > 1 ? n - 1 : 0, 0.0);
    std::vector<cd> a(psi, psi + ((size_t)1 << n));
    int r = 1;
    for (int q = 0; q + 1 < n; ++q) {
        const size_t nr = (size_t)1 << (n - 1 - q);
        const int c = 2 * r, count = (size_t)c < nr ? c : (int)nr;
        const std::vector<cd> fac = mps_fromvec_r(nr, c, a.data());
        std::vector<cd> rt((size_t)c * count), u((size_t)c * count), m((size_t)c * nr);
        std::vector<double> s(count);
        for (int i = 0; i < c; ++i)
            for (int j = 0; j < count; ++j) rt[(size_t)i * count + j] = fac[(size_t)j * c + i];
        svd(c, count, rt.data(), u.data(), s.data());
        for (size_t row = 0; row < nr; ++row)
            for (int i = 0; i < c; ++i) m[(size_t)i * nr + row] = a[row * c + i];
        const MpsCompressStep st = mps_compress_step(c, (int)nr, m.data(), u.data(), count, s.data(), q > 0 ? out.lam[q - 1].data() : nullptr, trunc_thr, max_bond);
        if (!st.d.ok) { out.status = kMpsCompressNonFinite; out.failed_at = q; return out; }
        r = st.d.rank;
        out.bonds[q + 1] = r;
        out.dropped[q] = st.d.total - st.d.kept;
        out.discarded += out.dropped[q];
        out.lam.push_back(st.lam);
        out.site.push_back(st.site);
        a.assign(nr * r, cd(0.0, 0.0));
        for (size_t row = 0; row < nr; ++row)
            for (int j = 0; j < r; ++j) a[row * r + j] = st.carry[(size_t)j * nr + row];   // Y = carry^T, row stride r
    }
    std::vector<cd> last((size_t)2 * r);
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l < r; ++l) last[(size_t)s * r + l] = a[(size_t)s * r + l] * mps_compress_site_factor(1.0, n > 1 ? out.lam[n - 2][l] : 1.0);
    out.site.push_back(last);
    out.bonds[n] = 1;
    return out;
}

}  // namespace aqc
