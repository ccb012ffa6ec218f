// The rules of operator sums on MPS states (aqc_mps_opsum.hip, aqc_mps_opsum_api.cpp), HIP-free: the same text is compiled into the
// library and by a plain C++ compiler (tests/native/mps_opsum_rule_selftest.cpp); tests/mps_opsum_ref.py states the result in NumPy.
// Notation of aqc_mps_combine_rule.h: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], site tensors [2][chi_q][chi_{q+1}], any gauge, qubit q is
// index bit q of the dense vector.  Output j = sum_t c_t O_t psi_t over its terms, O_t an operator (MPO) or absent (the identity):
//   operator  sites W_q [D_q][D_{q+1}][2][2], complex, indexed [a][b][s_out][s_in], D_0 = D_n = 1:
//             O(b_out, b_in) = W_0[., ., b_out0, b_in0] ... W_{n-1}[...] as a product of D x D matrices; no gauge, no Hermiticity
//   product   the sites P_q of O psi have bonds Pi_q = D_q chi_q; P_q[s][(a, i), (b, j)] = sum_{s'} W_q[a][b][s][s'] T_q[s'][i][j], summed
//             s' = 0 then s' = 1; the operator index is the major one: row a chi_q + i, column b chi_{q+1} + j.  A term without an
//             operator is the state's own site (Pi_q = chi_q): a copy, no arithmetic
//   sum       the direct sum of the terms as aqc_mps_combine_rule.h states it, the widths Pi^t_q in place of chi^k_q: mps_combine_dims,
//             _block_offsets, _site_offsets, _max_bond, _owner and _source on the [nterms][n + 1] array of product bonds.  c_t
//             multiplies site 0.  n = 1: the 2-vector sum_t c_t W^t_0[0][0] T^t_0, summed in the order of the terms
//   result    compress(S, trunc_thr, max_bond) of aqc_mps_compress_rule.h, as for linear combinations; the discarded weight is what the
//             cuts of this call dropped.  A result that is exactly zero or not finite has status 2 and fails its output alone
//   errors    are relative to scale = sum_t |c_t| |O_t|_2 |psi_t| (|identity|_2 = 1), not to the norm of the result
//   route     fused when every summed product bond <= kMpsEntFusedCap, else canonical, as for linear combinations
//   table     term_off, term_state as there; term_op[t] in [-1, nops), -1: no operator
//   packing   the operators of a call lie in one array of complex elements: operator o has dims D^o_0 .. D^o_n and its site q lies at
//             element site_off[o][q], 4 D_q D_{q+1} elements long; entry n is the operator's end
#pragma once
#include "aqc_mps_combine_rule.h"

namespace aqc {

// Pi_0 .. Pi_n of one term in 64 bits (a product of two ints cannot wrap there); op_dims null: no operator.  False when a product bond
// does not fit an int: such a term cannot be a row of the int arrays the sum is stated on
inline bool mps_opsum_term_dims(int n, const int* state_dims, const int* op_dims, long long* wide, int* out) {
    bool fits = true;
    for (int q = 0; q <= n; ++q) {
        const long long p = (long long)state_dims[q] * (op_dims ? op_dims[q] : 1);
        if (wide) wide[q] = p;
        if (p > 2147483647ll) fits = false;
        if (out) out[q] = fits ? (int)p : 0;
    }
    return fits;
}
// largest summed product bond of an output, 64-bit before any comparison; state_dims, op_dims: [nterms][n + 1] (op_dims null: no
// operators; a row of ones is the identity)
inline long long mps_opsum_max_bond(int n, int nterms, const int* state_dims, const int* op_dims) {
    long long m = 1;
    for (int q = 1; q < n; ++q) {
        long long s = 0;
        for (int k = 0; k < nterms; ++k) {
            const size_t at = (size_t)k * (n + 1) + q;
            const long long p = (long long)state_dims[at] * (op_dims ? op_dims[at] : 1);
            s = p > 9223372036854775807ll - s ? 9223372036854775807ll : s + p;   // (saturates: 2^31 terms of 2^62 would wrap)
        }
        m = s > m ? s : m;
    }
    return m;
}
inline int mps_opsum_route(int n, int nterms, const int* state_dims, const int* op_dims) {
    return mps_opsum_max_bond(n, nterms, state_dims, op_dims) <= kMpsEntFusedCap ? kMpsEntFused : kMpsEntCanonical;
}
// a term table: 0 fine, 1 .. 3 as mps_combine_check_terms, 4 an operator index outside [-1, nops)
inline int mps_opsum_check_terms(int nstates, int nops, int nout, const int* term_off, const int* term_state, const int* term_op) {
    const int bad = mps_combine_check_terms(nstates, nout, term_off, term_state);
    if (bad) return bad;
    for (int t = 0; t < term_off[nout]; ++t)
        if (term_op[t] < -1 || term_op[t] >= nops) return 4;
    return 0;
}
// the packed layout of one operator: element offsets of its sites from `start` on (n + 1 entries, the last its end)
inline std::vector<long long> mps_opsum_op_offsets(int n, const int* op_dims, long long start) {
    std::vector<long long> off(n + 1, start);
    for (int q = 0; q < n; ++q) off[q + 1] = off[q] + (long long)4 * op_dims[q] * op_dims[q + 1];
    return off;
}
// an operator's dims and offsets: 0 fine, 1 an edge bond that is not 1 or a bond below 1, 2 offsets that are negative or not the packed
// layout of these dims
inline int mps_opsum_check_op(int n, const int* op_dims, const long long* site_off) {
    if (op_dims[0] != 1 || op_dims[n] != 1) return 1;
    for (int q = 0; q <= n; ++q)
        if (op_dims[q] < 1) return 1;
    if (site_off[0] < 0) return 2;
    for (int q = 0; q < n; ++q)
        if (site_off[q + 1] - site_off[q] != (long long)4 * op_dims[q] * op_dims[q + 1]) return 2;
    return 0;
}

#if defined(__HIPCC__)
#define AQC_OPS_HD __host__ __device__
#else
#define AQC_OPS_HD
#endif
// Element e of assembled site q, packed [2][Sigma_q][Sigma_{q+1}] (n >= 2).  off: mps_combine_block_offsets of the product bonds;
// chi: [nterms][n + 1] the bonds of every term's state; has_op[t] >= 0: the term has an operator.  kind 0: a zero.  kind 1: a copy of
// element x0 of the state's site.  kind 2: W_q[a][b][s][0] x0 + W_q[a][b][s][1] x1 with x0, x1 elements of the state's site.  Either
// times the term's coefficient when q = 0
enum { kMpsOpsumZero = 0, kMpsOpsumCopy = 1, kMpsOpsumProduct = 2 };
struct MpsOpsumSource { int term, kind, a, b, s; size_t x0, x1; };
AQC_OPS_HD inline MpsOpsumSource mps_opsum_source(int n, int nterms, const int* off, const int* chi, const int* has_op, int q, size_t e) {
    const MpsCombineSource src = mps_combine_source(n, nterms, off, q, e);
    if (src.term < 0) return {-1, kMpsOpsumZero, 0, 0, 0, 0, 0};
    if (has_op[src.term] < 0) return {src.term, kMpsOpsumCopy, 0, 0, 0, src.elem, 0};
    // src.elem indexes the term's block [2][Pi_q][Pi_{q+1}]; its widths are the block offsets' differences
    const int* mine = off + (size_t)src.term * (n + 1);
    const int pl = q > 0 ? mine[n + 1 + q] - mine[q] : 1, pr = q + 1 < n ? mine[n + 1 + q + 1] - mine[q + 1] : 1;
    const int* c = chi + (size_t)src.term * (n + 1);
    const int chi_l = c[q] > 0 ? c[q] : 1, chi_r = c[q + 1] > 0 ? c[q + 1] : 1;
    const int s = (int)(src.elem / ((size_t)pl * pr));
    const size_t in = src.elem - (size_t)s * pl * pr;
    const int row = (int)(in / pr), col = (int)(in - (size_t)row * pr);
    const int a = row / chi_l, i = row - a * chi_l, b = col / chi_r, j = col - b * chi_r;
    const size_t x0 = (size_t)i * chi_r + j;
    return {src.term, kMpsOpsumProduct, a, b, s, x0, x0 + (size_t)chi_l * chi_r};
}
#undef AQC_OPS_HD

// The host statement of one assembled site.  sites[t] is T^t_q ([2][chi^t_q][chi^t_{q+1}]), ops[t] is W^t_q ([D_q][D_{q+1}][2][2]) or
// null, state_dims and op_dims [nterms][n + 1] (the op_dims row of a term without operator is not read), coeffs [nterms]; out is
// resized to 2 Sigma_q Sigma_{q+1} and every element set
inline void mps_opsum_site(int n, int nterms, const int* state_dims, const int* op_dims, int q, const std::complex<double>* const* sites,
                           const std::complex<double>* const* ops, const std::complex<double>* coeffs, std::vector<std::complex<double>>& out) {
    typedef std::complex<double> cd;
    if (n == 1) {
        out.assign(2, cd(0.0, 0.0));
        for (int s = 0; s < 2; ++s)
            for (int t = 0; t < nterms; ++t) {
                const cd x = ops[t] ? ops[t][2 * s] * sites[t][0] + ops[t][2 * s + 1] * sites[t][1] : sites[t][s];
                out[s] += coeffs[t] * x;
            }
        return;
    }
    std::vector<int> widths((size_t)nterms * (n + 1)), has_op(nterms);
    for (int t = 0; t < nterms; ++t) {
        has_op[t] = ops[t] ? 0 : -1;
        mps_opsum_term_dims(n, state_dims + (size_t)t * (n + 1), ops[t] ? op_dims + (size_t)t * (n + 1) : nullptr, nullptr, widths.data() + (size_t)t * (n + 1));
    }
    const std::vector<int> off = mps_combine_block_offsets(n, nterms, widths.data());
    const int* end = off.data() + (size_t)nterms * (n + 1);
    out.resize((size_t)2 * end[q] * end[q + 1]);
    for (size_t e = 0; e < out.size(); ++e) {
        const MpsOpsumSource src = mps_opsum_source(n, nterms, off.data(), state_dims, has_op.data(), q, e);
        cd v(0.0, 0.0);
        if (src.kind == kMpsOpsumCopy) {
            v = sites[src.term][src.x0];
        } else if (src.kind == kMpsOpsumProduct) {
            const int d_r = op_dims[(size_t)src.term * (n + 1) + q + 1];
            const cd* w = ops[src.term] + ((size_t)src.a * d_r + src.b) * 4 + 2 * src.s;
            v = w[0] * sites[src.term][src.x0] + w[1] * sites[src.term][src.x1];
        }
        out[e] = src.kind != kMpsOpsumZero && q == 0 ? coeffs[src.term] * v : v;
    }
}

}  // namespace aqc
