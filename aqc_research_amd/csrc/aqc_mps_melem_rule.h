// The rules of matrix elements of operators between MPS states (aqc_mps_melem.hip, aqc_mps_melem_api.cpp), HIP-free: the same text is
// compiled into the library and by a plain C++ compiler (tests/native/mps_melem_rule_selftest.cpp); tests/mps_melem_ref.py states the
// result in NumPy.  Notation of aqc_mps_pauli_rule.h and aqc_mps_opsum_rule.h:
//   ket, bra    site tensors T_q, B_q [2][left][right], bonds chi_q, beta_q, any gauge, neither modified
//   operator    sites W_q [D_q][D_{q+1}][2][2], indexed [a][b][s_out][s_in], D_0 = D_n = 1, packed as aqc_mps_opsum_rule.h says; a job
//               without an operator (index -1) has the identity: D = 1 everywhere, W_q[0][0] = the 2 x 2 unit matrix
//   walk        E_0 = [1] (1 x 1 x 1);  E_{q+1}[b][u][v] = sum_a sum_{s,s'} W_q[a][b][s][s'] sum_xy conj(B_q[s][x][u]) E_q[a][x][y] T_q[s'][y][v]
//               (E_q: D_q matrices of beta_q x chi_q)
//   result      <phi|O|psi> = E_n[0][0][0], no normalisation; n = 1: sum_{s,s'} conj(B_0[s]) W_0[0][0][s][s'] T_0[s']
//   step        F_{a,s'} = E_q[a] T_q[s'];   G_{b,s} = sum_{a,s'} W_q[a][b][s][s'] F_{a,s'};   E_{q+1}[b] = sum_s B_q[s]^H G_{b,s}
//   skipping    an entry of W_q that is exactly zero (both parts +-0; a NaN is no zero) is SKIPPED, here, in the NumPy statement and on
//               both routes alike: mps_melem_entries lists the entries that are left, in the order a, s', b, s (the last the fastest).
//               An F_{a,s'} that no listed entry reads is not formed, and neither is a G_{b,s} that no listed entry writes; G_{b,s} is
//               the sum of its entries in the order of the list, the first one stored and the others added; E_{q+1}[b] is
//               B_q[0]^H G_{b,0} + B_q[1]^H G_{b,1} in that order over the G_{b,s} that exist, and an exact zero matrix when neither
//               does.  So a zero of W never meets a number of the states: 0 x NaN does not arise from a skipped entry
//   errors      are relative to scale = |phi| |O|_2 |psi|
//   route       per job: fused (one workgroup walks the whole chain inside one launch) when every bond of bra and ket is
//               <= kMpsMelemFusedCap and every operator bond is <= kMpsMelemOpCap, else gemm (batched zgemm launches per site)
//   scratch     a job keeps two sets of E matrices (the site's and the next one's) and the G matrices of the site: mps_melem_job_elems;
//               jobs run in groups whose scratch stays below a budget: mps_melem_group_size
// Every sum runs in a fixed order that depends on the bond dimensions of the two states and on the operator only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <complex>
#include <vector>

namespace aqc {

enum { kMpsMelemByRule = 0, kMpsMelemFused = 1, kMpsMelemGemm = 2, kMpsMelemFusedCap = 64, kMpsMelemOpCap = 32 };
enum { kMpsMelemGroupMax = 16384 };                         // jobs of one group (a grid dimension; the tables of a gemm group)
constexpr size_t kMpsMelemBudget = (size_t)512 << 20;       // bytes of scratch of one group: 256 XXZ jobs at bond 64 take 320 MiB

inline bool mps_melem_method_ok(int method) { return method == kMpsMelemByRule || method == kMpsMelemFused || method == kMpsMelemGemm; }

// dims: n + 1 bond dimensions; bra_dims null: the ket's; op_dims null: the identity
inline int mps_melem_max_bond(int n, const int* bra_dims, const int* ket_dims) {
    int m = 1;
    for (int q = 0; q <= n; ++q) {
        m = ket_dims[q] > m ? ket_dims[q] : m;
        if (bra_dims) m = bra_dims[q] > m ? bra_dims[q] : m;
    }
    return m;
}
inline int mps_melem_max_op_bond(int n, const int* op_dims) {
    int m = 1;
    for (int q = 0; op_dims && q <= n; ++q) m = op_dims[q] > m ? op_dims[q] : m;
    return m;
}
inline int mps_melem_route(int n, const int* bra_dims, const int* ket_dims, const int* op_dims) {
    return mps_melem_max_bond(n, bra_dims, ket_dims) <= kMpsMelemFusedCap && mps_melem_max_op_bond(n, op_dims) <= kMpsMelemOpCap ? kMpsMelemFused
                                                                                                                                   : kMpsMelemGemm;
}

// ---- the entries of one operator site that are not skipped, in the order a, s', b, s; first: the entry is the first of its G_{b,s}
struct MpsMelemEntry {
    int a, sp, b, s, first, pad;
    double wr, wi;
};
// W: [dl][dr][2][2] complex as (re, im) pairs; null: the identity site (dl = dr = 1).  entries is appended to; mask (resized to dr) gets
// bit s of entry b set when G_{b,s} exists
inline void mps_melem_entries(int dl, int dr, const double* W, std::vector<MpsMelemEntry>& entries, std::vector<int>& mask) {
    static const double unit[8] = {1, 0, 0, 0, 0, 0, 1, 0};
    if (!W) { W = unit; dl = dr = 1; }
    mask.assign((size_t)dr, 0);
    for (int a = 0; a < dl; ++a)
        for (int sp = 0; sp < 2; ++sp)
            for (int b = 0; b < dr; ++b)
                for (int s = 0; s < 2; ++s) {
                    const double* w = W + 2 * ((((size_t)a * dr + b) * 2 + s) * 2 + sp);
                    if (w[0] == 0.0 && w[1] == 0.0) continue;   // +-0 both: skipped.  A NaN compares unequal and stays
                    const int first = !(mask[b] >> s & 1);
                    mask[b] |= 1 << s;
                    entries.push_back(MpsMelemEntry{a, sp, b, s, first, 0, w[0], w[1]});
                }
}

// ---- scratch, in complex numbers, saturating at SIZE_MAX (three ints multiplied cannot wrap 64 bits, the sums are guarded)
inline size_t mps_melem_sat_add(size_t x, size_t y) { return x > ~(size_t)0 - y ? ~(size_t)0 : x + y; }
inline size_t mps_melem_sat_mul(size_t x, size_t y) { return y && x > ~(size_t)0 / y ? ~(size_t)0 : x * y; }
// the largest set of E matrices along the chain: max_q D_q beta_q chi_q
inline size_t mps_melem_e_elems(int n, const int* bra_dims, const int* ket_dims, const int* op_dims) {
    size_t m = 1;
    for (int q = 0; q <= n; ++q) {
        const size_t e = mps_melem_sat_mul(mps_melem_sat_mul((size_t)(op_dims ? op_dims[q] : 1), (size_t)(bra_dims ? bra_dims[q] : ket_dims[q])), (size_t)ket_dims[q]);
        m = e > m ? e : m;
    }
    return m;
}
// the largest set of G matrices: max_q 2 D_{q+1} beta_q chi_{q+1}
inline size_t mps_melem_g_elems(int n, const int* bra_dims, const int* ket_dims, const int* op_dims) {
    size_t m = 1;
    for (int q = 0; q < n; ++q) {
        const size_t e = mps_melem_sat_mul(mps_melem_sat_mul(2 * (size_t)(op_dims ? op_dims[q + 1] : 1), (size_t)(bra_dims ? bra_dims[q] : ket_dims[q])), (size_t)ket_dims[q + 1]);
        m = e > m ? e : m;
    }
    return m;
}
// the largest set of F matrices (gemm route only; the fused route keeps an F in its accumulators): max_q 2 D_q beta_q chi_{q+1}
inline size_t mps_melem_f_elems(int n, const int* bra_dims, const int* ket_dims, const int* op_dims) {
    size_t m = 1;
    for (int q = 0; q < n; ++q) {
        const size_t e = mps_melem_sat_mul(mps_melem_sat_mul(2 * (size_t)(op_dims ? op_dims[q] : 1), (size_t)(bra_dims ? bra_dims[q] : ket_dims[q])), (size_t)ket_dims[q + 1]);
        m = e > m ? e : m;
    }
    return m;
}
inline size_t mps_melem_job_elems(int n, const int* bra_dims, const int* ket_dims, const int* op_dims, bool gemm) {
    const size_t e = mps_melem_e_elems(n, bra_dims, ket_dims, op_dims);
    size_t total = mps_melem_sat_add(mps_melem_sat_add(e, e), mps_melem_g_elems(n, bra_dims, ket_dims, op_dims));
    if (gemm) total = mps_melem_sat_add(total, mps_melem_f_elems(n, bra_dims, ket_dims, op_dims));
    return total;
}
// jobs walked together so that their scratch stays below budget_bytes; at least one, at most kMpsMelemGroupMax
inline int mps_melem_group_size(size_t job_elems, size_t njobs, size_t budget_bytes) {
    const size_t per = mps_melem_sat_mul(16, job_elems);
    size_t g = per ? budget_bytes / per : njobs;
    if (g > njobs) g = njobs;
    if (g > (size_t)kMpsMelemGroupMax) g = (size_t)kMpsMelemGroupMax;
    return (int)(g < 1 ? 1 : g);
}

// ---- the host statement of one job, in the order of the step above with plain loops (products written out: no library rule for
// non-finite complex products takes part).  bra, ket: n site tensors [2][l][r]; op: n operator sites or null (the identity)
inline std::complex<double> mps_melem_value(int n, const int* bra_dims, const int* ket_dims, const int* op_dims, const std::complex<double>* const* bra,
                                            const std::complex<double>* const* ket, const std::complex<double>* const* op) {
    typedef std::complex<double> cd;
    auto mul = [](cd x, cd y) { return cd(x.real() * y.real() - x.imag() * y.imag(), x.real() * y.imag() + x.imag() * y.real()); };
    std::vector<std::vector<cd>> e(1, std::vector<cd>(1, cd(1.0, 0.0)));
    for (int q = 0; q < n; ++q) {
        const int dl = op ? op_dims[q] : 1, dr = op ? op_dims[q + 1] : 1, bl = bra_dims[q], br = bra_dims[q + 1], kl = ket_dims[q], kr = ket_dims[q + 1];
        std::vector<MpsMelemEntry> ent;
        std::vector<int> mask;
        mps_melem_entries(dl, dr, op ? reinterpret_cast<const double*>(op[q]) : nullptr, ent, mask);
        std::vector<std::vector<cd>> g((size_t)2 * dr);
        std::vector<cd> f;
        int fa = -1, fs = -1;
        for (const MpsMelemEntry& t : ent) {
            if (t.a != fa || t.sp != fs) {   // F_{a,s'} = E[a] T[s']
                fa = t.a; fs = t.sp;
                f.assign((size_t)bl * kr, cd(0.0, 0.0));
                for (int x = 0; x < bl; ++x)
                    for (int y = 0; y < kl; ++y)
                        for (int v = 0; v < kr; ++v) f[(size_t)x * kr + v] += mul(e[fa][(size_t)x * kl + y], ket[q][((size_t)fs * kl + y) * kr + v]);
            }
            std::vector<cd>& dst = g[2 * t.b + t.s];
            if (t.first) dst.assign(f.size(), cd(0.0, 0.0));
            for (size_t i = 0; i < f.size(); ++i) {
                const cd p = mul(cd(t.wr, t.wi), f[i]);
                dst[i] = t.first ? p : dst[i] + p;
            }
        }
        std::vector<std::vector<cd>> next((size_t)dr, std::vector<cd>((size_t)br * kr, cd(0.0, 0.0)));
        for (int b = 0; b < dr; ++b) {
            bool have = false;
            for (int s = 0; s < 2; ++s) {
                if (!(mask[b] >> s & 1)) continue;
                std::vector<cd> part((size_t)br * kr, cd(0.0, 0.0));
                for (int x = 0; x < bl; ++x)
                    for (int u = 0; u < br; ++u)
                        for (int v = 0; v < kr; ++v) part[(size_t)u * kr + v] += mul(std::conj(bra[q][((size_t)s * bl + x) * br + u]), g[2 * b + s][(size_t)x * kr + v]);
                for (size_t i = 0; i < part.size(); ++i) next[b][i] = have ? next[b][i] + part[i] : part[i];
                have = true;
            }
        }
        e.swap(next);
    }
    return e[0][0];
}

}  // namespace aqc
