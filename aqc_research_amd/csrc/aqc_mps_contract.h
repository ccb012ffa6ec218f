// The transfer-matrix site step of the single-lane MPS side, stated ONCE: how the pair of states (A, B) is contracted through site p,
// from the left and from the right, and the chain of left steps that gives <a|b>.  For the bit values 0 and 1 of the site
//   left  step:  T = E . B_p[bit]        (xa x vb)    E'  (+)= A_p[bit]^H . T    (ua x vb)
//   right step:  T = Rc . B_p[bit]^H     (ua x yb)    Rc' (+)= A_p[bit] . T      (xa x yb)
// with site tensors stored [2][chi_l][chi_r] row-major, E[x][y] the contraction of the sites < p and Rc the CONJUGATE of that of the
// sites > p (launch_mps_env_dot closes the two: sum_i E[i] conj(Rc[i])).  Which leading dimension, which accumulate flag and how much
// scratch a step takes live here and nowhere else.  Executed by the gradient walk's environments (aqc_mps_engine.cpp), the observables'
// environments (aqc_mps_obs_api.cpp), aqc_mps_dot_ops and aqc_ws_mps_dot (aqc_ws_extra.cpp), and on the host by
// tests/native/mps_contract_selftest.cpp against dense vectors.  The small-bond one-launch form of a step is a choice of the device
// side (env_left / env_right of aqc_mps_host.h); the overlap chain stays on the products for every site.
// HIP-free like aqc_mps_walk.h; private to csrc/, internal linkage.
//
// An executor `ops` provides the products on elements Z (each returns 0, or non-zero after reporting the failure itself):
//   ops.gemm   (conj_t, accum, M, N, K, A, lda, B, ldb, C, ldc)   C (+)= op(A) . B     as launch_zgemm    (op(A) = A^H: A stored K x M)
//   ops.gemm_bh(conj_t, accum, M, N, K, A, lda, B, ldb, C, ldc)   C (+)= op(A) . B^H   as launch_zgemm_bh (B stored N x K)
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>

namespace {

// bond dimensions of site p of the pair: A_p is [2][xa][ua], B_p is [2][yb][vb]
struct SiteDims { int xa, ua, yb, vb; };
[[maybe_unused]] SiteDims site_dims(const int* dims_a, const int* dims_b, int p) { return {dims_a[p], dims_a[p + 1], dims_b[p], dims_b[p + 1]}; }

// out[u][v] = sum_bit sum_xy conj(A_p[bit][x][u]) in[x][y] B_p[bit][y][v];  tmp: xa * vb elements
template <class Ops, class Z>
int contract_left(Ops& ops, const Z* in, const Z* a_p, const Z* b_p, const SiteDims& d, Z* tmp, Z* out) {
    for (int bit = 0; bit < 2; ++bit) {
        if (ops.gemm(false, false, d.xa, d.vb, d.yb, in, d.yb, b_p + (size_t)bit * d.yb * d.vb, d.vb, tmp, d.vb)) return 1;
        if (ops.gemm(true, bit == 1, d.ua, d.vb, d.xa, a_p + (size_t)bit * d.xa * d.ua, d.ua, tmp, d.vb, out, d.vb)) return 1;
    }
    return 0;
}

// out[x][y] = sum_bit sum_uv A_p[bit][x][u] rc[u][v] conj(B_p[bit][y][v]);  tmp: ua * yb elements
template <class Ops, class Z>
int contract_right(Ops& ops, const Z* rc, const Z* a_p, const Z* b_p, const SiteDims& d, Z* tmp, Z* out) {
    for (int bit = 0; bit < 2; ++bit) {
        if (ops.gemm_bh(false, false, d.ua, d.yb, d.vb, rc, d.vb, b_p + (size_t)bit * d.yb * d.vb, d.vb, tmp, d.yb)) return 1;
        if (ops.gemm(false, bit == 1, d.xa, d.yb, d.ua, a_p + (size_t)bit * d.xa * d.ua, d.ua, tmp, d.yb, out, d.yb)) return 1;
    }
    return 0;
}

// the first site of <a|b>: out[u][v] = sum_bit conj(A_0[bit][0][u]) B_0[bit][0][v], the two bits as ONE product with K = 2
template <class Ops, class Z>
int overlap_first(Ops& ops, const Z* a_0, const Z* b_0, int ua, int vb, Z* out) {
    return ops.gemm(true, false, ua, vb, 2, a_0, ua, b_0, vb, out, vb);
}

// elements each of the three buffers (e, en, t) of an overlap chain takes
[[maybe_unused]] size_t overlap_scratch_elems(int n, const int* dims_a, const int* dims_b) {
    size_t need = 1;
    for (int q = 0; q <= n; ++q) need = std::max(need, (size_t)dims_a[q] * dims_b[q]);
    for (int q = 0; q < n; ++q) need = std::max(need, (size_t)dims_a[q] * dims_b[q + 1]);
    return need;
}

// <a|b>: the first site, then left steps up to site n - 1.  site_a(q) / site_b(q) give the site tensors (site_b may hand in the site seen
// through an operator; null after a reported failure).  Returns the buffer (e or en) that holds the 1 x 1 result, null after a failure.
template <class Ops, class Z, class SiteA, class SiteB>
const Z* overlap_chain(Ops& ops, int n, const int* dims_a, const int* dims_b, SiteA site_a, SiteB site_b, Z* e, Z* en, Z* t) {
    const Z* b_q = site_b(0);
    if (!b_q || overlap_first(ops, (const Z*)site_a(0), b_q, dims_a[1], dims_b[1], e)) return nullptr;
    for (int q = 1; q < n; ++q) {
        b_q = site_b(q);
        if (!b_q || contract_left(ops, (const Z*)e, (const Z*)site_a(q), b_q, site_dims(dims_a, dims_b, q), t, en)) return nullptr;
        std::swap(e, en);
    }
    return e;
}

}  // namespace
