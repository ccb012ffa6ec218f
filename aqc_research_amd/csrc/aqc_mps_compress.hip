// MPS compression, fused route (rules and notation: aqc_mps_compress_rule.h; host side: aqc_mps_compress_api.cpp).
//
// After the right walk of mps_ent_chain_kernel (aqc_mps_ent.hip) has left D_1 .. D_{n-1} of every state, the sweep is, per bond q:
//   mps_compress_form_kernel   the carry W_q (r_q x chi_q) into the E planes of aqc_mps_planes.h; M_s = W_q T_q[s] (MFMA, the site streamed
//                              from memory) into the F planes (s = 0) and over the E planes (s = 1) and, packed, into memory for the split;
//                              B_s = M_s D_{q+1}^T with the factor streamed transposed, written as rows s r_q .. of the state's matrix of the
//                              SVD batch, rows[i] = 2 r_q, cols[i] = chi_{q+1}: r_q is read from the ranks the split before has written;
//   launch_svd_batch           (aqc_svd_batch.hip) over the states of the chunk;
//   mps_compress_split_kernel  the cut by the steps of aqc_mps_cut.h (thread 0 takes mps_compress_decide, the host's text; the bond vector;
//                              the new site, packed at the ranks just decided); rank, dropped weight and sweeps; the new carry
//                              W_{q+1} = rescale (U_0^H M_0 + U_1^H M_1) on the matrix cores, M back in the planes, U streamed.
// The form kernel of q = n - 1 writes the last site instead of B.  One workgroup per state in every launch; a state whose SVD gave a
// status, or whose spectrum is zero or not finite, gets its status written by its own workgroup and is skipped from then on (rows = 0:
// the SVD kernel leaves at once).  No atomics, every sum in a fixed order, no loop bound depends on data other than bond dimensions
// and ranks, nothing is read from or written to another state's stores.  planes_zero, plane_load, acc_to_mem and the grant of the
// planes' dynamic LDS: aqc_mps_planes.h.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_compress_rule.h"
#include "aqc_mps_cut.h"
#include "aqc_mps_planes.h"

namespace aqc {

static_assert((int)kMpsEntFusedCap == (int)kMpsObsFusedCap, "the planes of aqc_mps_planes.h are sized by the observables' cap");

// grid (states of the chunk); 256 threads; dynamic LDS kFusedLds
__global__ __launch_bounds__(256) void mps_compress_form_kernel(MpsCompressArgs a) {
    extern __shared__ __attribute__((aligned(16))) double cmp_smem[];
    double* er = cmp_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const int item = blockIdx.x, tid = threadIdx.x, q = a.q;
    const MpsCompressState st = a.states[a.first + item];
    const bool last = q == a.n - 1;
    if (st.status[0] != kMpsCompressOk) {   // (written by this state's split kernel of an earlier step)
        if (!last && tid == 0) { a.rows[item] = 0; a.cols[item] = 0; }
        return;
    }
    const int chi_q = st.in.dims[q], chi = st.in.dims[q + 1], r = q > 0 ? st.ranks[q - 1] : 1;   // r <= chi_q <= kCap
    cplx* carry = a.carry + (size_t)item * kCap * kCap;
    cplx* m = a.m + (size_t)item * 2 * kCap * kCap;
    planes_zero(cmp_smem);
    __syncthreads();
    if (q > 0) plane_load(carry, r, chi_q, er, ei);
    else if (tid == 0) er[0] = 1.0;
    __syncthreads();
    const cplx* T0 = st.in.sites[q];
    const cplx* T1 = T0 + (size_t)chi_q * chi;
    Acc p0, p1;
    prod_lds_mem<false>(er, ei, T0, r, chi_q, chi, p0);
    prod_lds_mem<false>(er, ei, T1, r, chi_q, chi, p1);
    if (last) {   // chi = 1: T'_{n-1}[s][l] = M_s[l][0] / lambda'_{n-2}[l]
        cplx* out = st.out_sites + st.site_off[q];
        const double* lam_left = q > 0 ? st.out_lam + st.lam_off[q - 1] : nullptr;
        const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
        if (li == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int l = 16 * wave + 4 * rr + lk;
                if (l < r) {
                    const double f = mps_compress_site_factor(1.0, lam_left ? lam_left[l] : 1.0);
                    out[l] = make_double2(f * p0.re[0][rr], f * p0.im[0][rr]);
                    out[r + l] = make_double2(f * p1.re[0][rr], f * p1.im[0][rr]);
                }
            }
        }
        return;
    }
    acc_to_mem(p0, m, chi, r, chi);
    acc_to_mem(p1, m + (size_t)r * chi, chi, r, chi);
    __syncthreads();   // every wave is done reading the carry
    acc_store(p0, fr, fi, r, chi);
    acc_store(p1, er, ei, r, chi);
    __syncthreads();
    const cplx* D = st.in.factors + st.in.fac_off[a.n] + st.in.fac_off[q + 1];   // chi x chi
    prod_lds_mem<true>(fr, fi, D, r, chi, chi, p0);   // B_s[i][j] = sum_k M_s[i][k] D[j][k]
    prod_lds_mem<true>(er, ei, D, r, chi, chi, p1);
    cplx* B = a.a + (size_t)item * 2 * a.k * a.k;     // 2 r <= 2 k rows, chi <= k columns
    acc_to_mem(p0, B, a.k, r, chi);
    acc_to_mem(p1, B + (size_t)r * a.k, a.k, r, chi);
    if (tid == 0) { a.rows[item] = 2 * r; a.cols[item] = chi; }
}

// grid (states of the chunk); 256 threads; dynamic LDS kFusedLds.  q = 0 .. n - 2
__global__ __launch_bounds__(256) void mps_compress_split_kernel(MpsCompressArgs a) {
    extern __shared__ __attribute__((aligned(16))) double cmp_smem[];
    __shared__ double lam[kCap];
    __shared__ MpsCompressDecision dec;
    double* er = cmp_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const int item = blockIdx.x, tid = threadIdx.x, q = a.q;
    const MpsCompressState st = a.states[a.first + item];
    if (st.status[0] != kMpsCompressOk) return;
    const int svd_status = a.svd_status[item];
    const int chi = st.in.dims[q + 1], r = q > 0 ? st.ranks[q - 1] : 1;
    const int count = 2 * r < chi ? 2 * r : chi;   // <= kCap
    const double* s = a.s + (size_t)item * a.k;
    const MpsCompressDecision d = cut_decide(svd_status, count, s, a.trunc_thr, a.max_bond, &dec);
    if (!d.ok) {
        if (tid == 0) st.status[0] = cut_failure(svd_status);
        return;
    }
    const int rk = d.rank;   // 1 .. count
    cut_bond(d, s, lam, st.out_lam + st.lam_off[q]);
    if (tid == 0) { st.ranks[q] = rk; st.dropped[q] = d.total - d.kept; st.sweeps[q] = a.svd_sweeps[item]; }
    planes_zero(cmp_smem);
    __syncthreads();
    const cplx* u = a.u + (size_t)item * 2 * a.k * a.k;   // [2 r][k], the leading `count` columns
    const cplx* m = a.m + (size_t)item * 2 * kCap * kCap;
    plane_load(m, r, chi, fr, fi);
    plane_load(m + (size_t)r * chi, r, chi, er, ei);
    cut_left_site(u, a.k, r, rk, lam, q > 0 ? st.out_lam + st.lam_off[q - 1] : nullptr, st.out_sites + st.site_off[q]);
    __syncthreads();
    // W_{q+1} = rescale (U_0^H M_0 + U_1^H M_1): U_s is [r][k] in memory, every one of its k columns is taken (zero beyond count)
    Acc w0, w1;
    prod_memh_lds<false>(u, fr, fi, a.k, r, chi, w0);
    prod_memh_lds<false>(u + (size_t)r * a.k, er, ei, a.k, r, chi, w1);
#pragma unroll
    for (int t = 0; t < 4; ++t) { w0.re[t] += w1.re[t]; w0.im[t] += w1.im[t]; }
    acc_to_mem(w0, a.carry + (size_t)item * kCap * kCap, chi, rk, chi, d.rescale);
}

namespace {
constexpr auto grant_planes = grant_dynamic_lds<kFusedLds, mps_compress_form_kernel, mps_compress_split_kernel>;
}  // namespace

hipError_t launch_mps_compress_form(const MpsCompressArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_planes();
    if (e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    mps_compress_form_kernel<<<count, 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_compress_split(const MpsCompressArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_planes();
    if (e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    mps_compress_split_kernel<<<count, 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

}  // namespace aqc
