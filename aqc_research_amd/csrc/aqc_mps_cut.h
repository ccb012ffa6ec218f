// The truncating cut of a sweep on the device, after launch_svd_batch has left U, Sigma and a status for the workgroup's matrix: what the
// split kernels of aqc_mps_compress.hip, aqc_mps_layers.hip and aqc_mps_fromvec.hip have in common.  The rule itself (rank, weights,
// rescaling, the factor and the index of a site element) is the host-and-device text of aqc_mps_compress_rule.h; here are its four
// steps as a workgroup of 256 threads takes them.  What differs between the kernels stays in them: where U, Sigma and the outputs
// live, their own guards (a rank beyond a static bound), and their bookkeeping (ranks or dims, dropped, sweeps, status, failed_at).
// Device code, internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include "aqc_mps_compress_rule.h"

namespace aqc {
namespace {

// The decision of the cut on s[0 .. count): thread 0 takes it (ok = 0 without looking at s when the SVD gave a status) and stores it
// in *slot, the caller's __shared__ MpsCompressDecision; every thread returns it.  One barrier.
__device__ __forceinline__ MpsCompressDecision cut_decide(int svd_status, int count, const double* s, double trunc_thr, int max_bond,
                                                          MpsCompressDecision* slot) {
    if (threadIdx.x == 0) {
        MpsCompressDecision d = {0, 0, 0.0, 0.0, 0.0, 1.0};
        if (svd_status == 0) d = mps_compress_decide(count, s, trunc_thr, max_bond);
        *slot = d;
    }
    __syncthreads();   // (every thread has read the status before thread 0 writes it)
    return *slot;
}

// the status of a state whose cut was refused: the SVD at its sweep limit, else a zero or non-finite spectrum
__device__ __forceinline__ int cut_failure(int svd_status) { return svd_status == 1 ? kMpsCompressSweepLimit : kMpsCompressNonFinite; }

// lambda'_q = rescale Sigma[:rank], into LDS for the site and into memory; no barrier: the caller has one before the site is written
__device__ __forceinline__ void cut_bond(const MpsCompressDecision& d, const double* s, double* lam_lds, double* out_lam) {
    const int tid = threadIdx.x;
    if (tid < d.rank) {
        const double v = d.rescale * s[tid];
        lam_lds[tid] = v;
        out_lam[tid] = v;
    }
}

// T'_q[s][l][j] = U[(s, l), j] lambda'_q[j] / lambda'_{q-1}[l] (lam_left null: ones), packed [2][r][rk] into out; u has leading
// dimension ldu.  kCarry: also W[(s, l)][j] = rescale conj(U[(s, l), j]), packed alike into w (what aqc_mps_fromvec.hip projects with)
template <bool kCarry = false>
__device__ __forceinline__ void cut_left_site(const double2* u, int ldu, int r, int rk, const double* lam_lds, const double* lam_left,
                                              double2* out, double rescale = 1.0, double2* w = nullptr) {
    for (int e = threadIdx.x; e < 2 * r * rk; e += 256) {
        const MpsCompressSiteIndex at = mps_compress_site_index(e, r, rk);
        const double f = mps_compress_site_factor(lam_lds[at.j], lam_left ? lam_left[at.l] : 1.0);
        const double2 x = u[(size_t)at.row * ldu + at.j];
        out[e] = make_double2(f * x.x, f * x.y);
        if (kCarry) w[e] = make_double2(rescale * x.x, -(rescale * x.y));
    }
}

}  // namespace
}  // namespace aqc
