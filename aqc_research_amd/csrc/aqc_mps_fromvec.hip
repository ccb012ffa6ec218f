// Dense vectors into MPS states, fused route (rules and notation: aqc_mps_fromvec_rule.h; host side: aqc_mps_fromvec_api.cpp).
//
// Per site q, with A_q = [N_r][c = 2 r_q] row-major in the lane's source buffer:
//   mps_fromvec_qr_kernel       grid (parts, lanes).  Level 0: a workgroup keeps a running R (c x c) in the F planes of aqc_mps_planes.h,
//                               loads one block of 64 rows of A_q into the E planes beneath it (conjugation-free; the first block of its
//                               part into the F planes themselves) and reduces the stacked 128 x c matrix in place with householder_lds
//                               (aqc_mps_householder.h), block after block of its part; it writes its c x c factor.  Level > 0: the same
//                               step with the factors of the level before as blocks of c rows, four to a workgroup, until one factor
//                               per lane is left; that level writes R^T as matrix `lane` of the batched SVD, rows = c, cols = min(c, N_r).
//   launch_svd_batch            (aqc_svd_batch.hip) over the lanes of the chunk;
//   mps_fromvec_split_kernel    the cut by the steps of aqc_mps_cut.h (thread 0 takes mps_compress_decide, the host's text; the bond vector;
//                               the new site and, in the same loop, W = rescale conj(U[:, :r]) for the projection); r_{q+1}, the weight of
//                               the cut, sweeps and status.  A matrix wider than the planes or a rank beyond the cap is this kernel's own refusal.
//   mps_fromvec_project_kernel  grid (row groups, lanes).  Y = A_q W on the fp64 matrix cores: W (c x r) in LDS planes, A_q streamed in
//                               chunks of 64 rows, a wave owning 16 of them with its whole strip of A_q loaded before the products, Y
//                               written with row stride r.  The memory-bound pass of the call.
// mps_fromvec_last_kernel writes the last site from A_{n-1}.  Every workgroup reads its lane's r_q from device memory; a lane whose status
// is set is skipped by every later launch (rows = 0: the SVD kernel leaves at once).  No atomics, every sum in a fixed order, no loop
// bound depends on data other than the ranks: a lane of NaNs runs to its first split and fails there alone.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_cut.h"
#include "aqc_mps_fromvec_rule.h"
#include "aqc_mps_householder.h"
#include "aqc_mps_planes.h"

namespace aqc {

static_assert(2 * (int)kMpsFromVecCap == (int)kCap && (int)kMpsFromVecBlockRows == (int)kCap, "[R; block] is the 128 x 64 of the four planes");

namespace {
constexpr int kFacElems = kCap * kCap;            // a lane's factor of one part
constexpr int kLdW = kMpsFromVecCap + 2;          // leading dimension of a W plane (doubles)
constexpr int kStrip = kCap / 4;                  // MFMA steps over the 64 columns of A_q
}  // namespace

// grid (parts of the level, lanes of the chunk); 256 threads; dynamic LDS kFusedLds
__global__ __launch_bounds__(256) void mps_fromvec_qr_kernel(MpsFromVecArgs a) {
    extern __shared__ __attribute__((aligned(16))) double fv_smem[];
    __shared__ double v[2 * kEntRows], wp[8 * kCap], np[4];
    double* er = fv_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const int lane = blockIdx.y, g = a.first + lane, p = blockIdx.x, tid = threadIdx.x;
    if (a.status[g] != kMpsCompressOk) {   // (written by this lane's split kernel of an earlier site)
        if (a.last && p == 0 && tid == 0) { a.rows[lane] = 0; a.cols[lane] = 0; }
        return;
    }
    const int r = a.bonds[(size_t)g * (a.n + 1) + a.q], c = 2 * r;   // c <= kCap: a rank never passes the bound of its bond
    if (c > kCap) return;
    const size_t height = a.level == 0 ? (size_t)kMpsFromVecBlockRows : (size_t)c;
    const cplx* src = a.level == 0 ? a.src + (size_t)lane * a.lane_elems : a.fac_in + (size_t)lane * a.max_parts * kFacElems;
    const size_t src_rows = a.level == 0 ? a.nr : a.in_blocks * (size_t)c;
    const size_t b0 = (size_t)p * a.blocks_per_part, b1 = b0 + a.blocks_per_part < a.in_blocks ? b0 + a.blocks_per_part : a.in_blocks;
    planes_zero(fv_smem);
    __syncthreads();
    for (size_t b = b0; b < b1; ++b) {
        const size_t row0 = b * height;
        const int h = (int)(src_rows - row0 < height ? src_rows - row0 : height);   // <= kCap rows into the E planes; the rows below are zero
        const cplx* blk = src + row0 * c;
        double* pr = b == b0 ? fr : er;   // the first block of the part by itself: R in its leading min(h, c) rows, exact zeros below
        double* pi = b == b0 ? fi : ei;
        plane_load(blk, h, c, pr, pi);
        __syncthreads();
        householder_lds(fv_smem, kCap, c, v, wp, np);   // leaves R in the leading rows of the F planes and zeros in the E planes
    }
    if (!a.last) {
        cplx* out = a.fac_out + ((size_t)lane * a.max_parts) * kFacElems + (size_t)p * c * c;
        for (int e = tid; e < c * c; e += 256) {
            const int i = e / c, col = e - i * c;
            out[e] = make_double2(fr[i * kLd + col], fi[i * kLd + col]);
        }
        return;
    }
    const int cols = (size_t)c < a.nr ? c : (int)a.nr;
    cplx* out = a.a + (size_t)lane * a.kc * a.kc;   // c <= kc
    for (int e = tid; e < c * cols; e += 256) {
        const int i = e / cols, j = e - i * cols;   // R^T[i][j] = R[j][i]
        out[(size_t)i * a.kc + j] = make_double2(fr[j * kLd + i], fi[j * kLd + i]);
    }
    if (tid == 0) { a.rows[lane] = c; a.cols[lane] = cols; }
}

// grid (lanes of the chunk); 256 threads.  q = 0 .. n - 2
__global__ __launch_bounds__(256) void mps_fromvec_split_kernel(MpsFromVecArgs a) {
    __shared__ double lam[kMpsFromVecCap];
    __shared__ MpsCompressDecision dec;
    const int lane = blockIdx.x, g = a.first + lane, tid = threadIdx.x, q = a.q, cuts = a.n - 1;
    if (a.status[g] != kMpsCompressOk) return;
    const int svd_status = a.svd_status[lane];
    int* bonds = a.bonds + (size_t)g * (a.n + 1);
    const int r = bonds[q], c = 2 * r;
    const int count = (size_t)c < a.nr ? c : (int)a.nr;   // <= kCap
    const double* s = a.s + (size_t)lane * a.kc;
    MpsCompressDecision d = cut_decide(c <= kCap ? svd_status : -1, count, s, a.trunc_thr, a.max_bond, &dec);   // (c <= kCap always)
    if (d.ok && d.rank > kMpsFromVecCap) d.ok = 0;   // (never: a rank stays within the bound of its bond)
    if (!d.ok) {
        if (tid == 0) { a.status[g] = cut_failure(svd_status); a.failed_at[g] = q; }
        return;
    }
    const int rk = d.rank;   // 1 .. min(count, kMpsFromVecCap)
    double* out_lam = a.lam + (size_t)g * a.lam_off[cuts];
    cut_bond(d, s, lam, out_lam + a.lam_off[q]);
    if (tid == 0) {
        bonds[q + 1] = rk;
        a.dropped[(size_t)g * cuts + q] = d.total - d.kept;
        a.sweeps[(size_t)g * cuts + q] = a.svd_sweeps[lane];
    }
    __syncthreads();
    const cplx* u = a.u + (size_t)lane * a.kc * a.kc;   // [c][kc], the leading `count` columns
    cplx* site = a.sites + (size_t)g * a.site_off[a.n] + a.site_off[q];   // T'_q[s][l][j], packed [2][r][rk]
    cplx* w = a.w + (size_t)lane * kCap * kMpsFromVecCap;                 // W[(s, l)][j], packed [c][rk]
    cut_left_site<true>(u, a.kc, r, rk, lam, q > 0 ? out_lam + a.lam_off[q - 1] : nullptr, site, d.rescale, w);
}

// grid (ceil(N_r / (64 kMpsFromVecProjectChunks)), lanes of the chunk); 256 threads
__global__ __launch_bounds__(256) void mps_fromvec_project_kernel(MpsFromVecArgs a) {
    __shared__ double wr[kCap * kLdW], wi[kCap * kLdW];
    const int lane = blockIdx.y, g = a.first + lane, tid = threadIdx.x;
    if (a.status[g] != kMpsCompressOk) return;   // (this site's split may have set it: nothing follows for the lane)
    const int* bonds = a.bonds + (size_t)g * (a.n + 1);
    const int r = bonds[a.q], c = 2 * r, rk = bonds[a.q + 1];   // c <= kCap, rk <= kMpsFromVecCap
    const cplx* w = a.w + (size_t)lane * kCap * kMpsFromVecCap;
    for (int e = tid; e < kCap * kLdW; e += 256) { wr[e] = 0.0; wi[e] = 0.0; }
    __syncthreads();
    for (int e = tid; e < c * rk; e += 256) {
        const cplx x = w[e];
        const int k = e / rk, j = e - k * rk;
        wr[k * kLdW + j] = x.x;
        wi[k * kLdW + j] = x.y;
    }
    __syncthreads();
    const cplx* A = a.src + (size_t)lane * a.lane_elems;
    cplx* Y = a.dst + (size_t)lane * a.lane_elems;
    const int ln = tid & 63, wave = tid >> 6, li = ln & 15, lk = ln >> 4;
    for (int ch = 0; ch < kMpsFromVecProjectChunks; ++ch) {
        const size_t row0 = ((size_t)blockIdx.x * kMpsFromVecProjectChunks + ch) * kCap + 16 * wave;   // the wave's 16 rows
        if (row0 >= a.nr) break;
        const size_t row = row0 + li;
        cplx strip[kStrip];   // this thread's elements of the wave's 16 x c strip of A_q: all loads before the products
#pragma unroll
        for (int it = 0; it < kStrip; ++it) {
            const int kk = 4 * it + lk;
            strip[it] = (kk < c && row < a.nr) ? A[row * c + kk] : make_double2(0.0, 0.0);
        }
        double4_t re[2], im[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { re[t] = double4_t{0, 0, 0, 0}; im[t] = double4_t{0, 0, 0, 0}; }
#pragma unroll
        for (int it = 0; it < kStrip; ++it) {
            if (4 * it >= c) continue;
            const int kk = 4 * it + lk;   // < kCap: a row of the zero-filled planes
            const double ar = strip[it].x, ai = strip[it].y;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (16 * t >= rk) continue;
                const double br = wr[kk * kLdW + 16 * t + li], bi = wi[kk * kLdW + 16 * t + li];
                re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, re[t], 0, 0, 0);
                im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, im[t], 0, 0, 0);
                re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, re[t], 0, 0, 0);
                im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, im[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const size_t i = row0 + 4 * rr + lk;
                const int j = 16 * t + li;
                if (i < a.nr && j < rk) Y[i * rk + j] = make_double2(re[t][rr], im[t][rr]);
            }
    }
}

// grid (lanes of the chunk); 64 threads.  q = n - 1: T'_{n-1}[s][l] = A_{n-1}[0][s r + l] / lambda'_{n-2}[l]
__global__ __launch_bounds__(64) void mps_fromvec_last_kernel(MpsFromVecArgs a) {
    const int lane = blockIdx.x, g = a.first + lane, tid = threadIdx.x, n = a.n;
    if (a.status[g] != kMpsCompressOk) return;
    int* bonds = a.bonds + (size_t)g * (n + 1);
    const int r = bonds[n - 1];   // <= 2
    const cplx* A = a.src + (size_t)lane * a.lane_elems;
    const double* lam_left = a.lam + (size_t)g * a.lam_off[n - 1] + a.lam_off[n - 2];
    cplx* site = a.sites + (size_t)g * a.site_off[n] + a.site_off[n - 1];
    if (tid < 2 * r) {
        const int l = tid < r ? tid : tid - r;
        const double f = mps_compress_site_factor(1.0, lam_left[l]);
        const cplx x = A[tid];
        site[tid] = make_double2(f * x.x, f * x.y);
    }
    if (tid == 0) bonds[n] = 1;
}

hipError_t launch_mps_fromvec_qr(const MpsFromVecArgs& a, int parts, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_fromvec_qr_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0 || parts <= 0) return hipSuccess;
    mps_fromvec_qr_kernel<<<dim3(parts, count), 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_fromvec_split(const MpsFromVecArgs& a, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    mps_fromvec_split_kernel<<<count, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_fromvec_project(const MpsFromVecArgs& a, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const size_t per = (size_t)kCap * kMpsFromVecProjectChunks, groups = (a.nr + per - 1) / per;   // <= 2^19 at n = 30
    mps_fromvec_project_kernel<<<dim3((unsigned)groups, count), 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_fromvec_last(const MpsFromVecArgs& a, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    mps_fromvec_last_kernel<<<count, 64, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace aqc
