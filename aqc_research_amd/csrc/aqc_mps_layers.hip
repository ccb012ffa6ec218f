// Gate layers on MPS states, fused route (rules and notation: aqc_mps_layers_rule.h; host side: aqc_mps_layers_api.cpp).
//
// The working copy of every unit (an evolved state) lives in flat stores of the call: sites packed at the current bond dimensions, bond
// vectors, and the dims on the device.  Per layer of the program and chunk of its matrices (gates x units):
//   mps_layer_form_kernel    reads dims[q .. q + 2]; P_ab = T_q[a] T_{q+1}[b] into block (a, b) of the unit's matrix of the SVD batch
//                            (middle bond above 16: T_q[a] in the LDS planes of aqc_mps_planes.h, T_{q+1}[b] streamed, on
//                            v_mfma_f64_16x16x4_f64; up to 16: a plain loop per element), then in place
//                            theta[(a', l), (b', r)] = lambda_{q-1}[l] sum_ab G[2a' + b'][2a + b] P_ab[l][r]; rows = 2 chi_q, cols = 2 chi_{q+2}
//   launch_svd_batch         (aqc_svd_batch.hip) over the chunk; a wide theta goes through its transpose there
//   mps_layer_split_kernel   the cut by the steps of aqc_mps_cut.h (thread 0 takes mps_compress_decide, the host's text; the decision in
//                            static LDS, the new bond vector in dynamic LDS); rank into dims[q + 1], total - kept onto the bond's
//                            dropped weight, sweeps; T'_q = U Sigma rescale / lambda_{q-1}, T'_{q+1} = V^H, lambda'_q = Sigma rescale
//                            packed at the new dims over the old sites (theta has consumed them).  A rank beyond bounds[q + 1] is this
//                            kernel's own refusal.
// mps_layer_load_kernel copies the inputs into the stores first; the inputs are never written.  One workgroup per (gate, unit).  The
// gates of a layer touch disjoint sites and bonds: a workgroup writes T_q, T_{q+1}, lambda_q, dims[q + 1] and the words of bond q alone,
// and reads lambda_{q-1}, dims[q], dims[q + 2], which no gate of the same layer writes.  A unit whose spectrum is zero or not finite, whose
// SVD reached its sweep limit, or whose rank passes its bound is marked by its own workgroup and skipped from then on (rows = 0: the SVD
// kernel leaves at once).  No atomics, every sum in a fixed order, nothing is read from or written to another unit's stores.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_cut.h"
#include "aqc_mps_layers_rule.h"
#include "aqc_mps_planes.h"

namespace aqc {

static_assert((int)kMpsLayersCap == (int)kMpsObsFusedCap, "the planes of aqc_mps_planes.h are sized by the observables' cap");
static_assert((int)kMpsLayersSweepLimit == (int)kMpsCompressSweepLimit && (int)kMpsLayersNonFinite == (int)kMpsCompressNonFinite, "cut_failure");

namespace {

constexpr int kLayerSmallBond = 16;                                // middle bonds up to here take the plain loop
constexpr size_t kSplitLds = sizeof(double) * 2 * kCap;            // the new bond vector

__device__ __forceinline__ const cplx* const* unit_sites(const MpsLayersArgs& a, int unit) {
    return reinterpret_cast<const cplx* const*>(a.table + (size_t)unit * a.per + a.at_sites);
}
__device__ __forceinline__ const double* const* unit_lams(const MpsLayersArgs& a, int unit) {
    return reinterpret_cast<const double* const*>(a.table + (size_t)unit * a.per + a.at_lams);
}
__device__ __forceinline__ const int* unit_dims(const MpsLayersArgs& a, int unit) {
    return reinterpret_cast<const int*>(a.table + (size_t)unit * a.per + a.at_dims);
}

}  // namespace

// grid (units, n); 256 threads
__global__ __launch_bounds__(256) void mps_layer_load_kernel(MpsLayersArgs a) {
    const int unit = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    const int* din = unit_dims(a, unit);
    const int dl = din[q], dr = din[q + 1];   // <= bounds[q], bounds[q + 1]: the host sized the stores by them
    const cplx* src = unit_sites(a, unit)[q];
    cplx* dst = a.sites + (size_t)unit * a.site_total + a.site_off[q];
    for (int e = tid; e < 2 * dl * dr; e += 256) dst[e] = src[e];
    if (q < a.n - 1) {
        const double* ls = unit_lams(a, unit)[q];
        double* ld = a.lam + (size_t)unit * a.lam_total + a.lam_off[q];
        for (int e = tid; e < dr; e += 256) ld[e] = ls[e];
    }
    if (tid == 0) {
        int* dims = a.dims + (size_t)unit * (a.n + 1);
        dims[q] = dl;
        if (q == a.n - 1) dims[a.n] = dr;
    }
}

// grid (matrices of the chunk); 256 threads; dynamic LDS kFusedLds when a middle bond can pass kLayerSmallBond, else none
__global__ __launch_bounds__(256) void mps_layer_form_kernel(MpsLayersArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lay_smem[];
    const int item = blockIdx.x, tid = threadIdx.x;
    const int idx = a.first + item, unit = idx / a.gates, g = idx - unit * a.gates, q = a.gate_q[g];
    const int failed = a.failed[unit];
    if (failed && failed <= a.layer) {   // 1 + the layer that failed the unit, written by its split kernels: every gate of that layer still runs
        if (tid == 0) { a.rows[item] = 0; a.cols[item] = 0; }
        return;
    }
    const int* dims = a.dims + (size_t)unit * (a.n + 1);
    const int cl = dims[q], cm = dims[q + 1], cr = dims[q + 2];   // each <= its bound <= kCap
    const cplx* tq = a.sites + (size_t)unit * a.site_total + a.site_off[q];
    const cplx* tn = a.sites + (size_t)unit * a.site_total + a.site_off[q + 1];
    const int ld = a.m;                                           // 2 cl, 2 cr <= m
    cplx* theta = a.a + (size_t)item * ld * ld;
    if (cm > kLayerSmallBond) {
        double* er = lay_smem;
        double* ei = er + kPlane;
        double* fr = ei + kPlane;
        double* fi = fr + kPlane;
        planes_zero(lay_smem);
        __syncthreads();
        for (int e = tid; e < 2 * cl * cm; e += 256) {
            const cplx x = tq[e];
            const int s = e / (cl * cm), rest = e - s * cl * cm, i = rest / cm, c = rest - i * cm;
            (s ? fr : er)[i * kLd + c] = x.x;
            (s ? fi : ei)[i * kLd + c] = x.y;
        }
        __syncthreads();
        Acc p;
#pragma unroll 1
        for (int ab = 0; ab < 4; ++ab) {
            const int s = ab >> 1, b = ab & 1;
            prod_lds_mem<false>(s ? fr : er, s ? fi : ei, tn + (size_t)b * cm * cr, cl, cm, cr, p);
            acc_to_mem(p, theta + (size_t)s * cl * ld + (size_t)b * cr, ld, cl, cr);
        }
    } else {
        for (int e = tid; e < cl * cr; e += 256) {
            const int l = e / cr, r = e - l * cr;
#pragma unroll
            for (int ab = 0; ab < 4; ++ab) {
                const int s = ab >> 1, b = ab & 1;
                const cplx* x = tq + ((size_t)s * cl + l) * cm;
                const cplx* y = tn + (size_t)b * cm * cr + r;
                double re = 0.0, im = 0.0;
                for (int m = 0; m < cm; ++m) {
                    const cplx u = x[m], v = y[(size_t)m * cr];
                    re += u.x * v.x - u.y * v.y;
                    im += u.x * v.y + u.y * v.x;
                }
                theta[((size_t)s * cl + l) * ld + (size_t)b * cr + r] = make_double2(re, im);
            }
        }
    }
    __threadfence_block();
    __syncthreads();   // the four blocks of P are in memory, for every thread of the workgroup
    const cplx* G = a.mats + ((size_t)a.unit_set[unit] * a.ngates + a.gate_id[g]) * 16;
    const double* lam_left = q > 0 ? a.lam + (size_t)unit * a.lam_total + a.lam_off[q - 1] : nullptr;
    for (int e = tid; e < cl * cr; e += 256) {
        const int l = e / cr, r = e - l * cr;
        const double f = lam_left ? lam_left[l] : 1.0;
        cplx p[4];
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) p[ab] = theta[((size_t)(ab >> 1) * cl + l) * ld + (size_t)(ab & 1) * cr + r];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int ab = 0; ab < 4; ++ab) {
                const cplx w = G[4 * o + ab];
                re += w.x * p[ab].x - w.y * p[ab].y;
                im += w.x * p[ab].y + w.y * p[ab].x;
            }
            theta[((size_t)(o >> 1) * cl + l) * ld + (size_t)(o & 1) * cr + r] = make_double2(f * re, f * im);
        }
    }
    if (tid == 0) { a.rows[item] = 2 * cl; a.cols[item] = 2 * cr; }
}

// grid (matrices of the chunk); 256 threads; dynamic LDS kSplitLds
__global__ __launch_bounds__(256) void mps_layer_split_kernel(MpsLayersArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lay_smem[];
    __shared__ MpsCompressDecision dec;
    double* lam = lay_smem;                        // [2 kCap]
    const int item = blockIdx.x, tid = threadIdx.x;
    const int idx = a.first + item, unit = idx / a.gates, g = idx - unit * a.gates, q = a.gate_q[g];
    if (a.rows[item] == 0) return;   // the form kernel of this chunk has skipped the unit
    const int* dims = a.dims + (size_t)unit * (a.n + 1);
    const int cl = dims[q], cr = dims[q + 2], ld = a.m;
    const int count = 2 * (cl < cr ? cl : cr);     // <= m
    const int svd_status = a.svd_status[item];
    const double* s = a.s + (size_t)item * ld;
    const MpsCompressDecision d = cut_decide(svd_status, count, s, a.trunc_thr, a.max_bond, &dec);
    const int rk = d.rank;
    const size_t bond = (size_t)unit * (a.n - 1) + q;
    if (!d.ok || rk > a.bounds[q + 1]) {
        if (tid == 0) {
            a.fail_code[bond] = !d.ok ? cut_failure(svd_status) : kMpsLayersOverflow;
            a.fail_layer[bond] = a.layer;
            a.failed[unit] = a.layer + 1;   // (every failing gate of the layer writes the same value)
        }
        return;
    }
    cut_bond(d, s, lam, a.lam + (size_t)unit * a.lam_total + a.lam_off[q]);
    __syncthreads();   // (every thread has read dims before thread 0 writes the rank)
    if (tid == 0) {
        a.dims[(size_t)unit * (a.n + 1) + q + 1] = rk;
        a.dropped[bond] += d.total - d.kept;
        a.sweeps[(size_t)unit * a.ngates + a.gate_id[g]] = a.svd_sweeps[item];
    }
    const cplx* u = a.u + (size_t)item * ld * ld;
    const cplx* vh = a.vh + (size_t)item * ld * ld;
    const double* lam_left = q > 0 ? a.lam + (size_t)unit * a.lam_total + a.lam_off[q - 1] : nullptr;
    cplx* out_q = a.sites + (size_t)unit * a.site_total + a.site_off[q];        // [2][cl][rk], rk <= bounds[q + 1]
    cplx* out_n = a.sites + (size_t)unit * a.site_total + a.site_off[q + 1];    // [2][rk][cr]
    cut_left_site(u, ld, cl, rk, lam, lam_left, out_q);
    for (int e = tid; e < 2 * rk * cr; e += 256) {
        const int b = e / (rk * cr), rest = e - b * rk * cr, j = rest / cr, r = rest - j * cr;
        out_n[e] = vh[(size_t)j * ld + (size_t)b * cr + r];
    }
}

hipError_t launch_mps_layer_load(const MpsLayersArgs& a, int units, hipStream_t s) {
    if (units <= 0 || a.n <= 0) return hipSuccess;
    mps_layer_load_kernel<<<dim3(units, a.n), 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_layer_form(const MpsLayersArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_layer_form_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    const size_t lds = a.m / 2 > kLayerSmallBond ? kFusedLds : 0;   // no middle bond passes K = m / 2
    mps_layer_form_kernel<<<count, 256, lds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_layer_split(const MpsLayersArgs& a, int count, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    mps_layer_split_kernel<<<count, 256, kSplitLds, s>>>(a);
    return hipGetLastError();
}

}  // namespace aqc
