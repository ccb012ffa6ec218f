// Products of complex matrices held as split re / im planes in LDS, on v_mfma_f64_16x16x4_f64: what the fused walks of
// aqc_mps_obs.hip (pair density matrices), aqc_mps_sample.hip (measurement) and aqc_mps_pauli.hip (Pauli strings) are made of.  Device
// code, internal linkage.
// A plane is [kCap][kLd] doubles; a workgroup is 4 waves, wave w owns rows [16w, 16w + 16) of a product and all four 16-column tiles.
// Operand layout of the instruction: top of aqc_mps.hip.  Operand tiles are zero-filled beyond the given dimensions, so accumulators
// there are exact zeros and whole tiles are stored; reads never leave the tiles written for the current dimensions.
#pragma once
#include <hip/hip_runtime.h>

#include "aqc_mps_obs_rule.h"

namespace aqc {

typedef double2 cplx;
typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr int kCap = kMpsObsFusedCap, kLd = kCap + 2;          // leading dimension of an LDS plane (doubles)
constexpr int kPlane = kCap * kLd;                              // doubles per plane; four planes: E re, E im, F re, F im
constexpr size_t kFusedLds = sizeof(double) * 4 * kPlane;       // 135168 bytes

struct Acc { double4_t re[4], im[4]; };
__device__ __forceinline__ void acc_zero(Acc& a) {
#pragma unroll
    for (int t = 0; t < 4; ++t) { a.re[t] = double4_t{0, 0, 0, 0}; a.im[t] = double4_t{0, 0, 0, 0}; }
}

// acc (rows [16 wave, +16) x cols [0, 64)) = S[0..m)[0..k) . T[0..k)[0..nn): S from the LDS planes (sr, si), T [k][nn] from memory
// (TR: the site matrix is read transposed, memory holds [nn][k] -- the right environments contract a site's second bond)
template <bool TR = false>
__device__ __forceinline__ void prod_lds_mem(const double* sr, const double* si, const cplx* __restrict__ T, int m, int k, int nn, Acc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    acc_zero(acc);
    if (16 * wave >= m) return;
    for (int k0 = 0; k0 < k; k0 += 4) {
        const int kk = k0 + lk;
        const double ar = sr[(16 * wave + li) * kLd + kk], ai = si[(16 * wave + li) * kLd + kk];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (16 * t >= nn) continue;
            const int col = 16 * t + li;
            cplx b = make_double2(0.0, 0.0);
            if (kk < k && col < nn) b = TR ? T[(size_t)col * k + kk] : T[(size_t)kk * nn + col];
            acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b.x, acc.re[t], 0, 0, 0);
            acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b.y, acc.im[t], 0, 0, 0);
            acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, b.y, acc.re[t], 0, 0, 0);
            acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, b.x, acc.im[t], 0, 0, 0);
        }
    }
}
// acc = T^H . F: T [k][m] from memory (conjugate-transposed; TR: memory holds [m][k]), F [0..k)[0..nn) from the LDS planes (fr, fi)
template <bool TR = false>
__device__ __forceinline__ void prod_memh_lds(const cplx* __restrict__ T, const double* fr, const double* fi, int m, int k, int nn, Acc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    acc_zero(acc);
    if (16 * wave >= m) return;
    const int row = 16 * wave + li;
    for (int k0 = 0; k0 < k; k0 += 4) {
        const int kk = k0 + lk;
        cplx a = make_double2(0.0, 0.0);
        if (kk < k && row < m) a = TR ? T[(size_t)row * k + kk] : T[(size_t)kk * m + row];
        const double ar = a.x, ai = -a.y;   // conj
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (16 * t >= nn) continue;
            const double br = fr[kk * kLd + 16 * t + li], bi = fi[kk * kLd + 16 * t + li];
            acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, acc.re[t], 0, 0, 0);
            acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, acc.im[t], 0, 0, 0);
            acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, bi, acc.re[t], 0, 0, 0);
            acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, acc.im[t], 0, 0, 0);
        }
    }
}
// the wave's tiles of acc (rows below m, column tiles below nn) into LDS planes, whole tiles
__device__ __forceinline__ void acc_store(const Acc& acc, double* pr, double* pi, int m, int nn) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    if (16 * wave >= m) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (16 * t >= nn) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int at = (16 * wave + 4 * r + lk) * kLd + 16 * t + li;   // < kCap * kLd
            pr[at] = acc.re[t][r];
            pi[at] = acc.im[t][r];
        }
    }
}

// sum over the workgroup (4 waves) in a fixed order; every thread gets the result.  red: 8 doubles of LDS
__device__ __forceinline__ cplx block_sum(double re, double im, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { re += __shfl_xor(re, off, 64); im += __shfl_xor(im, off, 64); }
    __syncthreads();   // (the previous sum's readers are done with red)
    if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = re; red[2 * (threadIdx.x >> 6) + 1] = im; }
    __syncthreads();
    return make_double2((red[0] + red[2]) + (red[4] + red[6]), (red[1] + red[3]) + (red[5] + red[7]));
}

// sum_uv W[u][v] R[v][u]  (adj: sum_uv conj(W[u][v]) R[u][v]) over the chi x chi corner, this thread's share
__device__ __forceinline__ void acc_dot(const Acc& w, const cplx* __restrict__ R, int chi, bool adj, double& re, double& im) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    re = 0.0; im = 0.0;
    if (16 * wave >= chi) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (16 * t >= chi) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * wave + 4 * r + lk, v = 16 * t + li;
            if (u < chi && v < chi) {
                const double wr = w.re[t][r], wi = adj ? -w.im[t][r] : w.im[t][r];
                const cplx b = adj ? R[(size_t)u * chi + v] : R[(size_t)v * chi + u];
                re += wr * b.x - wi * b.y;
                im += wr * b.y + wi * b.x;
            }
        }
    }
}

}  // namespace
}  // namespace aqc
