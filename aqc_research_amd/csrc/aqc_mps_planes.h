// Products of complex matrices held as split re / im planes in LDS, on v_mfma_f64_16x16x4_f64: what the fused walks of
// aqc_mps_obs.hip (pair density matrices), aqc_mps_sample.hip (measurement), aqc_mps_pauli.hip (Pauli strings) and aqc_mps_melem.hip (operator matrix elements) and the sweeps of
// aqc_mps_ent.hip, aqc_mps_compress.hip, aqc_mps_layers.hip, aqc_mps_fromvec.hip and aqc_mps_tovec.hip are made of: the products, the
// moves between memory, planes and accumulators (planes_zero, plane_load, plane_fill, acc_store, acc_to_mem, acc_axpy), the workgroup's sums, and -- host side,
// at the end -- grant_dynamic_lds, the one way these nine files ask for the planes' dynamic LDS.  The truncating cut that follows an SVD of
// such a sweep is in aqc_mps_cut.h.  Device code but for the grant, internal linkage.
// A plane is [kCap][kLd] doubles; a workgroup is 4 waves, wave w owns rows [16w, 16w + 16) of a product and all four 16-column tiles.
// Operand layout of the instruction: top of aqc_mps.hip.  Operand tiles are zero-filled beyond the given dimensions, so accumulators
// there are exact zeros and whole tiles are stored; reads never leave the tiles written for the current dimensions.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

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

// the four planes zeroed, then a packed rows x cols matrix (rows, cols <= kCap) into the pair (pr, pi); the caller synchronises after each
__device__ __forceinline__ void planes_zero(double* smem) {
    for (int e = threadIdx.x; e < 4 * kPlane; e += 256) smem[e] = 0.0;
}
__device__ __forceinline__ void plane_load(const cplx* __restrict__ src, int rows, int cols, double* pr, double* pi) {
    for (int e = threadIdx.x; e < rows * cols; e += 256) {
        const cplx x = src[e];
        const int i = e / cols, c = e - i * cols;
        pr[i * kLd + c] = x.x;
        pi[i * kLd + c] = x.y;
    }
}
// the same with the tiles made whole: a packed rows x cols matrix into the planes (pr, pi), zeros up to rows_to x cols_to (<= kCap
// each), which are the whole tiles that the next product reads; the caller synchronises
__device__ __forceinline__ void plane_fill(const cplx* src, int rows, int cols, int rows_to, int cols_to, double* pr, double* pi) {
    for (int e = threadIdx.x; e < rows_to * cols_to; e += 256) {
        const int i = e / cols_to, c = e - i * cols_to;
        cplx x = make_double2(0.0, 0.0);
        if (i < rows && c < cols) x = src[(size_t)i * cols + c];
        pr[i * kLd + c] = x.x;
        pi[i * kLd + c] = x.y;
    }
}
// the wave's part of acc, rows below m and columns below nn, times f (1: exact) into dst with leading dimension ld
__device__ __forceinline__ void acc_to_mem(const Acc& acc, cplx* __restrict__ dst, int ld, int m, int nn, double f = 1.0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * wave + 4 * r + lk, j = 16 * t + li;
            if (i < m && j < nn) dst[(size_t)i * ld + j] = make_double2(f * acc.re[t][r], f * acc.im[t][r]);
        }
}

// dst (m x nn, packed) = w acc (first) or += w acc, element (i, j) written by the thread that writes it in acc_to_mem: the same thread in
// every product of one shape, so a read-modify-write of memory that only this mapping touches needs no atomics and no barrier
__device__ __forceinline__ void acc_axpy(const Acc& acc, double wr, double wi, cplx* dst, int m, int nn, bool first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * wave + 4 * r + lk, j = 16 * t + li;
            if (i < m && j < nn) {
                cplx* at = dst + (size_t)i * nn + j;
                const double re = wr * acc.re[t][r] - wi * acc.im[t][r], im = wr * acc.im[t][r] + wi * acc.re[t][r];
                if (first) {
                    *at = make_double2(re, im);
                } else {
                    const cplx old = *at;
                    *at = make_double2(old.x + re, old.y + im);
                }
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

// Host side: dynamic LDS beyond the default for `Kernels` on the current device (hipFuncSetAttribute applies to that one alone), before
// their launches.  Every set of kernels and size is an instantiation with a memo of its own: a known device is set once, an unknown
// one every time and nothing is remembered.  Two host threads may make the first call at the same time: both set the same value
template <size_t kBytes, auto... Kernels>
hipError_t grant_dynamic_lds() {
    static std::atomic<bool> granted[64];
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev >= 0 && granted[dev].load(std::memory_order_acquire)) return hipSuccess;
    for (const void* f : {reinterpret_cast<const void*>(Kernels)...}) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBytes);
        if (e != hipSuccess) return e;
    }
    if (dev >= 0) granted[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

}  // namespace
}  // namespace aqc
