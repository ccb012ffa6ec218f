// Matrix-free XXZ chain Hamiltonian on [lanes][2^n] complex128 state vectors (rules: aqc_xxz_rule.h) and the Chebyshev series of
// exp(-i H t) in that action.  One step kernel with three modes, grid (tiles, lanes), 256 threads:
//   a tile is the 2^T amplitudes that share their high index bits, T = min(n, 11): 32 KiB of LDS; a thread owns the 8 amplitudes
//   tid + 256 j.  The block loads its tile of the current vector with 16-byte loads into LDS; bonds i <= T - 2 resolve there at
//   l ^ (3 << i); the straddling bond T - 1 and the high bonds i >= T read the partner tile from global memory at the same low
//   offset (coalesced).  Whether a high bond is anti-aligned depends on the tile index alone, so those branches are uniform.
//   mode MUL     dst = H cur
//   mode STEP    next = scale * H cur - prev;  out += c_k * next      (first step: next = scale * H cur, out = c_0 cur + c_1 next)
//   mode ENERGY  partial[lane][tile] = sum over the tile of Re conj(cur) (H cur); xxz_energy_final adds the tiles in order
// Neighbours are read only from `cur`, which no thread writes in the launch; prev / next / out are touched by a thread at its own
// indices only, so prev and next may share a buffer.  Every sum runs in a fixed order (no atomics): the results of two calls are
// the same bits.
#include <hip/hip_runtime.h>

#include "aqc_lanes.h"
#include "aqc_launch.h"
#include "aqc_math.h"
#include "aqc_xxz_rule.h"

namespace aqc {

namespace {

constexpr int kXxzPer = (1 << kXxzTileBits) / kXxzThreads;   // amplitudes of a tile per thread
enum { kXxzMul = 0, kXxzStep = 1, kXxzEnergy = 2 };

// the wave's total in every lane, by the exchanges of aqc_lanes.h (each lane forms a fixed tree of additions)
__device__ __forceinline__ double xxz_wave_sum(double v) {
    v += dpp<0xB1>(v);    // lane ^ 1
    v += dpp<0x4E>(v);    // lane ^ 2
    v += lane_xor4(v);    // quads q and q ^ 1
    v += lane_xor12(v);   // ... and q ^ 3, q ^ 2: the row of 16
    v = add_xor16(v);
    v = add_xor32(v);
    return v;
}

template <int MODE>
__global__ __launch_bounds__(kXxzThreads) void xxz_step_kernel(XxzArgs a) {
    __shared__ cplx tile[1 << kXxzTileBits];
    __shared__ double red[kXxzThreads / 64];
    const int n = a.n, T = a.tile_bits, tid = threadIdx.x;
    const unsigned tsize = 1u << T;
    const uint64_t dim = (uint64_t)1 << n, base = (uint64_t)blockIdx.x << T;
    const unsigned low_mask = (tsize >> 1) - 1;   // bonds 0 .. T-2
    for (int lane = blockIdx.y; lane < a.lanes; lane += gridDim.y) {
        const cplx* __restrict__ cur = a.cur + (size_t)lane * a.cur_stride;
        if (lane != (int)blockIdx.y) __syncthreads();   // the previous lane's reads of the tile
#pragma unroll
        for (int j = 0; j < kXxzPer; ++j) {
            const unsigned l = tid + kXxzThreads * j;
            if (l < tsize) tile[l] = cur[base + l];
        }
        __syncthreads();
        cplx own[kXxzPer], acc[kXxzPer];
        uint64_t am[kXxzPer];
#pragma unroll
        for (int j = 0; j < kXxzPer; ++j) {
            const unsigned l = tid + kXxzThreads * j;
            own[j] = acc[j] = make_double2(0.0, 0.0);
            am[j] = 0;
            if (l < tsize) {
                am[j] = xxz_anti(base | l, n);
                own[j] = tile[l];
                const unsigned alow = (unsigned)am[j] & low_mask;
                for (int i = 0; i + 1 < T; ++i) {   // unconditional LDS reads, selected afterwards: no divergent branches
                    const cplx p = tile[l ^ (3u << i)];
                    const bool on = (alow >> i) & 1u;
                    acc[j].x += on ? p.x : 0.0; acc[j].y += on ? p.y : 0.0;
                }
            }
        }
        if (n > T) {   // T = kXxzTileBits here: every thread owns kXxzPer valid amplitudes
            // straddling bond T-1: the neighbouring tile, low offset with bit T-1 flipped
#pragma unroll
            for (int j = 0; j < kXxzPer; ++j) {
                const unsigned l = tid + kXxzThreads * j;
                if ((am[j] >> (T - 1)) & 1u) {
                    const cplx p = cur[xxz_partner(base | l, T - 1)];
                    acc[j].x += p.x; acc[j].y += p.y;
                }
            }
            // high bonds: anti-aligned or not for the whole tile
            const uint64_t ahigh = xxz_anti(base, n) >> T;
            for (int i = T; i + 1 < n; ++i) {
                if (!((ahigh >> (i - T)) & 1u)) continue;
                const cplx* __restrict__ pt = cur + xxz_partner(base, i);
#pragma unroll
                for (int j = 0; j < kXxzPer; ++j) {
                    const cplx p = pt[tid + kXxzThreads * j];
                    acc[j].x += p.x; acc[j].y += p.y;
                }
            }
        }
        double esum = 0.0;
#pragma unroll
        for (int j = 0; j < kXxzPer; ++j) {
            const unsigned l = tid + kXxzThreads * j;
            if (l >= tsize) continue;
            const double d = xxz_diag(am[j], n, a.delta);
            const cplx h = make_double2(d * own[j].x - 0.5 * acc[j].x, d * own[j].y - 0.5 * acc[j].y);
            const size_t idx = (size_t)lane * dim + base + l;
            if (MODE == kXxzMul) {
                a.next[idx] = h;
            } else if (MODE == kXxzStep) {
                const cplx c = a.coef[lane];
                cplx nx, o;
                if (a.first) {
                    const cplx c0 = a.coef0[lane];
                    nx = make_double2(a.scale * h.x, a.scale * h.y);
                    o = make_double2(c0.x * own[j].x - c0.y * own[j].y, c0.x * own[j].y + c0.y * own[j].x);
                } else {
                    const cplx pv = a.prev[(size_t)lane * a.prev_stride + base + l];
                    nx = make_double2(a.scale * h.x - pv.x, a.scale * h.y - pv.y);
                    o = a.out[idx];
                }
                a.next[idx] = nx;
                a.out[idx] = make_double2(o.x + (c.x * nx.x - c.y * nx.y), o.y + (c.x * nx.y + c.y * nx.x));
            } else {
                esum += own[j].x * h.x + own[j].y * h.y;
            }
        }
        if (MODE == kXxzEnergy) {
            const double w = xxz_wave_sum(esum);
            if ((tid & 63) == 0) red[tid >> 6] = w;
            __syncthreads();
            if (tid == 0) {
                double s = red[0];
                for (int k = 1; k < kXxzThreads / 64; ++k) s += red[k];
                a.partial[(size_t)lane * gridDim.x + blockIdx.x] = s;
            }
        }
    }
}

// energy[lane] = sum of the lane's tile partials: strided per-thread sums in tile order, then a fixed tree in LDS
__global__ __launch_bounds__(kXxzThreads) void xxz_energy_final(const double* __restrict__ partial, size_t ntiles, int lanes, double* __restrict__ energy) {
    __shared__ double red[kXxzThreads];
    for (int lane = blockIdx.x; lane < lanes; lane += gridDim.x) {
        double s = 0.0;
        for (size_t t = threadIdx.x; t < ntiles; t += kXxzThreads) s += partial[(size_t)lane * ntiles + t];
        __syncthreads();
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = kXxzThreads / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) energy[lane] = red[0];
    }
}

dim3 xxz_grid(const XxzArgs& a) {
    const size_t ntiles = (size_t)1 << (a.n - a.tile_bits);
    return dim3((unsigned)ntiles, (unsigned)(a.lanes < 65535 ? a.lanes : 65535), 1);
}

}  // namespace

int xxz_tile_bits(int n) { return n < kXxzTileBits ? n : kXxzTileBits; }

hipError_t launch_xxz_mul(const XxzArgs& a, hipStream_t s) {
    xxz_step_kernel<kXxzMul><<<xxz_grid(a), kXxzThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_xxz_step(const XxzArgs& a, hipStream_t s) {
    xxz_step_kernel<kXxzStep><<<xxz_grid(a), kXxzThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_xxz_energy(const XxzArgs& a, double* energy, hipStream_t s) {
    xxz_step_kernel<kXxzEnergy><<<xxz_grid(a), kXxzThreads, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t ntiles = (size_t)1 << (a.n - a.tile_bits);
    xxz_energy_final<<<(unsigned)(a.lanes < 65535 ? a.lanes : 65535), kXxzThreads, 0, s>>>(a.partial, ntiles, a.lanes, energy);
    return hipGetLastError();
}

}  // namespace aqc
