// Measuring MPS states: shots drawn from |psi(b)|^2 and the amplitudes of given bit strings (rules and notation:
// aqc_mps_sample_rule.h; host side: aqc_mps_sample_api.cpp).
//
// fused route (every bond <= kMpsSampleFusedCap = 64): grid (ceil(shots / 64), states), 256 threads.  A workgroup owns 64 shots and
// walks the whole chain inside one launch.  The 64 row vectors v live in LDS as split re / im planes [64 shots][kLd]; a second pair
// of planes holds the current w_c.  Per site q and physical index c
//     W_c = V T_q[c]        (MFMA, A operand = V from LDS, B operand = T_q[c] streamed from memory)   -> planes
//     G_c = W_c R_{q+1}     (the same product shape, R_{q+1} from memory)                              in accumulators
//     m_c[s] = Re sum_v G_c[s][v] conj(W_c[s][v])
// W_0 is stored to the W planes; W_1 takes V's place as soon as every wave has read V, so one set of accumulators is alive at a
// time and the registers go to keeping the streamed operand's loads in flight (prod_stream).  The weights are read off G's
// accumulators against W in its planes at the accumulator layout (aqc_mps_planes.h): lane l holds row 4r + l / 16 of its wave's 16
// rows in register r, column 16t + l % 16 of tile t.  A row's sum runs over the four column tiles in order, then over the 16 lanes
// of the row by a butterfly of shuffles, after which all 16 lanes hold the same bits and take the same decision; the rows that took
// 0 copy W_0 over W_1.  No atomics.  Amplitudes of given bit strings are the same kernel without G and without weights (AMPS).
// Operand tiles are zero beyond the bonds, LDS is cleared once, every global store is guarded, rows beyond `shots` in the last block
// compute but store nothing.
//
// gemm route (any bond dimension): V, W_c, G_c are [rows][chi] matrices in memory, the products are zgemm launches (aqc_mps.hip), and
// mps_sample_rows_kernel does weights, draw, bit and select, a wave per row with a fixed-order sum.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_planes.h"
#include "aqc_mps_sample_rule.h"

namespace aqc {

namespace {

constexpr int kDepth = 4;   // k-steps of the streamed operand whose loads are in flight together

// prod_lds_mem of aqc_mps_planes.h (same operands, same order of the k-steps, all 64 rows) with the memory operand loaded kDepth k-steps
// at a time, one group ahead of the products that use it: a workgroup has one wave per SIMD, so nothing else hides the latency of T.
// (aqc_mps_obs.hip keeps the plain product: its code is not to change with this file.)
__device__ __forceinline__ void prod_stream(const double* sr, const double* si, const cplx* __restrict__ T, int k, int nn, Acc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    acc_zero(acc);
    cplx cur[kDepth][4], nxt[kDepth][4];
    auto load = [&](int k0, cplx (&b)[kDepth][4]) {
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            const int kk = k0 + 4 * d + lk;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = 16 * t + li;
                b[d][t] = kk < k && col < nn ? T[(size_t)kk * nn + col] : make_double2(0.0, 0.0);
            }
        }
    };
    load(0, cur);
    for (int k0 = 0; k0 < k; k0 += 4 * kDepth) {
        if (k0 + 4 * kDepth < k) load(k0 + 4 * kDepth, nxt);
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            if (k0 + 4 * d >= k) break;
            const int kk = k0 + 4 * d + lk;   // < kCap: k <= kCap and the k-steps are whole
            const double ar = sr[(16 * wave + li) * kLd + kk], ai = si[(16 * wave + li) * kLd + kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t >= nn) continue;
                const cplx b = cur[d][t];
                acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b.x, acc.re[t], 0, 0, 0);
                acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b.y, acc.im[t], 0, 0, 0);
                acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, b.y, acc.re[t], 0, 0, 0);
                acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, b.x, acc.im[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int d = 0; d < kDepth; ++d)
#pragma unroll
            for (int t = 0; t < 4; ++t) cur[d][t] = nxt[d][t];
    }
}

// m[r] = Re sum_v G[row][v] conj(W[row][v]) for the four rows this lane holds a share of: G in accumulators, W in the planes (pr, pi)
// it was stored to from accumulators of the same layout.  Tiles in order, then the 16 lanes of the row; all 16 get the same bits.
__device__ __forceinline__ void row_weights(const Acc& g, const double* pr, const double* pi, int nn, double m[4]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (16 * t >= nn) continue;   // G is exactly zero there, and the planes hold tiles of earlier sites
            const int at = (16 * wave + 4 * r + lk) * kLd + 16 * t + li;
            s += g.re[t][r] * pr[at] + g.im[t][r] * pi[at];
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        m[r] = s;
    }
}

}  // namespace

// grid (ceil(shots / 64), states); 256 threads; dynamic LDS kFusedLds (V re, V im, W re, W im)
template <bool AMPS>
__global__ __launch_bounds__(256) void mps_sample_fused_kernel(MpsSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sample_smem[];
    double* vr = sample_smem;
    double* vi = vr + kPlane;
    double* wr = vi + kPlane;
    double* wi = wr + kPlane;
    const MpsSampleState st = a.states[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    for (int e = tid; e < 4 * kPlane; e += 256) sample_smem[e] = 0.0;
    __syncthreads();
    if (tid < kCap) vr[tid * kLd] = 1.0;   // v = [1] in every row
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * kMpsSampleBlockShots + 16 * wave + lk;   // + 4r: the row of accumulator register r
    const unsigned long long my_shot = a.first_shot + (unsigned long long)(row0 + 4 * (li & 3));   // the row this lane draws for
    uint64_t words[4] = {0, 0, 0, 0};
    Acc acc;
    for (int q = 0; q < a.n; ++q) {
        const int chil = st.dims[q], chir = st.dims[q + 1];
        const cplx* T0 = st.sites[q];
        const cplx* T1 = T0 + (size_t)chil * chir;
        // W_0 goes to the W planes, W_1 takes V's place once every wave has read V: one accumulator set is alive at a time
        prod_stream(vr, vi, T0, chil, chir, acc);
        acc_store(acc, wr, wi, kCap, chir);
        prod_stream(vr, vi, T1, chil, chir, acc);
        __syncthreads();
        acc_store(acc, vr, vi, kCap, chir);
        __syncthreads();
        bool one[4];
        if (!AMPS) {
            const cplx* R = st.env_r + st.env_off[q + 1];
            double m0[4], m1[4];
            prod_stream(wr, wi, R, chir, chir, acc);
            row_weights(acc, wr, wi, chir, m0);
            prod_stream(vr, vi, R, chir, chir, acc);
            row_weights(acc, vr, vi, chir, m1);
            if ((q & 3) == 0) mps_sample_block(a.seed, st.lane, my_shot, (uint64_t)(q >> 2), words);
            const int k = q & 3;
            const double u_mine = philox_uniform(k == 0 ? words[0] : k == 1 ? words[1] : k == 2 ? words[2] : words[3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double u = __shfl(u_mine, (lane & 48) | r, 64);
                one[r] = mps_sample_decide(u, m0[r], m1[r]) != 0;
                const long long row = row0 + 4 * r;
                if (li == 0 && row < a.shots) {
                    st.bits[(size_t)row * a.n + q] = one[r] ? 1 : 0;
                    if (!mps_sample_weights_ok(m0[r], m1[r])) st.status[row] = 1;
                    if (q == 0 && row == 0) st.norm2[0] = m0[r] + m1[r];
                }
            }
            __syncthreads();   // every wave has read both plane pairs
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = row0 + 4 * r;
                one[r] = row < a.shots && a.bits_in[(size_t)row * a.n + q] != 0;
            }
        }
        // V holds W_1: the rows that took 0 get theirs from the W planes, whole tiles
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t >= chir || one[r]) continue;
                const int at = (16 * wave + 4 * r + lk) * kLd + 16 * t + li;
                vr[at] = wr[at];
                vi[at] = wi[at];
            }
        __syncthreads();   // V' is in place; W_0 has been read
    }
    // the last bond is 1: column 0 of V is psi(b)
    const long long row = (long long)blockIdx.x * kMpsSampleBlockShots + tid;
    if (tid < kMpsSampleBlockShots && row < a.shots) st.amps[row] = make_double2(vr[tid * kLd], vi[tid * kLd]);
}

// gemm route, after the products of site q: a wave per row, 4 rows per workgroup
template <bool AMPS>
__global__ __launch_bounds__(256) void mps_sample_rows_kernel(MpsSampleRowArgs a) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const size_t base = (size_t)row * a.chi;
    const long long shot = a.shot0 + row;   // within the call
    bool one;
    if (!AMPS) {
        double m0 = 0.0, m1 = 0.0;
        for (int v = lane; v < a.chi; v += 64) {
            const cplx g0 = a.g0[base + v], x0 = a.w0[base + v], g1 = a.g1[base + v], x1 = a.w1[base + v];
            m0 += g0.x * x0.x + g0.y * x0.y;
            m1 += g1.x * x1.x + g1.y * x1.y;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { m0 += __shfl_xor(m0, off, 64); m1 += __shfl_xor(m1, off, 64); }
        const double u = mps_sample_uniform(a.seed, a.lane, a.first_shot + (unsigned long long)shot, (uint64_t)a.q);
        one = mps_sample_decide(u, m0, m1) != 0;
        if (lane == 0) {
            a.bits[(size_t)shot * a.n + a.q] = one ? 1 : 0;
            if (!mps_sample_weights_ok(m0, m1)) a.status[shot] = 1;
            if (a.q == 0 && shot == 0) a.norm2[0] = m0 + m1;
        }
    } else {
        one = a.bits_in[(size_t)shot * a.n + a.q] != 0;
    }
    const cplx* src = one ? a.w1 : a.w0;
    for (int v = lane; v < a.chi; v += 64) a.v[base + v] = src[base + v];
    if (a.q == a.n - 1 && lane == 0) a.amps[shot] = src[base];   // the last bond is 1
}

__global__ void mps_sample_ones_kernel(cplx* v, long long rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) v[i] = make_double2(1.0, 0.0);
}

hipError_t launch_mps_sample_fused(const MpsSampleArgs& a, int nstates, bool amplitudes, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_sample_fused_kernel<false>, mps_sample_fused_kernel<true>>();
    if (e != hipSuccess) return e;
    if (nstates <= 0 || a.shots <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.shots + kMpsSampleBlockShots - 1) / kMpsSampleBlockShots), (unsigned)nstates);
    if (amplitudes) mps_sample_fused_kernel<true><<<grid, 256, kFusedLds, s>>>(a);
    else mps_sample_fused_kernel<false><<<grid, 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_sample_rows(const MpsSampleRowArgs& a, bool amplitudes, hipStream_t s) {
    if (a.rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.rows + 3) / 4);
    if (amplitudes) mps_sample_rows_kernel<true><<<grid, 256, 0, s>>>(a);
    else mps_sample_rows_kernel<false><<<grid, 256, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_sample_ones(void* v, long long rows, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    mps_sample_ones_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, s>>>(static_cast<cplx*>(v), rows);
    return hipGetLastError();
}

}  // namespace aqc
