// Pauli strings between MPS states: <phi|P|psi> for many strings and pairs per call (rules and notation: aqc_mps_pauli_rule.h; host
// side: aqc_mps_pauli_api.cpp).
//
// fused route (every bond of bra and ket <= kMpsPauliFusedCap = 64): one workgroup per (string, pair) walks its whole string inside one
// launch.  M (beta x chi) lives in LDS as split re / im planes [64][kLd]; the step across site q is, per physical index c,
//     F_c = M T_q[c]              (MFMA, A operand = M from LDS, B operand = T_q[c] streamed from memory)      -> LDS planes
//     W_c = B_q[c ^ f]^H F_c      (MFMA, A operand = conj B_q[c ^ f] streamed from memory, B operand = F_c from LDS)
// and M' = ph(0) W_0 + ph(1) W_1 goes back into the M planes: the step of mps_obs_env_kernel with a rectangular M, the second product's
// A operand taken from the bra, and the phase applied where the two accumulator sets are added (+-1 flips signs, +-i swaps re / im with
// signs: no multiplication).  Expectation mode opens with L_i of the ket and closes against R_{j+1} straight from the accumulators;
// bra / ket mode opens with [1] and reads M_n[0][0].  The plane products are those of aqc_mps_planes.h (here with the memory operand's
// first k-steps loaded one product ahead: prod_lds_mem_ahead, prod_memh_lds_ahead): operand tiles are zero-filled beyond the bonds, so
// accumulators there are exact zeros and whole tiles are stored; reads never leave the tiles written for the current dimensions.  Every sum runs in a fixed order that depends on the bonds and the string only: no atomics, and a value does not depend on
// which other strings or pairs are in the call.
//
// gemm route (any bond): the products are zgemm table launches (aqc_mps.hip); here are the elementwise kernel that dresses the bra's
// sites and the one that closes a walk against R.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_pauli_rule.h"
#include "aqc_mps_planes.h"

namespace aqc {

static_assert((int)kMpsPauliFusedCap == (int)kMpsObsFusedCap, "the planes of aqc_mps_planes.h are sized by the observables' cap");

namespace {

// The two plane products of aqc_mps_planes.h with their memory operand loaded ahead of the product: same operands, same zero fill,
// same order of the k-steps, so the same bits.  A workgroup has one wave per SIMD, nothing else hides the latency of a site tensor,
// and a walk over many different states finds little of them in the L2.
constexpr int kDepth = 4;         // k-steps of the B operand loaded together
constexpr int kDepthA = 8;         // k-steps of the A operand loaded together
struct OperandA { cplx a[kDepthA]; };       // this lane's share of kDepthA k-steps of the A operand of prod_memh_lds
struct OperandB { cplx b[kDepth][4]; };     // this lane's share of kDepth k-steps of the B operand of prod_lds_mem

__device__ __forceinline__ void load_a(const cplx* __restrict__ T, int m, int k, int k0, OperandA& o) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    const int row = 16 * wave + li;
#pragma unroll
    for (int s = 0; s < kDepthA; ++s) {
        const int kk = k0 + 4 * s + lk;
        o.a[s] = kk < k && row < m ? T[(size_t)kk * m + row] : make_double2(0.0, 0.0);
    }
}
__device__ __forceinline__ void load_b(const cplx* __restrict__ T, int m, int k, int nn, int k0, OperandB& o) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int d = 0; d < kDepth; ++d) {
        const int kk = k0 + 4 * d + lk;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = 16 * t + li;
            o.b[d][t] = 16 * wave < m && kk < k && col < nn ? T[(size_t)kk * nn + col] : make_double2(0.0, 0.0);
        }
    }
}
// prod_lds_mem(sr, si, T, m, k, nn, acc); `cur` holds load_b(T, m, k, nn, 0) and is used for the later k-steps too
__device__ __forceinline__ void prod_lds_mem_ahead(const double* sr, const double* si, const cplx* __restrict__ T, OperandB& cur, int m, int k, int nn,
                                                   Acc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    acc_zero(acc);
    if (16 * wave >= m) return;
    for (int k0 = 0; k0 < k; k0 += 4 * kDepth) {
        if (k0) load_b(T, m, k, nn, k0, cur);
#pragma unroll
        for (int d = 0; d < kDepth; ++d) {
            if (k0 + 4 * d >= k) break;
            const int kk = k0 + 4 * d + lk;   // < kCap: k <= kCap and the k-steps are whole
            const double ar = sr[(16 * wave + li) * kLd + kk], ai = si[(16 * wave + li) * kLd + kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t >= nn) continue;
                const cplx b = cur.b[d][t];
                acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b.x, acc.re[t], 0, 0, 0);
                acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, b.y, acc.im[t], 0, 0, 0);
                acc.re[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, b.y, acc.re[t], 0, 0, 0);
                acc.im[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, b.x, acc.im[t], 0, 0, 0);
            }
        }
    }
}
// prod_memh_lds(T, fr, fi, m, k, nn, acc); `o` holds load_a(T, m, k, 0) and is used for the later k-steps too
__device__ __forceinline__ void prod_memh_lds_ahead(const cplx* __restrict__ T, OperandA& o, const double* fr, const double* fi, int m, int k, int nn,
                                                    Acc& acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    acc_zero(acc);
    if (16 * wave >= m) return;
    for (int k0 = 0; k0 < k; k0 += 4 * kDepthA) {
        if (k0) load_a(T, m, k, k0, o);
#pragma unroll
        for (int s = 0; s < kDepthA; ++s) {
            if (k0 + 4 * s >= k) break;
            const int kk = k0 + 4 * s + lk;
            const double ar = o.a[s].x, ai = -o.a[s].y;   // conj
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
}

// what the step across site q reads: the ket's and the (flipped) bra's matrices and the letter's two phases
struct SiteOperands {
    int bl, br, kl, kr, turns0, turns1;
    const cplx *T0, *T1, *B0, *B1;   // T_q[0], T_q[1], B_q[0 ^ f], B_q[1 ^ f]
};
__device__ __forceinline__ SiteOperands site_operands(const MpsPauliState& bra, const MpsPauliState& ket, const unsigned char* str, int q) {
    SiteOperands o;
    o.bl = bra.dims[q]; o.br = bra.dims[q + 1]; o.kl = ket.dims[q]; o.kr = ket.dims[q + 1];
    const int letter = str[q], f = mps_pauli_flip(letter);
    o.T0 = ket.sites[q];
    o.T1 = o.T0 + (size_t)o.kl * o.kr;
    o.B0 = bra.sites[q] + (size_t)(f ? 1 : 0) * o.bl * o.br;
    o.B1 = bra.sites[q] + (size_t)(f ? 0 : 1) * o.bl * o.br;
    o.turns0 = mps_pauli_turns(letter, 0);
    o.turns1 = mps_pauli_turns(letter, 1);
    return o;
}

}  // namespace

// grid (strings, pairs); 256 threads; dynamic LDS kFusedLds
__global__ __launch_bounds__(256) void mps_pauli_fused_kernel(MpsPauliFusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double pauli_smem[];
    __shared__ double red[8];
    double* er = pauli_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const int s = blockIdx.x, pair = blockIdx.y, tid = threadIdx.x;
    const MpsPauliState ket = a.kets[pair];
    const MpsPauliState bra = a.expectation ? ket : a.bras[pair];
    const unsigned char* str = a.strings + (size_t)s * a.n;
    const int start = a.expectation ? a.first[s] : 0, last = a.expectation ? a.last[s] : a.n - 1;
    for (int e = tid; e < 4 * kPlane; e += 256) pauli_smem[e] = 0.0;
    __syncthreads();
    if (a.expectation) {   // M = L_start of the ket
        const int chi = ket.dims[start];
        const cplx* L = ket.env_l + ket.env_off[start];
        for (int e = tid; e < chi * chi; e += 256) {
            const cplx v = L[e];
            const int x = e / chi, y = e - x * chi;
            er[x * kLd + y] = v.x;
            ei[x * kLd + y] = v.y;
        }
    } else if (tid == 0) {
        er[0] = 1.0;
    }
    __syncthreads();
    Acc acc, tmp;
    OperandB tb;   // the next product's memory operands, in flight while the current one runs
    OperandA ta;
    SiteOperands o = site_operands(bra, ket, str, start);
    load_b(o.T0, o.bl, o.kl, o.kr, 0, tb);
    load_a(o.B0, o.br, o.bl, 0, ta);
    for (int q = start; q <= last; ++q) {
        const int bl = o.bl, br = o.br, kl = o.kl, kr = o.kr, turns0 = o.turns0, turns1 = o.turns1;
        const cplx* B1 = o.B1;
        // c = 0
        prod_lds_mem_ahead(er, ei, o.T0, tb, bl, kl, kr, tmp);
        load_b(o.T1, bl, kl, kr, 0, tb);
        acc_store(tmp, fr, fi, bl, kr);
        __syncthreads();
        prod_memh_lds_ahead(o.B0, ta, fr, fi, br, bl, kr, acc);
        load_a(o.B1, br, bl, 0, ta);
        __syncthreads();   // F_0 has been read
        // c = 1
        prod_lds_mem_ahead(er, ei, o.T1, tb, bl, kl, kr, tmp);
        if (q < last) {
            o = site_operands(bra, ket, str, q + 1);
            load_b(o.T0, o.bl, o.kl, o.kr, 0, tb);
        }
        acc_store(tmp, fr, fi, bl, kr);
        __syncthreads();   // (also: every wave is done reading M)
        prod_memh_lds_ahead(B1, ta, fr, fi, br, bl, kr, tmp);
        if (q < last) load_a(o.B0, o.br, o.bl, 0, ta);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double x0, y0, x1, y1;
                mps_pauli_turn(turns0, acc.re[t][r], acc.im[t][r], x0, y0);
                mps_pauli_turn(turns1, tmp.re[t][r], tmp.im[t][r], x1, y1);
                acc.re[t][r] = x0 + x1;
                acc.im[t][r] = y0 + y1;
            }
        if (q < last) acc_store(acc, er, ei, br, kr);
        __syncthreads();   // M' is in place; F_1 has been read
    }
    cplx* out = a.out[pair] + s;
    if (a.expectation) {   // sum_uv M_{last+1}[u][v] R_{last+1}[v][u]
        double re, im;
        acc_dot(acc, ket.env_r + ket.env_off[last + 1], ket.dims[last + 1], false, re, im);
        const cplx total = block_sum(re, im, red);
        if (tid == 0) *out = total;
    } else if (tid == 0) {   // M_n[0][0]: register 0 of tile 0 of wave 0, lane 0
        *out = make_double2(acc.re[0][0], acc.im[0][0]);
    }
}

// grid (blocks over the largest site, n sites): the dressed copies of site q, X: B[c ^ 1], Y: (-i B[1], i B[0]), Z: (B[0], -B[1])
__global__ void mps_pauli_dress_kernel(const cplx* const* sites, const int* dims, const size_t* site_off, size_t total, cplx* __restrict__ out) {
    const int q = blockIdx.y;
    const size_t half = (size_t)dims[q] * dims[q + 1];
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 2 * half) return;
    const cplx* B = sites[q];
    const int c = e >= half;
    const cplx same = B[e], other = B[c ? e - half : e + half];
    cplx* o = out + site_off[q] + e;
    o[0] = other;
    o[total] = c ? make_double2(-other.y, other.x) : make_double2(other.y, -other.x);
    o[2 * total] = c ? make_double2(-same.x, -same.y) : same;
}

// grid (jobs): out[idx[k]] = sum_uv M_k[u][v] R_k[v][u]
__global__ __launch_bounds__(256) void mps_pauli_close_kernel(const cplx* const* m_tab, const cplx* const* r_tab, const int* __restrict__ idx, int chi,
                                                              cplx* __restrict__ out) {
    __shared__ double red[8];
    const cplx* M = m_tab[blockIdx.x];
    const cplx* R = r_tab[blockIdx.x];
    const size_t count = (size_t)chi * chi;
    double re = 0.0, im = 0.0;
    for (size_t i = threadIdx.x; i < count; i += 256) {
        const int u = (int)(i / chi), v = (int)(i - (size_t)u * chi);
        const cplx m = M[i], r = R[(size_t)v * chi + u];
        re += m.x * r.x - m.y * r.y;
        im += m.x * r.y + m.y * r.x;
    }
    const cplx total = block_sum(re, im, red);
    if (threadIdx.x == 0) out[idx[blockIdx.x]] = total;
}

hipError_t launch_mps_pauli_fused(const MpsPauliFusedArgs& a, int npairs, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_pauli_fused_kernel>();
    if (e != hipSuccess) return e;
    if (npairs <= 0 || a.nstrings <= 0) return hipSuccess;
    mps_pauli_fused_kernel<<<dim3(a.nstrings, npairs), 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_pauli_dress(const double2* const* sites, const int* dims, const size_t* site_off, int n, size_t total, int max_site_elems, void* out,
                                  hipStream_t s) {
    if (n <= 0 || max_site_elems <= 0) return hipSuccess;
    mps_pauli_dress_kernel<<<dim3((unsigned)((max_site_elems + 255) / 256), n), 256, 0, s>>>(sites, dims, site_off, total, static_cast<cplx*>(out));
    return hipGetLastError();
}

hipError_t launch_mps_pauli_close(const void* const* m_tab, const void* const* r_tab, const int* idx, int count, int chi, void* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    mps_pauli_close_kernel<<<count, 256, 0, s>>>(reinterpret_cast<const cplx* const*>(m_tab), reinterpret_cast<const cplx* const*>(r_tab), idx, chi,
                                                 static_cast<cplx*>(out));
    return hipGetLastError();
}

}  // namespace aqc
