// Pair density matrices of MPS states (rules and notation: aqc_mps_obs_rule.h; host side: aqc_mps_obs_api.cpp).
//
// Both routes leave, per emission (chain i read at site j) and component of E, four complex sums
//     sums[emit][ecomp][k]      = sum_xy E^{ecomp}[x][y] K^{k}[y][x]     k = 0, 1, 2  (components 00, 01, 11 of K)
//     sums[emit][ecomp = 1][3]  = sum_xy conj(E^{01}[y][x]) K^{01}[y][x]               (the entry that needs E^{10} = (E^{01})^H)
// from which the host takes the upper triangle of the 4 x 4 and mirrors it (mps_obs_upper).  Every sum runs in a fixed order that depends
// on the state's bond dimensions only: no atomics, and a matrix does not depend on which other pairs or states are in the call.
//
// gemm route (any bond dimension): E, K come from zgemm launches (aqc_mps.hip); mps_obs_sums_kernel forms the sums, a workgroup per
// emission.
//
// fused route (every bond <= kMpsObsFusedCap = 64): one workgroup per (chain, component) walks its whole chain inside one launch.  E
// lives in LDS as split re / im planes [64][kLd]; the step across site q is, per physical index c,
//     F_c = E T_q[c]   (MFMA, A operand = E from LDS, B operand = T_q[c] streamed from memory)      -> LDS planes
//     W_cc = T_q[c]^H F_c   (MFMA, A operand = conj T_q[c] streamed from memory, B operand = F_c from LDS)
// and E' = W_00 + W_11 goes back into the E planes.  At an emitting site the closing tensors are never formed: with
// K^{cd} = T_j[c] R_{j+1} T_j[d]^H,
//     sum_xy E[x][y] K^{cd}[y][x] = sum_uv (T_j[d]^H E T_j[c])[u][v] R_{j+1}[v][u] = sum_uv W_cd[u][v] R[v][u]
// so the sums are read off the step's own products (W_00, W_11) and one more, W_01 = T_j[1]^H F_0 (component 01 also W_10 for its
// adjoint entry), straight from the accumulators.  The plane products are those of aqc_mps_planes.h (shared with aqc_mps_sample.hip).
// Operand layout of v_mfma_f64_16x16x4_f64: top of aqc_mps.hip; wave w owns rows
// [16w, 16w + 16) of a product and all four 16-column tiles.  Operand tiles are zero-filled beyond the bond dimensions, so accumulators
// there are exact zeros and whole tiles are stored; reads never leave the tiles written for the current dimensions.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_obs_rule.h"
#include "aqc_mps_planes.h"

namespace aqc {

namespace {

// the chi x chi corner of acc to memory, row-major (cj: conjugated)
__device__ __forceinline__ void acc_store_global(const Acc& acc, cplx* __restrict__ out, int chi, bool cj) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    if (16 * wave >= chi) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (16 * t >= chi) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = 16 * wave + 4 * r + lk, v = 16 * t + li;
            if (u < chi && v < chi) out[(size_t)u * chi + v] = make_double2(acc.re[t][r], cj ? -acc.im[t][r] : acc.im[t][r]);
        }
    }
}

// one environment step on the planes: E <- sum_c S_c^H E S_c with S_c = T_c [din][dout] (TR: S_c = T_c^T, memory holds [dout][din]); the
// new E also goes to `out` (conjugated for the right sweep, whose planes hold conj R)
template <bool TR>
__device__ __forceinline__ void env_step(double* er, double* ei, double* fr, double* fi, const cplx* __restrict__ T0, const cplx* __restrict__ T1,
                                         int din, int dout, cplx* __restrict__ out) {
    Acc acc, tmp;
    prod_lds_mem<TR>(er, ei, T0, din, din, dout, tmp);
    acc_store(tmp, fr, fi, din, dout);
    __syncthreads();
    prod_memh_lds<TR>(T0, fr, fi, dout, din, dout, acc);
    __syncthreads();   // F_0 has been read
    prod_lds_mem<TR>(er, ei, T1, din, din, dout, tmp);
    acc_store(tmp, fr, fi, din, dout);
    __syncthreads();   // (also: every wave is done reading E)
    prod_memh_lds<TR>(T1, fr, fi, dout, din, dout, tmp);
#pragma unroll
    for (int t = 0; t < 4; ++t) { acc.re[t] += tmp.re[t]; acc.im[t] += tmp.im[t]; }
    acc_store(acc, er, ei, dout, dout);
    acc_store_global(acc, out, dout, TR);
    __syncthreads();
}

}  // namespace

// The environments of <psi|psi> for bonds <= 64, two workgroups: block 0 sweeps L_1 .. L_{n-1} from the left, block 1 sweeps
// R_{n-1} .. R_1 from the right (its planes hold conj R: conj R_q = sum_c S_c^H conj(R_{q+1}) S_c with S_c = T_q[c]^T, the same step
// with the site read transposed).  L_0 = R_n = [1] are written by the host.
__global__ __launch_bounds__(256) void mps_obs_env_kernel(MpsObsFusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double obs_smem[];
    double* er = obs_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const bool right = blockIdx.x == 1;
    for (int e = threadIdx.x; e < 4 * kPlane; e += 256) obs_smem[e] = e == 0 ? 1.0 : 0.0;
    __syncthreads();
    for (int s = 0; s + 1 < a.n; ++s) {
        const int q = right ? a.n - 1 - s : s;
        const int dl = a.dims[q], dr = a.dims[q + 1];
        const cplx* T0 = a.sites[q];
        const cplx* T1 = T0 + (size_t)dl * dr;
        if (right) env_step<true>(er, ei, fr, fi, T0, T1, dr, dl, a.env_r + a.env_off[q]);
        else env_step<false>(er, ei, fr, fi, T0, T1, dl, dr, a.env_l + a.env_off[q + 1]);
    }
}

// grid (3 components, chains); 256 threads; dynamic LDS kFusedLds
__global__ __launch_bounds__(256) void mps_obs_fused_kernel(MpsObsFusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double obs_smem[];
    __shared__ double red[8];
    double* er = obs_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const int comp = blockIdx.x, chain = blockIdx.y, tid = threadIdx.x;
    const int start = a.chain_start[chain], last = a.chain_last[chain];
    for (int e = tid; e < 4 * kPlane; e += 256) obs_smem[e] = 0.0;
    __syncthreads();
    Acc acc, tmp;
    {   // opening: E^{ab} = T_b^H (L_start T_a); components 00, 01 (a = 0, b = 1), 11
        const int chil = a.dims[start], chir = a.dims[start + 1];
        const cplx* L = a.env_l + a.env_off[start];
        for (int e = tid; e < chil * chil; e += 256) {
            const cplx v = L[e];
            const int x = e / chil, y = e - x * chil;
            er[x * kLd + y] = v.x;
            ei[x * kLd + y] = v.y;
        }
        __syncthreads();
        const cplx* T = a.sites[start];
        const int ca = comp == 2 ? 1 : 0, cb = comp == 0 ? 0 : 1;
        prod_lds_mem(er, ei, T + (size_t)ca * chil * chir, chil, chil, chir, acc);
        acc_store(acc, fr, fi, chil, chir);
        __syncthreads();
        prod_memh_lds(T + (size_t)cb * chil * chir, fr, fi, chir, chil, chir, acc);
        __syncthreads();   // (every wave has read L out of the E planes and F)
        acc_store(acc, er, ei, chir, chir);
        __syncthreads();
    }
    for (int q = start + 1; q <= last; ++q) {
        const int chil = a.dims[q], chir = a.dims[q + 1];
        const cplx* T0 = a.sites[q];
        const cplx* T1 = T0 + (size_t)chil * chir;
        const int emit = a.emit_of[(size_t)chain * a.n + q];
        const cplx* R = a.env_r + a.env_off[q + 1];
        cplx* out = emit >= 0 ? a.sums + ((size_t)emit * kMpsObsComps + comp) * 4 : nullptr;
        double re, im;
        // c = 0
        prod_lds_mem(er, ei, T0, chil, chil, chir, tmp);
        acc_store(tmp, fr, fi, chil, chir);
        __syncthreads();
        prod_memh_lds(T0, fr, fi, chir, chil, chir, acc);            // W_00
        if (emit >= 0) {
            acc_dot(acc, R, chir, false, re, im);
            const cplx s0 = block_sum(re, im, red);
            prod_memh_lds(T1, fr, fi, chir, chil, chir, tmp);        // W_01 = T_1^H F_0
            acc_dot(tmp, R, chir, false, re, im);
            const cplx s1 = block_sum(re, im, red);
            if (tid == 0) { out[0] = s0; out[1] = s1; }
        }
        __syncthreads();   // F_0 has been read
        // c = 1
        prod_lds_mem(er, ei, T1, chil, chil, chir, tmp);
        acc_store(tmp, fr, fi, chil, chir);
        __syncthreads();   // (also: every wave is done reading E)
        prod_memh_lds(T1, fr, fi, chir, chil, chir, tmp);            // W_11
        if (emit >= 0) {
            acc_dot(tmp, R, chir, false, re, im);
            const cplx s2 = block_sum(re, im, red);
            cplx s3 = make_double2(0.0, 0.0);
            if (comp == 1) {
                Acc w10;
                prod_memh_lds(T0, fr, fi, chir, chil, chir, w10);    // W_10 = T_0^H F_1; the adjoint entry reads (W_10)^H
                acc_dot(w10, R, chir, true, re, im);
                s3 = block_sum(re, im, red);
            }
            if (tid == 0) { out[2] = s2; out[3] = s3; }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) { acc.re[t] += tmp.re[t]; acc.im[t] += tmp.im[t]; }
        acc_store(acc, er, ei, chir, chir);
        __syncthreads();   // E' is in place; F_1 has been read
    }
}

// gemm route: grid (emissions of one site); E slots [slot][3][slot_stride] (chi x chi each), K [3][k_stride]
__global__ __launch_bounds__(256) void mps_obs_sums_kernel(const cplx* __restrict__ e_base, const int* __restrict__ slots, const int* __restrict__ emits,
                                                           size_t slot_stride, const cplx* __restrict__ k_base, size_t k_stride, int chi,
                                                           cplx* __restrict__ sums) {
    __shared__ double red[8];
    const cplx* E = e_base + (size_t)slots[blockIdx.x] * kMpsObsComps * slot_stride;
    cplx* out = sums + (size_t)emits[blockIdx.x] * kMpsObsComps * 4;
    const size_t count = (size_t)chi * chi;
    for (int ec = 0; ec < kMpsObsComps; ++ec)
        for (int k = 0; k < 4; ++k) {
            const bool adj = k == 3;
            cplx total = make_double2(0.0, 0.0);
            if (!adj || ec == 1) {
                const cplx* e = E + (size_t)ec * slot_stride;
                const cplx* kk = k_base + (size_t)(adj ? 1 : k) * k_stride;
                double re = 0.0, im = 0.0;
                for (size_t i = threadIdx.x; i < count; i += 256) {
                    const int x = (int)(i / chi), y = (int)(i - (size_t)x * chi);
                    cplx ev = e[i];                                           // E[x][y]
                    cplx kv = kk[(size_t)y * chi + x];                        // K[y][x]
                    if (adj) { ev.y = -ev.y; kv = kk[i]; }                    // conj(E[x][y]) K[x][y]
                    re += ev.x * kv.x - ev.y * kv.y;
                    im += ev.x * kv.y + ev.y * kv.x;
                }
                total = block_sum(re, im, red);
            }
            if (threadIdx.x == 0) out[ec * 4 + k] = total;
        }
}

namespace {
constexpr auto grant_planes = grant_dynamic_lds<kFusedLds, mps_obs_fused_kernel, mps_obs_env_kernel>;
}  // namespace

hipError_t launch_mps_obs_env(const MpsObsFusedArgs& a, hipStream_t s) {
    const hipError_t e = grant_planes();
    if (e != hipSuccess) return e;
    mps_obs_env_kernel<<<2, 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_obs_fused(const MpsObsFusedArgs& a, int nchains, hipStream_t s) {
    const hipError_t e = grant_planes();
    if (e != hipSuccess) return e;
    if (nchains <= 0) return hipSuccess;
    mps_obs_fused_kernel<<<dim3(kMpsObsComps, nchains), 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_obs_sums(const void* e_base, const int* slots, const int* emits, int count, size_t slot_stride, const void* k_base, size_t k_stride,
                               int chi, void* sums, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    mps_obs_sums_kernel<<<count, 256, 0, s>>>(static_cast<const cplx*>(e_base), slots, emits, slot_stride, static_cast<const cplx*>(k_base), k_stride, chi,
                                              static_cast<cplx*>(sums));
    return hipGetLastError();
}

}  // namespace aqc
