// Schmidt spectra of MPS states, fused route (rules and notation: aqc_mps_ent_rule.h; host side: aqc_mps_ent_api.cpp).
//
// mps_ent_chain_kernel, grid (2, states): block x = 0 walks the left factors C_1 .. C_{n-1}, block x = 1 the right factors
// D_{n-1} .. D_1 (grid (1, states) with walk0 = 1: the right walk alone, what aqc_mps_compress.hip starts from), each its whole chain inside one launch.  The factor (chi x chi, upper triangular) lives in the E planes of
// aqc_mps_planes.h.  The step across site q with chi_in bonds on the factor's side and chi_out on the other:
//     P_0 = F T_q[0], P_1 = F T_q[1]        (MFMA, A operand = the factor from LDS, B operand = the site streamed from memory; the right
//                                            walk reads the site transposed) into two accumulator sets;
//     after a barrier P_0 goes to the F planes and P_1 overwrites the E planes: the four planes hold the stacked 2 chi_in x chi_out
//     matrix, logical row r in F at r < chi_in and in E at r - chi_in (mps_ent_stacked_row);
//     Householder in place in LDS, column by column (mps_ent_reflection; householder_lds of aqc_mps_householder.h): a thread owns column c = tid % 64 for the rows
//     j + tid / 64, + 4, ...; the four partial inner products of a column are added in a fixed order; the norm of the next column
//     is taken by the threads that have just updated it, so a column costs three barriers;
//     the leading rows are gathered back into the E planes as the next factor, zero-filled to the whole 64 x 64, and written to memory.
// No loop bound depends on data, only on bond dimensions: a state of NaNs runs to its end and leaves NaN factors.  No atomics.
//
// mps_ent_cut_kernel, one workgroup per (state, cut) of a chunk: C_q into planes, S_q = C_q D_q^T with the D operand streamed
// transposed, stored as matrix i of the [count][K][K] store of the batched SVD (aqc_svd_batch.hip), rows[i] = cols[i] = chi_q.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_ent_rule.h"
#include "aqc_mps_householder.h"
#include "aqc_mps_planes.h"

namespace aqc {

static_assert((int)kMpsEntFusedCap == (int)kMpsObsFusedCap, "the planes of aqc_mps_planes.h are sized by the observables' cap");

namespace {

constexpr size_t kEntCutLds = sizeof(double) * 2 * kPlane;
}  // namespace

// grid (2, states); 256 threads; dynamic LDS kFusedLds
__global__ __launch_bounds__(256) void mps_ent_chain_kernel(MpsEntChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ent_smem[];
    __shared__ double v[2 * kEntRows], wp[8 * kCap], np[4];
    double* er = ent_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const bool right = blockIdx.x + a.walk0 == 1;
    const MpsEntState st = a.states[blockIdx.y];
    const int n = a.n, tid = threadIdx.x;
    cplx* out_base = st.factors + (right ? st.fac_off[n] : 0);
    for (int e = tid; e < 4 * kPlane; e += 256) ent_smem[e] = e == 0 ? 1.0 : 0.0;   // the factor of the boundary: [1]
    __syncthreads();
    for (int s = 0; s + 1 < n; ++s) {
        const int q = right ? n - 1 - s : s;
        const int chi_in = right ? st.dims[q + 1] : st.dims[q], chi_out = right ? st.dims[q] : st.dims[q + 1];
        const cplx* T0 = st.sites[q];
        const cplx* T1 = T0 + (size_t)st.dims[q] * st.dims[q + 1];
        {
            Acc p0, p1;
            if (right) {
                prod_lds_mem<true>(er, ei, T0, chi_in, chi_in, chi_out, p0);
                prod_lds_mem<true>(er, ei, T1, chi_in, chi_in, chi_out, p1);
            } else {
                prod_lds_mem<false>(er, ei, T0, chi_in, chi_in, chi_out, p0);
                prod_lds_mem<false>(er, ei, T1, chi_in, chi_in, chi_out, p1);
            }
            __syncthreads();   // every wave is done reading the factor
            acc_store(p0, fr, fi, chi_in, chi_out);
            acc_store(p1, er, ei, chi_in, chi_out);
        }
        __syncthreads();
        householder_lds(ent_smem, chi_in, chi_out, v, wp, np);
        // the next factor: the upper triangle of the leading rows, zero elsewhere in the whole 64 x 64
        const int rrows = mps_ent_r_rows(2 * chi_in, chi_out);
        double gr[kCap * kCap / 256], gi[kCap * kCap / 256];
#pragma unroll
        for (int k = 0; k < kCap * kCap / 256; ++k) {
            const int e = tid + 256 * k, i = e >> 6, c = e & (kCap - 1);
            const bool keep = i < rrows && c >= i && c < chi_out;
            const int at = keep ? stacked_at(i, c, chi_in) : 0;
            gr[k] = keep ? ent_smem[at] : 0.0;
            gi[k] = keep ? ent_smem[at + kPlane] : 0.0;
        }
        __syncthreads();
        cplx* out = out_base + st.fac_off[right ? q : q + 1];   // the factor of bond q (right) or q + 1 (left): chi_out x chi_out
#pragma unroll
        for (int k = 0; k < kCap * kCap / 256; ++k) {
            const int e = tid + 256 * k, i = e >> 6, c = e & (kCap - 1);
            er[i * kLd + c] = gr[k];
            ei[i * kLd + c] = gi[k];
            if (i < chi_out && c < chi_out) out[(size_t)i * chi_out + c] = make_double2(gr[k], gi[k]);
        }
        __syncthreads();
    }
}

// grid (matrices of the chunk); 256 threads; dynamic LDS kEntCutLds
__global__ __launch_bounds__(256) void mps_ent_cut_kernel(MpsEntCutArgs a) {
    extern __shared__ __attribute__((aligned(16))) double ent_smem[];
    double* er = ent_smem;
    double* ei = er + kPlane;
    const int item = blockIdx.x, tid = threadIdx.x;
    const int q = a.cut[a.first + item];
    const MpsEntState st = a.states[a.state[a.first + item]];
    const int chi = st.dims[q];
    const cplx* C = st.factors + st.fac_off[q];
    const cplx* D = st.factors + st.fac_off[a.n] + st.fac_off[q];
    for (int e = tid; e < 2 * kPlane; e += 256) ent_smem[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < chi * chi; e += 256) {
        const cplx x = C[e];
        const int i = e / chi, c = e - i * chi;
        er[i * kLd + c] = x.x;
        ei[i * kLd + c] = x.y;
    }
    __syncthreads();
    Acc acc;
    prod_lds_mem<true>(er, ei, D, chi, chi, chi, acc);   // S[i][j] = sum_k C[i][k] D[j][k]
    cplx* S = a.a + (size_t)item * a.k * a.k;
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * wave + 4 * r + lk, j = 16 * t + li;
            if (i < chi && j < chi) S[(size_t)i * a.k + j] = make_double2(acc.re[t][r], acc.im[t][r]);   // chi <= a.k
        }
    if (tid == 0) { a.rows[item] = chi; a.cols[item] = chi; }
}

hipError_t launch_mps_ent_chain(const MpsEntChainArgs& a, int nstates, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_ent_chain_kernel>();
    if (e != hipSuccess) return e;
    if (nstates <= 0 || a.n < 2) return hipSuccess;
    mps_ent_chain_kernel<<<dim3(2, nstates), 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_ent_chain_right(const MpsEntChainArgs& a, int nstates, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_ent_chain_kernel>();
    if (e != hipSuccess) return e;
    if (nstates <= 0 || a.n < 2) return hipSuccess;
    MpsEntChainArgs r = a;
    r.walk0 = 1;
    mps_ent_chain_kernel<<<dim3(1, nstates), 256, kFusedLds, s>>>(r);
    return hipGetLastError();
}

hipError_t launch_mps_ent_cut(const MpsEntCutArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kEntCutLds, mps_ent_cut_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    mps_ent_cut_kernel<<<count, 256, kEntCutLds, s>>>(a);
    return hipGetLastError();
}

}  // namespace aqc
