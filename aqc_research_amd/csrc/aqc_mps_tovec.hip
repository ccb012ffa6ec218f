// MPS states into dense vectors and into blocks of amplitudes, fused route (rules and notation: aqc_mps_tovec_rule.h; host side:
// aqc_mps_tovec_api.cpp): every bond <= kCap = 64, all states of a chunk in every launch whatever their bonds are -- the dimensions are
// read from the call's table, the grids are sized by what the host knows of n.
//
//   head   grid (halves, lanes), four planes.  The first steps of a half, while its factor has at most 64 rows: the factor stays in one
//          pair of planes, both bit products L T_q[b] (low half) or H T_q[b]^T (high half, prod_lds_mem<true>) are formed on the matrix
//          cores and stored into the other pair at the doubled row index: b 2^j + l for the low half (the new site is the highest bit of
//          l), 2 r + b for the high half (the new site is the lowest bit of r, so r ends in the register's bit order).  The result goes to
//          store 0 of the half, packed [rows][chi].
//   step   grid (tiles of 64 rows, halves, lanes), two planes.  One further site: a workgroup loads 64 rows of the factor, forms both
//          products and writes them with acc_to_mem at the doubled row index into the half's other store.
//   rows   grid (tiles of 64 listed rows, lanes), four planes.  Blocks only: V [64][chi] walks from site n - 1 down to site k, both
//          products V T_q[b]^T per site, every row keeps the one of its own bit (the select of aqc_mps_sample.hip).  Result: store 0 of the
//          high half, [rows][chi_k].
//   outer  grid (column groups, row tiles, lanes), two planes.  out[r 2^k + l] = sum_j H[r][j] L[l][j]: the tile of 64 rows of H goes into
//          the planes once, L streams as the memory-side operand in chunks of 64 rows (read transposed), and the accumulators go straight
//          to the output lane with leading dimension 2^k: 16-byte stores, a wave writes 16 rows of 1 KiB per chunk.  No scratch copy of
//          the vector exists.
// No atomics, no loop bound that depends on data, every sum in the fixed order of the k-steps of prod_lds_mem.  Operand tiles are zero
// beyond the bonds; rows of a tile beyond the factor's are computed and never stored.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_planes.h"
#include "aqc_mps_tovec_rule.h"

namespace aqc {

namespace {

constexpr size_t kPairLds = sizeof(double) * 2 * kPlane;   // one pair of planes: 67584 bytes
static_assert(kMpsToVecTile == kCap, "a tile of rows fills the planes");

struct Lane {
    const cplx* const* sites;
    cplx* const* bufs;     // low store 0, 1, high store 0, 1, output
    const int* dims;       // n + 1, then the route
};
__device__ __forceinline__ Lane lane_of(const MpsToVecArgs& a, int z) {
    const unsigned long long* rec = a.table + (size_t)(a.first + z) * a.per;
    return Lane{reinterpret_cast<const cplx* const*>(rec + a.at_sites), reinterpret_cast<cplx* const*>(rec + a.at_bufs),
                reinterpret_cast<const int*>(rec + a.at_dims)};
}
__device__ __forceinline__ bool lane_fused(const MpsToVecArgs& a, const Lane& l) { return l.dims[a.n + 1] == kMpsToVecFused; }

__device__ __forceinline__ void pair_zero(double* smem) {
    for (int e = threadIdx.x; e < 2 * kPlane; e += 256) smem[e] = 0.0;
}

// rows below `rows` of acc into the planes at row 2 i + b (interleave) or b rows + i, whole column tiles below nn
__device__ __forceinline__ void acc_store_doubled(const Acc& acc, double* pr, double* pi, int rows, int nn, int b, bool interleave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (16 * t >= nn) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * wave + 4 * r + lk;
            if (i >= rows) continue;
            const int at = (interleave ? 2 * i + b : b * rows + i) * kLd + 16 * t + li;   // 2 rows <= kCap
            pr[at] = acc.re[t][r];
            pi[at] = acc.im[t][r];
        }
    }
}

// the site of step j of a half, and the bond the factor has before and after it
struct Step { const cplx *t0, *t1; int chi_in, chi_out; };
__device__ __forceinline__ Step step_of(const MpsToVecArgs& a, const Lane& l, bool high, int j) {
    const int q = high ? a.n - 1 - j : j;
    const int x = l.dims[q], u = l.dims[q + 1];
    const cplx* t0 = l.sites[q];
    return Step{t0, t0 + (size_t)x * u, high ? u : x, high ? x : u};
}

}  // namespace

__global__ __launch_bounds__(256) void mps_tovec_head_kernel(MpsToVecArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tovec_smem[];
    const Lane l = lane_of(a, blockIdx.y);
    if (!lane_fused(a, l)) return;
    const bool high = blockIdx.x == 1;
    const int len = high ? a.high_len : a.low_len;
    const int steps = len < kMpsToVecHeadSteps ? len : (int)kMpsToVecHeadSteps;
    double* cr = tovec_smem;
    double* ci = cr + kPlane;
    double* nr = ci + kPlane;
    double* ni = nr + kPlane;
    planes_zero(tovec_smem);
    __syncthreads();
    if (threadIdx.x == 0) cr[0] = 1.0;   // the factor of no sites: [1]
    __syncthreads();
    Acc acc;
    int chi = 1;
    for (int j = 0; j < steps; ++j) {
        const Step s = step_of(a, l, high, j);
        const int rows = 1 << j;
        for (int b = 0; b < 2; ++b) {
            if (high) prod_lds_mem<true>(cr, ci, b ? s.t1 : s.t0, rows, s.chi_in, s.chi_out, acc);
            else prod_lds_mem<false>(cr, ci, b ? s.t1 : s.t0, rows, s.chi_in, s.chi_out, acc);
            acc_store_doubled(acc, nr, ni, rows, s.chi_out, b, high);
        }
        __syncthreads();   // the new factor is whole; every wave has read the old one
        double* t = cr; cr = nr; nr = t;
        t = ci; ci = ni; ni = t;
        chi = s.chi_out;
    }
    cplx* dst = l.bufs[high ? 2 : 0];
    const int total = (1 << steps) * chi;   // <= kCap * kCap
    for (int e = threadIdx.x; e < total; e += 256) {
        const int i = e / chi, c = e - i * chi;
        dst[e] = make_double2(cr[i * kLd + c], ci[i * kLd + c]);
    }
}

__global__ __launch_bounds__(256) void mps_tovec_step_kernel(MpsToVecArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tovec_smem[];
    const Lane l = lane_of(a, blockIdx.z);
    if (!lane_fused(a, l)) return;
    const bool high = blockIdx.y == 1;
    const int j = a.step, len = high ? a.high_len : a.low_len;
    const size_t rows = (size_t)1 << j, row0 = (size_t)blockIdx.x * kMpsToVecTile;
    if (j >= len || row0 >= rows) return;   // (uniform over the workgroup)
    const Step s = step_of(a, l, high, j);
    const int from = (j - kMpsToVecHeadSteps) & 1;
    const cplx* src = l.bufs[(high ? 2 : 0) + from];
    cplx* dst = l.bufs[(high ? 2 : 0) + (from ^ 1)];
    double* er = tovec_smem;
    double* ei = er + kPlane;
    pair_zero(tovec_smem);
    __syncthreads();
    plane_load(src + row0 * s.chi_in, kMpsToVecTile, s.chi_in, er, ei);   // rows >= 64: the tile is whole
    __syncthreads();
    Acc acc;
    for (int b = 0; b < 2; ++b) {
        if (high) {
            prod_lds_mem<true>(er, ei, b ? s.t1 : s.t0, kMpsToVecTile, s.chi_in, s.chi_out, acc);
            acc_to_mem(acc, dst + (2 * row0 + b) * s.chi_out, 2 * s.chi_out, kMpsToVecTile, s.chi_out);
        } else {
            prod_lds_mem<false>(er, ei, b ? s.t1 : s.t0, kMpsToVecTile, s.chi_in, s.chi_out, acc);
            acc_to_mem(acc, dst + (b * rows + row0) * s.chi_out, s.chi_out, kMpsToVecTile, s.chi_out);
        }
    }
}

__global__ __launch_bounds__(256) void mps_tovec_rows_kernel(MpsToVecArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tovec_smem[];
    const Lane l = lane_of(a, blockIdx.y);
    if (!lane_fused(a, l)) return;
    double* vr = tovec_smem;
    double* vi = vr + kPlane;
    double* wr = vi + kPlane;
    double* wi = wr + kPlane;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    planes_zero(tovec_smem);
    __syncthreads();
    if (tid < kCap) vr[tid * kLd] = 1.0;   // v = [1] in every row
    __syncthreads();
    const long long row0 = (long long)blockIdx.x * kMpsToVecTile;
    const int width = a.n - a.k;
    Acc acc;
    for (int q = a.n - 1; q >= a.k; --q) {
        const int x = l.dims[q], u = l.dims[q + 1];
        const cplx* t0 = l.sites[q];
        prod_lds_mem<true>(vr, vi, t0, kCap, u, x, acc);
        acc_store(acc, wr, wi, kCap, x);
        prod_lds_mem<true>(vr, vi, t0 + (size_t)x * u, kCap, u, x, acc);
        __syncthreads();   // every wave has read V
        acc_store(acc, vr, vi, kCap, x);
        __syncthreads();
        // V holds the product of bit 1: the rows whose bit is 0 take theirs from the W planes, whole tiles
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = row0 + 16 * wave + 4 * r + lk;
            const bool one = row < a.high_rows && a.high_bits[(size_t)row * width + (q - a.k)] != 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t >= x || one) continue;
                const int at = (16 * wave + 4 * r + lk) * kLd + 16 * t + li;
                vr[at] = wr[at];
                vi[at] = wi[at];
            }
        }
        __syncthreads();   // V' is in place; W has been read
    }
    const int chi = l.dims[a.k];
    cplx* dst = l.bufs[2] + (size_t)row0 * chi;
    const long long left = a.high_rows - row0;
    const int rows = left < kMpsToVecTile ? (int)left : (int)kMpsToVecTile;
    for (int e = tid; e < rows * chi; e += 256) {
        const int i = e / chi, c = e - i * chi;
        dst[e] = make_double2(vr[i * kLd + c], vi[i * kLd + c]);
    }
}

__global__ __launch_bounds__(256) void mps_tovec_outer_kernel(MpsToVecArgs a) {
    extern __shared__ __attribute__((aligned(16))) double tovec_smem[];
    const Lane l = lane_of(a, blockIdx.z);
    if (!lane_fused(a, l)) return;
    const int chi = l.dims[a.k];
    const cplx* H = l.bufs[2 + a.high_store];
    const cplx* L = l.bufs[a.low_store];
    cplx* out = l.bufs[4];
    const long long r0 = (long long)blockIdx.y * kMpsToVecTile, left = a.high_rows - r0;
    const int nrows = left < kMpsToVecTile ? (int)left : (int)kMpsToVecTile;   // >= 1: the grid has no tile beyond the rows
    const size_t cols = (size_t)1 << a.k;
    double* er = tovec_smem;
    double* ei = er + kPlane;
    pair_zero(tovec_smem);
    __syncthreads();
    plane_load(H + (size_t)r0 * chi, nrows, chi, er, ei);
    __syncthreads();
    Acc acc;
    for (int c = 0; c < kMpsToVecChunksPerBlock; ++c) {
        const size_t l0 = ((size_t)blockIdx.x * kMpsToVecChunksPerBlock + c) * kMpsToVecTile;
        if (l0 >= cols) break;
        const int ncols = cols - l0 < kMpsToVecTile ? (int)(cols - l0) : (int)kMpsToVecTile;
        prod_lds_mem<true>(er, ei, L + l0 * chi, nrows, chi, ncols, acc);
        acc_to_mem(acc, out + (size_t)r0 * cols + l0, (int)cols, nrows, ncols);
    }
}

hipError_t launch_mps_tovec_head(const MpsToVecArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_tovec_head_kernel, mps_tovec_rows_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    mps_tovec_head_kernel<<<dim3(a.high_len > 0 ? 2 : 1, (unsigned)count), 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_tovec_step(const MpsToVecArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kPairLds, mps_tovec_step_kernel, mps_tovec_outer_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0) return hipSuccess;
    const unsigned tiles = (unsigned)mps_tovec_tiles((size_t)1 << a.step);
    mps_tovec_step_kernel<<<dim3(tiles, a.high_len > 0 ? 2 : 1, (unsigned)count), 256, kPairLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_tovec_rows(const MpsToVecArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_tovec_head_kernel, mps_tovec_rows_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0 || a.high_rows <= 0) return hipSuccess;
    mps_tovec_rows_kernel<<<dim3((unsigned)mps_tovec_tiles((size_t)a.high_rows), (unsigned)count), 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_tovec_outer(const MpsToVecArgs& a, int count, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kPairLds, mps_tovec_step_kernel, mps_tovec_outer_kernel>();
    if (e != hipSuccess) return e;
    if (count <= 0 || a.high_rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)mps_tovec_col_groups(a.k), (unsigned)mps_tovec_row_tiles((size_t)a.high_rows), (unsigned)count);
    mps_tovec_outer_kernel<<<grid, 256, kPairLds, s>>>(a);
    return hipGetLastError();
}

}  // namespace aqc
