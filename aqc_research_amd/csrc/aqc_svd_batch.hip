// Batched complex SVD by BLOCK one-sided Jacobi on the fp64 matrix cores: many two-site matrices per call, one workgroup per matrix
// (the step of mps_operations.py:252-257 for many lanes at once).  Conventions of aqc_svd.hip: the work matrix W is column-major,
// rotations are accumulated in V, on exit W = A V and sigma_j = |W_j|, sorted descending; a wide matrix goes through its conjugate
// transpose; a column below kNegligible2 |A|_F^2 is left alone.
// The columns are cut into blocks of 16 (csrc/aqc_svd_blocks.h: blocks, tournament, transposition, LDS bytes).  For a block pair:
//   G = P^H P of the panel's <= 32 columns by v_mfma_f64_16x16x4_f64, complex by three real products;
//   converged when every |g_pq|^2 <= tol^2 g_pp g_qq -- then nothing is touched;
//   otherwise G is diagonalised in LDS by cyclic two-sided Jacobi (kSvdbInnerSweeps sweeps of 31 rounds x 16 disjoint pairs; G is
//   formed afresh at the next visit, and more inner sweeps save no outer ones), the accumulated 32 x 32 J is brought back to a
//   unitary by one Newton-Schulz step, and J is applied to the panel's columns of W and of V as matrix-core products.
// G is recomputed from W at every visit, so what the Gram step loses on graded columns costs sweeps, not the accuracy of values and
// reconstruction.  There is no closing step of scalar sweeps: with the Newton-Schulz step the NumPy statement of this rule
// (tests/svd_block_ref.py) meets the bounds of the scalar routes at every size up to 256 x 256; without it V collects J's defect
// at every visit and |V V^H - 1| passes its bound at 256 rows.
// Deterministic: fixed pair order, fixed-order reductions, no float atomics; a matrix never reads another matrix's data.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/aqc_hip.h"
#include "aqc_devbuf.h"
#include "aqc_launch.h"
#include "aqc_math.h"
#include "aqc_mps_dev.h"
#include "aqc_svd_blocks.h"

namespace aqc {

typedef double svdb_d4 __attribute__((ext_vector_type(4)));

struct SvdBatchArgs {
    const cplx* a; cplx* u; double* s; cplx* vh; int* sweeps; int* status;
    const int* rows; const int* cols;   // null: all m / n
    cplx* W;                            // [count][k][ld] column-major work matrices
    cplx* V;                            // [count][k][k]
    int m, n, k, ld;
    double tol;
};

// (c, s e) of the rotation that diagonalises [[a, g], [conj(g), b]]: x' = c x - (s e) y, y' = conj(s e) x + c y
__device__ __forceinline__ bool svdb_rotation(double a, double b, cplx g, double tol, double negligible, double* c, double* sr, double* si) {
    const double g2 = g.x * g.x + g.y * g.y;
    if (!(g2 > tol * tol * a * b && g2 != 0.0 && fmin(a, b) > negligible)) return false;
    const double d = b - a, h = sqrt(d * d + 4.0 * g2);
    const double u2 = 2.0 / (fabs(d) + h);
    const double cc = 1.0 / sqrt(1.0 + g2 * u2 * u2);
    const double f = d >= 0.0 ? cc * u2 : -cc * u2;
    *c = cc; *sr = f * g.x; *si = -f * g.y;
    return true;
}

__global__ __launch_bounds__(kSvdbThreads) void svd_batch_kernel(const SvdBatchArgs p) {
    constexpr int N = kSvdbPanel;
    __shared__ cplx sG[N * N], sJ[N * N];            // column-major: (i, j) at j * 32 + i
    __shared__ double sRot[kSvdbBlock * 4];          // per pair of an inner round: c, re(s e), im(s e), rotate?
    __shared__ int sPQ[2 * kSvdbBlock], sCol[N];
    __shared__ double sSig[kSvdbMaxDim];
    __shared__ int sOrd[kSvdbMaxDim];
    __shared__ double sRed[kSvdbThreads / 64];
    static_assert(sizeof(sG) + sizeof(sJ) + sizeof(sRot) + sizeof(sPQ) + sizeof(sCol) + sizeof(sSig) + sizeof(sOrd) + sizeof(sRed) == svdb_lds_bytes(kSvdbMaxDim, kSvdbMaxDim),
                  "svdb_lds_bytes must count exactly the arrays above");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int rows = p.rows ? p.rows[b] : p.m, cols = p.cols ? p.cols[b] : p.n;
    if (rows < 1 || rows > p.m || cols < 1 || cols > p.n) {   // (the exported wrapper refuses these; a caller of the core gets status 2)
        if (tid == 0) { p.status[b] = kSvdbNonFinite; if (p.sweeps) p.sweeps[b] = 0; }
        return;
    }
    const int mode = svdb_mode(rows, cols), wr = svdb_work_rows(rows, cols), wc = svdb_work_cols(rows, cols), ld = p.ld, ldv = p.k;
    cplx* W = p.W + (size_t)b * p.k * ld;
    cplx* V = p.V + (size_t)b * p.k * p.k;
    const cplx* a = p.a + (size_t)b * p.m * p.n;

    // ---- load: W = A (mode 0) or A^H (mode 1), V = 1, |A|_F^2, non-finite entries
    double fr = 0.0;
    int bad = 0;
    for (int idx = tid; idx < rows * cols; idx += kSvdbThreads) {
        const int i = idx / cols, j = idx - i * cols;
        const cplx v = a[(size_t)i * p.n + j];
        if (!(isfinite(v.x) && isfinite(v.y))) bad = 1;
        fr += v.x * v.x + v.y * v.y;
        if (mode == 0) W[(size_t)j * ld + i] = v;
        else W[(size_t)i * ld + j] = make_double2(v.x, -v.y);
    }
    for (int idx = tid; idx < wc * wc; idx += kSvdbThreads) {
        const int c = idx / wc, r = idx - c * wc;
        V[(size_t)c * ldv + r] = make_double2(r == c ? 1.0 : 0.0, 0.0);
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) { p.status[b] = kSvdbNonFinite; if (p.sweeps) p.sweeps[b] = 0; }
        return;   // the outputs were zeroed before the launch
    }
    fr = wave_sum(fr);
    if (lane == 0) sRed[wave] = fr;
    __syncthreads();
    double fro2 = 0.0;
    for (int w = 0; w < kSvdbThreads / 64; ++w) fro2 += sRed[w];
    const double negligible = kNegligible2 * fro2, tol = p.tol;

    // ---- sweeps
    const int nb = svdb_blocks(wc), rounds = svdb_rounds(nb), slots = svdb_slots(nb);
    int sweep = 0, status = kSvdbSweepLimit;
    for (; sweep < kSvdbMaxSweeps; ++sweep) {
        int rotated_sweep = 0;
        for (int rs = 0; rs < rounds * slots; ++rs) {
            int bx, by;
            svdb_pair(nb, rs / slots, rs % slots, &bx, &by);
            __syncthreads();   // the previous pair is done with sCol, sG, sJ and its stores to W and V
            if (tid < N) {
                const int blk = tid < kSvdbBlock ? bx : by, c = blk * kSvdbBlock + (tid & (kSvdbBlock - 1));
                sCol[tid] = (blk >= 0 && c < wc) ? c : -1;
            }
            __syncthreads();
            // -- G = P^H P: wave 0 the tile (x, x), wave 1 (x, y), wave 2 (y, y); the rest follows from G = G^H
            if (wave < 3) {
                const int ti = wave == 2 ? 1 : 0, tj = wave == 0 ? 0 : 1, kq = lane >> 4;
                const int ca = sCol[ti * kSvdbBlock + (lane & 15)], cb = sCol[tj * kSvdbBlock + (lane & 15)];
                const cplx* pa = W + (size_t)(ca >= 0 ? ca : 0) * ld;
                const cplx* pb = W + (size_t)(cb >= 0 ? cb : 0) * ld;
                svdb_d4 t1 = {0.0, 0.0, 0.0, 0.0}, t2 = t1, t3 = t1;
                for (int r0 = 0; r0 < wr; r0 += 4) {
                    const int row = r0 + kq, rr = row < wr ? row : wr - 1;
                    cplx xa = pa[rr], xb = pb[rr];
                    if (ca < 0 || row >= wr) xa = make_double2(0.0, 0.0);
                    if (cb < 0 || row >= wr) xb = make_double2(0.0, 0.0);
                    // conj(xa) xb = (T1 + T2) + i (T3 - T1 + T2), T1 = ar br, T2 = ai bi, T3 = (ar - ai)(br + bi)
                    t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.x, xb.x, t1, 0, 0, 0);
                    t2 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.y, xb.y, t2, 0, 0, 0);
                    t3 = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.x - xa.y, xb.x + xb.y, t3, 0, 0, 0);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {   // D row 4 t + lane / 16 = i, D column lane % 16 = j
                    const int i = ti * kSvdbBlock + 4 * t + kq, j = tj * kSvdbBlock + (lane & 15);
                    sG[j * N + i] = make_double2(t1[t] + t2[t], t3[t] - t1[t] + t2[t]);
                }
            }
            __syncthreads();
            int need = 0;
            for (int e = tid; e < N * N; e += kSvdbThreads) {
                const int i = e & (N - 1), j = e >> 5;
                sJ[e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
                if (i > j) sG[e] = make_double2(sG[i * N + j].x, -sG[i * N + j].y);   // (reads the upper triangle only)
                else if (i == j) sG[e].y = 0.0;
            }
            __syncthreads();
            for (int e = tid; e < N * N; e += kSvdbThreads) {
                const int i = e & (N - 1), j = e >> 5;
                if (i < j) {
                    const cplx g = sG[e];
                    const double ga = sG[i * N + i].x, gb = sG[j * N + j].x, g2 = g.x * g.x + g.y * g.y;
                    if (g2 > tol * tol * ga * gb && g2 != 0.0 && fmin(ga, gb) > negligible) need = 1;
                }
            }
            if (!__syncthreads_or(need)) continue;   // the pair's columns are orthogonal to the tolerance: nothing is touched
            rotated_sweep = 1;
            // -- J^H G J diagonal: cyclic two-sided Jacobi, 16 disjoint pairs per round
            for (int isw = 0; isw < kSvdbInnerSweeps; ++isw) {
                int swept = 0;
                for (int r = 0; r < N - 1; ++r) {
                    int rot = 0;
                    if (tid < kSvdbBlock) {
                        int pp, qq;
                        svdb_pair(N, r, tid, &pp, &qq);
                        double c = 1.0, sr = 0.0, si = 0.0;
                        rot = svdb_rotation(sG[pp * N + pp].x, sG[qq * N + qq].x, sG[qq * N + pp], tol, negligible, &c, &sr, &si) ? 1 : 0;
                        sPQ[2 * tid] = pp; sPQ[2 * tid + 1] = qq;
                        sRot[4 * tid] = c; sRot[4 * tid + 1] = sr; sRot[4 * tid + 2] = si; sRot[4 * tid + 3] = (double)rot;
                    }
                    if (!__syncthreads_or(rot)) continue;
                    swept = 1;
                    for (int e = tid; e < 2 * kSvdbBlock * N; e += kSvdbThreads) {   // columns of G and of J
                        const int pr = (e >> 5) & (kSvdbBlock - 1), i = e & (N - 1);
                        if (sRot[4 * pr + 3] != 0.0) {
                            cplx* mat = (e >> 9) ? sJ : sG;
                            const double c = sRot[4 * pr], sr = sRot[4 * pr + 1], si = sRot[4 * pr + 2];
                            const int pp = sPQ[2 * pr], qq = sPQ[2 * pr + 1];
                            const cplx x = mat[pp * N + i], y = mat[qq * N + i];
                            mat[pp * N + i] = make_double2(c * x.x - (sr * y.x - si * y.y), c * x.y - (sr * y.y + si * y.x));
                            mat[qq * N + i] = make_double2(c * y.x + (sr * x.x + si * x.y), c * y.y + (sr * x.y - si * x.x));
                        }
                    }
                    __syncthreads();
                    for (int e = tid; e < kSvdbBlock * N; e += kSvdbThreads) {       // rows of G: the conjugate
                        const int pr = e >> 5, j = e & (N - 1);
                        if (sRot[4 * pr + 3] != 0.0) {
                            const double c = sRot[4 * pr], sr = sRot[4 * pr + 1], si = sRot[4 * pr + 2];
                            const int pp = sPQ[2 * pr], qq = sPQ[2 * pr + 1];
                            const cplx x = sG[j * N + pp], y = sG[j * N + qq];
                            cplx xn = make_double2(c * x.x - (sr * y.x + si * y.y), c * x.y - (sr * y.y - si * y.x));
                            cplx yn = make_double2(c * y.x + (sr * x.x - si * x.y), c * y.y + (sr * x.y + si * x.x));
                            if (j == pp) { xn.y = 0.0; yn = make_double2(0.0, 0.0); }   // the annihilated entry is zero, the diagonal real
                            if (j == qq) { yn.y = 0.0; xn = make_double2(0.0, 0.0); }
                            sG[j * N + pp] = xn;
                            sG[j * N + qq] = yn;
                        }
                    }
                    __syncthreads();
                }
                if (!swept) break;
            }
            // -- one Newton-Schulz step J <- J + J (1 - J^H J) / 2, the defect D = 1 - J^H J in G's place: the rounding of up to 62
            // rotations per column leaves J unitary to some tens of eps only, and V would collect that defect at every visit
            for (int e = tid; e < N * N; e += kSvdbThreads) {
                const int i = e & (N - 1), j = e >> 5;
                double dr = i == j ? 1.0 : 0.0, di = 0.0;
                for (int k0 = 0; k0 < N; ++k0) {
                    const int k = (k0 + i) & (N - 1);   // (a start of its own per column i: the lanes of a wave on different LDS banks)
                    const cplx x = sJ[i * N + k], y = sJ[j * N + k];
                    dr -= x.x * y.x + x.y * y.y;
                    di -= x.x * y.y - x.y * y.x;
                }
                sG[e] = make_double2(dr, di);
            }
            __syncthreads();
            cplx jn[N * N / kSvdbThreads];
#pragma unroll
            for (int t = 0; t < N * N / kSvdbThreads; ++t) {
                const int e = tid + t * kSvdbThreads, i = e & (N - 1), j = e >> 5;
                double ar = 0.0, ai = 0.0;
                for (int k = 0; k < N; ++k) {
                    const cplx x = sJ[k * N + i], d = sG[j * N + k];
                    ar += x.x * d.x - x.y * d.y;
                    ai += x.x * d.y + x.y * d.x;
                }
                jn[t] = make_double2(sJ[e].x + 0.5 * ar, sJ[e].y + 0.5 * ai);
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < N * N / kSvdbThreads; ++t) sJ[tid + t * kSvdbThreads] = jn[t];
            __syncthreads();
            // -- (W, V)[:, panel] <- (W, V)[:, panel] J on the matrix cores, a tile of 16 rows per wave at a time:
            // D[c'][row] = sum_c J[c][c'] P[row][c]; lane l feeds A[l % 16][l / 16] = J[4 kk + l / 16][c'] and B[l / 16][l % 16] = P[row][c]
            const int ntw = (wr + 15) >> 4, ntv = (wc + 15) >> 4, kq = lane >> 4;
            for (int tile = wave; tile < ntw + ntv; tile += kSvdbThreads / 64) {
                const bool isw = tile < ntw;
                cplx* M = isw ? W : V;
                const int ldm = isw ? ld : ldv, nr = isw ? wr : wc, row = 16 * (isw ? tile : tile - ntw) + (lane & 15);
                const int rr = row < nr ? row : nr - 1;
                cplx xb[8];
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const int c = sCol[4 * kk + kq];
                    const cplx v = M[(size_t)(c >= 0 ? c : 0) * ldm + rr];
                    xb[kk] = (c >= 0 && row < nr) ? v : make_double2(0.0, 0.0);
                }
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    svdb_d4 t1 = {0.0, 0.0, 0.0, 0.0}, t2 = t1, t3 = t1;
#pragma unroll
                    for (int kk = 0; kk < 8; ++kk) {
                        const cplx jv = sJ[(ct * kSvdbBlock + (lane & 15)) * N + 4 * kk + kq];
                        // j x = (T1 - T2) + i (T3 - T1 - T2), T1 = jr xr, T2 = ji xi, T3 = (jr + ji)(xr + xi)
                        t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(jv.x, xb[kk].x, t1, 0, 0, 0);
                        t2 = __builtin_amdgcn_mfma_f64_16x16x4f64(jv.y, xb[kk].y, t2, 0, 0, 0);
                        t3 = __builtin_amdgcn_mfma_f64_16x16x4f64(jv.x + jv.y, xb[kk].x + xb[kk].y, t3, 0, 0, 0);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int c = sCol[ct * kSvdbBlock + 4 * t + kq];
                        if (c >= 0 && row < nr) M[(size_t)c * ldm + row] = make_double2(t1[t] - t2[t], t3[t] - t1[t] - t2[t]);
                    }
                }
            }
        }
        if (!rotated_sweep) { ++sweep; status = kSvdbConverged; break; }
    }
    __syncthreads();

    // ---- singular values = column norms (fixed order), their descending order (stable), U and V^H
    if (tid < wc) {
        double acc = 0.0;
        for (int i = 0; i < wr; ++i) { const cplx x = W[(size_t)tid * ld + i]; acc += x.x * x.x + x.y * x.y; }
        sSig[tid] = sqrt(acc);
        sOrd[tid] = tid;   // (every entry a valid column even if norms that are not numbers defeat the ranking below)
    }
    __syncthreads();
    if (tid < wc) {
        int rank = 0;
        const double mine = sSig[tid];
        for (int j = 0; j < wc; ++j) rank += (sSig[j] > mine || (sSig[j] == mine && j < tid)) ? 1 : 0;
        sOrd[rank] = tid;
    }
    __syncthreads();
    const int ki = wc;
    cplx* u = p.u + (size_t)b * p.m * p.k;
    cplx* vh = p.vh + (size_t)b * p.k * p.n;
    for (int idx = tid; idx < rows * ki; idx += kSvdbThreads) {
        const int i = idx / ki, j = idx - i * ki, c = sOrd[j];
        const double inv = sSig[c] > 0.0 ? 1.0 / sSig[c] : 0.0;
        cplx v = mode == 0 ? W[(size_t)c * ld + i] : V[(size_t)c * ldv + i];
        if (mode == 0) { v.x *= inv; v.y *= inv; }
        u[(size_t)i * p.k + j] = v;
    }
    for (int idx = tid; idx < ki * cols; idx += kSvdbThreads) {
        const int j = idx / cols, i = idx - j * cols, c = sOrd[j];
        const double inv = sSig[c] > 0.0 ? 1.0 / sSig[c] : 0.0;
        cplx v = mode == 0 ? V[(size_t)c * ldv + i] : W[(size_t)c * ld + i];
        if (mode == 1) { v.x *= inv; v.y *= inv; }
        vh[(size_t)j * p.n + i] = make_double2(v.x, -v.y);
    }
    if (tid < ki) p.s[(size_t)b * p.k + tid] = sSig[sOrd[tid]];
    if (tid == 0) { p.status[b] = status; if (p.sweeps) p.sweeps[b] = sweep; }
}

size_t svd_batch_work_elems(int count, int m, int n) { return (size_t)count * std::min(m, n) * std::max(m, n); }
size_t svd_batch_v_elems(int count, int m, int n) { return (size_t)count * std::min(m, n) * std::min(m, n); }

// The device-pointer core: every pointer is device memory; work / vmat hold svd_batch_work_elems / svd_batch_v_elems complex numbers.
// d_rows / d_cols / d_sweeps may be null.  Enqueues on `st` and returns; nothing is synchronised.
hipError_t launch_svd_batch(int count, int m, int n, const int* d_rows, const int* d_cols, const void* d_a, void* d_u, double* d_s, void* d_vh,
                            int* d_sweeps, int* d_status, void* work, void* vmat, hipStream_t st) {
    const int k = std::min(m, n);
    hipError_t e;
    if ((e = hipMemsetAsync(d_u, 0, sizeof(cplx) * (size_t)count * m * k, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_s, 0, sizeof(double) * (size_t)count * k, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(d_vh, 0, sizeof(cplx) * (size_t)count * k * n, st)) != hipSuccess) return e;
    SvdBatchArgs args{static_cast<const cplx*>(d_a), static_cast<cplx*>(d_u), d_s, static_cast<cplx*>(d_vh), d_sweeps, d_status, d_rows, d_cols,
                      static_cast<cplx*>(work), static_cast<cplx*>(vmat), m, n, k, std::max(m, n), 1e-15};
    svd_batch_kernel<<<count, kSvdbThreads, 0, st>>>(args);
    return hipGetLastError();
}

static thread_local double g_svd_batch_core_ms = -1.0;   // aqc_svd_batch_core_ms

}  // namespace aqc

extern "C" double aqc_svd_batch_core_ms(void) { return aqc::g_svd_batch_core_ms; }

extern "C" int aqc_svd_batch(int device, int count, int m, int n, const int32_t* rows, const int32_t* cols, const double* a, double* u, double* s,
                             double* vh, int32_t* sweeps, int32_t* status) {
    using namespace aqc;
    if (!a || !u || !s || !vh || !status) return fail("aqc_svd_batch: null argument");
    if (count < 1) return fail("aqc_svd_batch: count must be at least 1");
    if (m < 1 || n < 1 || m > kSvdbMaxDim || n > kSvdbMaxDim) return fail("aqc_svd_batch: m and n must lie in 1..%d", (int)kSvdbMaxDim);
    for (int i = 0; i < count; ++i) {
        if (rows && (rows[i] < 1 || rows[i] > m)) return fail("aqc_svd_batch: rows[%d] = %d is outside 1..%d", i, rows[i], m);
        if (cols && (cols[i] < 1 || cols[i] > n)) return fail("aqc_svd_batch: cols[%d] = %d is outside 1..%d", i, cols[i], n);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device out of range");
    if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
    const int k = std::min(m, n);
    const size_t na = (size_t)count * m * n, nu = (size_t)count * m * k, nv = (size_t)count * k * n, ns = (size_t)count * k;
    DevBuf<double2> da, du, dvh, dw, dv;
    DevBuf<double> ds;
    DevBuf<int> dint;   // rows | cols | sweeps | status
    hipStream_t st = nullptr;
    if (hipStreamCreate(&st) != hipSuccess) return fail("hipStreamCreate failed");
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the device core: the copies are not in aqc_svd_batch_core_ms
    g_svd_batch_core_ms = -1.0;
    int rc = 1;
    do {
        if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) { fail("aqc_svd_batch: hipEventCreate failed"); break; }
        if (da.alloc(na) || du.alloc(nu) || dvh.alloc(nv) || ds.alloc(ns) || dint.alloc((size_t)4 * count) ||
            dw.alloc(svd_batch_work_elems(count, m, n)) || dv.alloc(svd_batch_v_elems(count, m, n))) break;
        int* d_rows = dint;
        int* d_cols = d_rows + count;
        int* d_sweeps = d_cols + count;
        int* d_status = d_sweeps + count;
        if (hipMemcpyAsync(da, a, sizeof(double2) * na, hipMemcpyHostToDevice, st) != hipSuccess ||
            (rows && hipMemcpyAsync(d_rows, rows, sizeof(int) * count, hipMemcpyHostToDevice, st) != hipSuccess) ||
            (cols && hipMemcpyAsync(d_cols, cols, sizeof(int) * count, hipMemcpyHostToDevice, st) != hipSuccess)) { fail("aqc_svd_batch: upload failed"); break; }
        (void)hipEventRecord(ev0, st);
        const hipError_t e = launch_svd_batch(count, m, n, rows ? d_rows : nullptr, cols ? d_cols : nullptr, da, du, ds, dvh, d_sweeps, d_status, dw, dv, st);
        if (e != hipSuccess) { fail("aqc_svd_batch: launch failed: %s", hipGetErrorString(e)); break; }
        (void)hipEventRecord(ev1, st);
        if (hipMemcpyAsync(u, du, sizeof(double2) * nu, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(vh, dvh, sizeof(double2) * nv, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(s, ds, sizeof(double) * ns, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(status, d_status, sizeof(int) * count, hipMemcpyDeviceToHost, st) != hipSuccess ||
            (sweeps && hipMemcpyAsync(sweeps, d_sweeps, sizeof(int) * count, hipMemcpyDeviceToHost, st) != hipSuccess)) { fail("aqc_svd_batch: download failed"); break; }
        const hipError_t es = hipStreamSynchronize(st);
        if (es != hipSuccess) { fail("aqc_svd_batch: the kernel failed: %s", hipGetErrorString(es)); break; }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) g_svd_batch_core_ms = ms;
        rc = 0;
    } while (false);
    if (rc) (void)hipStreamSynchronize(st);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    (void)hipStreamDestroy(st);
    return rc;
}
