// Sketched AQC on the device (sk_core.py:329-464, aqc_sketching.py:53-104, optimizer.py:178-189): the sketching-vector
// generators, a batched tall-skinny QR and the ADAM step, so that an iteration of the stochastic optimisation never visits the host.
//
// QR of (d x k) complex matrices, k <= 64 <= d rows in HBM, one per lane: CholeskyQR2.  A pass is three launches
//   gram : G = A^H A on v_mfma_f64_16x16x4_f64; every wave sums a slab of rows and stores its partial k x k block
//   chol : one workgroup per lane adds the partials in slab order (no float atomics: bit-reproducible), factors G = L L^H in LDS
//          and inverts L by forward substitution; R^-1 = L^-H goes to HBM
//   apply: Q <- A R^-1 on the matrix cores, each wave its own 16 rows
// and the QR is two passes: the first writes Q1 = A R1^-1 to a scratch matrix of A's layout, the second reads Q1 and writes
// Q = Q1 R2^-1 over A.  k < 16 (and a row count that is no multiple of 4 or 16) is padded with zeros in registers.
// Status 0 means an orthonormal Q.  A lane is marked AQC_QR_RANK_DEFICIENT in its status word, and skipped by every later launch, when
//   - a pivot of either factorisation is not finite, not above kPivotRel times its diagonal entry of that pass's G, or not above the
//     caller's absolute floor: a (numerically) dependent column;
//   - the second pass's Gram matrix G2 = Q1^H Q1 has an entry further than kOrthTol from I.  The per-column pivot test does not
//     bound the condition number (Kahan matrices pass it with kappa = 1e16), and the first pass leaves |G2 - I| ~ eps kappa^2, kappa
//     the condition number of A with its columns scaled to norm 1: when that is O(1) the second pass repairs nothing.
// A is written by the second apply only, so a flagged lane keeps its matrix bit for bit whichever test flagged it.
//
// MFMA operand layout (as in aqc_mps.hip): lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16] and receives
// D[4 r + l / 16][l % 16] in accumulator register r.
#include <hip/hip_runtime.h>

#include "../../include/aqc_hip.h"
#include "aqc_launch.h"
#include "aqc_philox.h"

namespace aqc {

typedef double2 cplx;
typedef double double4_t __attribute__((ext_vector_type(4)));

namespace {

constexpr double kPivotRel = 1e-10;
// |G2 - I| <= 1e-4 entrywise: |G2 - I|_2 <= 64e-4, so kappa(Q1) < 1.01 and the second pass ends at k eps.  eps kappa^2 = 1e-4 is
// kappa = 7e5, the geometric middle between what the callers need accepted (kappa <= 1e4: eps kappa^2 = 2e-8) and the kappa = 7e7 from
// which on 64 eps kappa > 1e-6 and a range in double precision is no longer one.  (tests/sketch_ref.py: ORTH_TOL)
constexpr double kOrthTol = 1e-4;
constexpr int kSlabRows = 64;   // rows of A one wave of the gram kernel sums

__device__ __forceinline__ double4_t sk_mfma(double a, double b, double4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// partial[lane][slab][k][k] <- sum over the slab's rows r of conj(A[r][i]) A[r][j].  NT = tiles of 16 columns.
template <int NT>
__global__ __launch_bounds__(256) void qr_gram_kernel(const cplx* __restrict__ a, size_t lane_stride, int lda, int d, int k, int nslabs,
                                                      const int* __restrict__ status, cplx* __restrict__ partial) {
    const int lane_id = blockIdx.y;
    if (status[lane_id]) return;
    const int l = threadIdx.x & 63, slab = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slab >= nslabs) return;   // (whole waves; no barrier in this kernel)
    const int li = l & 15, lk = l >> 4;
    const cplx* A = a + (size_t)lane_id * lane_stride;
    double4_t cre[NT][NT], cim[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) { cre[i][j] = double4_t{0, 0, 0, 0}; cim[i][j] = double4_t{0, 0, 0, 0}; }
    const int r_end = min(d, (slab + 1) * kSlabRows);
    for (int r0 = slab * kSlabRows; r0 < r_end; r0 += 4) {
        const int r = r0 + lk;
        double vr[NT], vi[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = 16 * t + li;
            cplx v = make_double2(0.0, 0.0);
            if (r < d && c < k) v = A[(size_t)r * lda + c];
            vr[t] = v.x; vi[t] = v.y;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {   // conj(a_i) a_j = (ar_i ar_j + ai_i ai_j) + i (ar_i ai_j - ai_i ar_j)
                cre[i][j] = sk_mfma(vr[i], vr[j], cre[i][j]);
                cre[i][j] = sk_mfma(vi[i], vi[j], cre[i][j]);
                cim[i][j] = sk_mfma(vr[i], vi[j], cim[i][j]);
                cim[i][j] = sk_mfma(-vi[i], vr[j], cim[i][j]);
            }
    }
    cplx* P = partial + ((size_t)lane_id * nslabs + slab) * k * k;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * i + 4 * q + lk, col = 16 * j + li;
                if (row < k && col < k) P[(size_t)row * k + col] = make_double2(cre[i][j][q], cim[i][j][q]);
            }
}

// G = sum of the partials (slab order), G = L L^H, X = L^-1, rinv[lane][c][i] = conj(X[i][c]) (R^-1 = L^-H, upper triangular).
// second: this is the second pass, whose G has to be I to kOrthTol.  LDS: g[k][k] | x[k][k].
__global__ __launch_bounds__(256) void qr_chol_kernel(const cplx* __restrict__ partial, int nslabs, int k, double abs_floor, int second,
                                                      int* __restrict__ status, cplx* __restrict__ rinv) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    __shared__ int s_bad;
    __shared__ double s_diag[64];
    const int lane_id = blockIdx.x, tid = threadIdx.x, kk = k * k;
    if (status[lane_id]) return;   // (uniform over the workgroup)
    cplx* g = reinterpret_cast<cplx*>(sk_smem);
    cplx* x = g + kk;
    const cplx* P = partial + (size_t)lane_id * nslabs * kk;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int e = tid; e < kk; e += 256) {
        double re = 0.0, im = 0.0;
        for (int s = 0; s < nslabs; ++s) { const cplx v = P[(size_t)s * kk + e]; re += v.x; im += v.y; }
        g[e] = make_double2(re, im);
        x[e] = make_double2(0.0, 0.0);
        if (second) {   // (a flag: every writer stores the same value; a NaN fails the comparison)
            const double dr = re - (e / k == e % k ? 1.0 : 0.0);
            if (!(dr * dr + im * im <= kOrthTol * kOrthTol)) s_bad = 1;
        }
    }
    __syncthreads();
    const int drifted = s_bad;   // (read between two barriers: the next writer is the pivot test below)
    if (tid < k) s_diag[tid] = g[tid * k + tid].x;   // the columns' squared norms: what the relative pivot test refers to
    __syncthreads();
    // right-looking Cholesky on the lower triangle
    for (int j = 0; j < k && !drifted; ++j) {
        const double piv = g[j * k + j].x;
        if (tid == 0 && (!(piv > kPivotRel * s_diag[j]) || !(piv > abs_floor) || !isfinite(piv))) s_bad = 1;
        __syncthreads();
        if (s_bad) break;
        const double ljj = sqrt(piv), inv = 1.0 / ljj;
        for (int i = j + 1 + tid; i < k; i += 256) { cplx v = g[i * k + j]; g[i * k + j] = make_double2(v.x * inv, v.y * inv); }
        __syncthreads();
        if (tid == 0) g[j * k + j] = make_double2(ljj, 0.0);
        const int m = k - j - 1;   // trailing block: rows i > j, columns c in (j, i]
        for (int e = tid; e < m * m; e += 256) {
            const int i = j + 1 + e / m, c = j + 1 + e % m;
            if (c > i) continue;
            const cplx li = g[i * k + j], lc = g[c * k + j];
            cplx v = g[i * k + c];
            v.x -= li.x * lc.x + li.y * lc.y;     // L[i][j] conj(L[c][j])
            v.y -= li.y * lc.x - li.x * lc.y;
            g[i * k + c] = v;
        }
        __syncthreads();
    }
    if (s_bad) {
        if (tid == 0) status[lane_id] = AQC_QR_RANK_DEFICIENT;
        return;
    }
    // X = L^-1, column c by thread c: x[c][c] = 1 / L[c][c]; x[i][c] = -(sum_{m = c}^{i-1} L[i][m] x[m][c]) / L[i][i]
    if (tid < k) {
        const int c = tid;
        x[c * k + c] = make_double2(1.0 / g[c * k + c].x, 0.0);
        for (int i = c + 1; i < k; ++i) {
            double re = 0.0, im = 0.0;
            for (int m = c; m < i; ++m) {
                const cplx a = g[i * k + m], b = x[m * k + c];
                re += a.x * b.x - a.y * b.y;
                im += a.x * b.y + a.y * b.x;
            }
            const double inv = -1.0 / g[i * k + i].x;
            x[i * k + c] = make_double2(re * inv, im * inv);
        }
    }
    __syncthreads();
    cplx* R = rinv + (size_t)lane_id * kk;
    for (int e = tid; e < kk; e += 256) {
        const int c = e / k, i = e % k;   // R^-1[c][i] = conj(X[i][c]); zero below the diagonal
        const cplx v = i >= c ? x[i * k + c] : make_double2(0.0, 0.0);
        R[e] = make_double2(v.x, -v.y);
    }
}

// out <- A R^-1 (out has A's layout and is another matrix): every wave its own 16 rows
template <int NT>
__global__ __launch_bounds__(256) void qr_apply_kernel(const cplx* __restrict__ a, cplx* __restrict__ out, size_t lane_stride, int lda, int d, int k,
                                                       const int* __restrict__ status, const cplx* __restrict__ rinv) {
    const int lane_id = blockIdx.y;
    if (status[lane_id]) return;
    const int l = threadIdx.x & 63, row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (row0 >= d) return;
    const int li = l & 15, lk = l >> 4;
    const cplx* A = a + (size_t)lane_id * lane_stride;
    cplx* O = out + (size_t)lane_id * lane_stride;
    const cplx* R = rinv + (size_t)lane_id * k * k;
    double4_t cre[NT], cim[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { cre[t] = double4_t{0, 0, 0, 0}; cim[t] = double4_t{0, 0, 0, 0}; }
    const int ksteps = (k + 3) / 4;
    for (int s = 0; s < ksteps; ++s) {
        const int kc = 4 * s + lk, r = row0 + li;
        cplx av = make_double2(0.0, 0.0);
        if (r < d && kc < k) av = A[(size_t)r * lda + kc];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int c = 16 * t + li;
            cplx bv = make_double2(0.0, 0.0);
            if (kc < k && c < k) bv = R[(size_t)kc * k + c];
            cre[t] = sk_mfma(av.x, bv.x, cre[t]);
            cre[t] = sk_mfma(-av.y, bv.y, cre[t]);
            cim[t] = sk_mfma(av.x, bv.y, cim[t]);
            cim[t] = sk_mfma(av.y, bv.x, cim[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = row0 + 4 * q + lk, c = 16 * t + li;
            if (r < d && c < k) O[(size_t)r * lda + c] = make_double2(cre[t][q], cim[t][q]);
        }
}

// alt: X <- one-hot columns, Y <- U[:, idx]   (sk_core.py:385-399)
__global__ void sk_alt_kernel(cplx* __restrict__ x, cplx* __restrict__ y, size_t lane_stride, int pitch, int d, int k,
                              const cplx* __restrict__ u, size_t u_stride, const int* __restrict__ idx) {
    const int lane_id = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)d * k) return;
    const int r = (int)(e / k), c = (int)(e % k), col = idx[(size_t)lane_id * k + c];
    const size_t at = (size_t)lane_id * lane_stride + (size_t)r * pitch + c;
    x[at] = make_double2(r == col ? 1.0 : 0.0, 0.0);
    y[at] = u[(size_t)lane_id * u_stride + (size_t)r * d + col];
}

// Omega of every lane by the draw rule of aqc_philox.h; normal = 0: uniform planes 0 / 1, 1: Box-Muller on planes (0, 1) / (2, 3)
__global__ void sk_omega_kernel(cplx* __restrict__ out, size_t lane_stride, int pitch, int d, int k, unsigned long long seed,
                                unsigned long long stream, unsigned long long iteration, int normal) {
    const int lane_id = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)d * k) return;
    double re, im;
    if (normal) {
        const double u0 = philox_plane_uniform(seed, stream, iteration, lane_id, 0, e), u1 = philox_plane_uniform(seed, stream, iteration, lane_id, 1, e);
        const double u2 = philox_plane_uniform(seed, stream, iteration, lane_id, 2, e), u3 = philox_plane_uniform(seed, stream, iteration, lane_id, 3, e);
        re = sqrt(-2.0 * log(1.0 - u0)) * cos(6.283185307179586 * u1);
        im = sqrt(-2.0 * log(1.0 - u2)) * cos(6.283185307179586 * u3);
    } else {
        re = philox_plane_uniform(seed, stream, iteration, lane_id, 0, e);
        im = philox_plane_uniform(seed, stream, iteration, lane_id, 1, e);
    }
    out[(size_t)lane_id * lane_stride + (e / k) * pitch + e % k] = make_double2(re, im);
}

// a <- a - b over the (d x k) blocks of all lanes
__global__ void sk_sub_kernel(cplx* __restrict__ a, const cplx* __restrict__ b, size_t lane_stride, int pitch, int d, int k) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)d * k) return;
    const size_t at = (size_t)blockIdx.y * lane_stride + (e / k) * pitch + e % k;
    a[at].x -= b[at].x;
    a[at].y -= b[at].y;
}

// ADAM, one workgroup per lane (optimizer.py:178-189 on sk_core.py:194-200): see SkAdam in aqc_launch.h
__global__ __launch_bounds__(256) void sk_adam_kernel(SkAdam s, int col, int do_update) {
    __shared__ double red[256];
    __shared__ int s_take;
    const int lane_id = blockIdx.x, tid = threadIdx.x, T = s.T;
    double* th = s.thetas + (size_t)lane_id * T;
    const int flag = s.flag[lane_id];
    const double fobj = 1.0 - s.trace[lane_id].x / s.k;
    if (tid == 0) {
        s.profile[(size_t)lane_id * s.profile_stride + col] = fobj;
        s_take = flag < 2 && fobj < s.best_f[lane_id];
    }
    __syncthreads();
    if (s_take) {   // the best value seen and the point it was seen at (sk_core.py:198-200)
        for (int i = tid; i < T; i += 256) s.best_x[(size_t)lane_id * T + i] = th[i];
        if (tid == 0) s.best_f[lane_id] = fobj;
    }
    if (flag == 1 && tid == 0) s.flag[lane_id] = 2;   // that was the evaluation at the final point
    if (flag != 0 || !do_update) return;
    const int t = s.t[lane_id] + 1;
    const double lr = s.lr[lane_id];
    const double scale = lr * sqrt(1.0 - pow(s.beta2, (double)t)) / (1.0 - pow(s.beta1, (double)t));
    double acc = 0.0;
    for (int i = tid; i < T; i += 256) {
        const size_t at = (size_t)lane_id * T + i;
        const double g = -s.grads[at].x / s.k;
        const double m = s.beta1 * s.m[at] + (1.0 - s.beta1) * g;
        const double v = s.beta2 * s.v[at] + (1.0 - s.beta2) * g * g;
        const double step = scale * m / (sqrt(v) + s.eps);
        s.m[at] = m;
        s.v[at] = v;
        th[i] -= step;
        acc += step * step;
    }
    red[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {   // fixed order
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        s.t[lane_id] = t;
        s.nit[lane_id] += 1;
        if (sqrt(red[0]) < s.tol) s.flag[lane_id] = 1;
    }
}

template <typename K>
hipError_t grant_lds(K kernel, size_t bytes) {
    static size_t granted[64] = {};   // hipFuncSetAttribute applies to the current device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (granted[dev] < bytes || dev == 0) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        granted[dev] = bytes;
    }
    return hipSuccess;
}

}  // namespace

int sk_qr_slabs(int d) { return (d + kSlabRows - 1) / kSlabRows; }

hipError_t launch_sk_qr(void* a, void* scratch, size_t lane_stride, int lda, int d, int k, int batch, double abs_floor, void* partial, void* rinv,
                        int* status, hipStream_t s) {
    const int nslabs = sk_qr_slabs(d), nt = k <= 16 ? 1 : (k <= 32 ? 2 : 4);
    cplx* P = static_cast<cplx*>(partial);
    cplx* R = static_cast<cplx*>(rinv);
    const size_t lds = 2 * sizeof(cplx) * (size_t)k * k;
    hipError_t e = grant_lds(qr_chol_kernel, 2 * sizeof(cplx) * 64 * 64);
    if (e != hipSuccess) return e;
    const dim3 ggrid((nslabs + 3) / 4, batch), agrid((d + 63) / 64, batch);
    for (int pass = 0; pass < 2; ++pass) {   // A -> scratch -> A
        const cplx* A = static_cast<const cplx*>(pass == 0 ? a : scratch);
        cplx* O = static_cast<cplx*>(pass == 0 ? scratch : a);
        if (nt == 1) qr_gram_kernel<1><<<ggrid, 256, 0, s>>>(A, lane_stride, lda, d, k, nslabs, status, P);
        else if (nt == 2) qr_gram_kernel<2><<<ggrid, 256, 0, s>>>(A, lane_stride, lda, d, k, nslabs, status, P);
        else qr_gram_kernel<4><<<ggrid, 256, 0, s>>>(A, lane_stride, lda, d, k, nslabs, status, P);
        qr_chol_kernel<<<batch, 256, lds, s>>>(P, nslabs, k, abs_floor, pass, status, R);
        if (nt == 1) qr_apply_kernel<1><<<agrid, 256, 0, s>>>(A, O, lane_stride, lda, d, k, status, R);
        else if (nt == 2) qr_apply_kernel<2><<<agrid, 256, 0, s>>>(A, O, lane_stride, lda, d, k, status, R);
        else qr_apply_kernel<4><<<agrid, 256, 0, s>>>(A, O, lane_stride, lda, d, k, status, R);
    }
    return hipGetLastError();
}

hipError_t launch_sk_alt(void* x, void* y, size_t lane_stride, int pitch, int d, int k, const void* u, size_t u_stride, const int* idx, int batch,
                         hipStream_t s) {
    const size_t total = (size_t)d * k;
    sk_alt_kernel<<<dim3((unsigned)((total + 255) / 256), batch), 256, 0, s>>>(static_cast<cplx*>(x), static_cast<cplx*>(y), lane_stride, pitch, d, k,
                                                                                static_cast<const cplx*>(u), u_stride, idx);
    return hipGetLastError();
}

hipError_t launch_sk_omega(void* out, size_t lane_stride, int pitch, int d, int k, unsigned long long seed, unsigned long long stream,
                           unsigned long long iteration, int normal, int batch, hipStream_t s) {
    const size_t total = (size_t)d * k;
    sk_omega_kernel<<<dim3((unsigned)((total + 255) / 256), batch), 256, 0, s>>>(static_cast<cplx*>(out), lane_stride, pitch, d, k, seed, stream,
                                                                                  iteration, normal);
    return hipGetLastError();
}

hipError_t launch_sk_sub(void* a, const void* b, size_t lane_stride, int pitch, int d, int k, int batch, hipStream_t s) {
    const size_t total = (size_t)d * k;
    sk_sub_kernel<<<dim3((unsigned)((total + 255) / 256), batch), 256, 0, s>>>(static_cast<cplx*>(a), static_cast<const cplx*>(b), lane_stride, pitch, d, k);
    return hipGetLastError();
}

hipError_t launch_sk_adam(const SkAdam& st, int col, int do_update, hipStream_t s) {
    sk_adam_kernel<<<st.B, 256, 0, s>>>(st, col, do_update);
    return hipGetLastError();
}

}  // namespace aqc
