// Device-resident multi-start L-BFGS on the lane-batched surrogate objective (one optimisation per lane, all lanes
// advance together; thetas, gradients and the L-BFGS history never leave HBM -- the host reads a few flags per step).
//
// The objective is the reference's surrogate f = 1 - (1 - w) |h_0|^2 - w |h_max|^2 with its 10 % hysteresis on the
// leading flip state and the smoothed weight (objective_lhs_sur_max.py:82-191); the optimizer stands in for the
// scipy L-BFGS-B behind the reference's AqcOptimizer (optimizer.py:579-590): two-loop recursion, Armijo
// backtracking with lane-wise step lengths, the state update once per accepted step.  Same algorithm as the host
// version in aqc_research_amd/batched_optimizer.py, which stays as its cross-check.
//
// One workgroup per lane for everything that reduces over the T parameters.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_math.h"

namespace aqc {

namespace {

constexpr int kLbThreads = 256;

__device__ __forceinline__ double block_sum(double v, double* red) {   // all threads get the total (fixed order)
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}
__device__ __forceinline__ double block_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double t = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = fmax(t, red[w]);
    return t;
}

// State update of one lane from its amplitudes: 10 % hysteresis on the leading flip state and the smoothed weight
// (objective_lhs_sur_max.py:113-117, :186).
__device__ __forceinline__ void lb_update(const cplx* h, int S, int& max_no, double& w, bool smooth = true) {
    double best = h[max_no].x * h[max_no].x + h[max_no].y * h[max_no].y;
    for (int i = 0; i < S; ++i) {
        const double v = h[i].x * h[i].x + h[i].y * h[i].y;
        if (1.1 * best < v) { best = v; max_no = i; }
    }
    if (!smooth) return;   // objective() alone: the weight moves when the gradient has been taken (objective_lhs_sur_max.py:186)
    const double h0 = h[0].x * h[0].x + h[0].y * h[0].y, hm = h[max_no].x * h[max_no].x + h[max_no].y * h[max_no].y;
    const double f_old = 1.0 - (1.0 - w) * h0 - w * hm;
    w = w + 0.1 * (sqrt(fabs(f_old)) - w);
}

// First half of an evaluation (one thread per lane): from the gathered amplitudes hs[b][S] the optional state update, the
// value, and the lhs state of the lane's ONE sweep.  The surrogate's gradient is Re(c_0 g_0 + c_max g_max) with
// c_0 = -2 (1 - w) conj(h_0) (-2 conj(h_0) while |state_0> leads), c_max = -2 w conj(h_max), g_s the complex gradient of
// the sweep from |state_s> (objective_lhs_sur_max.py:147-191).  That gradient is conjugate-linear in the lhs state, so the
// sum is the gradient of the sweep from conj(c_0)|state_0> + conj(c_max)|state_max>: the two amplitudes go into X2 here
// (the previous call's positions are cleared), and the sweep that follows delivers the combination directly.
__global__ void lb_prepare_kernel(LbState st, const cplx* hs, int update, double* f_out, cplx* raw_hs, cplx* x2, size_t lane_stride,
                                  const long long* index, long long* prev) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= st.B) return;
    const cplx* h = hs + (size_t)b * st.S;
    int max_no = st.max_no[b];
    double w = st.weight[b];
    if (update) lb_update(h, st.S, max_no, w, update == 1);   // update == 2: hysteresis only
    const double h0 = h[0].x * h[0].x + h[0].y * h[0].y, hm = h[max_no].x * h[max_no].x + h[max_no].y * h[max_no].y;
    const bool lead = max_no != 0;
    f_out[b] = 1.0 - (1.0 - w) * h0 - w * hm;
    if (update) { st.max_no[b] = max_no; st.weight[b] = w; st.fidelity[b] = h0; }
    cplx* x = x2 + (size_t)b * lane_stride;
    for (int k = 0; k < 2; ++k)
        if (prev[2 * b + k] >= 0) x[(size_t)prev[2 * b + k]] = make_double2(0.0, 0.0);
    const double k0 = lead ? -2.0 * (1.0 - w) : -2.0;
    const long long i0 = index[0], im = lead ? index[max_no] : -1;
    x[(size_t)i0] = make_double2(k0 * h[0].x, k0 * h[0].y);                      // conj(c_0) = k0 h_0
    if (lead) x[(size_t)im] = make_double2(-2.0 * w * h[max_no].x, -2.0 * w * h[max_no].y);   // conj(c_max) = -2 w h_max
    prev[2 * b] = i0; prev[2 * b + 1] = im;
    if (raw_hs) for (int i = 0; i < st.S; ++i) raw_hs[(size_t)b * st.S + i] = h[i];
}
// Second half: the real gradient and a copy of the complex one
__global__ void lb_take_kernel(LbState st, const cplx* grads, double* g_out, cplx* raw_g) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)st.B * st.T) return;
    const cplx g = grads[i];
    g_out[i] = g.x;
    if (raw_g) raw_g[i] = g;
}
// Probe of the state update on the accepted points (no change of state): flags[1] |= some lane leads with a flip state now
// or WOULD after the update -- the accepted points' gradients then have to be swept again under the new state
__global__ void lb_probe_kernel(LbState st, const cplx* hs, int* flags) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= st.B) return;
    int max_no = st.max_no[b];
    double w = st.weight[b];
    const bool lead_now = max_no != 0;
    lb_update(hs + (size_t)b * st.S, st.S, max_no, w);
    if (lead_now || max_no != 0) atomicOr(&flags[1], 1);
}
// State update at the accepted points while |state_0> leads everywhere (before and after): the value 1 - |h_0|^2 and the
// gradient Re(-2 conj(h_0) g_0) do not depend on the weight, so the raw results of the accepted trials are final
__global__ void lb_commit0_kernel(LbState st, const cplx* hs, const cplx* raw_g, double* f_out, double* g_out) {
    const int b = blockIdx.x, t = threadIdx.x;
    const cplx* h = hs + (size_t)b * st.S;
    for (int i = t; i < st.T; i += blockDim.x) g_out[(size_t)b * st.T + i] = raw_g[(size_t)b * st.T + i].x;
    if (t == 0) {
        int max_no = st.max_no[b];
        double w = st.weight[b];
        lb_update(h, st.S, max_no, w);
        const double h0 = h[0].x * h[0].x + h[0].y * h[0].y;
        f_out[b] = 1.0 - h0;
        st.max_no[b] = max_no; st.weight[b] = w; st.fidelity[b] = h0;
    }
}

// State-free mode: does a lane at a point of value f, max|g| gm and |tr|^2/k^2 fid go on to another iteration?
__device__ __forceinline__ bool lb_mat_goes_on(const LbMat& m, double f, double gm, double fid) {
    if (!(gm > m.gtol)) return false;
    if (m.fobj_thr > 0.0 && f <= m.fobj_thr) return false;
    if (m.fid_thr > 0.0 && fid >= m.fid_thr) return false;
    return true;
}
// The matrix objective of one lane from what an evaluation leaves (trace = <X|V^H Y>, grads = the complex gradient of the sweep
// from X): f = 1 - Re tr / k, g = -Re grads / k (sk_core.py:192-197, as sk_adam_kernel takes them), max|g| and |tr|^2 / k^2 (the
// Hilbert-Schmidt fidelity when X = I).  A lane whose trace or g is not finite gets its status word set and stops where it is (done,
// inactive, step 0); lanes with a status word are skipped from then on.  init: the start point -- results into the current
// point's rows and the first kLbAnyActive; else into the trial rows.
__global__ __launch_bounds__(kLbThreads) void lb_mat_value_kernel(LbState st, LbMat m, const cplx* trace, const cplx* grads, int init) {
    __shared__ double red[8];
    const int b = blockIdx.x, t = threadIdx.x, T = st.T;
    if (!init && b == 0 && t == 0) *m.flags = 0;   // a trial starts with a clear flag word (the start point's is cleared by the driver)
    if (m.status[b]) return;
    const size_t off = (size_t)b * T;
    double* g_out = init ? st.g : m.gt;
    const cplx tr = trace[b];
    const double f = 1.0 - tr.x / m.k, fid = (tr.x * tr.x + tr.y * tr.y) / ((double)m.k * m.k);
    double gm = 0.0, bad = (isfinite(f) && isfinite(fid)) ? 0.0 : 1.0;   // fid: the trace's imaginary part too
    for (int i = t; i < T; i += blockDim.x) {
        const double g = -grads[off + i].x / m.k;
        g_out[off + i] = g;
        gm = fmax(gm, fabs(g));
        if (!isfinite(g)) bad = 1.0;
    }
    gm = block_max(gm, red);
    bad = block_max(bad, red);
    if (t == 0) {
        (init ? st.f : m.ft)[b] = f;
        (init ? st.fidelity : m.fid_t)[b] = fid;
        (init ? m.gmax : m.gmax_t)[b] = gm;
        if (bad > 0.0) {
            m.status[b] = kLbNonFinite;
            st.active[b] = 0; st.done[b] = 1; st.step[b] = 0.0;
        } else if (init) {
            const int a = lb_mat_goes_on(m, f, gm, fid) ? 1 : 0;
            st.active[b] = a;
            if (a) atomicOr(m.flags, (int)kLbAnyActive);
        }
    }
}

// active &= max|g| > gtol [and fidelity < thr]; flags[2] |= some lane is active
__global__ __launch_bounds__(kLbThreads) void lb_active_kernel(LbState st, double gtol, double fid_thr, int* flags) {
    __shared__ double red[8];
    const int b = blockIdx.x;
    double m = 0.0;
    for (int i = threadIdx.x; i < st.T; i += blockDim.x) m = fmax(m, fabs(st.g[(size_t)b * st.T + i]));
    m = block_max(m, red);
    if (threadIdx.x == 0) {
        int a = st.active[b];
        if (!(m > gtol)) a = 0;
        if (fid_thr > 0.0 && st.fidelity[b] >= fid_thr) a = 0;
        st.active[b] = a;
        if (a) atomicOr(&flags[2], 1);
    }
}

// The step kernels below are written once, as bodies with a mode: kMat = false is the surrogate's state machine (amplitude rows, raw
// copies of the complex gradient), kMat = true the state-free matrix objective (S = 0; see LbMat in aqc_launch.h).  Each mode is a
// kernel of its own, so the surrogate's kernels are exactly the kMat = false instances.

// Two-loop recursion, search direction, slope; step = active ? 1 : 0, done = !active, x_new = x
template <bool kMat>
__device__ __forceinline__ void lb_direction_body(const LbState& st, int count, const LbMat* mat) {
    __shared__ double red[8];
    __shared__ double alpha[32];
    const int b = blockIdx.x, t = threadIdx.x, T = st.T, m = st.memory;
    if constexpr (kMat) { if (mat->status[b]) return; }   // a flagged lane is skipped (done and inactive since it was flagged)
    const size_t off = (size_t)b * T;
    const int k = count < m ? count : m;
    double* q = st.d + off;
    for (int i = t; i < T; i += blockDim.x) q[i] = st.g[off + i];
    for (int j = k - 1; j >= 0; --j) {
        const int slot = (count - k + j) % m;
        const double* s = st.Smem + ((size_t)slot * st.B + b) * T;
        const double* y = st.Ymem + ((size_t)slot * st.B + b) * T;
        double acc = 0.0;
        for (int i = t; i < T; i += blockDim.x) acc += s[i] * q[i];
        const double a = st.rho[(size_t)slot * st.B + b] * block_sum(acc, red);
        if (t == 0) alpha[j] = a;
        for (int i = t; i < T; i += blockDim.x) q[i] -= a * y[i];
    }
    if (k) {
        const int last = (count - 1) % m;
        const double* y = st.Ymem + ((size_t)last * st.B + b) * T;
        double acc = 0.0;
        for (int i = t; i < T; i += blockDim.x) acc += y[i] * y[i];
        const double yy = block_sum(acc, red), r = st.rho[(size_t)last * st.B + b];
        const double gamma = (yy > 0.0 && r > 0.0) ? 1.0 / (r * yy) : 1.0;
        for (int i = t; i < T; i += blockDim.x) q[i] *= gamma;
    } else {   // first step: at most unit length
        double acc = 0.0;
        for (int i = t; i < T; i += blockDim.x) acc += st.g[off + i] * st.g[off + i];
        const double nrm = sqrt(block_sum(acc, red)), sc = 1.0 / fmax(nrm, 1.0);
        for (int i = t; i < T; i += blockDim.x) q[i] *= sc;
    }
    __syncthreads();
    for (int j = 0; j < k; ++j) {
        const int slot = (count - k + j) % m;
        const double* s = st.Smem + ((size_t)slot * st.B + b) * T;
        const double* y = st.Ymem + ((size_t)slot * st.B + b) * T;
        double acc = 0.0;
        for (int i = t; i < T; i += blockDim.x) acc += y[i] * q[i];
        const double beta = st.rho[(size_t)slot * st.B + b] * block_sum(acc, red);
        const double a = alpha[j];
        for (int i = t; i < T; i += blockDim.x) q[i] += (a - beta) * s[i];
    }
    double acc = 0.0;
    for (int i = t; i < T; i += blockDim.x) { q[i] = -q[i]; acc += st.g[off + i] * q[i]; }
    double slope = block_sum(acc, red);
    if (slope >= 0.0) {   // not a descent direction: steepest descent
        double gg = 0.0;
        for (int i = t; i < T; i += blockDim.x) { q[i] = -st.g[off + i]; gg += st.g[off + i] * st.g[off + i]; }
        slope = -block_sum(gg, red);
    }
    for (int i = t; i < T; i += blockDim.x) st.x_new[off + i] = st.x[off + i];
    if constexpr (kMat) {   // a lane that accepts nothing keeps the current point's results
        for (int i = t; i < T; i += blockDim.x) mat->g_acc[off + i] = st.g[off + i];
        if (t == 0) { mat->f_acc[b] = st.f[b]; mat->gmax_acc[b] = mat->gmax[b]; mat->fid_acc[b] = st.fidelity[b]; }
    }
    if (t == 0) {
        const int a = st.active[b];
        st.slope[b] = slope;
        st.step[b] = a ? 1.0 : 0.0;
        st.done[b] = a ? 0 : 1;
    }
}
__global__ __launch_bounds__(kLbThreads) void lb_direction_kernel(LbState st, int count) { lb_direction_body<false>(st, count, nullptr); }
__global__ __launch_bounds__(kLbThreads) void lb_mat_direction_kernel(LbState st, LbMat mat, int count) { lb_direction_body<true>(st, count, &mat); }
// trial point into the workspace's theta buffer
__global__ void lb_trial_kernel(LbState st, double* thetas) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)st.B * st.T) return;
    const int b = (int)(i / st.T);
    thetas[i] = st.x[i] + st.step[b] * st.d[i];
}
// Armijo test per lane; accepted lanes keep the trial point and its raw device results (kMat: its value and gradient, which are
// final); flags[3] |= some lane not done (kMat: kLbNotDone of the one flag word)
template <bool kMat>
__device__ __forceinline__ void lb_armijo_body(const LbState& st, double c1, const double* thetas, const double* ft, const cplx* raw_hs_t,
                                               const cplx* raw_g0_t, int* flags, const LbMat* mat) {
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t off = (size_t)b * st.T;
    const bool was_done = st.done[b] != 0;
    const double step = st.step[b];
    const bool ok = !was_done && ft[b] <= st.f[b] + c1 * step * st.slope[b];
    if (ok) {
        if constexpr (kMat) {
            for (int i = t; i < st.T; i += blockDim.x) { st.x_new[off + i] = thetas[off + i]; mat->g_acc[off + i] = mat->gt[off + i]; }
        } else {
            for (int i = t; i < st.T; i += blockDim.x) { st.x_new[off + i] = thetas[off + i]; st.acc_g0[off + i] = raw_g0_t[off + i]; }
            for (int i = t; i < st.S; i += blockDim.x) st.acc_hs[(size_t)b * st.S + i] = raw_hs_t[(size_t)b * st.S + i];
        }
    }
    __syncthreads();
    if (t == 0) {
        if constexpr (kMat) {
            if (ok) { mat->f_acc[b] = ft[b]; mat->gmax_acc[b] = mat->gmax_t[b]; mat->fid_acc[b] = mat->fid_t[b]; }
        }
        if (ok) st.done[b] = 1;
        else if (!was_done) { st.step[b] = 0.5 * step; atomicOr(kMat ? flags : &flags[3], kMat ? (int)kLbNotDone : 1); }
    }
}
__global__ __launch_bounds__(kLbThreads) void lb_armijo_kernel(LbState st, double c1, const double* thetas, const double* ft,
                                                              const cplx* raw_hs_t, const cplx* raw_g0_t, int* flags) {
    lb_armijo_body<false>(st, c1, thetas, ft, raw_hs_t, raw_g0_t, flags, nullptr);
}
__global__ __launch_bounds__(kLbThreads) void lb_mat_armijo_kernel(LbState st, LbMat mat, double c1, const double* thetas) {
    lb_armijo_body<true>(st, c1, thetas, mat.ft, nullptr, nullptr, mat.flags, &mat);
}
// rows of lanes that will not move start as the current point's raw results
__global__ void lb_copy_raw_kernel(LbState st) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)st.B * st.T) st.acc_g0[i] = st.cur_g0[i];
    if (i < (size_t)st.B * st.S) st.acc_hs[i] = st.cur_hs[i];
}
// History update and convergence flags after the accepted points have been evaluated under the new state
// (kMat: the accepted results are the trials' own, and the next iteration's "any lane active" test -- max|g| > gtol and the two
// thresholds -- is taken here, into the flag word Armijo has just written, so that the host reads that one word and nothing else)
template <bool kMat>
__device__ __forceinline__ void lb_history_body(const LbState& st, int count, double ftol, const double* f_acc, const double* g_acc, const LbMat* mat) {
    __shared__ double red[8];
    const int b = blockIdx.x, t = threadIdx.x, T = st.T;
    const size_t off = (size_t)b * T;
    const int slot = count % st.memory;
    double* s = st.Smem + ((size_t)slot * st.B + b) * T;
    double* y = st.Ymem + ((size_t)slot * st.B + b) * T;
    double sy = 0.0, yy = 0.0, moved_any = 0.0;
    for (int i = t; i < T; i += blockDim.x) {
        const double si = st.x_new[off + i] - st.x[off + i], yi = g_acc[off + i] - st.g[off + i];
        s[i] = si; y[i] = yi;
        sy += si * yi; yy += yi * yi;
        if (si != 0.0) moved_any = 1.0;
    }
    sy = block_sum(sy, red); yy = block_sum(yy, red); moved_any = block_max(moved_any, red);
    const bool active = st.active[b] != 0;
    const bool moved = st.done[b] != 0 && active && moved_any > 0.0;
    const bool good = moved && sy > 1e-12 * yy;
    if (!good) for (int i = t; i < T; i += blockDim.x) { s[i] = 0.0; y[i] = 0.0; }
    for (int i = t; i < T; i += blockDim.x) { st.x[off + i] = st.x_new[off + i]; st.g[off + i] = g_acc[off + i]; }
    if constexpr (!kMat) {
        for (int i = t; i < T; i += blockDim.x) st.cur_g0[off + i] = st.acc_g0[off + i];
        for (int i = t; i < st.S; i += blockDim.x) st.cur_hs[(size_t)b * st.S + i] = st.acc_hs[(size_t)b * st.S + i];
    }
    __syncthreads();
    if (t == 0) {
        st.rho[(size_t)slot * st.B + b] = good ? 1.0 / sy : 0.0;
        const double f = st.f[b], fa = f_acc[b];
        const bool small = fabs(f - fa) <= ftol * fmax(1.0, fabs(f));
        if (active) st.nit[b] += 1;
        if constexpr (kMat) {
            const double gm = mat->gmax_acc[b], fid = mat->fid_acc[b];
            const int a = (active && moved && !small && lb_mat_goes_on(*mat, fa, gm, fid)) ? 1 : 0;
            st.active[b] = a;
            mat->gmax[b] = gm;
            st.fidelity[b] = fid;
            if (a) atomicOr(mat->flags, (int)kLbAnyActive);
        } else {
            st.active[b] = (active && moved && !small) ? 1 : 0;
        }
        st.f[b] = fa;
    }
}
__global__ __launch_bounds__(kLbThreads) void lb_history_kernel(LbState st, int count, double ftol, const double* f_acc, const double* g_acc) {
    lb_history_body<false>(st, count, ftol, f_acc, g_acc, nullptr);
}
// One launch per line-search trial, enqueued behind Armijo: it acts once no lane backtracks any more -- the flag word of that
// trial, complete since the Armijo kernel has finished -- or after the last trial allowed.  (The word is only OR-ed into by this
// kernel, and with another bit, so every workgroup reads the same kLbNotDone.)
__global__ __launch_bounds__(kLbThreads) void lb_mat_history_kernel(LbState st, LbMat mat, int count, double ftol, int last) {
    if (!last && (__atomic_load_n(mat.flags, __ATOMIC_RELAXED) & kLbNotDone)) return;
    if (mat.status[blockIdx.x]) return;
    lb_history_body<true>(st, count, ftol, mat.f_acc, mat.g_acc, &mat);
}

}  // namespace

hipError_t lb_prepare(const LbState& st, const void* hs, int update, double* f_out, void* raw_hs, void* x2, size_t lane_stride,
                      const long long* index, long long* prev, hipStream_t s) {
    lb_prepare_kernel<<<(st.B + 63) / 64, 64, 0, s>>>(st, (const cplx*)hs, update, f_out, (cplx*)raw_hs, (cplx*)x2, lane_stride, index, prev);
    return hipGetLastError();
}
hipError_t lb_take(const LbState& st, const void* grads, double* g_out, void* raw_g, hipStream_t s) {
    const size_t n = (size_t)st.B * st.T;
    lb_take_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(st, (const cplx*)grads, g_out, (cplx*)raw_g);
    return hipGetLastError();
}
hipError_t lb_probe(const LbState& st, const void* hs, int* flags, hipStream_t s) {
    lb_probe_kernel<<<(st.B + 63) / 64, 64, 0, s>>>(st, (const cplx*)hs, flags);
    return hipGetLastError();
}
hipError_t lb_commit0(const LbState& st, const void* hs, const void* raw_g, double* f_out, double* g_out, hipStream_t s) {
    lb_commit0_kernel<<<st.B, kLbThreads, 0, s>>>(st, (const cplx*)hs, (const cplx*)raw_g, f_out, g_out);
    return hipGetLastError();
}
hipError_t lb_active(const LbState& st, double gtol, double fid_thr, int* flags, hipStream_t s) {
    lb_active_kernel<<<st.B, kLbThreads, 0, s>>>(st, gtol, fid_thr, flags);
    return hipGetLastError();
}
hipError_t lb_direction(const LbState& st, int count, hipStream_t s) {
    lb_direction_kernel<<<st.B, kLbThreads, 0, s>>>(st, count);
    return hipGetLastError();
}
hipError_t lb_trial(const LbState& st, double* thetas, hipStream_t s) {
    const size_t n = (size_t)st.B * st.T;
    lb_trial_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(st, thetas);
    return hipGetLastError();
}
hipError_t lb_armijo(const LbState& st, double c1, const double* thetas, const double* ft, const void* raw_hs_t, const void* raw_g0_t,
                     int* flags, hipStream_t s) {
    lb_armijo_kernel<<<st.B, kLbThreads, 0, s>>>(st, c1, thetas, ft, (const cplx*)raw_hs_t, (const cplx*)raw_g0_t, flags);
    return hipGetLastError();
}
hipError_t lb_copy_raw(const LbState& st, hipStream_t s) {
    const size_t n = (size_t)st.B * (st.T > st.S ? st.T : st.S);
    lb_copy_raw_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(st);
    return hipGetLastError();
}
hipError_t lb_history(const LbState& st, int count, double ftol, const double* f_acc, const double* g_acc, hipStream_t s) {
    lb_history_kernel<<<st.B, kLbThreads, 0, s>>>(st, count, ftol, f_acc, g_acc);
    return hipGetLastError();
}

hipError_t lb_mat_value(const LbState& st, const LbMat& m, const void* trace, const void* grads, int init, hipStream_t s) {
    lb_mat_value_kernel<<<st.B, kLbThreads, 0, s>>>(st, m, (const cplx*)trace, (const cplx*)grads, init);
    return hipGetLastError();
}
hipError_t lb_mat_direction(const LbState& st, const LbMat& m, int count, hipStream_t s) {
    lb_mat_direction_kernel<<<st.B, kLbThreads, 0, s>>>(st, m, count);
    return hipGetLastError();
}
hipError_t lb_mat_armijo(const LbState& st, const LbMat& m, double c1, const double* thetas, hipStream_t s) {
    lb_mat_armijo_kernel<<<st.B, kLbThreads, 0, s>>>(st, m, c1, thetas);
    return hipGetLastError();
}
hipError_t lb_mat_history(const LbState& st, const LbMat& m, int count, double ftol, int last, hipStream_t s) {
    lb_mat_history_kernel<<<st.B, kLbThreads, 0, s>>>(st, m, count, ftol, last);
    return hipGetLastError();
}

}  // namespace aqc
