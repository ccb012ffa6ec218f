// C ABI (include/aqc_hip.h): sketched AQC on the device -- resident targets, the sketching-vector generators, the device-resident
// ADAM run and the tall-skinny QR as a call of its own (kernels: aqc_sketch.hip).
#include "aqc_ws.h"

using namespace aqc;

namespace {

// what the sketch entries ask of a workspace (cd_checks of aqc_ws_extra.cpp is the model)
int sk_checks(const aqc_ws* ws) {
    const Program& prog = ws->ctx->prog;
    const int k = ws->ncols, d = 1 << prog.n;
    if (prog.trotter) return fail("matrix path does not support the Trotter ansatz");
    if (k == 1) return fail("sketching needs a matrix workspace (ncols = number of sketching vectors), not a state-vector one");
    if (k >= d) return fail("sketching needs fewer columns than the dimension: a square workspace is full AQC (aqc_ws_set_identity)");
    if (k > 64) return fail("at most 64 sketching vectors (got %d)", k);
    if (k & (k - 1)) return fail("the number of sketching vectors must be a power of two (got %d)", k);
    return 0;
}

int sk_kind_ok(int kind) {
    if (kind != AQC_SKETCH_RAND && kind != AQC_SKETCH_ALT && kind != AQC_SKETCH_EIGEN) return fail("unknown sketching kind %d", kind);
    return 0;
}

int sk_alloc(aqc_ws* ws) {
    const int B = ws->batch, k = ws->ncols, d = 1 << ws->ctx->prog.n;
    if (ws->sk.status) return 0;
    if (ws->sk.qr_part.alloc((size_t)B * sk_qr_slabs(d) * k * k) || ws->sk.qr_rinv.alloc((size_t)B * k * k) ||
        ws->sk.tmp.alloc((size_t)B * ws->lane_elems) || ws->sk.status.alloc(B)) return 1;
    HIP_OK(hipMemsetAsync(ws->sk.status, 0, sizeof(int) * B, ws->stream));
    return 0;
}

// alt indices [sets][batch][k] -> the device, after a range check
int sk_upload_idx(aqc_ws* ws, const int32_t* idx, size_t sets) {
    const int B = ws->batch, k = ws->ncols, d = 1 << ws->ctx->prog.n;
    const size_t n = sets * B * k;
    for (size_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= d) return fail("alt column index %d out of range [0, %d)", (int)idx[i], d);
    if (n > ws->sk.idx.capacity()) {
        HIP_OK(hipStreamSynchronize(ws->stream));
        if (ws->sk.idx.reserve(n)) return 1;
    }
    HIP_OK(hipMemcpyAsync(ws->sk.idx, idx, sizeof(int) * n, hipMemcpyHostToDevice, ws->stream));
    HIP_OK(hipStreamSynchronize(ws->stream));   // the caller's array may go away
    return 0;
}

// X, Y = U X of every lane for sketch number `it`, enqueued on the workspace's stream; nothing here waits for the device unless a
// host-supplied omega has to be copied in.  d_idx: this sketch's [batch][k] column indices on the device (alt).
int sk_generate(aqc_ws* ws, int kind, unsigned long long seed, unsigned long long it, const int* d_idx, const double* omega) {
    const int B = ws->batch, k = ws->ncols, n = ws->ctx->prog.n, d = 1 << n, pitch = ws->pitch;
    const size_t ls = ws->lane_elems, us = ws->sk.shared ? 0 : (size_t)d * d;
    double2 *X = ws->bufs[AQC_BUF_X], *Y = ws->bufs[AQC_BUF_Y];
    if (before_write(ws, AQC_BUF_X) || before_write(ws, AQC_BUF_Y)) return 1;
    if (kind == AQC_SKETCH_ALT) {
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(launch_sk_alt(X, Y, ls, pitch, d, k, ws->sk.target, us, d_idx, B, ws->stream));
        return 0;
    }
    double floor = 0.0;
    if (kind == AQC_SKETCH_RAND) {   // X = qr(uniform + i uniform)   (sk_core.py:350-356)
        if (omega) { if (copy_in(ws, X, omega, (size_t)B << n)) return 1; }
        else { ProfScope ps(ws, AQC_K_MISC); HIP_OK(launch_sk_omega(X, ls, pitch, d, k, seed, AQC_SKETCH_RAND, it, 0, B, ws->stream)); }
    } else {                         // X = qr(V^H Omega - U^H Omega)   (sk_core.py:447-463)
        if (ensure_coef(ws)) return 1;
        if (omega) { if (copy_in(ws, Y, omega, (size_t)B << n)) return 1; }
        else { ProfScope ps(ws, AQC_K_MISC); HIP_OK(launch_sk_omega(Y, ls, pitch, d, k, seed, AQC_SKETCH_EIGEN, it, 1, B, ws->stream)); }
        if (run_apply(ws, true, AQC_BUF_Y, AQC_BUF_X)) return 1;
        {
            ProfScope ps(ws, AQC_K_MISC);
            HIP_OK(launch_zgemm_batched(true, false, d, k, d, ws->sk.target, d, Y, pitch, ws->sk.tmp, pitch, us, ls, ls, B, ws->stream));
            HIP_OK(launch_sk_sub(X, ws->sk.tmp, ls, pitch, d, k, B, ws->stream));
        }
        // V = U to rounding leaves noise of ~1e-15 per entry where a draw has columns of squared norm ~2 d: a column below
        // 1e-12 of the draw's scale is "no difference left" (rank deficient), not something to orthonormalise
        floor = 2.0 * d * 1e-24;
        if (before_write(ws, AQC_BUF_X) || before_write(ws, AQC_BUF_Y)) return 1;
    }
    ProfScope ps(ws, AQC_K_MISC);
    HIP_OK(launch_sk_qr(X, ws->sk.tmp, ls, pitch, d, k, B, floor, ws->sk.qr_part, ws->sk.qr_rinv, ws->sk.status, ws->stream));
    HIP_OK(launch_zgemm_batched(false, false, d, k, d, ws->sk.target, d, X, pitch, Y, pitch, us, ls, ls, B, ws->stream));
    return 0;
}

}  // namespace

extern "C" {

int aqc_qr(int device, int m, int k, const double* a, double* q_out, int32_t* status) {
    if (!a || !q_out) return fail("null argument");
    if (k < 1 || k > 64 || (k & (k - 1)) || m < k) return fail("aqc_qr takes k a power of two in [1, 64] and m >= k rows (got %d x %d)", m, k);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device out of range");
    HIP_OK(hipSetDevice(device));
    const size_t na = sizeof(double2) * (size_t)m * k;
    DevBuf<double2> dA, dT, dP, dR;
    DevBuf<int> dS;
    int st = 0;
    if (dA.alloc((size_t)m * k) || dT.alloc((size_t)m * k) || dP.alloc((size_t)sk_qr_slabs(m) * k * k) || dR.alloc((size_t)k * k) || dS.alloc(1)) return 1;
    hipError_t e = hipMemcpy(dA, a, na, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dS, 0, sizeof(int));
    if (e == hipSuccess) e = launch_sk_qr(dA, dT, 0, k, m, k, 1, 0.0, dP, dR, dS, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(q_out, dA, na, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&st, dS, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail("aqc_qr failed: %s", hipGetErrorString(e));
    if (status) *status = st;
    else if (st) return fail("aqc_qr: the matrix is rank deficient");
    return 0;
}

int aqc_ws_sketch_target(aqc_ws* ws, const double* U, int shared) {
    if (!ws || !U) return fail("null argument");
    if (sk_checks(ws)) return 1;
    HIP_OK(hipSetDevice(ws->device));
    const size_t d = (size_t)1 << ws->ctx->prog.n, count = shared ? 1 : (size_t)ws->batch;
    HIP_OK(hipStreamSynchronize(ws->stream));
    if (ws->sk.target && ws->sk.shared != (shared != 0) && ws->batch > 1 && ws->sk.target.release()) return 1;
    if (!ws->sk.target && ws->sk.target.alloc(count * d * d)) return 1;
    ws->sk.shared = shared != 0;
    HIP_OK(hipMemcpyAsync(ws->sk.target, U, sizeof(double2) * count * d * d, hipMemcpyHostToDevice, ws->stream));
    HIP_OK(hipStreamSynchronize(ws->stream));
    return sk_alloc(ws);
}

int aqc_ws_sketch_draw(aqc_ws* ws, int kind, uint64_t seed, int64_t iteration, int buf) {
    if (check_buf(ws, buf)) return 1;
    if (sk_checks(ws)) return 1;
    if (kind != AQC_SKETCH_RAND && kind != AQC_SKETCH_EIGEN) return fail("only the rand and eigen generators draw on the device");
    if (iteration < 0) return fail("the sketch number must not be negative");
    HIP_OK(hipSetDevice(ws->device));
    if (before_write(ws, buf)) return 1;
    ProfScope ps(ws, AQC_K_MISC);
    HIP_OK(launch_sk_omega(ws->bufs[buf], ws->lane_elems, ws->pitch, 1 << ws->ctx->prog.n, ws->ncols, seed, (unsigned long long)kind,
                           (unsigned long long)iteration, kind == AQC_SKETCH_EIGEN, ws->batch, ws->stream));
    return 0;
}

int aqc_ws_sketch_generate(aqc_ws* ws, int kind, uint64_t seed, int64_t iteration, const int32_t* alt_idx, const double* omega, int32_t* status) {
    if (!ws) return fail("null workspace");
    if (sk_checks(ws) || sk_kind_ok(kind)) return 1;
    if (!ws->sk.target) return fail("aqc_ws_sketch_target has not been called");
    if (kind == AQC_SKETCH_ALT && !alt_idx) return fail("the alt generator needs its column indices");
    if (iteration < 0) return fail("the sketch number must not be negative");
    HIP_OK(hipSetDevice(ws->device));
    if (kind == AQC_SKETCH_ALT && sk_upload_idx(ws, alt_idx, 1)) return 1;
    HIP_OK(hipMemsetAsync(ws->sk.status, 0, sizeof(int) * ws->batch, ws->stream));
    if (sk_generate(ws, kind, seed, (unsigned long long)iteration, ws->sk.idx, omega)) return 1;
    if (status) {
        std::vector<int> st(ws->batch);
        HIP_OK(hipMemcpyAsync(st.data(), ws->sk.status, sizeof(int) * ws->batch, hipMemcpyDeviceToHost, ws->stream));
        HIP_OK(hipStreamSynchronize(ws->stream));
        for (int b = 0; b < ws->batch; ++b) status[b] = st[b];
    }
    return 0;
}

int aqc_ws_sketch_adam(aqc_ws* ws, int kind, const double* x0, int niter, const double* lr, double beta1, double beta2, double eps, double tol,
                       uint64_t seed, int64_t iter0, const int32_t* reset, const int32_t* alt_idx, double* x_out, double* fobj_profile,
                       double* best_f, double* best_x, int64_t* nit, int32_t* status) {
    if (!ws || !lr || !x_out || !fobj_profile) return fail("null argument");
    if (sk_checks(ws) || sk_kind_ok(kind)) return 1;
    if (!ws->sk.target) return fail("aqc_ws_sketch_target has not been called");
    if (kind == AQC_SKETCH_ALT && !alt_idx) return fail("the alt generator needs its column indices");
    if (niter < 1 || iter0 < 0) return fail("niter must be positive and iter0 non-negative");
    if (!(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0)) return fail("invalid ADAM parameters");
    const int B = ws->batch, T = ws->ctx->prog.num_thetas(), k = ws->ncols;
    const size_t BT = (size_t)B * T, sets = (size_t)niter + 1;
    for (int b = 0; b < B; ++b) {
        const int r = reset ? reset[b] : (ws->sk.adam_started ? 0 : 1);
        if (r < 0 || r > 2) return fail("reset[%d] must be 0 (continue), 1 (restart from x0) or 2 (lane parked)", b);
        if (r == 0 && !ws->sk.adam_started) return fail("lane %d continues a run that has not started", b);
        if (r == 1 && !x0) return fail("lane %d restarts without x0", b);
        if (!(lr[b] > 0)) return fail("lr[%d] must be positive", b);
    }
    HIP_OK(hipSetDevice(ws->device));
    hipStream_t st = ws->stream;
    if (!ws->sk.adam) {
        if (ws->sk.adam.alloc(3 * BT + 2 * (size_t)B) || ws->sk.adam_i.alloc(3 * (size_t)B)) return 1;
        HIP_OK(hipMemsetAsync(ws->sk.adam, 0, sizeof(double) * (3 * BT + 2 * (size_t)B), st));
        HIP_OK(hipMemsetAsync(ws->sk.adam_i, 0, sizeof(int) * 3 * B, st));
    }
    if (!ws->sk.adam_x) {   // (a lane parked before it ever ran sits at the thetas in use now)
        if (ws->sk.adam_x.alloc(BT)) return 1;
        HIP_OK(hipMemcpyAsync(ws->sk.adam_x, ws->d_thetas, sizeof(double) * BT, hipMemcpyDeviceToDevice, st));
    }
    if ((size_t)B * sets > ws->sk.profile.capacity()) {
        HIP_OK(hipStreamSynchronize(st));
        if (ws->sk.profile.reserve((size_t)B * sets)) return 1;
    }
    const size_t profile_stride = ws->sk.profile.capacity() / B;   // what the buffer was last grown for
    if (kind == AQC_SKETCH_ALT && sk_upload_idx(ws, alt_idx, sets)) return 1;
    SkAdam s;
    memset(&s, 0, sizeof s);
    s.B = B; s.T = T; s.k = k; s.profile_stride = (int)profile_stride;
    s.thetas = ws->d_thetas_own;
    s.grads = ws->d_grads;
    s.m = ws->sk.adam; s.v = s.m + BT; s.best_x = s.v + BT; s.best_f = s.best_x + BT;
    double* d_lr = s.best_f + B;
    s.lr = d_lr;
    s.profile = ws->sk.profile;
    s.t = ws->sk.adam_i; s.nit = s.t + B; s.flag = s.nit + B;
    s.beta1 = beta1; s.beta2 = beta2; s.eps = eps; s.tol = tol;
    // per lane: restart (state cleared, thetas from x0), continue, or parked
    static const double kInf = HUGE_VAL;
    static const int kZero = 0, kDone = 2;
    for (int b = 0; b < B; ++b) {
        const int r = reset ? reset[b] : (ws->sk.adam_started ? 0 : 1);
        if (r == 1) {
            HIP_OK(hipMemsetAsync(s.m + (size_t)b * T, 0, sizeof(double) * T, st));
            HIP_OK(hipMemsetAsync(s.v + (size_t)b * T, 0, sizeof(double) * T, st));
            HIP_OK(hipMemcpyAsync(s.best_f + b, &kInf, sizeof(double), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(s.t + b, &kZero, sizeof(int), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(s.flag + b, &kZero, sizeof(int), hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(ws->d_thetas_own + (size_t)b * T, x0 + (size_t)b * T, sizeof(double) * T, hipMemcpyHostToDevice, st));
        } else {   // the run's own last point, not whatever set_thetas, an evaluation or another driver has put in use since
            HIP_OK(hipMemcpyAsync(ws->d_thetas_own + (size_t)b * T, ws->sk.adam_x + (size_t)b * T, sizeof(double) * T, hipMemcpyDeviceToDevice, st));
            if (r == 2) HIP_OK(hipMemcpyAsync(s.flag + b, &kDone, sizeof(int), hipMemcpyHostToDevice, st));
        }
    }
    HIP_OK(hipMemsetAsync(s.nit, 0, sizeof(int) * B, st));
    HIP_OK(hipMemcpyAsync(d_lr, lr, sizeof(double) * B, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(ws->sk.status, 0, sizeof(int) * B, st));
    HIP_OK(hipStreamSynchronize(st));   // x0 / lr may go away; from here to the fetch nothing waits for the device
    ws->sk.adam_started = true;
    // evaluation e (0-based) runs under sketch iter0 + e + 1; the last one only evaluates (the cost optimizer._adam reports: fun(x))
    for (size_t e = 0; e < sets; ++e) {
        if (run_coef(ws, ws->d_thetas_own)) return 1;
        if (sk_generate(ws, kind, seed, (unsigned long long)iter0 + e + 1, kind == AQC_SKETCH_ALT ? ws->sk.idx + e * B * k : nullptr, nullptr)) return 1;
        if (run_apply(ws, true, AQC_BUF_Y, AQC_BUF_Z)) return 1;                 // V^H Y       (sk_core.py:191)
        if (aqc_ws_vdot_launch(ws, AQC_BUF_X, AQC_BUF_Z)) return 1;              // <X|V^H Y>   (:192)
        if (aqc_ws_grad_from(ws, AQC_BUF_X, -1, 0, 1)) return 1;                 // the sweep   (:193)
        s.trace = ws->d_vdot_out;
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(launch_sk_adam(s, (int)e, e + 1 < sets ? 1 : 0, st));
    }
    HIP_OK(hipMemcpyAsync(ws->sk.adam_x, ws->d_thetas_own, sizeof(double) * BT, hipMemcpyDeviceToDevice, st));   // kept with m, v and t
    std::vector<int> h_nit(B), h_status(B);
    HIP_OK(hipMemcpyAsync(x_out, ws->d_thetas_own, sizeof(double) * BT, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpy2DAsync(fobj_profile, sizeof(double) * sets, ws->sk.profile, sizeof(double) * profile_stride, sizeof(double) * sets, B,
                            hipMemcpyDeviceToHost, st));
    if (best_f) HIP_OK(hipMemcpyAsync(best_f, s.best_f, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (best_x) HIP_OK(hipMemcpyAsync(best_x, s.best_x, sizeof(double) * BT, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_nit.data(), s.nit, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_status.data(), ws->sk.status, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
        if (nit) nit[b] = h_nit[b];
        if (status) status[b] = h_status[b];
    }
    return 0;
}

}  // extern "C"
