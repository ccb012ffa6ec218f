// C ABI (include/aqc_hip.h): device-resident multi-start L-BFGS (surrogate and matrix objectives) and the one-call surrogate evaluation.
#include "aqc_ws.h"

using namespace aqc;

extern "C" {

// ---- device-resident multi-start L-BFGS on the lane-batched surrogate objective (aqc_lbfgs.hip) ---------------
// Preconditions (what BatchedSurrogateObjective sets up): targets in Y, |state_0> one-hot in X, the flip-state indices
// registered with aqc_ws_gather_setup (state 0 first).  thetas, gradients and the history stay in HBM; per evaluation
// the host reads one flag word, per line-search trial another.
int aqc_ws_lbfgs(aqc_ws* ws, const double* x0, int maxiter, int memory, double gtol, double ftol, double fid_thr, int max_backtracks,
                 int block_from, int block_to, int front_layer, double* x_out, double* f_out, double* fidelity_out, int64_t* nit_out,
                 int64_t* nfev_out, double* weight_out, int64_t* max_no_out) {
    if (!ws || !x0 || !x_out || !f_out) return fail("null argument");
    if (check_block_range(ws, block_from, block_to)) return 1;
    if (block_from < 0) { block_from = 0; block_to = ws->ctx->prog.num_blocks; }
    if (ws->ncols != 1) return fail("the L-BFGS driver works on state-vector workspaces");
    if (ws->gather_count < 1) return fail("aqc_ws_gather_setup has not been called (flip-state indices, state 0 first)");
    if (memory < 1 || memory > 32 || maxiter < 1 || max_backtracks < 1) return fail("invalid L-BFGS parameters");
    HIP_OK(hipSetDevice(ws->device));
    const Program& prog = ws->ctx->prog;
    const int B = ws->batch, T = prog.num_thetas(), S = ws->gather_count;
    const size_t BT = (size_t)B * T, BS = (size_t)B * S;
    hipStream_t st_ = ws->stream;
    HIP_OK(hipStreamSynchronize(st_));
    // one allocation for all double arrays, one for the complex ones, one for the integers
    const size_t nd = BT * (7 + 2 * (size_t)memory) + (size_t)B * (6 + memory + 2 + 2);
    DevBuf<double> dd;
    DevBuf<double2> dc;
    DevBuf<int> di;
    DevBuf<long long> dl;
    PinBuf<int> h_flags;
    if (dd.alloc(nd) || dc.alloc(3 * BT + 3 * BS) || di.alloc((size_t)(3 * B + 8)) || dl.alloc(B)) return 1;
    if (ws->d_combo_prev[AQC_BUF_X2].reserve(2 * (size_t)B) || h_flags.alloc(8)) return 1;
    HIP_OK(hipMemsetAsync(dd, 0, nd * sizeof(double), st_));
    HIP_OK(hipMemsetAsync(di, 0, (size_t)(3 * B + 8) * sizeof(int), st_));
    LbState L;
    double* p = dd;
    auto take = [&](size_t n) { double* r = p; p += n; return r; };
    L.B = B; L.T = T; L.S = S; L.memory = memory;
    L.x = take(BT); L.g = take(BT); L.d = take(BT); L.x_new = take(BT);
    double* gt = take(BT);        // gradient at the trial points
    double* g_acc = take(BT);     // gradient at the accepted points under the new state
    double* spare = take(BT); (void)spare;
    L.Smem = take(BT * memory); L.Ymem = take(BT * memory);
    L.f = take(B); L.slope = take(B); L.step = take(B); L.weight = take(B); L.fidelity = take(B);
    double* ft = take(B);
    L.rho = take((size_t)B * memory);
    (void)take(2 * (size_t)B);
    double* f_acc = take(2 * (size_t)B);
    L.cur_g0 = dc; L.acc_g0 = dc + BT;
    double2* raw_g0_t = dc + 2 * BT;
    L.cur_hs = dc + 3 * BT; L.acc_hs = L.cur_hs + BS;
    double2* raw_hs_t = L.acc_hs + BS;
    L.active = di; L.done = di + B; L.max_no = di + 2 * B;
    int* d_flags = di + 3 * B;
    L.nit = dl;
    long long* d_prev = ws->d_combo_prev[AQC_BUF_X2];   // [B][2]: positions of X2 written by the previous evaluation (the support of the lhs states)
    {   // weight = 1, max_no = 0, active = 1, X2 empty
        std::vector<double> ones(B, 1.0);
        std::vector<int> one_i(B, 1);
        HIP_OK(hipMemcpyAsync(L.weight, ones.data(), sizeof(double) * B, hipMemcpyHostToDevice, st_));
        HIP_OK(hipMemcpyAsync(L.active, one_i.data(), sizeof(int) * B, hipMemcpyHostToDevice, st_));
        HIP_OK(hipMemsetAsync(dl, 0, sizeof(long long) * B, st_));
        HIP_OK(hipMemsetAsync(d_prev, 0xff, sizeof(long long) * 2 * B, st_));   // -1: nothing written yet
        HIP_OK(hipMemcpyAsync(L.x, x0, sizeof(double) * BT, hipMemcpyHostToDevice, st_));
        HIP_OK(hipMemsetAsync(ws->bufs[AQC_BUF_X2], 0, sizeof(double2) * (size_t)B * ws->lane_elems, st_));
        lhs_support_changed(ws, AQC_BUF_X2);   // (nothing, so far)
        HIP_OK(hipStreamSynchronize(st_));
    }
    int64_t nfev = 0;
    auto read_flags = [&]() -> int {
        HIP_OK(hipMemcpyAsync(h_flags, d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, st_));
        HIP_OK(hipStreamSynchronize(st_));
        return 0;
    };
    // f, g at the point in the workspace's theta buffer; raw results to (raw_hs, raw_g).  V^H, the amplitudes, the lane's
    // combined lhs state (lb_prepare) and ONE sweep from it -- no host round trip inside an evaluation.
    auto evaluate = [&](int update, double* f_o, double* g_o, double2* raw_hs, double2* raw_g) -> int {
        if (run_coef(ws, ws->d_thetas_own)) return 1;
        EvalRoute route;   // V^H (where the gather and the sweep read it), the gather, the sweep; the lhs state is picked in between
        route.x_buf = AQC_BUF_X2; route.vdag = route.new_thetas = route.gather = route.grads = route.support_in_gather_set = true;
        if (eval_route(ws, route)) return 1;
        if (enqueue_vdag(ws, route) || enqueue_gather(ws, route)) return 1;
        HIP_OK(lb_prepare(L, ws->d_small, update, f_o, raw_hs, ws->bufs[AQC_BUF_X2], ws->lane_elems, ws->d_index, d_prev, st_));
        lhs_support_changed(ws, AQC_BUF_X2);   // (the leading flip state is chosen on the device: the support may have moved)
        if (grad_from_impl(ws, route, block_from, block_to, front_layer)) return 1;
        HIP_OK(lb_take(L, ws->d_grads, g_o, raw_g, st_));
        ++nfev;
        return 0;
    };
    HIP_OK(hipMemcpyAsync(ws->d_thetas_own, L.x, sizeof(double) * BT, hipMemcpyDeviceToDevice, st_));
    if (evaluate(1, L.f, L.g, L.cur_hs, L.cur_g0)) return 1;
    int count = 0;
    for (int it = 0; it < maxiter; ++it) {
        HIP_OK(hipMemsetAsync(d_flags, 0, 4 * sizeof(int), st_));
        HIP_OK(lb_active(L, gtol, fid_thr, d_flags, st_));
        if (read_flags()) return 1;
        if (!h_flags[2]) break;
        HIP_OK(lb_direction(L, count, st_));
        HIP_OK(lb_copy_raw(L, st_));
        for (int bt = 0; bt < max_backtracks; ++bt) {
            HIP_OK(lb_trial(L, ws->d_thetas_own, st_));
            if (evaluate(0, ft, gt, raw_hs_t, raw_g0_t)) return 1;
            HIP_OK(hipMemsetAsync(d_flags + 3, 0, sizeof(int), st_));
            HIP_OK(lb_armijo(L, 1e-4, ws->d_thetas_own, ft, raw_hs_t, raw_g0_t, d_flags, st_));
            // the probe of the state update rides on the same read of the flags (it is only used once no lane backtracks any more)
            HIP_OK(hipMemsetAsync(d_flags + 1, 0, sizeof(int), st_));
            HIP_OK(lb_probe(L, L.acc_hs, d_flags, st_));
            if (read_flags()) return 1;
            if (!h_flags[3]) break;
        }
        // state update at the accepted points: from their raw results when no lane would lead with a flip state,
        // else by a device evaluation at x_new (the second sweep depends on the state chosen now)
        if (h_flags[1]) {   // (the last round's probe: nothing has touched the accepted points since)
            HIP_OK(hipMemcpyAsync(ws->d_thetas_own, L.x_new, sizeof(double) * BT, hipMemcpyDeviceToDevice, st_));
            if (evaluate(1, f_acc, g_acc, L.acc_hs, L.acc_g0)) return 1;
        } else {
            HIP_OK(lb_commit0(L, L.acc_hs, L.acc_g0, f_acc, g_acc, st_));
        }
        HIP_OK(lb_history(L, count, ftol, f_acc, g_acc, st_));
        ++count;
    }
    HIP_OK(hipMemcpyAsync(x_out, L.x, sizeof(double) * BT, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipMemcpyAsync(f_out, L.f, sizeof(double) * B, hipMemcpyDeviceToHost, st_));
    if (fidelity_out) HIP_OK(hipMemcpyAsync(fidelity_out, L.fidelity, sizeof(double) * B, hipMemcpyDeviceToHost, st_));
    if (nit_out) HIP_OK(hipMemcpyAsync(nit_out, L.nit, sizeof(long long) * B, hipMemcpyDeviceToHost, st_));
    if (weight_out) HIP_OK(hipMemcpyAsync(weight_out, L.weight, sizeof(double) * B, hipMemcpyDeviceToHost, st_));
    std::vector<int> h_max_no(B, 0);
    if (max_no_out) HIP_OK(hipMemcpyAsync(h_max_no.data(), L.max_no, sizeof(int) * B, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
    if (max_no_out) for (int b = 0; b < B; ++b) max_no_out[b] = h_max_no[b];
    if (nfev_out) *nfev_out = nfev;
    return 0;
}

// ---- device-resident multi-start L-BFGS on the matrix objective of full / fixed-sketch AQC (aqc_lbfgs.hip, state-free mode) ----
// f = 1 - Re tr(X^H V^H Y) / k per lane (sk_core.py:167-212 with a fixed X; X = I: full AQC, aqc_sketching.py:35-50).
// Preconditions (what BatchedSketchingObjective sets up): Y = U X, X the sketching matrix (identity for full AQC).  One evaluation is
// the chain of aqc_ws_sketch_adam without the generator: V^H Y into Z, the trace, the sweep from X, lb_mat_value.  The objective has
// no state, so the accepted trial's f and g are final and an iteration is direction, then trial / evaluation / Armijo / history per
// backtrack -- ordinary launches on the workspace's stream, one flag word read per trial, at most maxiter * max_backtracks of them.
int aqc_ws_lbfgs_mat(aqc_ws* ws, const double* x0, int maxiter, int memory, double gtol, double ftol, double fobj_thr, double fidelity_thr,
                     int max_backtracks, double* x_out, double* f_out, double* fidelity_out, int64_t* nit_out, int64_t* nfev_out,
                     int32_t* status_out) {
    if (!ws || !x0 || !x_out || !f_out) return fail("null argument");
    if (memory < 1 || memory > 32) return fail("the L-BFGS memory must be in [1, 32] (got %d)", memory);
    if (maxiter < 1 || max_backtracks < 1) return fail("maxiter and max_backtracks must be positive (got %d, %d)", maxiter, max_backtracks);
    if (!(gtol >= 0.0) || !(ftol >= 0.0) || !(fobj_thr >= 0.0) || !(fidelity_thr >= 0.0)) return fail("tolerances and thresholds must not be negative");
    if (ws->ctx->prog.trotter) return fail("matrix path does not support the Trotter ansatz");
    HIP_OK(hipSetDevice(ws->device));
    const Program& prog = ws->ctx->prog;
    const int B = ws->batch, T = prog.num_thetas();
    const size_t BT = (size_t)B * T;
    hipStream_t st_ = ws->stream;
    if (wait_result_copies(ws)) return 1;
    // the call rewrites Z, W and ZW
    if (before_write(ws, AQC_BUF_ZW) || before_write(ws, AQC_BUF_Z) || before_write(ws, AQC_BUF_W)) return 1;
    HIP_OK(hipStreamSynchronize(st_));
    // one allocation for all double arrays, one for the integers (the flag word last), one for the iteration counters
    const size_t nd = BT * (6 + 2 * (size_t)memory) + (size_t)B * (11 + memory), ni = 3 * (size_t)B + 1;
    DevBuf<double> dd;
    DevBuf<int> di;
    DevBuf<long long> dl;
    PinBuf<int> h_flag;
    if (dd.alloc(nd) || di.alloc(ni) || dl.alloc(B) || h_flag.alloc(1)) return 1;
    HIP_OK(hipMemsetAsync(dd, 0, nd * sizeof(double), st_));
    HIP_OK(hipMemsetAsync(di, 0, ni * sizeof(int), st_));
    HIP_OK(hipMemsetAsync(dl, 0, sizeof(long long) * B, st_));
    LbState L;
    LbMat M;
    memset(&L, 0, sizeof L);
    memset(&M, 0, sizeof M);
    double* p = dd;
    auto take = [&](size_t n) { double* r = p; p += n; return r; };
    L.B = B; L.T = T; L.S = 0; L.memory = memory;
    L.x = take(BT); L.g = take(BT); L.d = take(BT); L.x_new = take(BT);
    M.gt = take(BT); M.g_acc = take(BT);
    L.Smem = take(BT * memory); L.Ymem = take(BT * memory);
    L.f = take(B); L.slope = take(B); L.step = take(B); L.fidelity = take(B);
    M.gmax = take(B); M.ft = take(B); M.gmax_t = take(B); M.fid_t = take(B);
    M.f_acc = take(B); M.gmax_acc = take(B); M.fid_acc = take(B);
    L.rho = take((size_t)B * memory);
    L.active = di; L.done = di + B; M.status = di + 2 * B; M.flags = di + 3 * B;
    L.nit = dl;
    M.k = ws->ncols; M.gtol = gtol; M.fobj_thr = fobj_thr; M.fid_thr = fidelity_thr;
    HIP_OK(hipMemcpyAsync(L.x, x0, sizeof(double) * BT, hipMemcpyHostToDevice, st_));
    HIP_OK(hipMemcpyAsync(ws->d_thetas_own, L.x, sizeof(double) * BT, hipMemcpyDeviceToDevice, st_));
    HIP_OK(hipStreamSynchronize(st_));   // x0 may go away
    int64_t nfev = 0;
    auto evaluate = [&](int init) -> int {   // at the point in the workspace's theta buffer
        if (run_coef(ws, ws->d_thetas_own)) return 1;
        if (run_apply(ws, true, AQC_BUF_Y, AQC_BUF_Z)) return 1;        // V^H Y       (sk_core.py:191)
        if (aqc_ws_vdot_launch(ws, AQC_BUF_X, AQC_BUF_Z)) return 1;     // <X|V^H Y>   (:192)
        if (aqc_ws_grad_from(ws, AQC_BUF_X, -1, 0, 1)) return 1;        // the sweep   (:193)
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(lb_mat_value(L, M, ws->d_vdot_out, ws->d_grads, init, st_));
        ++nfev;
        return 0;
    };
    auto read_flag = [&]() -> int {   // the one word the host reads per trial (and once for the start point)
        HIP_OK(hipMemcpyAsync(h_flag, M.flags, sizeof(int), hipMemcpyDeviceToHost, st_));
        HIP_OK(hipStreamSynchronize(st_));
        return 0;
    };
    if (evaluate(1) || read_flag()) return 1;
    bool go_on = (h_flag[0] & kLbAnyActive) != 0;
    for (int count = 0; count < maxiter && go_on; ++count) {
        {
            ProfScope ps(ws, AQC_K_MISC);
            HIP_OK(lb_mat_direction(L, M, count, st_));
        }
        for (int bt = 0; bt < max_backtracks; ++bt) {
            const int last = bt + 1 == max_backtracks;
            {
                ProfScope ps(ws, AQC_K_MISC);
                HIP_OK(lb_trial(L, ws->d_thetas_own, st_));
            }
            if (evaluate(0)) return 1;   // (lb_mat_value clears the flag word for this trial)
            {
                ProfScope ps(ws, AQC_K_MISC);
                HIP_OK(lb_mat_armijo(L, M, 1e-4, ws->d_thetas_own, st_));
                HIP_OK(lb_mat_history(L, M, count, ftol, last, st_));   // (acts once the line search is over: see the kernel)
            }
            if (read_flag()) return 1;
            if (last || !(h_flag[0] & kLbNotDone)) break;
        }
        go_on = (h_flag[0] & kLbAnyActive) != 0;
    }
    // The theta buffer holds the last trial, which is not x_out on a lane that rejected it or had stopped before: the point the call
    // returns goes back into use (Z, W and ZW keep what that trial left: unspecified)
    HIP_OK(hipMemcpyAsync(ws->d_thetas_own, L.x, sizeof(double) * BT, hipMemcpyDeviceToDevice, st_));
    if (run_coef(ws, ws->d_thetas_own)) return 1;
    std::vector<int> h_status(B, 0);
    HIP_OK(hipMemcpyAsync(x_out, L.x, sizeof(double) * BT, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipMemcpyAsync(f_out, L.f, sizeof(double) * B, hipMemcpyDeviceToHost, st_));
    if (fidelity_out) HIP_OK(hipMemcpyAsync(fidelity_out, L.fidelity, sizeof(double) * B, hipMemcpyDeviceToHost, st_));
    if (nit_out) HIP_OK(hipMemcpyAsync(nit_out, L.nit, sizeof(long long) * B, hipMemcpyDeviceToHost, st_));
    if (status_out) HIP_OK(hipMemcpyAsync(h_status.data(), M.status, sizeof(int) * B, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
    if (status_out) for (int b = 0; b < B; ++b) status_out[b] = h_status[b];
    if (nfev_out) *nfev_out = nfev;
    return 0;
}

// One evaluation of the lane-batched surrogate objective without the host inside it: V^H, the flip-state amplitudes, the
// optional state update (hysteresis + weight smoothing, objective_lhs_sur_max.py:113-117,186), the value, the combined lhs
// state of every lane and ONE sweep from it (see aqc_ws_set_combo) -- the evaluate step of aqc_ws_lbfgs as a call of its own.
// Same preconditions: targets in Y, flip-state indices registered (state 0 first), X2 is used for the lhs states.
int aqc_ws_surrogate_eval(aqc_ws* ws, const double* thetas, int update_state, double* weight_io, int64_t* max_no_io, int block_from,
                          int block_to, int front_layer, double* f_out, double* fidelity_out, double* hs_out, double* grads_out,
                          double* grad_real_out) {
    if (!ws || !thetas || !weight_io || !max_no_io || !f_out || !(grads_out || grad_real_out)) return fail("null argument");
    if (ws->ncols != 1) return fail("the surrogate objective works on state-vector workspaces");
    if (ws->gather_count < 1) return fail("aqc_ws_gather_setup has not been called (flip-state indices, state 0 first)");
    if (update_state < 0 || update_state > 2) return fail("update_state is 0 (none), 1 (hysteresis and weight) or 2 (hysteresis only)");
    if (check_block_range(ws, block_from, block_to)) return 1;
    HIP_OK(hipSetDevice(ws->device));
    if (wait_result_copies(ws)) return 1;
    const Program& prog = ws->ctx->prog;
    const int B = ws->batch, T = prog.num_thetas(), S = ws->gather_count;
    const size_t nth = (size_t)B * T;
    for (int b = 0; b < B; ++b)
        if (max_no_io[b] < 0 || max_no_io[b] >= S) return fail("leading state %lld of lane %d out of range", (long long)max_no_io[b], b);
    hipStream_t st = ws->stream;
    const size_t ndbl = (size_t)B * (3 + 2 * (size_t)S), bytes = ndbl * sizeof(double) + (size_t)B * sizeof(int);
    if (ws->sur_states != S) {
        HIP_OK(hipStreamSynchronize(st));
        if (ws->d_sur.release() || ws->h_sur.release()) return 1;
        ws->sur_states = 0;
        if (ws->d_sur.alloc(bytes) || ws->h_sur.alloc(bytes)) return 1;
        ws->sur_states = S;
    }
    double* hd = reinterpret_cast<double*>((char*)ws->h_sur);
    // Small problems (single evaluations above all): no copy nodes -- the kernels read the thetas and the objective state from
    // pinned host memory and write the state block and a second copy of the gradient straight back into it (as aqc_ws_eval does)
    const bool zero_copy = sizeof(double2) * (nth + (size_t)B * S) <= 65536;
    const bool direct = direct_thetas(ws, zero_copy);
    double* dd = zero_copy ? hd : reinterpret_cast<double*>((char*)ws->d_sur);
    MirrorScope mirror_scope(ws, zero_copy ? ws->h_pin + ws->pin_thetas : nullptr, nullptr);
    LbState L;
    memset(&L, 0, sizeof L);
    L.B = B; L.T = T; L.S = S;
    double* d_f = dd;
    L.fidelity = dd + B;
    L.weight = dd + 2 * (size_t)B;
    double2* d_hs = reinterpret_cast<double2*>(dd + 3 * (size_t)B);
    L.max_no = reinterpret_cast<int*>(dd + ndbl);
    int* h_max = reinterpret_cast<int*>(hd + ndbl);
    // state in: weight and leading state of every lane
    memcpy(hd + 2 * (size_t)B, weight_io, sizeof(double) * B);
    for (int b = 0; b < B; ++b) h_max[b] = (int)max_no_io[b];
    double* pin_th = ws->h_pin;
    double* pin_gr = ws->h_pin + ws->pin_thetas;
    memcpy(pin_th, thetas, sizeof(double) * nth);
    if (ws->d_combo_prev[AQC_BUF_X2].reserve(2 * (size_t)B)) return 1;   // (combo_valid is false without it)
    if (!ws->combo_valid[AQC_BUF_X2]) {   // (outside the replayed part: a whole-buffer clear is a one-off)
        HIP_OK(hipMemsetAsync(ws->bufs[AQC_BUF_X2], 0, sizeof(double2) * (size_t)B * ws->lane_elems, st));
        HIP_OK(hipMemsetAsync(ws->d_combo_prev[AQC_BUF_X2], 0xff, sizeof(long long) * 2 * B, st));   // -1: nothing to clear
        lhs_support_changed(ws, AQC_BUF_X2);
    }
    EvalRoute route;   // as the evaluate step of aqc_ws_lbfgs
    route.x_buf = AQC_BUF_X2; route.vdag = route.new_thetas = route.gather = route.grads = route.support_in_gather_set = true;
    if (eval_route(ws, route)) return 1;
    const bool real_only = !zero_copy && !grads_out;
    if (real_only && ws->d_sur_real.capacity() < nth) {
        HIP_OK(hipStreamSynchronize(st));
        if (ws->d_sur_real.reserve(nth)) return 1;
    }
    auto enqueue = [&]() -> int {   // everything between the host copies of the inputs and the final synchronisation
        if (!zero_copy) {
            HIP_OK(hipMemcpyAsync(L.weight, hd + 2 * (size_t)B, sizeof(double) * B, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(L.max_no, h_max, sizeof(int) * B, hipMemcpyHostToDevice, st));
        }
        if (!direct) HIP_OK(hipMemcpyAsync(ws->d_thetas_own, pin_th, sizeof(double) * nth, hipMemcpyHostToDevice, st));
        if (run_coef(ws, ws->d_thetas_own)) return 1;
        ws->theta_host = direct ? pin_th : nullptr;   // the U builder reads the pinned thetas and stores them to HBM
        if (enqueue_vdag(ws, route) || enqueue_gather(ws, route)) return 1;
        {
            ProfScope ps(ws, AQC_K_MISC);
            HIP_OK(lb_prepare(L, ws->d_small, update_state, d_f, d_hs, ws->bufs[AQC_BUF_X2], ws->lane_elems, ws->d_index,
                              ws->d_combo_prev[AQC_BUF_X2], st));
            lhs_support_changed(ws, AQC_BUF_X2);
        }
        // (update_state == 0 leaves weight / max_no / fidelity as they came in; fidelity is only written by an update)
        if (grad_from_impl(ws, route, block_from, block_to, front_layer)) return 1;
        ws->theta_host = nullptr;
        if (!zero_copy) {
            if (real_only) {   // the surrogate's gradient is the real part: half the bytes over the bus, no pass over them on the host
                HIP_OK(lb_take(L, ws->d_grads, ws->d_sur_real, nullptr, st));
                HIP_OK(hipMemcpyAsync(pin_gr, ws->d_sur_real, sizeof(double) * nth, hipMemcpyDeviceToHost, st));
            } else {
                HIP_OK(hipMemcpyAsync(pin_gr, ws->d_grads, sizeof(double2) * nth, hipMemcpyDeviceToHost, st));
            }
            HIP_OK(hipMemcpyAsync(hd, dd, bytes, hipMemcpyDeviceToHost, st));
        }
        return 0;
    };
    if (ws->sw.graph && !ws->profile) {   // the launch sequence is replayed as a graph, as in aqc_ws_eval
        const long long tag = 1000 + update_state + (zero_copy ? 10 : 0) + (real_only ? 20 : 0);   // (1000: no key of aqc_ws_eval)
        if (run_graph(ws, route, {tag, block_from, block_to, front_layer, (long long)S, (long long)(size_t)(double*)ws->d_sur_real, (long long)(size_t)(char*)ws->d_sur,
                                  (long long)(size_t)(char*)ws->h_sur}, enqueue)) return 1;
    } else if (enqueue()) {
        return 1;
    }
    HIP_OK(hipStreamSynchronize(st));
    if (real_only) {
        memcpy(grad_real_out, pin_gr, sizeof(double) * nth);
    } else {
        if (grads_out) memcpy(grads_out, pin_gr, sizeof(double2) * nth);
        if (grad_real_out)
            for (size_t i = 0; i < nth; ++i) grad_real_out[i] = pin_gr[2 * i];
    }
    memcpy(f_out, hd, sizeof(double) * B);
    if (update_state) {
        if (fidelity_out) memcpy(fidelity_out, hd + B, sizeof(double) * B);
        memcpy(weight_io, hd + 2 * (size_t)B, sizeof(double) * B);
        for (int b = 0; b < B; ++b) max_no_io[b] = h_max[b];
    }
    if (hs_out) memcpy(hs_out, hd + 3 * (size_t)B, sizeof(double2) * (size_t)B * S);
    return 0;
}

}  // extern "C"
