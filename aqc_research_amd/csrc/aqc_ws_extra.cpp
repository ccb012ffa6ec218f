// C ABI (include/aqc_hip.h): dense zgemm, gate-level building blocks, the XXZ chain, reduced density matrices, coordinate descent, MPS helpers.
#include "aqc_ws.h"

#include <chrono>

#include "aqc_cd_rule.h"
#include "aqc_mps_contract.h"
#include "aqc_obs_rule.h"
#include "aqc_xxz_rule.h"

using namespace aqc;

static double wall_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern "C" {

// the workspace's grow-only scratch (MPS helpers)
static int mps_scratch(aqc_ws* ws, size_t n_cplx) {
    if (n_cplx <= ws->d_mps_scratch.capacity()) return 0;
    HIP_OK(hipStreamSynchronize(ws->stream));   // launches in flight may still read the block that goes
    return ws->d_mps_scratch.reserve(n_cplx);
}

// ---- dense zgemm with host pointers ---------------------------------------------------------------

int aqc_zgemm(int device, int conj_trans_a, int M, int N, int K, const double* A, int lda, const double* B, int ldb,
              double* C, int ldc) {
    if (!A || !B || !C || M < 1 || N < 1 || K < 1) return fail("invalid zgemm arguments");
    const int a_rows = conj_trans_a ? K : M, a_cols = conj_trans_a ? M : K;
    if (lda < a_cols || ldb < N || ldc < N) return fail("invalid leading dimension");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device out of range");
    HIP_OK(hipSetDevice(device));
    DevBuf<double2> dA, dB, dC;
    const size_t na = (size_t)a_rows * lda, nb = (size_t)K * ldb, nc = (size_t)M * ldc;
    if (dA.alloc(na) || dB.alloc(nb) || dC.alloc(nc)) return 1;
    hipError_t e = hipMemcpy(dA, A, na * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dB, B, nb * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess && ldc != N) e = hipMemcpy(dC, C, nc * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_zgemm(conj_trans_a != 0, false, M, N, K, dA, lda, dB, ldb, dC, ldc, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(C, dC, nc * sizeof(double2), hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : fail("aqc_zgemm failed: %s", hipGetErrorString(e));
}

// ---- gate-level building blocks (one-shot, host pointers) ---------------------------------------

namespace {

int gate_args_ok(int device, int n, int64_t ncols) {
    if (n < 1 || n > 30 || ncols < 1 || ((size_t)ncols << n) > ((size_t)1 << kMaxBits)) return fail("invalid array shape");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device out of range");
    return 0;
}

}  // namespace

int aqc_gate_1q(int device, int n, int64_t ncols, int qubit, const double* gate, const double* src, double* dst) {
    if (!gate || !src || !dst) return fail("null argument");
    if (gate_args_ok(device, n, ncols)) return 1;
    if (qubit < 0 || qubit >= n) return fail("qubit out of range");
    HIP_OK(hipSetDevice(device));
    const size_t bytes = sizeof(double2) * ((size_t)ncols << n);
    DevBuf<double2> d;
    if (d.alloc((size_t)ncols << n)) return 1;
    HIP_OK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    HIP_OK(launch_gate1q(d, d, n, (size_t)ncols, qubit, gate, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int aqc_gate_2q(int device, int n, int64_t ncols, int ctrl, int targ, const double* gate, const double* src, double* dst) {
    if (!gate || !src || !dst) return fail("null argument");
    if (gate_args_ok(device, n, ncols)) return 1;
    if (n < 2 || ctrl < 0 || ctrl >= n || targ < 0 || targ >= n || ctrl == targ) return fail("invalid qubit pair");
    HIP_OK(hipSetDevice(device));
    const size_t bytes = sizeof(double2) * ((size_t)ncols << n);
    DevBuf<double2> d;
    if (d.alloc((size_t)ncols << n)) return 1;
    HIP_OK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    HIP_OK(launch_gate2q(d, d, n, (size_t)ncols, ctrl, targ, gate, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int aqc_gate_dot(int device, int n, int64_t ncols, int kind, int q0, int q1, const double* w, const double* z, double* out) {
    if (!w || !z || !out) return fail("null argument");
    if (gate_args_ok(device, n, ncols)) return 1;
    if (kind < 0 || kind > 3 || q0 < 0 || q0 >= n) return fail("invalid inner-product kind or qubit");
    if (kind == 3 && (n < 2 || q1 < 0 || q1 >= n || q1 == q0)) return fail("invalid qubit pair");
    HIP_OK(hipSetDevice(device));
    const size_t bytes = sizeof(double2) * ((size_t)ncols << n);
    DevBuf<double2> dw, dz, dp;
    if (dw.alloc((size_t)ncols << n) || dz.alloc((size_t)ncols << n) || dp.alloc((size_t)(gate_dot_parts(n, (size_t)ncols, kind) + 1))) return 1;
    HIP_OK(hipMemcpy(dw, w, bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dz, z, bytes, hipMemcpyHostToDevice));
    double2* parts = dp;
    HIP_OK(launch_gate_dot(dw, dz, n, (size_t)ncols, kind, q0, q1, parts + 1, parts, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, parts, sizeof(double2), hipMemcpyDeviceToHost));
    return 0;
}

// ---- matrix-free XXZ Hamiltonian and exact evolution (one-shot, host pointers; kernels: aqc_xxz.hip) -------------

namespace {

int xxz_args_ok(int device, int n, int lanes, double delta) {
    if (n < kXxzMinQubits || n > kXxzMaxQubits || lanes < 1 || ((size_t)lanes << n) > ((size_t)1 << kMaxBits))
        return fail("invalid state shape: %d lanes of %d qubits", lanes, n);
    if (!std::isfinite(delta)) return fail("delta is not finite");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return fail("device out of range");
    return 0;
}

XxzArgs xxz_args(int n, int lanes, double delta) {
    XxzArgs a{};
    a.n = n; a.tile_bits = xxz_tile_bits(n); a.lanes = lanes; a.delta = delta;
    return a;
}

}  // namespace

int aqc_xxz_mul_vec(int device, int n, int lanes, double delta, const double* src, double* dst) {
    if (!src || !dst) return fail("null argument");
    if (xxz_args_ok(device, n, lanes, delta)) return 1;
    HIP_OK(hipSetDevice(device));
    const size_t count = (size_t)lanes << n, bytes = sizeof(double2) * count;
    DevBuf<double2> d_src, d_dst;
    if (d_src.alloc(count) || d_dst.alloc(count)) return 1;
    HIP_OK(hipMemcpy(d_src, src, bytes, hipMemcpyHostToDevice));
    XxzArgs a = xxz_args(n, lanes, delta);
    a.cur = d_src; a.cur_stride = (size_t)1 << n; a.next = d_dst;
    HIP_OK(launch_xxz_mul(a, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dst, d_dst, bytes, hipMemcpyDeviceToHost));
    return 0;
}

int aqc_xxz_energy(int device, int n, int lanes, double delta, const double* src, double* energy) {
    if (!src || !energy) return fail("null argument");
    if (xxz_args_ok(device, n, lanes, delta)) return 1;
    HIP_OK(hipSetDevice(device));
    const size_t count = (size_t)lanes << n, ntiles = (size_t)1 << (n - xxz_tile_bits(n));
    DevBuf<double2> d_src;
    DevBuf<double> d_part, d_energy;
    if (d_src.alloc(count) || d_part.alloc(ntiles * (size_t)lanes) || d_energy.alloc((size_t)lanes)) return 1;
    HIP_OK(hipMemcpy(d_src, src, sizeof(double2) * count, hipMemcpyHostToDevice));
    XxzArgs a = xxz_args(n, lanes, delta);
    a.cur = d_src; a.cur_stride = (size_t)1 << n; a.partial = d_part;
    HIP_OK(launch_xxz_energy(a, d_energy, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(energy, d_energy, sizeof(double) * (size_t)lanes, hipMemcpyDeviceToHost));
    return 0;
}

int aqc_xxz_evolve(int device, int n, int lanes, int shared_src, double delta, const double* times, const double* src, double* dst,
                   int32_t* terms_out) {
    if (!times || !src || !dst) return fail("null argument");
    if (xxz_args_ok(device, n, lanes, delta)) return 1;
    for (int l = 0; l < lanes; ++l)
        if (!std::isfinite(times[l])) return fail("evolution time of lane %d is not finite", l);
    // the series of every lane: c_k = 2 (-i)^k J_k(R t), table [k][lane], zero beyond a lane's own length
    const double radius = xxz_radius(n, delta);
    std::vector<std::vector<double>> bessel((size_t)lanes);
    int kmax = 0;
    for (int l = 0; l < lanes; ++l) {
        const int k = xxz_series(std::fabs(radius * times[l]), bessel[(size_t)l]);
        if (k < 0) return fail("lane %d: |R t| = %g needs more than %d terms", l, std::fabs(radius * times[l]), (int)kXxzMaxTerms);
        if (terms_out) terms_out[l] = k;
        kmax = std::max(kmax, k);
    }
    std::vector<double2> coef((size_t)(kmax + 1) * (size_t)lanes, make_double2(0.0, 0.0));
    for (int l = 0; l < lanes; ++l) {
        const std::vector<double>& j = bessel[(size_t)l];
        for (size_t k = 0; k < j.size(); ++k) {
            double2& c = coef[k * (size_t)lanes + (size_t)l];
            xxz_coefficient((int)k, j[k], times[l] < 0.0, c.x, c.y);
        }
    }
    HIP_OK(hipSetDevice(device));
    const size_t dim = (size_t)1 << n, count = (size_t)lanes << n, src_count = shared_src ? dim : count;
    DevBuf<double2> d_src, d_a, d_b, d_out, d_coef;
    if (d_src.alloc(src_count) || d_a.alloc(count) || d_b.alloc(count) || d_out.alloc(count) || d_coef.upload(coef)) return 1;
    HIP_OK(hipMemcpy(d_src, src, sizeof(double2) * src_count, hipMemcpyHostToDevice));
    XxzArgs a = xxz_args(n, lanes, delta);
    a.out = d_out; a.coef0 = d_coef;
    const size_t src_stride = shared_src ? 0 : dim;
    double2 *pa = d_a, *pb = d_b;
    for (int k = 1; k <= kmax; ++k) {   // T_k = (2/R) H T_{k-1} - T_{k-2} into the buffer of T_{k-2}; out += c_k T_k
        a.coef = static_cast<const double2*>(d_coef) + (size_t)k * (size_t)lanes;
        a.first = k == 1;
        a.scale = (k == 1 ? 1.0 : 2.0) / radius;
        if (k == 1) { a.cur = d_src; a.cur_stride = src_stride; a.prev = nullptr; a.prev_stride = 0; a.next = pa; }
        else if (k == 2) { a.cur = pa; a.cur_stride = dim; a.prev = d_src; a.prev_stride = src_stride; a.next = pb; }
        else if (k & 1) { a.cur = pb; a.cur_stride = dim; a.prev = pa; a.prev_stride = dim; a.next = pa; }
        else { a.cur = pa; a.cur_stride = dim; a.prev = pb; a.prev_stride = dim; a.next = pb; }
        HIP_OK(launch_xxz_step(a, nullptr));
    }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dst, d_out, sizeof(double2) * count, hipMemcpyDeviceToHost));
    return 0;
}

// ---- reduced density matrices (one-shot, host pointers; kernels: aqc_obs.hip, plan and partial trace: aqc_obs_rule.h) ----

namespace {

static_assert(AQC_OBS_TILE_BITS == kObsTileBits && AQC_OBS_LOW_BITS == kObsLowBits && AQC_OBS_MAX_SUBSETS == kObsMaxSubsets,
              "the constants of the header and of the rule");

// requests [count][k] -> masks of qubits (a single qubit is paired with another one: the plan covers sets of 2 to 4)
int obs_requests(int n, int k, int count, const int32_t* qubits, std::vector<uint32_t>& req) {
    if (n < kObsMinQubits || n > kObsMaxQubits) return fail("invalid number of qubits %d (%d to %d)", n, (int)kObsMinQubits, (int)kObsMaxQubits);
    if (count < 1) return fail("expects at least one set of qubits");
    if (k < 1 || k > kObsSetBits || k > n) return fail("a set holds 1 to min(4, n) qubits, not %d", k);
    if (!qubits) return fail("null argument");
    req.assign((size_t)count, 0);
    for (int s = 0; s < count; ++s) {
        uint32_t m = 0;
        for (int i = 0; i < k; ++i) {
            const int q = qubits[(size_t)s * k + i];
            if (q < 0 || q >= n) return fail("set %d: qubit %d out of range (%d qubits)", s, q, n);
            if ((m >> q) & 1u) return fail("set %d: qubit %d is listed twice", s, q);
            m |= 1u << q;
        }
        if (k == 1) m |= (m & 1u) ? 2u : 1u;
        req[(size_t)s] = m;
    }
    return 0;
}

}  // namespace

int aqc_obs_plan(int n, int npairs, const int32_t* pairs, int max_passes, int max_subsets, int32_t* npasses, int32_t* nsubsets,
                 int32_t* pass_bits, int32_t* pass_nsub, int32_t* subsets, int32_t* serves) {
    if (!npasses || !nsubsets) return fail("null argument");
    std::vector<uint32_t> req;
    if (obs_requests(n, 2, npairs, pairs, req)) return 1;
    const ObsPlan plan = obs_plan(n, req);
    size_t total = 0;
    for (const ObsPass& p : plan.passes) total += p.subsets.size();
    *npasses = (int32_t)plan.passes.size();
    *nsubsets = (int32_t)total;
    if ((size_t)std::max(max_passes, 0) < plan.passes.size() || (size_t)std::max(max_subsets, 0) < total)
        return fail("the plan has %zu passes and %zu subsets: the arrays hold %d and %d", plan.passes.size(), total, max_passes, max_subsets);
    if (!pass_bits || !pass_nsub || !subsets || !serves) return fail("null argument");
    size_t at = 0;
    for (size_t p = 0; p < plan.passes.size(); ++p) {
        const ObsPass& ps = plan.passes[p];
        int32_t* row = pass_bits + p * kObsTileBits;
        int filled = 0;
        for (int q = 0; q < n; ++q)
            if ((ps.bits >> q) & 1u) row[filled++] = q;
        for (; filled < kObsTileBits; ++filled) row[filled] = -1;
        pass_nsub[p] = (int32_t)ps.subsets.size();
        for (const uint16_t S : ps.subsets) {
            int m = 0;
            for (int b = 0; b < kObsTileBits; ++b)
                if ((S >> b) & 1u) subsets[4 * at + m++] = b;
            ++at;
        }
    }
    for (int r = 0; r < npairs; ++r) {
        serves[2 * r] = plan.serve_pass[(size_t)r];
        serves[2 * r + 1] = plan.serve_subset[(size_t)r];
    }
    return 0;
}

int aqc_obs_rdm(int device, int n, int lanes, const double* src, int k, int nsets, const int32_t* qubits, double* out) {
    if (!src || !out) return fail("null argument");
    std::vector<uint32_t> req;
    if (obs_requests(n, k, nsets, qubits, req)) return 1;
    if (xxz_args_ok(device, n, lanes, 0.0)) return 1;
    const ObsPlan plan = obs_plan(n, req);
    std::vector<size_t> first(plan.passes.size() + 1, 0);
    size_t max_sub = 0;
    for (size_t p = 0; p < plan.passes.size(); ++p) {
        first[p + 1] = first[p] + plan.passes[p].subsets.size();
        max_sub = std::max(max_sub, plan.passes[p].subsets.size());
    }
    for (size_t r = 0; r < req.size(); ++r)
        if (plan.serve_pass[r] < 0) return fail("set %zu has no place in the plan", r);
    HIP_OK(hipSetDevice(device));
    const int tb = std::min(n, (int)kObsTileBits);
    const unsigned gx = obs_grid_x(n, tb);
    const size_t count = (size_t)lanes << n, total = first.back();
    DevBuf<double2> d_src, d_rho;
    DevBuf<double> d_part;
    if (d_src.alloc(count) || d_rho.alloc((size_t)lanes * total * 256) || d_part.alloc((size_t)lanes * gx * max_sub * 768)) return 1;
    HIP_OK(hipMemcpy(d_src, src, sizeof(double2) * count, hipMemcpyHostToDevice));
    for (size_t p = 0; p < plan.passes.size(); ++p) {
        const ObsPass& ps = plan.passes[p];
        ObsArgs a{};
        a.n = n; a.tile_bits = tb; a.lanes = lanes; a.nsub = (int)ps.subsets.size(); a.ksplit = obs_ksplit(a.nsub); a.bits = ps.bits;
        for (size_t s = 0; s < ps.subsets.size(); ++s) a.subsets[s] = ps.subsets[s];
        a.src = d_src; a.partial = d_part;
        HIP_OK(launch_obs_pass(a, nullptr));
        HIP_OK(launch_obs_final(d_part, gx, a.nsub, lanes, static_cast<double2*>(d_rho) + first[p] * 256, total * 256, nullptr));
    }
    HIP_OK(hipDeviceSynchronize());
    std::vector<double2> rho((size_t)lanes * total * 256);
    HIP_OK(hipMemcpy(rho.data(), d_rho, sizeof(double2) * rho.size(), hipMemcpyDeviceToHost));
    // the partial traces, on the host: the place of every listed qubit in its subset's row index
    const size_t msize = (size_t)2 << (2 * k);   // doubles of a 2^k x 2^k matrix
    for (int s = 0; s < nsets; ++s) {
        const ObsPass& ps = plan.passes[(size_t)plan.serve_pass[(size_t)s]];
        const uint32_t S = ps.subsets[(size_t)plan.serve_subset[(size_t)s]];
        int pos[kObsSetBits];
        for (int m = 0; m < k; ++m) {
            const int q = qubits[(size_t)s * k + m];
            const int local = __builtin_popcount(ps.bits & ((1u << q) - 1));
            pos[m] = __builtin_popcount(S & ((1u << local) - 1));
        }
        const size_t which = first[(size_t)plan.serve_pass[(size_t)s]] + (size_t)plan.serve_subset[(size_t)s];
        for (int l = 0; l < lanes; ++l)
            obs_partial_trace(reinterpret_cast<const double*>(rho.data() + ((size_t)l * total + which) * 256), k, pos,
                              out + ((size_t)l * nsets + (size_t)s) * msize);
    }
    return 0;
}

// ---- coordinate descent ------------------------------------------------------------------------

static int cd_checks(const aqc_ws* ws) {
    const Program& prog = ws->ctx->prog;
    if (ws->ncols != (1 << prog.n)) return fail("coordinate descent needs a square workspace (ncols == 2^n)");
    if (prog.entangler == AQC_CP) return fail("CPhase entangler is not supported yet");
    if (prog.trotter) return fail("matrix path does not support the Trotter ansatz");
    return 0;
}

// the walk of core_op_matrix.py:852-912 cut into segments (address bits of this workspace): the persistent kernel reads the list on
// the device, the wide walk issues its launches from the host copy
static std::vector<aqc::CdSegHost> cd_segments(const aqc_ws* ws) {
    const Program& prog = ws->ctx->prog;
    std::vector<aqc::CdSegHost> segs;
    for (const GateGroup& g : prog.groups) {
        aqc::CdSegHost sg{};
        if (g.type == GROUP_FRONT) {   // Rz(t2), Ry(t1), Rz(t0) on one qubit; the second bit of the 4-element groups: any other qubit
            sg.ha = ws->col_bits + g.q0; sg.hb = ws->col_bits + (g.q0 + 1) % prog.n; sg.ent = 0; sg.nrot = 3;
            const int kinds[3] = {1, 0, 1}, tix[3] = {g.theta0 + 2, g.theta0 + 1, g.theta0};
            for (int r = 0; r < 3; ++r) { sg.kind[r] = kinds[r]; sg.on_b[r] = 0; sg.tindex[r] = tix[r]; }
        } else {                       // entangler, Ry(t0) Rz(t1) on the control, Ry(t2) Rs(t3) on the target
            sg.ha = ws->col_bits + g.q0; sg.hb = ws->col_bits + g.q1; sg.ent = prog.entangler == AQC_CX ? 1 : 2; sg.nrot = 4;
            const int kinds[4] = {0, 1, 0, prog.entangler == AQC_CX ? 2 : 1};
            for (int r = 0; r < 4; ++r) { sg.kind[r] = kinds[r]; sg.on_b[r] = r >= 2; sg.tindex[r] = g.theta0 + r; }
        }
        segs.push_back(sg);
    }
    return segs;
}

// ... on the device, with the thetas [batch][T] the persistent kernel and the driver keep there
static int cd_ensure_prog(aqc_ws* ws) {
    if (ws->d_cd_prog) return 0;
    const std::vector<aqc::CdSegHost> segs = cd_segments(ws);
    if (ws->d_cd_prog.upload(segs, 0)) return 1;
    ws->cd_nsteps = (int)segs.size();
    return ws->d_cd_thetas.reserve((size_t)ws->batch * ws->ctx->prog.num_thetas());
}

// The thetas in use when a coordinate-descent call returns are the point it returns, on either route: one device-to-device copy
// and one coefficient launch (what the workspace derived from the thetas in use before is stale after it).
static int cd_use_thetas(aqc_ws* ws, const double* d_point) {
    const size_t BT = (size_t)ws->batch * ws->ctx->prog.num_thetas();
    HIP_OK(hipMemcpyAsync(ws->d_thetas_own, d_point, sizeof(double) * BT, hipMemcpyDeviceToDevice, ws->stream));
    return run_coef(ws, ws->d_thetas_own);
}

int aqc_ws_cd_fits_one_launch(const aqc_ws* ws) {
    if (!ws) return 0;
    return aqc::cd_persistent_lds_bytes(ws->nbits, ws->ctx->prog.num_thetas()) <= (size_t)160 * 1024 ? 1 : 0;
}

int aqc_ws_cd_sweeps(aqc_ws* ws, double* thetas_io, double* fobj, int nsweeps, int max_steps) {
    if (!ws || !thetas_io || !fobj) return fail("null argument");
    if (nsweeps < 1) return fail("nsweeps must be positive");
    if (cd_checks(ws)) return 1;
    if (!aqc_ws_cd_fits_one_launch(ws))
        return fail("the operands of this coordinate descent (2 x %zu KiB) do not fit one workgroup's LDS: use aqc_ws_cd_minimize (the wide walk, any number of lanes)",
                    (ws->lane_elems * sizeof(double2)) >> 10);
    const Program& prog = ws->ctx->prog;
    const int T = prog.num_thetas();
    HIP_OK(hipSetDevice(ws->device));
    if (cd_ensure_prog(ws)) return 1;
    const size_t nf = (size_t)ws->batch * nsweeps;
    if (ws->d_cd_fobj.reserve(nf)) return 1;
    HIP_OK(hipMemcpyAsync(ws->d_cd_thetas, thetas_io, sizeof(double) * (size_t)ws->batch * T, hipMemcpyHostToDevice, ws->stream));
    {
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(aqc::launch_cd_persistent(ws->d_cd_prog, ws->cd_nsteps, ws->nbits, ws->col_bits, ws->bufs[AQC_BUF_Y], ws->lane_elems, ws->d_cd_thetas,
                                         T, ws->d_cd_fobj, nsweeps, max_steps, ws->batch, ws->stream));
    }
    if (cd_use_thetas(ws, ws->d_cd_thetas)) return 1;   // the point the call returns is the one in use
    HIP_OK(hipMemcpyAsync(thetas_io, ws->d_cd_thetas, sizeof(double) * (size_t)ws->batch * T, hipMemcpyDeviceToHost, ws->stream));
    HIP_OK(hipMemcpyAsync(fobj, ws->d_cd_fobj, sizeof(double) * nf, hipMemcpyDeviceToHost, ws->stream));
    HIP_OK(hipStreamSynchronize(ws->stream));
    return 0;
}

// One sweep of the wide walk for all lanes, enqueued: z = V(theta)^H U and w = I by the workspace's own launches, the walk's
// T + (n + L) launches, <w|z>, the close kernel.  d_thetas_own holds the thetas at the start of the sweep (the close kernel of the
// previous one wrote them: run_coef announces that, as aqc_ws_sketch_adam does for its ADAM step), d_cd_thetas the sweep's.
static int cd_wide_sweep(aqc_ws* ws, const std::vector<aqc::CdSegHost>& segs, const aqc::CdRule& rule, int max_steps) {
    const int B = ws->batch, T = ws->ctx->prog.num_thetas(), dim = 1 << ws->ctx->prog.n;
    if (run_coef(ws, ws->d_thetas_own)) return 1;
    if (run_apply(ws, true, AQC_BUF_Y, AQC_BUF_Z)) return 1;                     // z = V^H U   (core_op_matrix.py:806-810)
    if (aqc_ws_set_identity(ws, AQC_BUF_X)) return 1;                            // w = I
    if (before_write(ws, AQC_BUF_X) || before_write(ws, AQC_BUF_Z)) return 1;    // the walk rewrites both in place
    aqc::CdWide a;
    memset(&a, 0, sizeof a);
    a.w = ws->bufs[AQC_BUF_X]; a.z = ws->bufs[AQC_BUF_Z];
    a.lane_stride = ws->lane_elems;
    a.ngroups = (int)(ws->lane_elems >> 2);
    a.nparts = aqc::cd_wide_parts(ws->lane_elems);
    a.T = T;
    a.theta_in = ws->d_thetas_own; a.theta_out = ws->d_cd_thetas;
    a.dmax = ws->d_cd_real + B;
    a.status = rule.status;
    a.inv_d2n = 1.0 / ((double)dim * dim);
    double* const part[2] = {ws->d_cd_part, ws->d_cd_part + 4 * (size_t)B * a.nparts};
    int step = 0;                                                                // parameters walked so far: its parity picks the partial set
    const int limit = max_steps >= 0 ? max_steps : 0x7fffffff;
    for (const aqc::CdSegHost& sg : segs) {
        if (step >= limit) break;
        a.ha = sg.ha; a.hb = sg.hb; a.ent = sg.ent;
        a.next_kind = sg.kind[0]; a.next_on_b = sg.on_b[0];
        a.part_in = nullptr; a.part_out = part[step & 1];
        {
            ProfScope ps(ws, AQC_K_MISC);
            HIP_OK(aqc::launch_cd_wide_open(a, B, ws->stream));
        }
        for (int r = 0; r < sg.nrot && step < limit; ++r, ++step) {
            const bool last = r + 1 == sg.nrot || step + 1 >= limit;             // nothing reads the partials of a parameter that is not walked
            a.kind = sg.kind[r]; a.on_b = sg.on_b[r]; a.tindex = sg.tindex[r];
            a.next_kind = last ? -1 : sg.kind[r + 1]; a.next_on_b = last ? 0 : sg.on_b[r + 1];
            a.part_in = part[step & 1]; a.part_out = part[(step + 1) & 1];
            ProfScope ps(ws, AQC_K_MISC);
            HIP_OK(aqc::launch_cd_wide_step(a, B, ws->stream));
        }
    }
    if (aqc_ws_vdot_launch(ws, AQC_BUF_X, AQC_BUF_Z)) return 1;                  // <w|z>   (:917)
    aqc::CdClose c;
    memset(&c, 0, sizeof c);
    c.rule = rule;
    c.trace = ws->d_vdot_out;
    c.dmax = a.dmax;
    c.theta_own = ws->d_thetas_own; c.theta_cur = ws->d_cd_thetas;
    c.T = T;
    c.inv_d2n = a.inv_d2n;
    ProfScope ps(ws, AQC_K_MISC);
    HIP_OK(aqc::launch_cd_close(c, B, ws->stream));
    return 0;
}

static int cd_wide_size_check(const aqc_ws* ws) {
    if (ws->ctx->prog.n < 2 || ws->nbits > 30) return fail("coordinate descent serves 2 to 15 qubits");
    return 0;
}

// The driver on a workspace and arguments that have passed the checks of its two callers below.
static int cd_minimize_checked(aqc_ws* ws, const double* thetas0, int maxiter, int chunk, double dtheta_thr, double fobj_thr, double time_limit_s,
                               bool persistent, int max_steps, double* best_thetas, double* best_f, int64_t* nit, int32_t* status, double* profile,
                               bool sweep_point = false) {
    const Program& prog = ws->ctx->prog;
    const int B = ws->batch, T = prog.num_thetas();
    const size_t BT = (size_t)B * T;
    HIP_OK(hipSetDevice(ws->device));
    hipStream_t st = ws->stream;
    if (cd_ensure_prog(ws)) return 1;
    const int nparts = aqc::cd_wide_parts(ws->lane_elems);
    HIP_OK(hipStreamSynchronize(st));   // a buffer that grows lets its old block go
    if (ws->d_cd_best.reserve(BT) || ws->d_cd_real.reserve(2 * (size_t)B) || ws->d_cd_int.reserve(2 * (size_t)B + 1) ||
        ws->d_cd_profile.reserve((size_t)B * maxiter) || (!persistent && ws->d_cd_part.reserve(8 * (size_t)B * nparts))) return 1;
    aqc::CdRule rule;
    rule.status = ws->d_cd_int; rule.nit = rule.status + B;
    int* d_running = rule.nit + B;
    rule.best_f = ws->d_cd_real; rule.best_thetas = ws->d_cd_best; rule.profile = ws->d_cd_profile;
    rule.fobj_thr = fobj_thr; rule.dtheta_thr = dtheta_thr; rule.maxiter = maxiter;
    std::vector<double> real0(2 * (size_t)B, 0.0);   // best_f = inf | dmax = 0
    for (int b = 0; b < B; ++b) real0[b] = HUGE_VAL;
    HIP_OK(hipMemcpyAsync(ws->d_cd_real, real0.data(), sizeof(double) * 2 * B, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(ws->d_cd_int, 0, sizeof(int) * (2 * (size_t)B + 1), st));
    HIP_OK(hipMemsetAsync(ws->d_cd_profile, 0, sizeof(double) * (size_t)B * maxiter, st));
    HIP_OK(hipMemcpyAsync(ws->d_cd_thetas, thetas0, sizeof(double) * BT, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(ws->d_cd_best, thetas0, sizeof(double) * BT, hipMemcpyHostToDevice, st));
    if (!persistent) HIP_OK(hipMemcpyAsync(ws->d_thetas_own, thetas0, sizeof(double) * BT, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));   // thetas0 and real0 may go away
    const std::vector<aqc::CdSegHost> segs = persistent ? std::vector<aqc::CdSegHost>() : cd_segments(ws);
    const double t0 = wall_seconds();
    for (int done = 0; done < maxiter;) {
        const int n = std::min(chunk, maxiter - done);
        if (persistent) {
            ProfScope ps(ws, AQC_K_MISC);
            HIP_OK(aqc::launch_cd_persistent(ws->d_cd_prog, ws->cd_nsteps, ws->nbits, ws->col_bits, ws->bufs[AQC_BUF_Y], ws->lane_elems, ws->d_cd_thetas,
                                             T, nullptr, n, max_steps, B, st, &rule));
        } else {
            for (int i = 0; i < n; ++i)
                if (cd_wide_sweep(ws, segs, rule, max_steps)) return 1;
        }
        done += n;
        int running = 0;
        HIP_OK(aqc::launch_cd_count(rule.status, B, 0, d_running, st));
        HIP_OK(hipMemcpyAsync(&running, d_running, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (running == 0) break;
        if (time_limit_s > 0 && wall_seconds() - t0 >= time_limit_s) {   // the reference's TimeoutStopper, between chunks
            HIP_OK(aqc::launch_cd_count(rule.status, B, AQC_CD_TIMEOUT, d_running, st));
            break;
        }
    }
    // The wide route's last close kernel left the last sweep's thetas in the workspace's buffer, the persistent launch never touched
    // it: either way the point the caller gets back goes into use (best_thetas; the sweep's own for aqc_ws_cd_sweep)
    if (cd_use_thetas(ws, sweep_point ? ws->d_cd_thetas : ws->d_cd_best)) return 1;
    std::vector<int> h_int(2 * (size_t)B);
    HIP_OK(hipMemcpyAsync(best_thetas, ws->d_cd_best, sizeof(double) * BT, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(best_f, ws->d_cd_real, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(profile, ws->d_cd_profile, sizeof(double) * (size_t)B * maxiter, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_int.data(), ws->d_cd_int, sizeof(int) * 2 * B, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) { status[b] = h_int[b]; nit[b] = h_int[B + b]; }
    return 0;
}

int aqc_ws_cd_minimize(aqc_ws* ws, const double* thetas0, int maxiter, int chunk, double dtheta_thr, double fobj_thr, double time_limit_s,
                       int route, int max_steps, double* best_thetas, double* best_f, int64_t* nit, int32_t* status, double* profile) {
    static_assert(AQC_CD_RUNNING == aqc::kCdRunning && AQC_CD_NORMAL == aqc::kCdNormal && AQC_CD_EARLY == aqc::kCdEarly &&
                  AQC_CD_TIMEOUT == aqc::kCdTimeout, "the status words of the header and of the rule");
    if (!ws || !thetas0 || !best_thetas || !best_f || !nit || !status || !profile) return fail("null argument");
    if (maxiter < 1 || chunk < 1) return fail("maxiter and chunk must be positive");
    if (route < AQC_CD_ROUTE_AUTO || route > AQC_CD_ROUTE_WIDE) return fail("unknown coordinate-descent route %d", route);
    if (cd_checks(ws) || cd_wide_size_check(ws)) return 1;
    const bool fits = aqc_ws_cd_fits_one_launch(ws) != 0;
    if (route == AQC_CD_ROUTE_PERSISTENT && !fits)
        return fail("the operands of this coordinate descent (2 x %zu KiB) do not fit one workgroup's LDS: the persistent route is not available",
                    (ws->lane_elems * sizeof(double2)) >> 10);
    const bool persistent = route == AQC_CD_ROUTE_PERSISTENT || (route == AQC_CD_ROUTE_AUTO && fits);
    return cd_minimize_checked(ws, thetas0, maxiter, chunk, dtheta_thr, fobj_thr, time_limit_s, persistent, max_steps, best_thetas, best_f, nit,
                               status, profile);
}

int aqc_ws_cd_sweep(aqc_ws* ws, double* thetas_io, double* fobj) {
    if (!ws || !thetas_io || !fobj) return fail("null argument");
    if (cd_checks(ws)) return 1;
    if (ws->batch != 1) return fail("aqc_ws_cd_sweep takes thetas_io[T] and one objective value: a single-lane workspace (aqc_ws_cd_sweeps serves lanes)");
    if (aqc_ws_cd_fits_one_launch(ws) && !switch_now("AQC_CD_CHAIN")) return aqc_ws_cd_sweeps(ws, thetas_io, fobj, 1, -1);
    if (cd_wide_size_check(ws)) return 1;
    // One sweep of the driver on the wide route, stop rules off.  The sweep's own thetas and value (profile[0]) go back, not the best
    // ones: the close rule records a best value only below best_f, so a NaN sweep would come back as the start and inf.
    const int T = ws->ctx->prog.num_thetas();
    std::vector<double> best_thetas(T);
    double best_f = 0;
    int64_t nit = 0;
    int32_t status = 0;
    if (cd_minimize_checked(ws, thetas_io, 1, 1, 0.0, 0.0, 0.0, false, -1, best_thetas.data(), &best_f, &nit, &status, fobj, true)) return 1;
    HIP_OK(hipMemcpyAsync(thetas_io, ws->d_cd_thetas, sizeof(double) * T, hipMemcpyDeviceToHost, ws->stream));
    HIP_OK(hipStreamSynchronize(ws->stream));
    return 0;
}

// ---- MPS helpers ------------------------------------------------------------------------------


static int check_mps_slot(const aqc_ws* ws, int slot, bool need_data) {
    if (!ws) return fail("null workspace");
    if (ws->ncols != 1) return fail("MPS helpers need a state-vector workspace (ncols == 1)");
    if (slot < 0 || slot >= AQC_MPS_SLOTS) return fail("MPS slot %d out of range", slot);
    if (need_data && !ws->mps[slot].d_t) return fail("MPS slot %d is empty", slot);
    return 0;
}

int aqc_ws_mps_upload(aqc_ws* ws, int slot, const int32_t* dims, const double* gammas, const double* lambdas) {
    if (check_mps_slot(ws, slot, false)) return 1;
    const int n = ws->ctx->prog.n;
    if (n > 64) return fail("MPS helpers of the workspace serve up to 64 qubits");
    if (!dims || !gammas || (n > 1 && !lambdas)) return fail("null MPS argument");
    if (dims[0] != 1 || dims[n] != 1) return fail("MPS boundary bond dimensions must be 1");
    HIP_OK(hipSetDevice(ws->device));
    aqc_ws::MpsSlot& m = ws->mps[slot];
    m.dims.assign(dims, dims + n + 1);
    m.offset.assign(n + 1, 0);
    MpsSites sites;
    memset(&sites, 0, sizeof sites);
    sites.n = n;
    size_t total = 0, lam_total = 0;
    for (int q = 0; q < n; ++q) {
        if (dims[q] < 1 || dims[q + 1] < 1) return fail("MPS bond dimensions must be positive");
        m.offset[q] = total;
        sites.offset[q] = total;
        sites.cols[q] = dims[q + 1];
        sites.lam_offset[q] = (int)lam_total;
        total += (size_t)2 * dims[q] * dims[q + 1];
        if (q < n - 1) lam_total += dims[q + 1];
    }
    m.offset[n] = total;
    sites.offset[n] = total;
    sites.total = total;
    if (total > m.d_t.capacity() || lam_total > ws->d_mps_lam.capacity()) {   // grow-only device buffers
        HIP_OK(hipStreamSynchronize(ws->stream));
        if (m.d_t.reserve(total) || ws->d_mps_lam.reserve(lam_total)) return 1;
    }
    HIP_OK(hipMemcpyAsync(m.d_t, gammas, total * sizeof(double2), hipMemcpyHostToDevice, ws->stream));
    if (lam_total) {
        HIP_OK(hipMemcpyAsync(ws->d_mps_lam, lambdas, lam_total * sizeof(double), hipMemcpyHostToDevice, ws->stream));
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(launch_mps_scale_all(m.d_t, ws->d_mps_lam, sites, ws->stream));   // _preprocess_mps: lambda on the right bond
    }
    HIP_OK(hipStreamSynchronize(ws->stream));   // the host arrays (and the shared lambda staging) may be reused right away
    return 0;
}

// MPS -> dense state (mps_to_vector, mps_operations.py:159-189; index bit q <-> site q), contracted from both ends:
//   L[lo][chi]   = sites 0 .. h-1       (rows grow by appending the next site as the next HIGHER bit)
//   Rt[chi][i]   = sites n-1 .. h       (columns grow likewise, so i is the BIT-REVERSED high part of the index)
//   G = L Rt, then out[(rev(i) << h) + lo] = G[lo][i].
// O(2^(n/2) chi^2 + 2^n chi) flops instead of the O(2^n chi^2) of a one-sided sweep; both values of the site's bit go
// through one batched GEMM launch.
int aqc_ws_mps_to_vec(aqc_ws* ws, int slot, int buf, int lane) {
    if (check_mps_slot(ws, slot, true) || check_buf(ws, buf)) return 1;
    if (lane < 0 || lane >= ws->batch) return fail("lane out of range");
    HIP_OK(hipSetDevice(ws->device));
    const int n = ws->ctx->prog.n;
    if (n >= 2) {   // one (slot, lane) pair of the batched chain below
        const int32_t s1 = slot, l1 = lane;
        return aqc_ws_mps_to_vec_batch(ws, 1, &s1, buf, &l1);
    }
    // n == 1: the state is the site tensor itself, [b][1][1]
    if (before_write(ws, buf, true)) return 1;
    ProfScope ps(ws, AQC_K_MISC);
    HIP_OK(hipMemcpyAsync(ws->bufs[buf] + (size_t)lane * ws->lane_elems, ws->mps[slot].d_t, sizeof(double2) * 2, hipMemcpyDeviceToDevice, ws->stream));
    return 0;
}

// MPS -> dense (mps_operations.py:159-189) for `count` (slot, lane) pairs at once: MPS slots[i] -> lane lanes[i] of `buf`.
// When all the slots have the same bond dimensions (the lanes of a batched objective) every step of the chain is ONE launch
// for all lanes (zgemm over device pointer tables): (n/2 - 1) + (n - n/2 - 1) + 1 launches whatever the number of lanes, ONE
// for product states; otherwise the pairs are served one after the other.
static int mps_to_vec_batch_uniform(aqc_ws* ws, int count, const int32_t* slots, int buf, const int32_t* lanes);

int aqc_ws_mps_to_vec_batch(aqc_ws* ws, int count, const int32_t* slots, int buf, const int32_t* lanes) {
    if (!ws || !slots || !lanes || count < 1) return fail("invalid batched MPS arguments");
    if (check_buf(ws, buf)) return 1;
    for (int i = 0; i < count; ++i) {
        if (check_mps_slot(ws, slots[i], true)) return 1;
        if (lanes[i] < 0 || lanes[i] >= ws->batch) return fail("lane out of range");
    }
    if (ws->ctx->prog.n / 2 == 0) {
        for (int i = 0; i < count; ++i)
            if (aqc_ws_mps_to_vec(ws, slots[i], buf, lanes[i])) return 1;
        return 0;
    }
    // lanes whose operands share their bond dimensions share every launch of the contraction chain: one chain per distinct
    // dimension vector (truncated canonical tensors -- the reference's trunc_thr = 1e-6 -- differ from target to target by a
    // few bond entries; taking every such lane through a chain of its own made a 64-lane step 14x slower than equal bonds)
    std::vector<int> group(count, -1);
    int ngroups = 0;
    for (int i = 0; i < count; ++i) {
        if (group[i] >= 0) continue;
        group[i] = ngroups;
        for (int j = i + 1; j < count; ++j)
            if (group[j] < 0 && ws->mps[slots[j]].dims == ws->mps[slots[i]].dims) group[j] = ngroups;
        ++ngroups;
    }
    if (ngroups == 1) return mps_to_vec_batch_uniform(ws, count, slots, buf, lanes);
    std::vector<int32_t> gs, gl;
    for (int g = 0; g < ngroups; ++g) {
        gs.clear(); gl.clear();
        for (int i = 0; i < count; ++i)
            if (group[i] == g) { gs.push_back(slots[i]); gl.push_back(lanes[i]); }
        if (mps_to_vec_batch_uniform(ws, (int)gs.size(), gs.data(), buf, gl.data())) return 1;
    }
    return 0;
}

static int mps_to_vec_batch_uniform(aqc_ws* ws, int count, const int32_t* slots, int buf, const int32_t* lanes) {
    const int n = ws->ctx->prog.n;
    const int h = n / 2, mh = n - h;
    HIP_OK(hipSetDevice(ws->device));
    const std::vector<int>& dims = ws->mps[slots[0]].dims;
    const std::vector<size_t>& off = ws->mps[slots[0]].offset;
    if (before_write(ws, buf, true)) return 1;   // (lanes of Z are rewritten, not all of it)
    std::vector<const void*> tabs;
    auto table = [&](auto fn) { const size_t at = tabs.size(); for (int i = 0; i < count; ++i) tabs.push_back(fn(i)); return at; };
    auto out_lane = [&](int i) { return (const void*)(ws->bufs[buf] + (size_t)lanes[i] * ws->lane_elems); };
    const void* const* T = nullptr;
    auto upload_tables = [&]() -> int {   // pointer tables of every launch of the chain: a resident set, or one copy
        aqc_ws::MpsTabs* hit = nullptr;
        aqc_ws::MpsTabs* lru = &ws->mps_tabs[0];
        for (auto& t : ws->mps_tabs) {
            if (t.dev && t.host == tabs) hit = &t;
            if (t.tick < lru->tick) lru = &t;
        }
        if (!hit) {
            HIP_OK(hipStreamSynchronize(ws->stream));   // launches in flight may still read the set that is recycled
            if (lru->dev.reserve(tabs.size())) return 1;
            lru->host = tabs;   // (stays alive next to the device copy: nothing to wait for after the upload)
            HIP_OK(hipMemcpyAsync(lru->dev, lru->host.data(), tabs.size() * sizeof(void*), hipMemcpyHostToDevice, ws->stream));
            hit = lru;
        }
        hit->tick = ++ws->mps_tabs_tick;
        T = hit->dev;
        return 0;
    };
    bool product = true;
    for (int q = 0; q <= n; ++q) product = product && dims[q] == 1;
    if (product) {   // product states (|0>, the Neel state, ...: the usual lhs operand): one launch, no chain
        const size_t ta = table([&](int i) { return (const void*)ws->mps[slots[i]].d_t; });
        const size_t tc = table(out_lane);
        if (upload_tables()) return 1;
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(launch_mps_product(T + ta, (void* const*)(T + tc), n, count, ws->stream));
        return 0;
    }
    // Left half L[l][chi] (sites 0 .. h-1, site 0 the lowest bit of l), right half transposed Rt[r][chi] (sites n-1 .. h, every
    // new site becoming the LOWEST bit of r, so that site h ends up there), and out[r 2^h + l] = sum_chi Rt[r][chi] L[l][chi]
    // written by the last product straight into the lane's buffer in the workspace's bit order (bit q = site q): no
    // scratch copy of the dense state, no permutation pass.
    size_t need_l = 2, need_r = 2;
    for (int q = 0; q < h; ++q) need_l = std::max(need_l, ((size_t)2 << q) * dims[q + 1]);
    for (int q = n - 1; q >= h; --q) need_r = std::max(need_r, ((size_t)2 << (n - 1 - q)) * dims[q]);
    const size_t per = 2 * need_l + 2 * need_r;
    if (mps_scratch(ws, per * (size_t)count)) return 1;
    struct Step { int kind, q; size_t a, b, c; };   // offsets (in pointers) of the three tables inside the upload
    std::vector<Step> steps;
    auto lb = [&](int i, int k) { return (const void*)(ws->d_mps_scratch + per * (size_t)i + need_l * (size_t)k); };
    auto rb = [&](int i, int k) { return (const void*)(ws->d_mps_scratch + per * (size_t)i + 2 * need_l + need_r * (size_t)k); };
    auto site = [&](int i, int q) { return (const void*)(ws->mps[slots[i]].d_t + off[q]); };
    for (int q = 1; q < h; ++q) {       // left part: L_q = L_{q-1} T_q, both values of the site's bit (inner = 2)
        Step st{0, q, 0, 0, 0};
        st.a = q == 1 ? table([&](int i) { return site(i, 0); }) : table([&](int i) { return lb(i, (q - 1) & 1); });
        st.b = table([&](int i) { return site(i, q); });
        st.c = table([&](int i) { return lb(i, q & 1); });
        steps.push_back(st);
    }
    // right part: Rt_0 = the last site as it is stored ([2][chi][1] = [r][chi]); Rt_j[2 c + b] = Rt_{j-1}[c] T_q[b]^T
    for (int q = n - 2; q >= h; --q) {
        const int j = n - 1 - q;
        Step st{2, q, 0, 0, 0};
        st.a = j == 1 ? table([&](int i) { return site(i, n - 1); }) : table([&](int i) { return rb(i, (j - 1) & 1); });
        st.b = table([&](int i) { return site(i, q); });
        st.c = table([&](int i) { return rb(i, j & 1); });
        steps.push_back(st);
    }
    Step fin{3, 0, 0, 0, 0};
    fin.a = mh == 1 ? table([&](int i) { return site(i, n - 1); }) : table([&](int i) { return rb(i, (mh - 1) & 1); });
    fin.b = h == 1 ? table([&](int i) { return site(i, 0); }) : table([&](int i) { return lb(i, (h - 1) & 1); });
    fin.c = table(out_lane);
    steps.push_back(fin);
    if (upload_tables()) return 1;
    ProfScope ps(ws, AQC_K_MISC);
    // the two halves are independent chains of small launches (latency-bound at small bond dimensions): the right half runs
    // on a second stream, forked after everything queued so far and joined before the last product
    const bool fork = !ws->profile && !ws->capturing && h > 1 && mh > 1;
    if (fork) {
        if (!ws->mps_stream) {
            HIP_OK(hipStreamCreateWithFlags(&ws->mps_stream, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&ws->ev_mps_fork, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&ws->ev_mps_join, hipEventDisableTiming));
        }
        HIP_OK(hipEventRecord(ws->ev_mps_fork, ws->stream));
        HIP_OK(hipStreamWaitEvent(ws->mps_stream, ws->ev_mps_fork, 0));
    }
    for (const Step& st : steps) {
        hipStream_t sst = (fork && st.kind == 2) ? ws->mps_stream : ws->stream;
        if (fork && st.kind == 3) {
            HIP_OK(hipEventRecord(ws->ev_mps_join, ws->mps_stream));
            HIP_OK(hipStreamWaitEvent(ws->stream, ws->ev_mps_join, 0));
        }
        if (st.kind == 0) {
            const int q = st.q, rows = 1 << q, kk = dims[q], nn = dims[q + 1];
            HIP_OK(launch_zgemm_tables(rows, nn, kk, T + st.a, kk, T + st.b, nn, (void* const*)(T + st.c), nn, 0, (size_t)kk * nn, (size_t)rows * nn,
                                       count, 2, sst));
        } else if (st.kind == 2) {   // C rows 2 c + b: ldc = 2 chil, the bit's block starts chil further; B = T_q[b] stored [chil][chir], used transposed
            const int q = st.q, j = n - 1 - q, cols = 1 << j, chil = dims[q], chir = dims[q + 1];
            HIP_OK(launch_zgemm_tables(cols, chil, chir, T + st.a, chir, T + st.b, chir, (void* const*)(T + st.c), 2 * chil, 0, (size_t)chil * chir,
                                       (size_t)chil, count, 2, sst, 1));
        } else {                     // out [2^mh][2^h] = Rt [2^mh][chi] . L^T, L stored [2^h][chi]
            const int chi = dims[h];
            HIP_OK(launch_zgemm_tables(1 << mh, 1 << h, chi, T + st.a, chi, T + st.b, chi, (void* const*)(T + st.c), 1 << h, 0, 0, 0, count, 1,
                                       sst, 1));
        }
    }
    return 0;
}

namespace {

// the left steps of aqc_mps_contract.h on the workspace's stream, every launch an AQC_K_MISC event of the profile (the overlap chain is
// all the workspace runs: it needs no gemm_bh)
struct WsOps {
    aqc_ws* ws;
    int gemm(bool conj_t, bool accum, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc) {
        ProfScope ps(ws, AQC_K_MISC);
        HIP_OK(launch_zgemm(conj_t, accum, M, N, K, A, lda, B, ldb, C, ldc, ws->stream));
        return 0;
    }
};

}  // namespace

// <a|b> of two MPS slots: the overlap chain of aqc_mps_contract.h
int aqc_ws_mps_dot(aqc_ws* ws, int slot_a, int slot_b, double* out) {
    if (check_mps_slot(ws, slot_a, true) || check_mps_slot(ws, slot_b, true)) return 1;
    if (!out) return fail("null output");
    HIP_OK(hipSetDevice(ws->device));
    const aqc_ws::MpsSlot& a = ws->mps[slot_a];
    const aqc_ws::MpsSlot& b = ws->mps[slot_b];
    const int n = ws->ctx->prog.n;
    const size_t need = overlap_scratch_elems(n, a.dims.data(), b.dims.data());
    if (mps_scratch(ws, 3 * need)) return 1;
    double2* e = ws->d_mps_scratch;
    WsOps ops{ws};
    const double2* res = overlap_chain(ops, n, a.dims.data(), b.dims.data(), [&](int q) { return (const double2*)(a.d_t + a.offset[q]); },
                                       [&](int q) { return (const double2*)(b.d_t + b.offset[q]); }, e, e + need, e + 2 * need);
    if (!res) return 1;
    HIP_OK(hipMemcpyAsync(out, res, sizeof(double2), hipMemcpyDeviceToHost, ws->stream));
    HIP_OK(hipStreamSynchronize(ws->stream));
    return 0;
}

}  // extern "C"
