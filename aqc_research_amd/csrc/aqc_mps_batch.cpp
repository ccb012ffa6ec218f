// Lockstep lanes of the native MPS engine (aqc_mpsb_*): L independent problems that share ONE ansatz -- the seeds / restarts /
// targets of a horizon, mps_dot_objective.py:41 called once per job in the reference (job_executor.py:141) -- walk the circuit
// together, device-resident from the first gate to the last inner product.
//
// The single-lane engine (aqc_mps_engine.cpp) is a chain of small dependent launches with one host decision (the truncation rank)
// per 2-qubit gate: one lane cannot fill the device and host threads saturate the runtime's launch path.  Here
//   * every step of the walk is ONE launch for all lanes (grid dimension = lane);
//   * a lane's bond dimensions live on the device: a truncated 2-qubit gate is one workgroup per lane that forms the two-site
//     tensor in LDS, runs the Jacobi sweeps there, orders the singular values, takes the rank / truncation decision of
//     gate_adjacent (aqc_mps_engine.cpp) on its own values and writes the new tensors, Schmidt values and bond dimension;
//   * gate matrices are worked out by the kernels from thetas[lane][index], so a launch's arguments do not depend on the lane,
//     the parameters or the data: the host enqueues the whole evaluation (V^H|target>, <lhs|.>, the gate-by-gate gradient with
//     its cached environments) without waiting once, and reads objective values, gradients' inner products, status words and
//     bond statistics in one transfer at the end.
// Workgroups are sized for the bonds seen so far (`hint`: LDS and threads for bonds <= 4 / 6 / 8 / ... / 32); a lane that outgrows
// the launch raises a status bit and the evaluation is repeated at full size -- never a wrong result.  Bonds above 32 (a work
// matrix larger than 64 x 64 does not fit one workgroup's LDS) are refused (AQC_LANES_REFUSED): the caller goes to the single-lane engine.
// Arithmetic and truncation rule are the single-lane engine's (same device bodies, aqc_mps_dev.h), lane by lane.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <map>
#include <string>
#include <utility>

#include "../../include/aqc_hip.h"
#include "aqc_launch.h"
#include "aqc_devbuf.h"
#include "aqc_mps_host.h"

using namespace aqc;

namespace {

struct Lanes {   // L MPS of n sites, flat device storage with fixed strides; T_q = Gamma_q diag(lambda_q) like the single-lane engine
    int n = 0, L = 0, nb = 1;
    DevBuf<char> base;           // one allocation: T | lam | discarded | dims, so that a state is cloned by ONE copy
    LaneMps dev{};
    int max_dim_in = 1;          // largest bond of what was loaded (host side)
    int alloc(int n_, int L_) {
        n = n_; L = L_; nb = std::max(n - 1, 1);
        const size_t t = sizeof(double2) * (size_t)L * n * kLaneSite, lam = sizeof(double) * (size_t)L * nb * kLaneCap;
        const size_t disc = sizeof(double) * (size_t)L, dims = sizeof(int) * (size_t)L * (n + 1);
        if (base.alloc(t + lam + disc + dims)) return 1;
        dev.T = (char*)base; dev.lam = reinterpret_cast<double*>(base + t); dev.discarded = reinterpret_cast<double*>(base + t + lam);
        dev.dims = reinterpret_cast<int*>(base + t + lam + disc);
        dev.n = n; dev.pad = 0;
        return 0;
    }
    double2* site(int l, int q) const { return static_cast<double2*>(dev.T) + ((size_t)l * n + q) * kLaneSite; }
    double* lambda(int l, int b) const { return dev.lam + ((size_t)l * nb + b) * kLaneCap; }
};

// the gates of V or V^H in levels of pairwise disjoint gates (apply_circuit_all below), cached per circuit
struct Level { int off1, n1, off2, n2; };
struct Schedule {
    std::vector<Level> levels;
    DevBuf<LaneOp1> ops1;      // device tables, level after level
    DevBuf<LaneOp2> ops2;
};

}  // namespace

struct aqc_mpsb {
    int device = 0, n = 0, L = 0;
    hipStream_t st = nullptr;
    Lanes target, lhs, vh, w, z;
    Lanes bank;                  // K lhs states shared by all lanes (aqc_mpsb_set_bank): amplitudes <bank_k|vh_l> of aqc_mpsb_vh_bank
    std::map<std::string, Schedule> schedules;
    bool have_target = false, have_lhs = false, have_bank = false;
    DevBuf<double> thetas;       // [L][T_cap] on the device
    PinBuf<double> h_thetas;     // pinned staging of the same
    int T_cap = 0;               // thetas per lane the two are laid out for (a shape, like nvals)
    DevBuf<int> status;          // [L] status bits | [L] largest bond a gate has produced
    // environments of the pair (w, z): which of them are current (aqc_mps_gradwalk.h), and their buffers
    PairEnvs envs;
    DevBuf<double2> env_l;       // [L][n + 1][kLaneEnv]
    DevBuf<double2> env_r;       // [L][n][kLaneEnv]
    DevBuf<double2> e0;          // [L][kLaneEnv]
    DevBuf<double2> e1;
    DevBuf<double2> vals;        // [L][nvals]
    PinBuf<char> h_out;          // pinned: vals | status+peak | discarded | dims of vh
    int nvals = 0;
    int hint = kLaneCap;         // bonds the launches are sized for
    int peak_vh = 0, peak_grad = 0;   // largest bond the gates of the last V^H / gradient phase produced (0: none yet)
    int active = 0;              // lanes the gate launches cover (all, or the first half while V^H runs for lanes that repeat it)
    int cur_T = 0, cur_max_bond = 0;   // what the last aqc_mpsb_vh / eval ran with (the gradient phase continues from it)
    double cur_trunc = 0.0;
    bool vh_ready = false;
    // statistics of the truncated 2-qubit gates (aqc_mpsb_gate2_stats): work of the Jacobi sweeps on the device, and -- while
    // profiling is on -- the duration of every lanes_gate2 launch from a pool of event pairs (read back when the pool is full
    // and when the figures are asked for)
    DevBuf<unsigned long long> jstats;      // device [4]
    bool prof = false;
    std::vector<hipEvent_t> ev;             // pairs
    size_t ev_used = 0;
    double gate2_ms = 0.0;
    long long gate2_launches = 0;
    DevBuf<uint8_t> bits;        // basis-state patterns of aqc_mpsb_set_lhs_basis and their pinned staging (both grow-only)
    PinBuf<uint8_t> h_bits;
};

namespace {

// A failure that sends the caller to the single-lane engine: failf's message with the status AQC_LANES_REFUSED (include/aqc_hip.h).
// Its callers are exactly the failures whose text named "the lockstep lanes" while callers decided the fallback by those words: the
// bond checks, but also a lane's SVD or state gone bad, the full-size workgroup and the allocation.  The decision moved from the
// wording to this code and was not taken again; narrowing the set changes behaviour and is a decision of its own.
int refuse(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error(buf);
    return AQC_LANES_REFUSED;
}
constexpr int kRepeatAtFullSize = -1;   // finish() to run_phase() only: never a status of the ABI

void destroy(aqc_mpsb* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->st) (void)hipStreamSynchronize(b->st);
    for (hipEvent_t e : b->ev) (void)hipEventDestroy(e);
    if (b->st) (void)hipStreamDestroy(b->st);
    delete b;   // the buffers, after the stream has drained
}

int clone(aqc_mpsb* b, const Lanes& src, Lanes& dst) {
    HIP_OK(hipMemcpyAsync(dst.base, src.base, src.base.capacity(), hipMemcpyDeviceToDevice, b->st));
    return 0;
}

int gate1_all(aqc_mpsb* b, Lanes& s, int q, const LaneGate1& g, int T, Lanes* s2 = nullptr) {
    HIP_OK(launch_lanes_gate1(s.dev, s2 ? &s2->dev : nullptr, nullptr, 1, LaneOp1{q, 0, g}, b->thetas, T, b->active, b->hint, b->st));
    return 0;
}

int gate2_events_flush(aqc_mpsb* b) {   // sums the recorded pairs (waits for the stream)
    if (b->ev_used == 0) return 0;
    HIP_OK(hipStreamSynchronize(b->st));
    for (size_t i = 0; i + 1 < b->ev_used; i += 2) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, b->ev[i], b->ev[i + 1]));
        b->gate2_ms += ms;
        b->gate2_launches += 1;
    }
    b->ev_used = 0;
    return 0;
}
struct Gate2Scope {   // brackets one lanes_gate2 launch with an event pair while profiling is on
    aqc_mpsb* b;
    bool on;
    explicit Gate2Scope(aqc_mpsb* b_) : b(b_), on(b_->prof) {
        if (!on) return;
        if (b->ev_used + 2 > b->ev.size() && gate2_events_flush(b)) { on = false; return; }
        if (hipEventRecord(b->ev[b->ev_used], b->st) != hipSuccess) on = false;
    }
    ~Gate2Scope() {
        if (on && hipEventRecord(b->ev[b->ev_used + 1], b->st) == hipSuccess) b->ev_used += 2;
    }
};

int gate_adjacent_all(aqc_mpsb* b, Lanes& s, Lanes* s2, int q, const LaneGate2& g, int T, double trunc_thr, int max_bond) {
    Gate2Scope scope(b);
    HIP_OK(launch_lanes_gate2(s.dev, s2 ? &s2->dev : nullptr, nullptr, 1, LaneOp2{q, 0, g}, b->thetas, T, trunc_thr, max_bond, b->status, b->status + b->L,
                              b->active, b->hint, b->st, b->jstats));
    return 0;
}

// entangler of a block on any pair of qubits of `s` (and of `s2`, when given: the two operands of the gradient walk take every gate in one
// launch), routed by route_pair (aqc_mps_walk.h)
int gate2_pair_all(aqc_mpsb* b, Lanes& s, Lanes* s2, int ctrl, int targ, const LaneGate2& g, int T, double trunc_thr, int max_bond) {
    for (const RouteStep& r : route_pair(ctrl, targ))
        if (gate_adjacent_all(b, s, s2, r.q, routed_gate(r, g), T, trunc_thr, max_bond)) return 1;
    return 0;
}

// V(theta_l) or V(theta_l)^H on every lane (circuit_ops of aqc_mps_walk.h), layer by layer:
// the gates in program order (long-range entanglers already routed by swaps) are levelled as soon as possible -- a gate goes one level
// above the last gate on any of its sites.  The gates of a level act on pairwise disjoint site tensors, Schmidt vectors and bond
// dimensions, so they run in ONE launch per kind (1-qubit, 2-qubit) and leave exactly the bits the one-after-the-other order leaves:
// a brickwork layer of n / 2 entanglers is one launch of n / 2 x lanes workgroups instead of n / 2 dependent launches.
int build_schedule(aqc_mpsb* b, const aqc_circuit* c, bool inverse, Schedule& out) {
    const int n = b->n;
    const std::vector<CircuitOp> ops = circuit_ops(c, n, inverse);
    // as-soon-as-possible levels in program order
    std::vector<int> site_level(n, -1), lev(ops.size());
    int depth = 0;
    for (size_t i = 0; i < ops.size(); ++i) {
        if (!ops[i].two) {
            lev[i] = ++site_level[ops[i].op1.q];
        } else {
            const int q = ops[i].op2.q;
            site_level[q] = site_level[q + 1] = lev[i] = std::max(site_level[q], site_level[q + 1]) + 1;
        }
        depth = std::max(depth, lev[i] + 1);
    }
    std::vector<LaneOp1> t1;
    std::vector<LaneOp2> t2;
    out.levels.assign(depth, Level{0, 0, 0, 0});
    for (int lv = 0; lv < depth; ++lv) {
        Level& L = out.levels[lv];
        L.off1 = (int)t1.size(); L.off2 = (int)t2.size();
        for (size_t i = 0; i < ops.size(); ++i)
            if (lev[i] == lv) { if (ops[i].two) t2.push_back(ops[i].op2); else t1.push_back(ops[i].op1); }
        L.n1 = (int)t1.size() - L.off1; L.n2 = (int)t2.size() - L.off2;
    }
    if ((!t1.empty() && out.ops1.upload(t1)) || (!t2.empty() && out.ops2.upload(t2))) return 1;
    return 0;
}

std::string circuit_key(const aqc_circuit* c, bool inverse) {
    std::string k(reinterpret_cast<const char*>(&c->num_qubits), sizeof(int32_t) * 5);
    k.append(reinterpret_cast<const char*>(c->blocks), sizeof(int32_t) * 2 * (size_t)std::max(c->num_blocks, 0));
    k.push_back(inverse ? 1 : 0);
    return k;
}

int apply_circuit_all(aqc_mpsb* b, Lanes& s, const aqc_circuit* c, int T, bool inverse, double trunc_thr, int max_bond) {
    const std::string key = circuit_key(c, inverse);
    auto it = b->schedules.find(key);
    if (it == b->schedules.end()) {
        if (b->schedules.size() >= 16) {   // (a driver walks a few horizons; nothing keeps more than a handful of circuits alive)
            HIP_OK(hipStreamSynchronize(b->st));
            b->schedules.clear();
        }
        Schedule sch;
        if (build_schedule(b, c, inverse, sch)) return 1;
        it = b->schedules.emplace(key, std::move(sch)).first;
    }
    const Schedule& sch = it->second;
    for (const Level& lv : sch.levels) {
        if (lv.n1)
            HIP_OK(launch_lanes_gate1(s.dev, nullptr, sch.ops1 + lv.off1, lv.n1, LaneOp1{}, b->thetas, T, b->active, b->hint, b->st));
        if (lv.n2) {
            Gate2Scope scope(b);
            HIP_OK(launch_lanes_gate2(s.dev, nullptr, sch.ops2 + lv.off2, lv.n2, LaneOp2{}, b->thetas, T, trunc_thr, max_bond, b->status, b->status + b->L,
                                      b->active, b->hint, b->st, b->jstats));
        }
    }
    return 0;
}

// ---- the lanes' executor of the gradient walk (aqc_mps_gradwalk.h), all lanes per launch: w = lhs, z = vh (both consumed) ------------------
constexpr size_t kEnvL(int n) { return (size_t)(n + 1) * kLaneEnv; }
constexpr size_t kEnvR(int n) { return (size_t)n * kLaneEnv; }

struct LanesExec {
    aqc_mpsb* b;
    int T; double trunc_thr; int max_bond;   // what the gates of a walk run with
    double2* env_l(int p) const { return b->env_l + (size_t)p * kLaneEnv; }
    double2* env_r(int p) const { return b->env_r + (size_t)p * kLaneEnv; }
    double2* scratch(int k) const { return k ? b->e1 : b->e0; }
    // out[u][v] = sum_bit sum_xy conj(A_p[bit][x][u]) in[x][y] B_p[bit][y][v]; `op` (may be null) sits on w's side of site p
    int step_left(int p, const double2* in, size_t in_stride, const M2* op, double2* out, size_t out_stride) {
        double g8[8];
        if (op) pack(adjoint(*op), g8);
        HIP_OK(launch_lanes_env_left(b->w.dev, b->z.dev, p, in, in_stride, out, out_stride, op ? g8 : nullptr, b->L, b->st));
        return 0;
    }
    int left(int p) { return step_left(p, env_l(p), kEnvL(b->n), nullptr, env_l(p + 1), kEnvL(b->n)); }
    int right(int p) {   // Rc[p - 1][x][y] = sum_bit A_p[bit][x][u] (Rc[p] B_p[bit]^H)[u][y]
        HIP_OK(launch_lanes_env_right(b->w.dev, b->z.dev, p, env_r(p), kEnvR(b->n), env_r(p - 1), kEnvR(b->n), b->L, b->st));
        return 0;
    }
    int chain(int p, bool first, int k, const M2* op) {
        return step_left(p, first ? env_l(p) : scratch(k ^ 1), first ? kEnvL(b->n) : kLaneEnv, op, scratch(k), kLaneEnv);
    }
    int close(int hi, int k, int slot) {
        if (slot >= b->nvals) return failf("inner-product slot out of range");
        HIP_OK(launch_lanes_env_dot(b->w.dev, b->z.dev, hi, scratch(k), kLaneEnv, env_r(hi), kEnvR(b->n), b->vals, b->nvals, slot, b->L, b->st));
        return 0;
    }
    int entangle(const GradStep& s) { return gate2_pair_all(b, b->z, &b->w, s.q, s.q2, s.ent, T, trunc_thr, max_bond); }
    int rotate(int q, const LaneGate1& g) { return gate1_all(b, b->w, q, g, T, &b->z); }
    // consecutive parameters on one site: per parameter the rotation on both operands + its inner product <P w|z>, up to three of
    // them in one launch (the environments do not involve the site: they are advanced once, in front)
    int rotate_recorded(PairEnvs& env, const GradStep& s, int slot) {
        if (slot + s.count > b->nvals) return failf("inner-product slot out of range");
        if (env_advance(*this, env, s.q, s.q)) return 1;
        LaneSteps st{};
        st.count = s.count;
        for (int k = 0; k < s.count; ++k) {
            st.g[k] = s.r[k].g;
            pack(adjoint(pauli_of(s.r[k].pauli)), st.gh[k]);
        }
        HIP_OK(launch_lanes_grad_step(b->w.dev, b->z.dev, s.q, st, b->thetas, T, env_l(s.q), kEnvL(b->n), env_r(s.q), kEnvR(b->n), b->e0, b->vals, b->nvals, slot,
                                      b->L, b->st));
        env.touched(s.q, s.q);
        return 0;
    }
};

// the gate-by-gate gradient walk on every lane; the inner products go to slots slot0, slot0 + 1, ... of vals; rec = (theta index, factor) per slot
int gradient_all(aqc_mpsb* b, const aqc_circuit* c, int T, double trunc_thr, int max_bond, int lo_blk, int hi_blk, bool front_layer, int slot0,
                 GradRecords& rec) {
    LanesExec ex{b, T, trunc_thr, max_bond};
    return gradient_walk(ex, b->envs, gradient_steps(c, b->n, lo_blk, hi_blk, front_layer), slot0, rec);
}

int load_lanes(aqc_mpsb* b, Lanes& dst, aqc_mps* const* src, int shared) {   // dst.L states (the lanes', or the bank's K)
    if (!src) return failf("null MPS list");
    const int n = b->n, L = dst.L, distinct = shared ? 1 : L;
    std::vector<int> dims_all((size_t)L * (n + 1));
    std::vector<double> disc(L);
    dst.max_dim_in = 1;
    for (int l = 0; l < distinct; ++l) {
        const aqc_mps* m = src[l];
        if (!m) return failf("null MPS handle (lane %d)", l);
        if (aqc_mps_num_qubits(m) != n) return failf("lane %d: the MPS has %d qubits, the batch %d", l, aqc_mps_num_qubits(m), n);
        std::vector<int32_t> dims(n + 1);
        if (aqc_mps_dims(m, dims.data())) return 1;
        for (int q = 0; q <= n; ++q) {
            if (dims[q] > kLaneCap)
                return refuse("lane %d: bond dimension %d exceeds the %d of the lockstep lanes (use the single-lane engine)", l, dims[q], kLaneCap);
            dims_all[(size_t)l * (n + 1) + q] = dims[q];
            dst.max_dim_in = std::max(dst.max_dim_in, (int)dims[q]);
        }
        disc[l] = aqc_mps_discarded_weight(m);
        for (int q = 0; q < n; ++q) {
            const void* site = nullptr;
            const double* lam = nullptr;
            if (mps_peek(m, q, &site, &lam)) return 1;
            HIP_OK(hipMemcpyAsync(dst.site(l, q), site, sizeof(double2) * 2 * dims[q] * dims[q + 1], hipMemcpyDeviceToDevice, b->st));
            if (q < n - 1) HIP_OK(hipMemcpyAsync(dst.lambda(l, q), lam, sizeof(double) * dims[q + 1], hipMemcpyDeviceToDevice, b->st));
        }
    }
    if (shared) {   // one state for all lanes: lane 0 is replicated by doubling (lanes [0, c) -> [c, 2c)), 2 log2(L) copies instead of 2 n L
        for (int l = 1; l < L; ++l) {
            std::copy(dims_all.begin(), dims_all.begin() + (n + 1), dims_all.begin() + (size_t)l * (n + 1));
            disc[l] = disc[0];
        }
        const size_t t_lane = sizeof(double2) * (size_t)n * kLaneSite, lam_lane = sizeof(double) * (size_t)dst.nb * kLaneCap;
        for (int c = 1; c < L; c *= 2) {
            const int cnt = std::min(c, L - c);
            HIP_OK(hipMemcpyAsync(static_cast<char*>(dst.dev.T) + t_lane * c, dst.dev.T, t_lane * cnt, hipMemcpyDeviceToDevice, b->st));
            HIP_OK(hipMemcpyAsync(reinterpret_cast<char*>(dst.dev.lam) + lam_lane * c, dst.dev.lam, lam_lane * cnt, hipMemcpyDeviceToDevice, b->st));
        }
    }
    HIP_OK(hipMemcpyAsync(dst.dev.dims, dims_all.data(), sizeof(int) * dims_all.size(), hipMemcpyHostToDevice, b->st));
    HIP_OK(hipMemcpyAsync(dst.dev.discarded, disc.data(), sizeof(double) * disc.size(), hipMemcpyHostToDevice, b->st));
    HIP_OK(hipStreamSynchronize(b->st));   // (the host vectors above must outlive their copies)
    return 0;
}

// launches are sized (LDS, threads) for one of a few bond limits: what the loaded states need exactly, what the gates of the previous
// evaluation produced plus a quarter of head room
int hint_for(int loaded, int produced) {
    const int want = std::max(loaded, produced + (produced + 3) / 4);
    for (int h : {4, 6, 8, 12, 16, 20, 24}) if (want <= h) return h;
    return kLaneCap;
}
// the size of the next phase's launches: full size until a phase has reported what its gates produce
int next_hint(const aqc_mpsb* b) {
    const int produced = std::max(b->peak_vh, b->peak_grad);
    return produced == 0 ? kLaneCap : hint_for(std::max(b->target.max_dim_in, b->lhs.max_dim_in), produced);
}

// validates, sizes the per-evaluation buffers for `circ` (inner-product slots: amplitudes, then one per parameter) and uploads thetas
int begin(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int num_amps, int* T_out) {
    if (check_circuit(circ, b->n)) return 1;
    if (!(trunc_thr >= 0.0)) return failf("trunc_thr must be non-negative");
    if (max_bond > kLaneCap) return refuse("the lockstep lanes keep bonds up to %d", kLaneCap);
    HIP_OK(hipSetDevice(b->device));
    const int n = b->n, L = b->L;
    const WalkSizes sz = walk_sizes(circ, n);
    const int T = sz.T, need = num_amps + sz.max_records;
    const auto out_size = [&](int nv) { return sizeof(double2) * (size_t)L * nv + sizeof(int) * 2 * (size_t)L + sizeof(double) * (size_t)L + sizeof(int) * (size_t)L * (n + 1); };
    if (need > b->nvals || T > b->T_cap) {
        HIP_OK(hipStreamSynchronize(b->st));
        const int nv = std::max(need, b->nvals), tc = std::max({T, b->T_cap, 1});
        b->nvals = 0; b->T_cap = 0;
        if (b->vals.reserve((size_t)L * nv) || b->thetas.reserve((size_t)L * tc) || b->h_thetas.reserve((size_t)L * tc) ||
            b->h_out.reserve(out_size(nv))) return 1;
        b->nvals = nv; b->T_cap = tc;
    }
    HIP_OK(hipStreamSynchronize(b->st));   // (the staging buffer may still feed the previous upload)
    memcpy(b->h_thetas, thetas, sizeof(double) * (size_t)L * T);
    HIP_OK(hipMemcpyAsync(b->thetas, b->h_thetas, sizeof(double) * (size_t)L * T, hipMemcpyHostToDevice, b->st));
    b->cur_T = T; b->cur_trunc = trunc_thr; b->cur_max_bond = max_bond;
    b->vh_ready = false;
    b->hint = next_hint(b);
    *T_out = T;
    return 0;
}

// lanes [L/2, L) of `s` <- lanes [0, L/2)
int replicate_half(aqc_mpsb* b, Lanes& s) {
    const size_t h = (size_t)b->L / 2, n = s.n;
    HIP_OK(hipMemcpyAsync(static_cast<double2*>(s.dev.T) + h * n * kLaneSite, s.dev.T, sizeof(double2) * h * n * kLaneSite, hipMemcpyDeviceToDevice, b->st));
    HIP_OK(hipMemcpyAsync(s.dev.lam + h * s.nb * kLaneCap, s.dev.lam, sizeof(double) * h * s.nb * kLaneCap, hipMemcpyDeviceToDevice, b->st));
    HIP_OK(hipMemcpyAsync(s.dev.discarded + h, s.dev.discarded, sizeof(double) * h, hipMemcpyDeviceToDevice, b->st));
    HIP_OK(hipMemcpyAsync(s.dev.dims + h * (n + 1), s.dev.dims, sizeof(int) * h * (n + 1), hipMemcpyDeviceToDevice, b->st));
    return 0;
}

// vh = V^H target on every lane (inverse = false: V target, aqc_mpsb_apply_circuit); half: on the first half of the lanes, copied to the second
int form_vh(aqc_mpsb* b, const aqc_circuit* circ, int T, bool half, bool inverse = true) {
    if (clone(b, b->target, b->vh)) return 1;
    b->active = half ? b->L / 2 : b->L;
    const int rc = apply_circuit_all(b, b->vh, circ, T, inverse, b->cur_trunc, b->cur_max_bond);
    b->active = b->L;
    if (rc) return 1;
    return half ? replicate_half(b, b->vh) : 0;
}

// (w, z) = (lhs, zsrc) with fresh environments: where a gradient walk and the amplitudes start
int start_pair(aqc_mpsb* b, const Lanes& zsrc) {
    if (clone(b, b->lhs, b->w) || clone(b, zsrc, b->z)) return 1;
    HIP_OK(launch_lanes_env_init(b->env_l, kEnvL(b->n), b->env_r + (size_t)(b->n - 1) * kLaneEnv, kEnvR(b->n), b->L, b->st));
    b->envs.reset(b->n);
    return 0;
}

// vh as above, (w, z) = (lhs, vh), and the amplitudes <lhs|vh> (slot 0), <X_q lhs|vh> (slots 1 + q)
int enqueue_vh(aqc_mpsb* b, const aqc_circuit* circ, int T, bool half, int num_amps) {
    if (form_vh(b, circ, T, half) || start_pair(b, b->vh)) return 1;
    LanesExec ex{b, T, b->cur_trunc, b->cur_max_bond};
    for (int k = 1; k < num_amps; ++k) {   // flips first: site 0 upwards, the right environments are built once on the way down to site 0
        const int q = k - 1;
        const M2* g = &kPauliX;
        if (env_dot(ex, b->envs, k, 1, &q, &g)) return 1;
    }
    const int q = b->n - 1;
    const M2 eye = {{1.0, 0.0, 0.0, 1.0}};
    const M2* g = &eye;
    return env_dot(ex, b->envs, 0, 1, &q, &g);
}

// The same for a bank of lhs states (aqc_mpsb_vh_bank): vh as above, then amps[l][k] = <bank_k|vh_l> in slots k of vals, one launch for all
// (k, active lane) pairs.  (w, z) and the environments are left alone: the gradient phase starts them itself.
int enqueue_vh_bank(aqc_mpsb* b, const aqc_circuit* circ, int T, bool half) {
    if (form_vh(b, circ, T, half)) return 1;
    const int h = std::max(b->hint, hint_for(b->bank.max_dim_in, 0));
    HIP_OK(launch_lanes_bank_dot(b->bank.dev, b->bank.L, b->vh.dev, half ? b->L / 2 : b->L, b->vals, b->nvals, 0, b->status, h, b->st));
    return 0;
}

// results of the enqueued work -> pinned host memory; 0 ok, kRepeatAtFullSize = a lane outgrew the launch size, else the failure's status
int finish(aqc_mpsb* b, bool may_retry, int* peak_out) {
    const int n = b->n, L = b->L;
    char* h_vals = b->h_out;
    char* h_status = h_vals + sizeof(double2) * (size_t)L * b->nvals;
    char* h_disc = h_status + sizeof(int) * 2 * (size_t)L;
    char* h_dims = h_disc + sizeof(double) * (size_t)L;
    HIP_OK(hipMemcpyAsync(h_vals, b->vals, sizeof(double2) * (size_t)L * b->nvals, hipMemcpyDeviceToHost, b->st));
    HIP_OK(hipMemcpyAsync(h_status, b->status, sizeof(int) * 2 * (size_t)L, hipMemcpyDeviceToHost, b->st));
    HIP_OK(hipMemcpyAsync(h_disc, b->vh.dev.discarded, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, b->st));
    HIP_OK(hipMemcpyAsync(h_dims, b->vh.dev.dims, sizeof(int) * (size_t)L * (n + 1), hipMemcpyDeviceToHost, b->st));
    HIP_OK(hipStreamSynchronize(b->st));
    const int* st = reinterpret_cast<const int*>(h_status);
    int flags = 0, peak = 1;
    for (int l = 0; l < L; ++l) { flags |= st[l]; peak = std::max(peak, st[L + l]); }
    if ((flags & kLaneLdsShort) && may_retry && b->hint < kLaneCap) {
        b->hint = kLaneCap;
        return kRepeatAtFullSize;
    }
    *peak_out = peak;
    for (int l = 0; l < L; ++l) {
        if (st[l] & kLaneOverflow)
            return refuse("lane %d: a bond grows beyond the %d of the lockstep lanes (set max_bond <= %d or use the single-lane engine)", l, kLaneCap, kLaneCap);
        if (st[l] & kLaneNoConv) return refuse("Jacobi SVD: no convergence within 60 sweeps (lane %d of the lockstep lanes)", l);
        if (st[l] & kLaneZero) return refuse("2-qubit gate produced a zero or non-finite state (lane %d of the lockstep lanes)", l);
        if (st[l] & kLaneLdsShort) return refuse("internal: workgroup of the lockstep lanes too small at full size (lane %d)", l);
    }
    return 0;
}

struct Readback {
    const cd* vals; const double* disc; const int* dims;
    int max_dim(int l, int n) const {
        int mx = 1;
        for (int q = 0; q <= n; ++q) mx = std::max(mx, dims[(size_t)l * (n + 1) + q]);
        return mx;
    }
};
Readback readback(const aqc_mpsb* b) {
    const size_t L = b->L;
    const char* h_vals = b->h_out;
    const char* h_disc = h_vals + sizeof(double2) * L * b->nvals + sizeof(int) * 2 * L;
    return Readback{reinterpret_cast<const cd*>(h_vals), reinterpret_cast<const double*>(h_disc), reinterpret_cast<const int*>(h_disc + sizeof(double) * L)};
}
// grad[lane][T] from the recorded inner products (slots slot0, slot0 + 1, ...)
void assemble(const aqc_mpsb* b, const Readback& r, const GradRecords& rec, int slot0, int T, cd* grad) {
    for (int l = 0; l < b->L; ++l) assemble_gradient(rec, r.vals + (size_t)l * b->nvals + slot0, T, grad + (size_t)l * T);
}

// One phase of work on all lanes, the skeleton of every evaluating entry point: the status words cleared, `enqueue` (the entry point's
// launches; it waits for nothing), the results brought to the host -- and all of it once more at full size when a lane outgrew the
// launches.  Then the bookkeeping: *peak = the largest bond a gate produced (also when a lane made finish fail), vh_ready = whether vh
// now holds V^H target for the thetas of begin, and per lane the discarded weight and largest bond of vh (either output may be null).
// The entry point copies its own values out of readback().
template <class Enqueue>
int run_phase(aqc_mpsb* b, int* peak, bool vh_ready, double* discarded_out, int32_t* max_bond_out, Enqueue enqueue) {
    int rc = kRepeatAtFullSize;
    for (int attempt = 0; rc == kRepeatAtFullSize; ++attempt) {
        HIP_OK(hipMemsetAsync(b->status, 0, sizeof(int) * 2 * (size_t)b->L, b->st));
        if (enqueue()) return 1;
        rc = finish(b, attempt == 0, peak);
    }
    if (rc) return rc;
    b->vh_ready = vh_ready;
    const Readback r = readback(b);
    for (int l = 0; l < b->L; ++l) {
        if (discarded_out) discarded_out[l] = r.disc[l];
        if (max_bond_out) max_bond_out[l] = r.max_dim(l, b->n);
    }
    return 0;
}

}  // namespace

extern "C" {

int aqc_mpsb_create(int device, int num_qubits, int lanes, aqc_mpsb** out) {
    if (!out) return failf("null output");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return failf("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return failf("device out of range");
    if (num_qubits < 2 || num_qubits > 4096) return failf("number of qubits out of range");
    if (lanes < 1 || lanes > 32767) return failf("lanes must be in [1, 32767] (a gate launch has two workgroups per lane in the y dimension of its grid)");
    HIP_OK(hipSetDevice(device));
    aqc_mpsb* b = new aqc_mpsb();
    b->device = device; b->n = num_qubits; b->L = lanes; b->active = lanes;
    auto bad = [&](int rc) { destroy(b); return rc; };
    if (hipStreamCreate(&b->st) != hipSuccess) return bad(failf("hipStreamCreate failed"));
    for (Lanes* s : {&b->target, &b->lhs, &b->vh, &b->w, &b->z})
        if (s->alloc(num_qubits, lanes)) return bad(1);
    const size_t L = lanes;
    if (b->status.alloc(2 * L) || b->env_l.alloc(L * kEnvL(num_qubits)) || b->env_r.alloc(L * kEnvR(num_qubits)) || b->e0.alloc(L * kLaneEnv) ||
        b->e1.alloc(L * kLaneEnv)) {
        return bad(refuse("allocation of the lockstep lanes failed (%d lanes, %d qubits)", lanes, num_qubits));
    }
    *out = b;
    return 0;
}

int aqc_mpsb_destroy(aqc_mpsb* b) {
    destroy(b);
    return 0;
}

/* Work and time of the truncated 2-qubit gates since the last reset.  enable: 1 starts counting (Jacobi work on the device; every
 * lanes_gate2 launch bracketed by an event pair), 0 stops, -1 leaves the switch alone.  out (may be null): [0] fp64 flops of the
 * Jacobi rotations that ran, [1] SVDs, [2] sweeps, [3] rotations, [4] lanes_gate2 launches timed, [5] their total duration in ms.
 * reset != 0 clears the figures after reading them. */
int aqc_mpsb_gate2_stats(aqc_mpsb* b, int enable, double* out, int reset) {
    if (!b) return failf("null batch");
    HIP_OK(hipSetDevice(b->device));
    if (!b->jstats) {
        if (b->jstats.alloc(4)) return 1;
        HIP_OK(hipMemset(b->jstats, 0, 4 * sizeof(unsigned long long)));
    }
    if (gate2_events_flush(b)) return 1;
    if (enable == 1 && b->ev.empty()) {
        b->ev.resize(2048);
        for (hipEvent_t& e : b->ev) HIP_OK(hipEventCreate(&e));
    }
    if (enable >= 0) b->prof = enable != 0;
    if (out) {
        unsigned long long h[4];
        HIP_OK(hipStreamSynchronize(b->st));
        HIP_OK(hipMemcpy(h, b->jstats, sizeof h, hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; ++i) out[i] = (double)h[i];
        out[4] = (double)b->gate2_launches;
        out[5] = b->gate2_ms;
    }
    if (reset) {
        HIP_OK(hipMemset(b->jstats, 0, 4 * sizeof(unsigned long long)));
        b->gate2_ms = 0.0;
        b->gate2_launches = 0;
    }
    return 0;
}

int aqc_mpsb_set_targets(aqc_mpsb* b, aqc_mps* const* targets, int shared) {
    if (!b) return failf("null batch");
    HIP_OK(hipSetDevice(b->device));
    if (const int rc = load_lanes(b, b->target, targets, shared)) return rc;
    b->have_target = true;
    return 0;
}

int aqc_mpsb_set_lhs(aqc_mpsb* b, aqc_mps* const* lhs, int shared) {
    if (!b) return failf("null batch");
    HIP_OK(hipSetDevice(b->device));
    if (const int rc = load_lanes(b, b->lhs, lhs, shared)) return rc;
    b->have_lhs = true;
    return 0;
}

/* lhs states of all lanes = computational-basis states, built on the device: bits[lane][n] (0 / 1), bit q = qubit q = site q */
int aqc_mpsb_set_lhs_basis(aqc_mpsb* b, const uint8_t* bits) {
    if (!b || !bits) return failf("null argument");
    HIP_OK(hipSetDevice(b->device));
    const size_t bytes = (size_t)b->L * b->n;
    if (bytes > b->bits.capacity()) {
        HIP_OK(hipStreamSynchronize(b->st));
        if (b->bits.reserve(bytes) || b->h_bits.reserve(bytes)) return 1;
    }
    HIP_OK(hipStreamSynchronize(b->st));   // (the staging buffer may still feed the previous upload)
    memcpy(b->h_bits, bits, bytes);
    HIP_OK(hipMemcpyAsync(b->bits, b->h_bits, bytes, hipMemcpyHostToDevice, b->st));
    HIP_OK(launch_lanes_basis(b->lhs.dev, b->bits, b->L, b->st));
    b->lhs.max_dim_in = 1;
    b->have_lhs = true;
    return 0;
}

/* v_mul_mps / v_dagger_mul_mps (mps_operations.py:326-371) for every lane: the working state of the batch <- V(theta_l)|phi_l> (inverse = 0) or
 * V(theta_l)^H|phi_l> (inverse = 1), layer by layer (apply_circuit_all); aqc_mpsb_export hands a lane's result out.  No lhs states needed. */
int aqc_mpsb_apply_circuit(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, int inverse, double trunc_thr, int max_bond, double* discarded_out,
                           int32_t* max_bond_out) {
    if (!b || !circ || !thetas) return failf("null argument");
    if (!b->have_target) return failf("set the states of the lanes first (aqc_mpsb_set_targets)");
    int T = 0;
    if (const int rc = begin(b, circ, thetas, trunc_thr, max_bond, 1, &T)) return rc;
    return run_phase(b, &b->peak_vh, inverse != 0, discarded_out, max_bond_out, [&] { return form_vh(b, circ, T, false, inverse != 0); });
}

/* lane `lane` of the working state (the result of aqc_mpsb_apply_circuit / aqc_mpsb_vh) as a single-lane MPS of its own */
int aqc_mpsb_export(aqc_mpsb* b, int lane, aqc_mps** out) {
    if (!b || !out) return failf("null argument");
    if (lane < 0 || lane >= b->L) return failf("lane out of range");
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->st));
    const int n = b->n;
    std::vector<int> dims(n + 1);
    double discarded = 0.0;
    HIP_OK(hipMemcpy(dims.data(), b->vh.dev.dims + (size_t)lane * (n + 1), sizeof(int) * (n + 1), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&discarded, b->vh.dev.discarded + lane, sizeof(double), hipMemcpyDeviceToHost));
    std::vector<const void*> sites(n);
    std::vector<const double*> lams(std::max(n - 1, 1), nullptr);
    for (int q = 0; q < n; ++q) {
        sites[q] = b->vh.site(lane, q);
        if (q < n - 1) lams[q] = b->vh.lambda(lane, q);
    }
    return mps_adopt(b->device, n, dims.data(), sites.data(), lams.data(), discarded, out);
}

/* Phase 1 of an evaluation: vh_l = V(theta_l)^H|phi_l> for every lane, kept in the batch, and the amplitudes
 * amps[lane][0] = <lhs_l|vh_l>, amps[lane][1 + q] = <X_q lhs_l|vh_l> (num_amps = 1 or 1 + n: with a basis state as lhs these are the
 * amplitudes of the flip states of objective_lhs_sur_max.py:82-117).  half != 0: lanes [L/2, L) repeat the targets and thetas of lanes
 * [0, L/2) (the same problems with another lhs state): V^H runs on the first half only and is copied. */
int aqc_mpsb_vh(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int half, int num_amps, double* amps,
                double* discarded_out, int32_t* max_bond_out) {
    if (!b || !circ || !thetas || !amps) return failf("null argument");
    if (!b->have_target || !b->have_lhs) return failf("set the targets and the lhs states of the lanes first");
    if (num_amps != 1 && num_amps != 1 + b->n) return failf("num_amps: 1 (<lhs|vh>) or 1 + n (and the single-flip amplitudes)");
    if (half && (b->L & 1)) return failf("half: the batch needs an even number of lanes");
    int T = 0;
    if (const int rc = begin(b, circ, thetas, trunc_thr, max_bond, num_amps, &T)) return rc;
    if (const int rc = run_phase(b, &b->peak_vh, true, discarded_out, max_bond_out, [&] { return enqueue_vh(b, circ, T, half != 0, num_amps); })) return rc;
    const Readback r = readback(b);
    cd* out = reinterpret_cast<cd*>(amps);
    for (int l = 0; l < b->L; ++l)
        for (int k = 0; k < num_amps; ++k) out[(size_t)l * num_amps + k] = r.vals[(size_t)l * b->nvals + k];
    return 0;
}

/* K lhs states shared by all lanes (the states S|0>, S X_i|0> of a general state preparation, objective_base.py:345-435), bonds <= 32 */
int aqc_mpsb_set_bank(aqc_mpsb* b, aqc_mps* const* states, int count) {
    if (!b) return failf("null argument");
    if (count < 1 || count > 32767) return failf("bank: count must be in [1, 32767]");
    if (!states) return failf("null argument");
    HIP_OK(hipSetDevice(b->device));
    b->have_bank = false;
    if (b->bank.L != count) {
        HIP_OK(hipStreamSynchronize(b->st));
        if (b->bank.base.release()) return 1;
        if (b->bank.alloc(b->n, count)) { b->bank.L = 0; return 1; }
    }
    if (const int rc = load_lanes(b, b->bank, states, 0)) return rc;
    b->have_bank = true;
    return 0;
}

/* Phase 1 with the bank as the lhs side: vh of every lane as aqc_mpsb_vh, and amps[lane][k] = <bank_k|vh_l> (num_amps = the bank's K),
 * all read back with the status words in one transfer.  half != 0: the overlaps of lanes [L/2, L) are those of lanes [0, L/2). */
int aqc_mpsb_vh_bank(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int half, int num_amps,
                     double* amps, double* discarded_out, int32_t* max_bond_out) {
    if (!b || !circ || !thetas || !amps) return failf("null argument");
    if (!b->have_target || !b->have_bank) return failf("set the targets and the bank of the lanes first (aqc_mpsb_set_bank)");
    if (num_amps != b->bank.L) return failf("num_amps: the bank holds %d states", b->bank.L);
    if (half && (b->L & 1)) return failf("half: the batch needs an even number of lanes");
    int T = 0;
    if (const int rc = begin(b, circ, thetas, trunc_thr, max_bond, num_amps, &T)) return rc;
    if (const int rc = run_phase(b, &b->peak_vh, true, discarded_out, max_bond_out, [&] { return enqueue_vh_bank(b, circ, T, half != 0); })) return rc;
    const Readback r = readback(b);
    cd* out = reinterpret_cast<cd*>(amps);
    const int L = b->L;
    for (int l = 0; l < L; ++l) {
        const int src = half && l >= L / 2 ? l - L / 2 : l;   // (the overlaps were taken for the first half only)
        for (int k = 0; k < num_amps; ++k) out[(size_t)l * num_amps + k] = r.vals[(size_t)src * b->nvals + k];
    }
    return 0;
}

/* Phase 2: the gate-by-gate gradient walk of every lane from its CURRENT lhs state (it may have been replaced since phase 1) and the
 * vh, thetas, trunc_thr and max_bond of the last aqc_mpsb_vh (same circuit). */
int aqc_mpsb_grad(aqc_mpsb* b, const aqc_circuit* circ, int block_from, int block_to, int front_layer, double* grad_out) {
    if (!b || !circ || !grad_out) return failf("null argument");
    if (!b->vh_ready) return failf("aqc_mpsb_grad follows aqc_mpsb_vh");
    if (!b->have_lhs) return failf("set the lhs states of the lanes first");
    if (check_circuit(circ, b->n)) return 1;
    HIP_OK(hipSetDevice(b->device));
    const WalkSizes sz = walk_sizes(circ, b->n);
    const int T = sz.T;
    if (T != b->cur_T || sz.max_records > b->nvals) return failf("aqc_mpsb_grad: not the circuit of the last aqc_mpsb_vh");
    if (check_block_range(circ, block_from, block_to)) return 1;
    GradRecords rec;
    b->hint = next_hint(b);
    if (const int rc = run_phase(b, &b->peak_grad, true, nullptr, nullptr, [&] {
            return start_pair(b, b->vh) || gradient_all(b, circ, T, b->cur_trunc, b->cur_max_bond, block_from, block_to, front_layer != 0, 0, rec);
        }))
        return rc;
    assemble(b, readback(b), rec, 0, T, reinterpret_cast<cd*>(grad_out));
    return 0;
}

/* fast_dot_gradient(circ, thetas, lvec, vh_phi, trunc_thr, block_range, front_layer) (mps_dot_objective.py:41-242) for every lane, with
 * vh_phi_l ALREADY formed by the caller: the states set by aqc_mpsb_set_targets are taken as vh_phi_l, those of aqc_mpsb_set_lhs as lvec_l. */
int aqc_mpsb_gradient_of(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int block_from, int block_to,
                         int front_layer, double* grad_out) {
    if (!b || !circ || !thetas || !grad_out) return failf("null argument");
    if (!b->have_target || !b->have_lhs) return failf("set the vh_phi states (aqc_mpsb_set_targets) and the lhs states of the lanes first");
    int T = 0;
    if (const int rc = begin(b, circ, thetas, trunc_thr, max_bond, 0, &T)) return rc;
    if (check_block_range(circ, block_from, block_to)) return 1;
    GradRecords rec;
    if (const int rc = run_phase(b, &b->peak_grad, false, nullptr, nullptr, [&] {   // (vh is not involved: z starts from the states given as targets)
            return start_pair(b, b->target) || gradient_all(b, circ, T, trunc_thr, max_bond, block_from, block_to, front_layer != 0, 0, rec);
        }))
        return rc;
    assemble(b, readback(b), rec, 0, T, reinterpret_cast<cd*>(grad_out));
    return 0;
}

/* both phases in one call, one wait: h[lane] = <lhs_l|vh_l> and the gradient */
int aqc_mpsb_eval(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int block_from, int block_to,
                  int front_layer, double* h_out, double* grad_out, double* discarded_out, int32_t* max_bond_out) {
    if (!b || !circ || !thetas || !h_out || !grad_out) return failf("null argument");
    if (!b->have_target || !b->have_lhs) return failf("set the targets and the lhs states of the lanes first");
    int T = 0;
    if (const int rc = begin(b, circ, thetas, trunc_thr, max_bond, 1, &T)) return rc;
    if (check_block_range(circ, block_from, block_to)) return 1;
    GradRecords rec;
    if (const int rc = run_phase(b, &b->peak_vh, true, discarded_out, max_bond_out, [&] {   // enqueue_vh leaves (w, z) = (lhs, vh), environments started
            return enqueue_vh(b, circ, T, false, 1) || gradient_all(b, circ, T, trunc_thr, max_bond, block_from, block_to, front_layer != 0, 1, rec);
        }))
        return rc;
    b->peak_grad = 0;   // (peak_vh covers the whole evaluation here)
    const Readback r = readback(b);
    cd* hh = reinterpret_cast<cd*>(h_out);
    for (int l = 0; l < b->L; ++l) hh[l] = r.vals[(size_t)l * b->nvals];
    assemble(b, r, rec, 1, T, reinterpret_cast<cd*>(grad_out));
    return 0;
}

}  // extern "C"
