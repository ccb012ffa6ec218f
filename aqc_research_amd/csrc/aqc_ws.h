// Internal declarations shared by the translation units behind the C ABI (include/aqc_hip.h):
//   aqc_api.cpp        contexts, workspaces, buffers, thetas, small results, one-shot entry points
//   aqc_ws_plan.cpp    lowering of stage plans to device tables (micro-ops, sub-stage slot tables), mirrored V^H plans
//   aqc_ws_sweep.cpp   V / V^H launches, the w/z sweep (dense and sparse-lhs routes), the route of an evaluation (eval_route), aqc_ws_eval
//   aqc_ws_optim.cpp   device-resident L-BFGS (surrogate and matrix objectives) and the one-call surrogate evaluation
//   aqc_ws_extra.cpp   zgemm, gate-level building blocks, the XXZ chain, reduced density matrices, coordinate descent, MPS helpers
//   aqc_ws_sketch.cpp  sketched AQC: resident targets, sketching-vector generators, device-resident ADAM, aqc_qr
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/aqc_hip.h"
#include "aqc_backwalk.h"
#include "aqc_devbuf.h"
#include "aqc_device.h"
#include "aqc_launch.h"
#include "aqc_plan.h"

namespace aqc {

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // sets the thread's error message; returns 1

#define HIP_OK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return ::aqc::fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline int ceil_log2(int v) {
    int b = 0;
    while ((1 << b) < v) ++b;
    return b;
}

// How much of a plan's operand buffer (d_umat) matches the coefficients in use.  The V^H and sweep plans are built by one launch and
// share the level; kURoute: only the plane sets the objective-by-projection route reads (ensure_umat, aqc_ws_sweep.cpp).
enum ULevel { kUNone = 0, kURoute = 1, kUAll = 2 };

// A lowered plan, host side only: what aqc_ctx::plan_cache keeps and the workspaces of one shape copy
struct HostPlan {
    Plan plan;
    std::vector<DevStage> h_stages;
    std::vector<DevOp> h_ops;
    std::vector<DevSub> h_subs;   // register-blocked kernels
    std::vector<DevMop> h_mops;
    int k = 0, ntiles = 0, reg_bits = 0;
    bool v2 = false;              // run the register-blocked kernels
    // matrix-core kernels (family 3)
    bool v3 = false;
    std::vector<DevSub3> h_subs3;
    std::vector<DevGrp> h_grps;
    int family() const { return v3 ? 3 : (v2 ? 2 : 1); }
};
static_assert(std::is_copy_constructible<HostPlan>::value && std::is_copy_assignable<HostPlan>::value,
              "a cached plan is copied out of the cache: it owns no device memory (a buffer member would make it move-only)");

// ... and with its device tables: one workspace's own
struct DevPlan : HostPlan {
    DevBuf<DevStage> d_stages;
    DevBuf<DevOp> d_ops;
    DevBuf<DevSub> d_subs;
    DevBuf<DevMop> d_mops;
    DevBuf<DevSub3> d_subs3;
    DevBuf<DevGrp> d_grps;
    DevBuf<double> d_umat;        // [batch][nsubs][12][64]
    DevBuf<double2> d_rpart;      // sweep plan only: [batch][nsubs][ntiles][256]
    int u_level = kUNone;         // how much of d_umat matches the coefficients in use (ULevel)
    DevPlan& operator=(const HostPlan& host) { HostPlan::operator=(host); return *this; }   // the host part alone
};

// What a derived list (a tile list, the virtual lhs pattern, a route verdict, the tiles of a partial Z) was built for: the support of
// one lhs buffer at one version, and the gather set at one generation (0: none; aqc_ws_gather_setup numbers the sets from 1)
struct ListKey {
    static constexpr int kUnknown = -2, kGatherOnly = -1;   // buf: nothing recorded / the gather set alone names the tiles
    int buf = kUnknown;
    unsigned long long supp = 0, gather = 0;
    bool operator==(const ListKey& o) const { return buf != kUnknown && buf == o.buf && supp == o.supp && gather == o.gather; }
};

// Route of one evaluation.  The caller states what the call does; eval_route (aqc_ws_sweep.cpp) alone decides how, before anything
// is enqueued, and runs the sparse route's allocations and one-off clears (a captured graph must not hold them).  enqueue_vdag,
// enqueue_gather, the sweep and route_state_after act on the value and ask nothing again.
struct EvalRoute {
    // what the call does (the caller's part)
    int x_buf = AQC_BUF_X;         // the lhs buffer of the sweep
    bool vdag = false;             // V^H from Y into Z
    bool new_thetas = false;       // thetas arrive with the call
    bool gather = false;           // the registered gather from Z ...
    bool gather_rides = false;     // ... inside the gradient walk instead of a launch of its own (aqc_ws_eval)
    bool grads = false;            // the sweep from x_buf
    // Surrogate objective: between V^H and the sweep a kernel of the call picks the lhs state among the gather indices.  The gather
    // set alone names V^H's tiles, and the support of x_buf counts as changed at that point (route_state_after restates it).
    bool support_in_gather_set = false;
    // how (eval_route's part)
    bool sparse = false;           // the sweep's first stage over the tiles of the lhs state only (head of aqc_ws_sweep.cpp)
    enum VdagKind { kStages, kRestricted, kProjected } vdag_kind = kStages;   // all stages / last stage where it is read / by projection
    bool skip_zero_w = false;      // zero groups of w skipped inside a stage (opt-in switch)
    int key_bits() const {         // what a captured graph's key must tell apart
        static_assert(AQC_NUM_BUFS <= 8, "x_buf takes the low three bits");
        return x_buf | (vdag ? 8 : 0) | (gather ? 16 : 0) | (gather_rides ? 32 : 0) | (grads ? 64 : 0) | (sparse ? 128 : 0) |
               (support_in_gather_set ? 256 : 0) | (skip_zero_w ? 512 : 0) | ((int)vdag_kind << 10);
    }
};

// Projected route of the sparse-lhs sweep (aqc_ws_project.cpp): the dense stages run on a virtual register
struct ProjRoute {
    bool ok = false;
    int t = 0, cb = 0, us = 0, nv = 0, nvp = 0, kv = 0, ntiles_v = 0;
    int first_subs = 0;            // sub-stages of the real sweep plan that still run on the real register (its first stage)
    Program vprog;                 // the gate groups of the dense stages on virtual qubits (group indices, thetas, slots: the real ones)
    std::vector<int> rest;         // their indices, in execution order
    DevPlan vsw;                   // sweep plan of the virtual register
    DevPlan vinv;                  // ... walked backwards (the objective's V^H by projection: Y_0 = (later stages)^H proj(y))
    DevBuf<double2> vm;            // [batch][2][2^nvp]: the virtual lhs pattern M_0 ...
    DevBuf<double2> vy;            // ... the virtual z ...
    DevBuf<double2> vme;           // ... and M after the later stages' gates (objective by projection)
    DevBuf<double2> cpart;         // partial tile products of the fused pass when its walk is split (few lanes)
    int cpart_shares = 0;
    int vy_copies = 1;             // vy holds this many copies of the virtual z (fused pass over more than 256 summed values: partial sums)
    unsigned l0_mask = 0;          // address bits local to the first stage
    DevBuf<unsigned> d_tab;        // off_t | off_usblk | off_cb
    std::vector<unsigned> h_tab;
    unsigned ff_mask = 0, cb_mask = 0, tf_mask = 0;
    DevBuf<TileItem> d_items;      // [2 batch ntiles_v]
    DevBuf<int> d_count;
    DevBuf<int> d_lane_parts;      // [batch]
    ListKey init_key;              // vm holds the pattern M_0 (and d_items the list) of this first-stage list (single virtual stage: nothing overwrites vm)
};

// aqc_ws_plan.cpp
void lower_plan(const Program& prog, const Plan& plan, HostPlan& out, int reg_bits, bool with_dots, bool mfma = false, bool presplit = false, int beam_width = 64);
int upload_plan(DevPlan& p);   // the device tables of a lowered plan
Plan mirror_plan(const Plan& plan);   // the same stages and sub-stages walked backwards: the plan of V^H whose intermediate states are the sweep's

}  // namespace aqc

// the two handle types of the C ABI live in the global namespace (include/aqc_hip.h)
using aqc::DevBuf; using aqc::DevPlan; using aqc::HostPlan; using aqc::PinBuf; using aqc::Program; using aqc::UJob;

struct aqc_ctx {
    Program prog;
    std::recursive_mutex mu;   // (recursive: a one-shot entry point holds it while it creates its workspace, which looks a plan up under it)
    // lowered plans (host side: stages, sub-stages, micro-ops) by (which, col_bits, tile bits, low bits, family): workspaces
    // of the same shape -- one per batch of jobs in the drivers -- share the planning work (the sub-stage search of a
    // deep Trotter ansatz takes a few tenths of a second)
    std::map<std::vector<int>, HostPlan> plan_cache;
    std::map<int, aqc_ws*> oneshot;  // ncols -> batch-1 workspace used by the host-pointer entry points
};

struct aqc_ws {
    aqc_ctx* ctx = nullptr;
    aqc::Switches sw;       // the create switches (include/aqc_switches.def), read once by aqc_ws_create
    int device = 0, batch = 1, ncols = 1, pitch = 1, col_bits = 0, nbits = 0, threads = 256;
    size_t lane_elems = 0;  // 2^nbits
    hipStream_t stream = nullptr;
    DevPlan fwd, inv, sweep;
    double* d_thetas = nullptr;       // parameters in use (own buffer or a slice of the bank)
    DevBuf<double> d_thetas_own;
    DevBuf<double> d_theta_bank;
    int bank_sets = 0, gather_count = 0;
    DevBuf<double> d_coef;
    DevBuf<double2> bufs[AQC_NUM_BUFS];
    PinBuf<double> h_pin;              // pinned staging: thetas | grads | gathered
    size_t pin_thetas = 0, pin_grads = 0, pin_small = 0;
    DevBuf<double2> d_partial;
    DevBuf<double2> d_grads;
    double* mirror_grads = nullptr;    // set by aqc_ws_eval around its launches: pinned host copies written by the kernels
    double* mirror_small = nullptr;
    DevBuf<double2> d_small;     // gather / vdot results (grow-only, like d_index and the two temporaries)
    DevBuf<double2> d_vdot_part;
    DevBuf<double2> d_vdot_out;
    DevBuf<long long> d_index;
    DevBuf<long long> d_tmp_index;      // one-shot gather / vdot: never disturb the persistent gather set-up
    DevBuf<double2> d_tmp_small;
    DevBuf<long long> d_basis_index;      // [batch], set_basis only (keeps the gather set-up intact)
    DevBuf<long long> d_combo_prev[AQC_NUM_BUFS];   // set_combo: positions written last time
    bool combo_valid[AQC_NUM_BUFS] = {false, false, false, false, false, false};   // buffer holds exactly that sparse pattern
    std::vector<long long> combo_last_elem[AQC_NUM_BUFS];   // host copy of the pattern (positions, coefficients) the HOST wrote last; device-side
    std::vector<double> combo_last_coef[AQC_NUM_BUFS];      // writers (lb_prepare) clear it
    // aqc_ws_surrogate_eval: device block [f B | fidelity B | weight B | hs 2 B S | max_no B ints], its pinned mirror
    DevBuf<char> d_sur;
    PinBuf<char> h_sur;
    int sur_states = 0;
    DevBuf<double> d_sur_real;        // real parts of the gradient when only those are asked for (grow-only)
    DevBuf<long long> d_combo_index;      // [batch][2] staging of set_combo
    DevBuf<double2> d_combo_coef;         // [batch][2]
    DevBuf<int> d_theta_slots;
    DevBuf<int> d_slot_theta;          // slot -> theta when every theta has exactly one slot (grads_direct), see rgrad_kernel
    bool grads_direct = false;
    DevBuf<int> d_slot_ntiles;
    int nslots = 0, vdot_parts = 0;
    bool coef_valid = false;
    bool need_coef = false;           // something besides the stage kernels reads d_coef (coordinate descent)
    // aqc_ws_eval as a HIP graph: the whole chain (thetas H2D, U builder, V^H stages, gather, sweep stages, gradient walk,
    // D2H copies) captured once per call signature and replayed -- one launch instead of ~11 host calls per evaluation
    std::map<std::vector<long long>, hipGraphExec_t> graphs;
    bool capturing = false;
    DevBuf<UJob> d_ujobs;             // family 3: [V^H subs | sweep subs | virtual sweep subs | V subs]; ujobs_mirror: no V^H jobs, the sweep's write both operand sets
    bool ujobs_mirror = false;
    // The jobs the objective-by-projection route reads, as a compact list of their own: [V^H's last stage (its own jobs only) | the
    // sweep's first stage | virtual sweep].  Null: the route builds everything (no projected route, or switched off).
    DevBuf<UJob> d_ujobs_route;
    int n_ujobs_route = 0;
    struct MpsSlot {
        std::vector<int> dims;          // n + 1 bond dimensions
        std::vector<size_t> offset;     // element offset of site q inside d_t
        DevBuf<double2> d_t;            // [q][2][dims[q]][dims[q+1]], lambda folded in (grow-only: re-uploads of the same shape allocate nothing)
    } mps[AQC_MPS_SLOTS];
    DevBuf<double> d_mps_lam;           // staging of the packed Schmidt vectors (grow-only)
    DevBuf<double2> d_mps_scratch;      // (grow-only)
    // device pointer tables of the batched MPS -> dense contraction: a few resident sets, found again by their contents (an
    // optimisation converts the same operands into the same lanes evaluation after evaluation: no upload, no synchronisation)
    struct MpsTabs { std::vector<const void*> host; DevBuf<const void*> dev; unsigned long long tick = 0; };
    // coordinate descent as one persistent launch: the walk's step list, thetas [batch][T] and objective values on the device
    DevBuf<aqc::CdSegHost> d_cd_prog;
    int cd_nsteps = 0;
    DevBuf<double> d_cd_thetas;
    DevBuf<double> d_cd_fobj;           // (grow-only)
    // the driver (aqc_ws_cd_minimize): best thetas [batch][T], best_f | dmax [batch] each, status | nit [batch] each and the running-lanes
    // word, the profile [batch][maxiter] (grow-only), the wide walk's two sets of partial sums [2][batch][nparts][4] (grow-only)
    DevBuf<double> d_cd_best;
    DevBuf<double> d_cd_real;
    DevBuf<int> d_cd_int;
    DevBuf<double> d_cd_profile;
    DevBuf<double> d_cd_part;
    MpsTabs mps_tabs[32];   // resident pointer-table sets (one per distinct chain: operands x lanes x bond dimensions)
    unsigned long long mps_tabs_tick = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, pev0 = nullptr, pev1 = nullptr;
    hipStream_t copy_stream = nullptr;        // aqc_ws_results_async: result copies run beside the next evaluation's kernels
    hipEvent_t ev_ready = nullptr, ev_copied = nullptr;
    hipStream_t mps_stream = nullptr;         // batched MPS -> dense: the right half's chain runs beside the left half's
    hipEvent_t ev_mps_fork = nullptr, ev_mps_join = nullptr;
    bool copy_pending = false;                // the producers of the next evaluation wait for ev_copied before they overwrite the results
    const double* theta_host = nullptr;      // aqc_ws_eval: pinned thetas the next U build reads directly (and copies to d_thetas)
    // mirrored V^H plan, its checkpoint, the sparse-lhs sweep (aqc_ws_sweep.cpp)
    bool inv_mirrored = false;     // inv = the sweep plan walked backwards: V^H into Z leaves the state before its last stage in ZW ...
    bool ckpt_valid = false;       // ... and ZW holds it for the thetas in use and the present contents of Z
    bool w_clean = true;           // W is zero outside the tiles named in d_sw_prev_tiles
    unsigned long long supp_version[AQC_NUM_BUFS] = {0, 0, 0, 0, 0, 0};   // bumped whenever d_combo_prev[buf] (the support of a sparse lhs) changes
    DevBuf<aqc::TileItem> d_sw_items;       // first-stage items of the sparse sweep [2 batch], and the tiles to clear in W
    DevBuf<aqc::TileItem> d_sw_clear;
    DevBuf<int> d_sw_counts;                // [0] items, [1] tiles to clear
    DevBuf<int> d_sw_lane_parts;            // items (= partial-R slots in use) per lane
    DevBuf<int> d_sw_prev_tiles;            // [batch][2] tiles of W written by the list in use
    int sw_lists_built = 0;                 // bit 0: the sweep's list has been built at least once, bit 1: V^H's
    aqc::ListKey sw_items_key;              // the list in d_sw_items belongs to this lhs support
    DevBuf<double2> w2;                     // second scratch pair of the sparse route (plans of >= 3 stages)
    DevBuf<double2> zw2;
    // "objective" V^H: the last stage of the mirrored V^H runs only over the tiles its readers touch -- the registered gather
    // indices and the support of the lhs state -- and Z is completed on demand (ensure_z_full) while the checkpoint is valid
    bool z_full = true;                     // Z holds V^H y everywhere (false: on the tiles of d_vd_items only)
    DevBuf<aqc::TileItem> d_vd_items;       // [batch][2 + gather_count] (grow-only)
    unsigned long long gather_gen = 0;      // bumped by aqc_ws_gather_setup
    aqc::ListKey vd_key;                    // what d_vd_items was built from
    aqc::ListKey z_key;                     // what the tiles of a partial Z were chosen for
    aqc::ProjRoute proj;                    // dense stages of the sparse route on a virtual register
    bool proj_y0_ready = false;             // the virtual z (proj.vy) holds Y_0 for the sweep that follows in the same call (run_vdag_projected)
    bool proj_vr_ready = false;             // ... and the virtual plan's partial-R rows hold this call's R: that launch walked the virtual stage back (projected_virtual_backwalk)
    bool z_from_y = false;                  // a partial Z without a checkpoint: completed by a full V^H from Y (thetas and Y unchanged since)
    std::vector<long long> h_gather;        // host copy of the registered gather indices (elements)
    aqc::ListKey projb_key;                 // what the verdict below was taken for
    bool projb_ok = false;
    // sketched AQC (aqc_ws_sketch.cpp): the d x d target(s) and everything a device-resident ADAM run keeps between its launches
    struct Sketch {
        DevBuf<double2> target;         // [batch or 1][d][d]
        bool shared = false;
        DevBuf<double2> qr_part;        // gram partials [batch][slabs][k][k]
        DevBuf<double2> qr_rinv;        // [batch][k][k]
        DevBuf<double2> tmp;            // [batch] lanes of scratch (U^H Omega, then the QR's first-pass Q)
        DevBuf<int> status;             // [batch] QR status words
        DevBuf<int> idx;                // alt column indices [sets][batch][k] (grow-only)
        DevBuf<double> adam;            // m | v | best_x [batch][T] each, then best_f | lr [batch]
        DevBuf<int> adam_i;             // t | nit | flag [batch]
        DevBuf<double> adam_x;          // [batch][T] the run's own last point: what reset = 0 resumes from, whatever thetas other calls put in use
        DevBuf<double> profile;         // [batch][capacity / batch] (grow-only)
        bool adam_started = false;
    } sk;
    bool profile = false;
    int64_t prof_count[AQC_NUM_KINDS] = {};
    double prof_ms[AQC_NUM_KINDS] = {};
    std::vector<std::pair<int, float>> prof_log;   // (kind, ms) of every profiled launch, in order (bounded)
};

namespace aqc {

struct ProfScope {  // brackets one launch with events when profiling is on
    aqc_ws* ws;
    int kind;
    ProfScope(aqc_ws* w, int k) : ws(w), kind(k) {
        if (ws->profile) (void)hipEventRecord(ws->pev0, ws->stream);
    }
    ~ProfScope() {
        if (!ws->profile) return;
        float ms = 0.f;
        if (hipEventRecord(ws->pev1, ws->stream) == hipSuccess && hipEventSynchronize(ws->pev1) == hipSuccess &&
            hipEventElapsedTime(&ms, ws->pev0, ws->pev1) == hipSuccess) {
            ws->prof_count[kind] += 1;
            ws->prof_ms[kind] += ms;
            if (ws->prof_log.size() < 100000) ws->prof_log.emplace_back(kind, ms);
        }
    }
};

// ---- what the two calls that replay graphs (aqc_ws_eval, aqc_ws_surrogate_eval) share before they enqueue ----
// result copies of an earlier aqc_ws_results_async: the call reuses the pinned staging buffer and may replay a graph
inline int wait_result_copies(aqc_ws* ws) {
    if (!ws->copy_pending) return 0;
    HIP_OK(hipStreamSynchronize(ws->copy_stream));
    ws->copy_pending = false;
    return 0;
}
// Small results skip the device-to-host copy nodes: the producing kernels write a second copy straight into pinned memory (null: no
// second copy).  Cleared on every exit, the error paths of enqueue() too: no stale pinned thetas in the next call.
struct MirrorScope {
    aqc_ws* w;
    MirrorScope(aqc_ws* w_, double* grads, double* small) : w(w_) { w->mirror_grads = grads; w->mirror_small = small; }
    ~MirrorScope() { w->mirror_grads = nullptr; w->mirror_small = nullptr; w->theta_host = nullptr; }
};
// matrix-core path, small batch: no copy node for the thetas -- the U builder (first kernel of V^H or of the sweep) reads the pinned
// thetas over the bus and stores them to HBM for the gradient walk
inline bool direct_thetas(const aqc_ws* ws, bool zero_copy) {
    return zero_copy && ws->fwd.v3 && ws->inv.v3 && ws->sweep.v3 && !ws->need_coef;
}

// aqc_api.cpp
int check_buf(const aqc_ws* ws, int buf);
int check_block_range(const aqc_ws* ws, int block_from, int block_to);
int ensure_coef(aqc_ws* ws);
int copy_in(aqc_ws* ws, double2* dst, const double* src, size_t rows);
int copy_out(aqc_ws* ws, double* dst, const double2* src, size_t rows);
int results_guard(aqc_ws* ws);
// aqc_ws_sweep.cpp: the host-side record of what the buffers hold (Z, ZW, W, the lhs supports, the derived lists) changes only here
int before_read(aqc_ws* ws, int buf);         // the host, or a kernel over all of it, reads the buffer: completes a partial Z
int before_gather(aqc_ws* ws, int buf);       // the registered gather reads it: a partial Z chosen for that set covers it
int before_write(aqc_ws* ws, int buf, bool some_lanes = false);   // a writer other than the V^H / sweep pair (the lanes not written are kept)
// written whole: the pattern d_combo_prev names, known to the host (elem, coef) or chosen on the device (none)
void lhs_support_changed(aqc_ws* ws, int buf, std::vector<long long> elem = {}, std::vector<double> coef = {});
int run_coef(aqc_ws* ws, double* d_thetas);   // new thetas in use (and their coefficients where the kernels need them)
void thetas_changed(aqc_ws* ws, double* d_thetas);
ListKey key_of(const aqc_ws* ws, int lhs_buf, bool gather);   // lhs_buf: ListKey::kGatherOnly for the gather set alone
bool built_for(const aqc_ws* ws, const ListKey& slot, const ListKey& key);   // the list `slot` names is built for `key`
void record_key(const aqc_ws* ws, ListKey& slot, const ListKey& key);         // ... it is now
void replay_state_after(aqc_ws* ws);          // forgets the lists a graph replay has rebuilt on the device behind the host's back
int eval_route(aqc_ws* ws, EvalRoute& route);             // completes the route (see EvalRoute)
int enqueue_vdag(aqc_ws* ws, const EvalRoute& route);     // Y -> Z by the route's kind of V^H
int enqueue_gather(aqc_ws* ws, const EvalRoute& route);   // the registered gather of that Z (a launch of its own)
void route_state_after(aqc_ws* ws, const EvalRoute& route);   // the record those and the sweep leave, restated after a graph replay
// enqueue() with new thetas, captured once per (call's own words, route, addresses the nodes hold) and replayed
int run_graph(aqc_ws* ws, const EvalRoute& route, std::initializer_list<long long> call, const std::function<int()>& enqueue);
void vdag_projected_state_after(aqc_ws* ws, int x_buf);
int grad_from_impl(aqc_ws* ws, const EvalRoute& route, int block_from, int block_to, int front_layer);   // the sweep and the gradient walk
int sweep_r_only_sub(const aqc_ws* ws);
int ensure_umat(aqc_ws* ws, DevPlan& p, int need = kUAll);   // need: kURoute when the caller reads the projected route's plane sets only
int run_apply(aqc_ws* ws, bool inverse, int src_buf, int dst_buf);
// descriptions of a matrix-core stage launch; the buffers and what is particular to the launch are the caller's
Stage3Args stage3_args(aqc_ws* ws, const DevPlan& p, size_t s);   // stage s of a plan on the full-size register, over all (tile, lane) pairs
void stage3_first_list(const aqc_ws* ws, Stage3Args& a);          // ... over the first-stage item list of the sparse sweep instead
void stage3_sweep_fields(Stage3Args& a, const DevPlan& p, int nparts, int chunk);   // the sweep-only fields: p's partial-R buffer with its slots per (lane,
                                                                                    // sub-stage), the persistent chunk, the first sub-stage's operand offsets
void drop_graphs(aqc_ws* ws);
// aqc_ws_project.cpp
void proj_plan(aqc_ws* ws, int low_bits);   // decides the route and lowers the virtual plan (host only)
int proj_alloc(aqc_ws* ws);                 // its device side (plan tables, buffers, offset tables)
// Launches over a tile list (the sparse route, its restricted V^H, the projected route) are persistent on 2^12 tiles: without the
// persistent V / V^H (AQC_APPLY_PERSIST <= 0) such a workspace has none of them and every evaluation takes the dense route
bool list_launches_allowed(const aqc_ws* ws);
bool sweep_route_projected(const aqc_ws* ws, bool sparse);
bool projected_pairs(const aqc_ws* ws);      // the route's independent tile launches run in pairs
bool backwalk_keeps_vdag_stage(const aqc_ws* ws);   // ... as single launches (pairs switched off): V^H's last stage still writes that tile, the walk stores nothing
bool projected_backwalk(const aqc_ws* ws);   // objective by projection: the sweep's first stage walks back from (psi, C) and writes the Z tile (no V^H stage at all)
Stage3Args virtual_stage3_args(aqc_ws* ws, const DevPlan& v, size_t s);   // stage s of a virtual plan (vsw, vinv) on the virtual register, over its item list
Stage3Args projected_sweep_stage(aqc_ws* ws, size_t s);   // arguments of stage s of the virtual sweep plan
int run_projected_stages(aqc_ws* ws);       // projection + the virtual stage launches (after the sweep's first stage)
bool projected_virtual_backwalk(const aqc_ws* ws);   // ... and the virtual stage walks back from (M_end, Y_end) inside the launch that leaves Y_0 (run_vdag_projected)
aqc::RgradSecond projected_rgrad_plan(aqc_ws* ws, bool walked_back);   // the virtual plan's gradient walk, to ride in the real plan's launch (walked_back: its R rows come from the backward walk)
bool vdag_route_projected(aqc_ws* ws, int x_buf);   // the objective's V^H by two passes over y instead of its stages (host-known single basis state)
int run_vdag_projected(aqc_ws* ws, int x_buf);      // Y -> Z on the lhs tiles, the virtual z for the sweep that follows
int proj_fix_amplitudes(aqc_ws* ws, int x_buf);     // after the gather: the amplitudes outside the lhs tiles, from the virtual z
int ensure_sweep_items(aqc_ws* ws, int x_buf);      // aqc_ws_sweep.cpp: the first-stage item list of the sparse sweep, rebuilt when the support changed

}  // namespace aqc
