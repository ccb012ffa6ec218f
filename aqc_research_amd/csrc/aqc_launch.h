// Host-visible launch interface of aqc_kernels.hip.
#pragma once
#include <string>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "aqc_device.h"
#include "aqc_mps_walk.h"
#include "aqc_switches.h"

namespace aqc {

struct StageArgs {
    const DevStage* stage;  // this stage's descriptor (device)
    const DevOp* ops;       // all ops of the plan (device)
    const DevSub* subs;     // register-blocked kernels: sub-stages of the plan
    const DevMop* mops;     // ... and their micro-ops
    const double* coef;     // [batch][ncoef][kCoefStride]
    int ncoef;
    const double2* in0;     // apply: src; sweep: w in
    const double2* in1;     // sweep: z in
    double2* out0;          // apply: dst; sweep: w out
    double2* out1;          // sweep: z out
    size_t lane_stride;     // elements between consecutive batch lanes
    double2* partial;       // [batch][nslots][ntiles_max] inner-product partials
    int nslots, ntiles_max;
    int from, to, front;    // block_range / front_layer (core_operations.py:829-830)
    int final_stage;        // register-blocked V / V^H: last launch applies the lane's overall sign
    int debug;              // work-skipping bits (tuning builds, timing experiments only): 1 skip micro-op bodies, 2 skip reductions
};

size_t apply_lds_bytes(int k);
size_t sweep_lds_bytes(int k, int threads);
hipError_t init_kernels();
hipError_t launch_apply(int ent, bool inverse, int ntiles, int batch, int threads, int k, hipStream_t s, const StageArgs& a);
hipError_t launch_sweep(int ent, int ntiles, int batch, int threads, int k, hipStream_t s, const StageArgs& a);
hipError_t launch_coef(const double* thetas, double* coef, int n, int nblocks, int tpb, int tail, int batch, hipStream_t s);
hipError_t launch_finalize(const void* partial, const int* theta_slots, const int* slot_ntiles, void* grads, int T,
                           int nslots, int ntiles_max, int n, int tpb, int from, int to, int front, int batch,
                           hipStream_t s, void* mirror = nullptr);   // mirror: optional pinned host copy of the result
hipError_t launch_scatter_one(void* buf, size_t lane_stride, int batch, const long long* elem, hipStream_t s);
hipError_t launch_scatter_two(void* buf, size_t lane_stride, int batch, const long long* elem, const void* coef, long long* prev, hipStream_t s);
hipError_t launch_set_identity(void* buf, size_t lane_stride, int dim, int pitch, int batch, hipStream_t s);
hipError_t launch_gather(const void* buf, size_t lane_stride, const long long* elem, int count, int batch, void* out,
                         hipStream_t s, void* mirror = nullptr);
hipError_t launch_vdot(const void* a, const void* b, size_t lane_stride, size_t count, int batch, void* part, int nparts,
                       void* out, hipStream_t s);

// aqc_kernels2.hip (register-blocked kernels)
hipError_t init_kernels2();
hipError_t launch_apply2(int ent, int ntiles, int batch, int k, hipStream_t s, const StageArgs& a);
hipError_t launch_sweep2(int ent, int ntiles, int batch, int k, int reg_bits, hipStream_t s, const StageArgs& a);

// aqc_kernels3.hip (matrix-core kernels)
struct TileItem { int lane, tile, slot, pad; };   // one (tile, lane) work item of a stage launch over a SUBSET of the tiles; slot: its partial-R slot
struct Stage3Args {
    DevStage stage;          // by value: kernel arguments live in the constant address space, so the offset tables are
                             // scalar loads that no store of the kernel can invalidate
    const DevSub3* subs;     // all sub-stages of the plan
    const double* umat;      // [batch][nsubs_total][3][4][64]: MFMA B operands of every sub-stage's 16 x 16 unitary
    int nsubs_total;
    const double2* in0;      // apply: src; sweep: w in
    const double2* in1;      // sweep: z in
    double2* out0;
    double2* out1;
    size_t lane_stride;
    double2* rpart;          // sweep: [batch][nsubs_total][ntiles][256] per-tile R = Z W^H of every sub-stage
    int ntiles;
    int batch;               // lanes of the batch (sweep: work items = ntiles x batch)
    int chunk, nparts;       // sweep: items per persistent workgroup (0: one item per workgroup) and partial-R slots per
                             // (lane, sub-stage) -- sweep3_chunk / sweep3_nparts
    int store_out;           // sweep: bit 0 store w, bit 1 store z; 0 for the last stage (its w and z are never read again)
    int r_only_last;         // sweep, last stage: its last sub-stage computes R from its INPUTS alone (no U products); the gradient walk
                             // conjugates that R by the sub-stage's U (launch_rgrad: conj_sub)
    int backwalk;            // sweep over an item list: the stage is the mirrored plan's (U^H of a sweep stage, walked backwards from the
                             // states the forward walk ends in); every sub-stage's R goes to the slot of the forward sub-stage it mirrors
                             // (aqc_backwalk.h), rpart is the SWEEP plan's buffer.  At least two sub-stages, no R-only form
    const long long* supp;  // sweep from basis states: supp[lane][2] = element index of the lane's (<= 2) basis states (-1: none), or null.
                             // The kernel then skips the W and R products of 16-chunk groups (and K-steps of the W product) where w is
                             // zero by construction (DevSub3::skipinfo, DevStage::fresh_nonlocal) -- exact zeros, so the results do not change
    const TileItem* items;   // launch over a subset of the (tile, lane) pairs: device table + its length on the device (null: all pairs);
    const int* nitems;       // the grid is sized for max_items, the kernels read the actual length
    int max_items;
    unsigned first_hi[16][4];   // persistent sweep: tile offset (elements) of the FIRST sub-stage's operand of (group, K-step);
                                // a lane adds the offset of its own (chunk l % 16, amplitude l / 16) position (stage3_first_offsets)
    int debug;               // tuning builds: work-skipping bits for timing experiments (1 LDS writes, 2 LDS reads, 4 R MFMAs, 8 U MFMAs)
    unsigned long long* stamps;   // tuning builds (-DAQC_TUNING): [workgroup][kStampSlots] s_memtime stamps of wave 0, else null
};
constexpr int kStampSlots = 40;
void stage3_first_offsets(Stage3Args& a, const DevSub3& first_sub);   // host: fills first_hi from the stage and its first sub-stage
hipError_t init_kernels3();
int mfma_threads(int k, bool sweep);
int mfma_occupancy(int k, bool sweep);
// k: tile size, 8..12; sw: the workspace's switches (the persistent grids of 2^12 tiles: sweep_grid, apply_persist) -- host arguments,
// never part of a kernel's argument block
hipError_t launch_apply3(int k, hipStream_t s, const Stage3Args& a, const Switches& sw);
hipError_t launch_sweep3(int k, hipStream_t s, const Stage3Args& a, const Switches& sw);
// Two independent item-list launches of the same tile size k in one grid: every workgroup walks its share of a's list, then of b's, each
// item exactly as the single launch computes it (apply_pair_kernel / sweep_pair_kernel).  The lists, partial-R slots and lane_parts are
// the single launches' own.
hipError_t launch_apply3_pair(int k, hipStream_t s, const Stage3Args& a, const Stage3Args& b, const Switches& sw);
hipError_t launch_sweep3_pair(int k, hipStream_t s, const Stage3Args& a, const Stage3Args& b, const Switches& sw);
void rgrad_print_stamps(int nsubs);   // tuning builds only
int sweep3_chunk(int ntiles, int batch, int k, long sweep_grid);    // sweep_grid: the workspace's (<= 0: one workgroup per CU); what sized
int sweep3_nparts(int ntiles, int batch, int k, long sweep_grid);   // d_rpart, what the sweep fills in and what launch_sweep3 checks
// Projected dense stages of the sparse-lhs sweep (aqc_project.hip, aqc_ws_project.cpp): the state that enters the stages after the
// first is psi (x) |e> on (first stage's local bits) x (the other bits), and those stages touch the qubits T only, so everything the
// gradient needs of z there is its projection y0[i_T, c] = sum_u conj(psi[u, c]) z[u, i_T] (u: local bits of the first stage outside T,
// c: those inside T) -- a register of |T| + |c| virtual qubits per lane instead of n.
struct ProjMap { const unsigned* tab; int shift; };   // index -> element offset: a table, or the index shifted (virtual register)
struct ProjArgs {
    // the product  out[keep, c] = sum_k conj(S[k, c]) Y[k, keep]  per item
    const double2* y;        // full-size operand, [batch][lane_stride]; read at (lane) + (the item's tile bits & ff_mask) + y_keep[keep] + y_k[k]
    const double2* s;        // small operand: real register (lane + the item's tile + s_k[k] + s_c[c]) or virtual ((2 lane + slot) << nvp + ...)
    double2* out;            // the same choice
    int s_virtual, out_virtual;
    int staged;              // k runs along contiguous memory of y and s (low four bits of k = address bits 0..3): fetch 256-byte runs through LDS
    int keep_bits, k_bits, cb;
    ProjMap y_keep, y_k, s_k, s_c, o_keep, o_c;
    size_t lane_stride;
    const TileItem* items;   // first-stage items of the sparse sweep (lane, tile of the first stage, slot) and their number
    const int* nitems;
    const int* lane_parts;   // items per lane
    int nub0, ubits0[32];    // non-local address bits of the first stage (tile index -> element offset)
    unsigned ff_mask, cb_mask, tf_mask;   // address bits outside the first stage's local set and outside T (fixed to the item's) / in both / in T only
    int nvp;
    // project_init_kernel: the virtual lhs pattern and the bookkeeping of the virtual stage launches
    const unsigned* off_t;   // [2^t]: element offset of the value i of the T bits;  [2^cb]: of the value c of the bits shared with the first stage
    const unsigned* off_cb;
    const unsigned* it_of_c; // [2^cb]: index on the T bits whose shared bits hold c (the others 0)
    const unsigned* off_us;  // [2^us]: element offset of the value u of the first stage's local bits outside T
    int us_bits;
    size_t part_stride;      // fused pass with more than 256 summed values: elements between the partial copies of the virtual z
    double2* cpart;          // fused pass with few items: [shares][2 batch][2^us][16] partial tile products (null: never split)
    int cpart_shares;
    int t, ntiles_v;
    double2* vm;             // [batch][2][2^nvp]
    TileItem* vitems;        // items of the virtual stage launches: (lane, slot ntiles_v + tile, the same as partial slot)
    int* vcount;
    int* vlane_parts;
    int batch;
    int item0;               // kernels with the items in grid.y: the first item of this launch (launch_project, the sums of the fused pass)
};
hipError_t launch_project_init(const ProjArgs& a, hipStream_t s);
hipError_t launch_project_fused(const ProjArgs& a, const void* mend, void* ctile, void* yout, hipStream_t s, int qb);   // qb: 2 or 4 blocks of u per wave; both products of the objective by projection, one fetch of y
hipError_t launch_project_amps(const ProjArgs& a, const long long* gather, int ngather, const long long* supp, void* small, const void* vy, const void* z,
                               hipStream_t s);   // the whole gather of an evaluation by projection: inside the lhs tile from z, outside from the virtual z
hipError_t launch_project(const ProjArgs& a, hipStream_t s);
struct UJob {               // one 16 x 16 unitary to build: sub-stage `index` of a plan with `nsubs` sub-stages
    const DevSub3* sub;
    const DevGrp* grps;      // the plan's gate groups
    double* umat;            // the plan's operand buffer [batch][nsubs][12][64]
    int index, nsubs;
    int inverse, entangler;  // V^H plans apply every group conjugate-transposed; 0 cx, 1 cz, 2 cp
    double* umat_mirror;     // mirrored V^H plan (or null): this sub-stage's U^H is sub-stage `mirror_index` of that plan's operand buffer
    int mirror_index, mirror_nsubs;
};
hipError_t launch_ubuild(const UJob* jobs, int njobs, const double* thetas, int T, int batch, hipStream_t s, double* thetas_copy = nullptr);
struct GatherJob {           // optional passenger of the gradient walk: out[lane][i] = buf[lane][elem[i]] (+ pinned host copy)
    const void* buf; size_t lane_stride; const long long* elem; int count; void* out; void* mirror;
};
struct RgradSecond {         // a second plan whose gradient walk rides in the same launch (projected route: the virtual sweep plan); all of its
    const DevSub3* subs;     // sub-stages hold lane_parts[lane] partials (item-list launches)
    const DevGrp* grps;
    const double2* rpart;
    const int* lane_parts;
    const double* umat;
    int nparts, nsubs_total, count;   // partial slots per (lane, sub-stage); sub-stages of the plan; how many of them walk here (0: none)
    int conj_sub;            // the plan's sub-stage whose R arrives as Z W^H of its INPUTS (the virtual stage walked backwards: aqc_backwalk.h), or -1
};
hipError_t launch_rgrad(const DevSub3* subs, const DevGrp* grps, int entangler, const double* thetas, int T, const void* rpart,
                        int ntiles, int nsubs_total, void* partial, int nslots, int from, int to, int front, int batch, hipStream_t s,
                        const int* slot_theta = nullptr, void* grads = nullptr, void* mirror = nullptr,
                        GatherJob gather = GatherJob{nullptr, 0, nullptr, 0, nullptr, nullptr},   // slot_theta: direct mode, see rgrad_kernel
                        int nparts = 0, int chunk = 0,   // partial-R slots per (lane, sub-stage) and the persistent sweep's chunk
                        int sparse_subs = 0, const int* lane_parts = nullptr,   // the first sparse_subs sub-stages hold lane_parts[lane] partials (item-list launch)
                        int conj_sub = -1, const double* umat = nullptr,        // sub-stage whose R arrives as Z W^H of its INPUTS: R <- U R U^H first (umat: the plan's operands)
                        int nsubs_run = -1,                                     // walk the first nsubs_run sub-stages only (-1: all)
                        const RgradSecond* second_plan = nullptr);
// Tile lists on the device (aqc_ws_sweep.cpp).  Per lane, the tiles of `stage` that hold the elements supp[lane][0 .. per_lane)
// (the support of the lane's sparse lhs state; -1 = none; may be null) and extra[0 .. nextra) (the same for every lane: the
// registered gather set; may be null), each tile once, in that order -> item list (lane-major, slot = position inside the lane),
// its length, items per lane.  prev_tiles (may be null; [lane][2], per_lane <= 2, no extras): tiles named by the previous list
// of this table that the new one drops -> clear list (they hold stale amplitudes in a buffer that is zero elsewhere); updated.
// One workgroup.
constexpr int kMaxTileCands = 72;   // per_lane + nextra
hipError_t launch_tile_items(const DevStage& stage, const long long* supp, int per_lane, const long long* extra, int nextra, int batch,
                             TileItem* items, int* nitems, int* lane_parts, int* prev_tiles, TileItem* clear_items, int* nclear, hipStream_t s);
hipError_t launch_clear_tiles(const DevStage& stage, void* buf, size_t lane_stride, const TileItem* clear_items, const int* nclear, int max_items,
                              hipStream_t s);

// aqc_lbfgs.hip (device-resident multi-start L-BFGS on the lane-batched surrogate objective)
struct LbState {
    int B, T, S, memory;          // lanes, parameters, gathered flip states, history length
    double *x, *g, *f;            // current point, gradient, value (under the current objective state)
    double *d, *slope, *step;     // search direction, g.d, step length per lane
    double *x_new;                // accepted trial points of the running line search
    double *Smem, *Ymem, *rho;    // history [memory][B][T], [memory][B]
    int *active, *done;
    long long* nit;
    double *weight, *fidelity;   // objective state: smoothed weight, |h_0|^2
    int* max_no;
    double2 *cur_hs, *cur_g0;     // raw device results of the current point: amplitudes, complex gradient of its one sweep
    double2 *acc_hs, *acc_g0;     // ... of the accepted trial points
};
hipError_t lb_prepare(const LbState& st, const void* hs, int update, double* f_out, void* raw_hs, void* x2, size_t lane_stride,
                      const long long* index, long long* prev, hipStream_t s);
hipError_t lb_take(const LbState& st, const void* grads, double* g_out, void* raw_g, hipStream_t s);
hipError_t lb_probe(const LbState& st, const void* hs, int* flags, hipStream_t s);
hipError_t lb_commit0(const LbState& st, const void* hs, const void* raw_g, double* f_out, double* g_out, hipStream_t s);
hipError_t lb_active(const LbState& st, double gtol, double fid_thr, int* flags, hipStream_t s);
hipError_t lb_direction(const LbState& st, int count, hipStream_t s);
hipError_t lb_trial(const LbState& st, double* thetas, hipStream_t s);
hipError_t lb_armijo(const LbState& st, double c1, const double* thetas, const double* ft, const void* raw_hs_t, const void* raw_g0_t,
                     int* flags, hipStream_t s);
hipError_t lb_copy_raw(const LbState& st, hipStream_t s);
hipError_t lb_history(const LbState& st, int count, double ftol, const double* f_acc, const double* g_acc, hipStream_t s);
// The state-free mode of the same step kernels (S = 0): L-BFGS on the matrix objective f = 1 - Re tr(X^H V^H Y) / k of full and
// fixed-sketch AQC.  The objective has no state, so an accepted trial's value and gradient are final: no amplitude rows, no raw
// copies, no probe / commit / second evaluation.  What the mode adds to LbState:
struct LbMat {
    int k;                                    // columns of the workspace (the trace's divisor)
    double gtol, fobj_thr, fid_thr;           // a lane stops at max|g| <= gtol, f <= fobj_thr, |tr|^2/k^2 >= fid_thr (thresholds: 0 = off)
    double *gmax;                             // max|g| at the current point (|tr|^2/k^2 there: LbState::fidelity)
    double *ft, *gt, *gmax_t, *fid_t;         // the trial points' results
    double *f_acc, *g_acc, *gmax_acc, *fid_acc;   // ... of the accepted points (the current point's for a lane that does not move)
    int* status;                              // per lane, 0 = fine (kLbNonFinite: f or g was not finite; the lane stopped where it was)
    int* flags;                               // ONE word per line-search trial: kLbNotDone | kLbAnyActive
};
enum { kLbNotDone = 1, kLbAnyActive = 2 };    // some lane still backtracks / some lane goes on to another iteration
enum { kLbNonFinite = 1 };
// f, g, max|g| and |tr|^2/k^2 of every lane from the trace and the complex gradient an evaluation leaves (init: at the start point, into
// the current point's rows, with the first "any lane active" flag; else into the trial rows)
hipError_t lb_mat_value(const LbState& st, const LbMat& m, const void* trace, const void* grads, int init, hipStream_t s);
hipError_t lb_mat_direction(const LbState& st, const LbMat& m, int count, hipStream_t s);
hipError_t lb_mat_armijo(const LbState& st, const LbMat& m, double c1, const double* thetas, hipStream_t s);
// runs once no lane backtracks any more (the flag word Armijo has just written) or `last`; sets kLbAnyActive
hipError_t lb_mat_history(const LbState& st, const LbMat& m, int count, double ftol, int last, hipStream_t s);

// aqc_mps.hip
hipError_t launch_mps_scale(void* g, const double* lam, int rows, int cols, hipStream_t s);
hipError_t launch_zgemm(bool conj_t, bool accum, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                        void* C, int ldc, hipStream_t s);
hipError_t launch_zgemm_bh(bool conj_t, bool accum, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                           void* C, int ldc, hipStream_t s);   // C = op(A) . B^H, B stored (N x K)
hipError_t launch_mps_env_dot(const void* e, const void* rc, size_t count, void* out, hipStream_t s);
hipError_t launch_zgemm_batched(bool conj_t, bool accum, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                                void* C, int ldc, size_t stride_a, size_t stride_b, size_t stride_c, int nbatch, hipStream_t s);
hipError_t launch_zgemm_tables(int M, int N, int K, const void* const* a_tab, int lda, const void* const* b_tab, int ldb, void* const* c_tab, int ldc,
                               size_t stride_a, size_t stride_b, size_t stride_c, int outer, int inner, hipStream_t s, int b_transposed = 0);
// the same with op(A) = A^H (A stored K x M) and / or accumulation into C
hipError_t launch_zgemm_tables_op(bool conj_t, bool accum, int M, int N, int K, const void* const* a_tab, int lda, const void* const* b_tab, int ldb,
                                  void* const* c_tab, int ldc, size_t stride_a, size_t stride_b, size_t stride_c, int outer, int inner, hipStream_t s);
hipError_t launch_mps_product(const void* const* t_tab, void* const* out_tab, int n, int count, hipStream_t s);
struct MpsSites {            // site table of one MPS (by value in the kernel arguments)
    int n;
    size_t total;            // complex elements of all site tensors
    size_t offset[65];       // element offset of site q
    int lam_offset[64];      // offset of lambda_q inside the packed Schmidt vectors
    int cols[64];            // right bond dimension of site q
};
hipError_t launch_mps_scale_all(void* t, const double* lam, const MpsSites& sites, hipStream_t s);

// aqc_cd.hip
// the whole walk as one persistent launch (a workgroup per lane, operands in LDS): segment list entry = CdSeg of aqc_cd.hip
struct CdSegHost { int32_t ha, hb, ent, nrot, kind[4], on_b[4], tindex[4]; };
size_t cd_persistent_lds_bytes(int nbits, int T);
// The driver's state of every lane (aqc_ws_cd_minimize), as both routes see it; the rules themselves: aqc_cd_rule.h
struct CdRule {
    int* status;           // [batch] kCdRunning / kCdNormal / kCdEarly / kCdTimeout
    int* nit;              // [batch] sweeps closed so far
    double* best_f;        // [batch]
    double* best_thetas;   // [batch][T]
    double* profile;       // [batch][maxiter]
    double fobj_thr, dtheta_thr;
    int maxiter;
};
// rule: null for the plain sweeps of aqc_ws_cd_sweeps (fobj[batch][nsweeps] is written: the kernel instance without the rules); with a
// rule the lanes that still run do up to nsweeps more sweeps, a lane leaves its loop when the rule ends it, and fobj is not used
hipError_t launch_cd_persistent(const void* prog, int nsegs, int nbits, int col_bits, const void* target, size_t lane_stride, double* thetas,
                                int T, double* fobj, int nsweeps, int max_steps, int batch, hipStream_t s, const CdRule* rule = nullptr);
// the walk with the operands in HBM (beyond 6 qubits), grid (nparts, batch): one opener per segment, one step per parameter
struct CdWide {
    void* w; void* z;              // [batch][lane_stride] complex
    size_t lane_stride;
    int ngroups, nparts;           // 4-element groups of a lane; workgroups (= partial sets) per lane, cd_wide_parts(lane_elems)
    int ha, hb, ent;               // the segment: address bits of its two qubits, 0 none / 1 CX / 2 CZ (opener)
    int kind, on_b, tindex;        // the step's parameter: 0 Ry / 1 Rz / 2 Rx, on bit a or b, its index
    int next_kind, next_on_b;      // the parameter whose partial sums the launch leaves (next_kind < 0: none, it closed the segment)
    int T;
    const double* theta_in;        // [batch][T] thetas at the start of the sweep: the old angles
    double* theta_out;             // [batch][T] the sweep's thetas
    double* dmax;                  // [batch] running max |theta_new - theta_old| of the sweep
    const int* status;             // [batch]
    const double* part_in;         // [batch][nparts][4] partial sums of this parameter ...
    double* part_out;              // ... and of the next one (the other buffer of the pair)
    double inv_d2n;
};
int cd_wide_parts(size_t lane_elems);
hipError_t launch_cd_wide_open(const CdWide& a, int batch, hipStream_t s);
hipError_t launch_cd_wide_step(const CdWide& a, int batch, hipStream_t s);
struct CdClose {
    CdRule rule;
    const double2* trace;          // [batch] <w|z> of the vdot launch
    double* dmax;                  // [batch], cleared for the next sweep
    double* theta_own;             // [batch][T] <- theta_cur: what the next sweep's V^H and old angles read
    const double* theta_cur;
    int T;
    double inv_d2n;
};
hipError_t launch_cd_close(const CdClose& a, int batch, hipStream_t s);
// running <- lanes whose status is kCdRunning; mark != 0: those lanes get that status first (the time limit) and running <- 0
hipError_t launch_cd_count(int* status, int batch, int mark, int* running, hipStream_t s);


// aqc_gate.hip (gate-level building blocks, one pass per call)
hipError_t launch_gate1q(const void* src, void* dst, int n, size_t ncols, int q, const double* g, hipStream_t s);
hipError_t launch_gate2q(const void* src, void* dst, int n, size_t ncols, int qc, int qt, const double* g, hipStream_t s);
int gate_dot_parts(int n, size_t ncols, int kind);
hipError_t launch_gate_dot(const void* w, const void* z, int n, size_t ncols, int kind, int q0, int q1, void* partial, void* out,
                           hipStream_t s);

// aqc_xxz.hip (matrix-free XXZ Hamiltonian and the Chebyshev step of exp(-iHt); rules: aqc_xxz_rule.h)
constexpr int kXxzThreads = 256, kXxzTileBits = 11;   // a tile = 2^min(n, 11) amplitudes = at most 32 KiB of LDS
struct XxzArgs {
    int n, tile_bits, lanes;       // tile_bits = xxz_tile_bits(n); grid (2^(n - tile_bits), lanes)
    double delta;
    const double2* cur;            // the vector whose neighbours are read; lane l at cur + l * cur_stride (0: one state for all lanes)
    size_t cur_stride;
    const double2* prev;           // step: T_{k-1}, lane l at prev + l * prev_stride (not read by the first step)
    size_t prev_stride;
    double2* next;                 // mul: H cur; step: T_{k+1} -- [lanes][2^n]; may be prev
    double2* out;                  // step: the running sum [lanes][2^n]
    const double2* coef;           // step: c_k of every lane, [lanes]
    const double2* coef0;          // first step: c_0 of every lane
    double scale;                  // step: 1/R (first) or 2/R
    int first;                     // step: next = scale H cur, out = c_0 cur + c_1 next
    double* partial;               // energy: [lanes][tiles]
};
int xxz_tile_bits(int n);
hipError_t launch_xxz_mul(const XxzArgs& a, hipStream_t s);
hipError_t launch_xxz_step(const XxzArgs& a, hipStream_t s);
hipError_t launch_xxz_energy(const XxzArgs& a, double* energy /* [lanes] */, hipStream_t s);   // partials, then their fixed-order sum

// aqc_obs.hip (reduced density matrices of 4-qubit sets on the matrix cores, one launch per pass of the plan; rules: aqc_obs_rule.h)
constexpr int kObsThreads = 256, kObsSubsetCap = 16, kObsGridCap = 512;
struct ObsArgs {
    int n, tile_bits, lanes, nsub;     // tile_bits = min(n, kObsTileBits) = |bits|; nsub <= kObsSubsetCap
    int ksplit;                        // = obs_ksplit(nsub): the waves that share a subset's columns
    uint32_t bits;                     // the pass's bit set B, a mask of qubits
    uint16_t subsets[kObsSubsetCap];   // masks of 4 tile-local positions (below max(tile_bits, 4)) each
    const double2* src;                // [lanes][2^n]
    double* partial;                   // [lanes][obs_grid_x][nsub][3][16][16]
};
int obs_ksplit(int nsub);                    // 4, 2, 1 for 1, 2, more subsets: nsub * ksplit <= kObsSubsetCap units of work, 4 per wave
unsigned obs_grid_x(int n, int tile_bits);   // blocks per lane: min(2^(n - tile_bits), kObsGridCap), whatever the number of lanes
hipError_t launch_obs_pass(const ObsArgs& a, hipStream_t s);
// rho[lane * lane_stride + subset * 256 + 16 a + b] <- the partials added in block order, exactly Hermitian
hipError_t launch_obs_final(const double* partial, unsigned nblocks, int nsub, int lanes, double2* rho, size_t lane_stride, hipStream_t s);

// aqc_mps_obs.hip (pair density matrices of MPS states; rules: aqc_mps_obs_rule.h)
struct MpsObsFusedArgs {
    int n;
    const double2* const* sites;   // [n] site tensors [2][dims[q]][dims[q+1]]
    const int* dims;               // [n + 1], every one <= kMpsObsFusedCap
    const size_t* env_off;         // [n + 1] element offset of L_q in env_l and of R_q in env_r
    double2* env_l;                // written by launch_mps_obs_env (L_0 and R_n by the host), read by launch_mps_obs_fused
    double2* env_r;
    const int* chain_start;        // [chains]
    const int* chain_last;
    const int* emit_of;            // [chains][n] emission index of (chain, site), -1: none
    double2* sums;                 // [emissions][3][4]
};
hipError_t launch_mps_obs_env(const MpsObsFusedArgs& a, hipStream_t s);                  // two workgroups: the left and the right sweep
hipError_t launch_mps_obs_fused(const MpsObsFusedArgs& a, int nchains, hipStream_t s);   // grid (3 components, chains)
// one workgroup per emission of a site: E of chain slot slots[e] ([slot][3][slot_stride], chi x chi each) against K [3][k_stride]
hipError_t launch_mps_obs_sums(const void* e_base, const int* slots, const int* emits, int count, size_t slot_stride, const void* k_base, size_t k_stride,
                               int chi, void* sums, hipStream_t s);

// aqc_mps_sample.hip (measurement of MPS states: shots and amplitudes; rules: aqc_mps_sample_rule.h)
struct MpsSampleState {            // one state of a fused launch: entry blockIdx.y of a device table
    const double2* const* sites;   // [n] site tensors [2][dims[q]][dims[q+1]]
    const int* dims;               // [n + 1], every one <= kMpsSampleFusedCap
    const size_t* env_off;         // [n + 1] element offset of R_q in env_r (shots only)
    const double2* env_r;
    unsigned char* bits;           // shots: [shots][n], written
    double2* amps;                 // [shots] psi(b) of every row
    unsigned char* status;         // shots: [shots], set to 1 where m_0 + m_1 is not finite or not positive (cleared by the host)
    double* norm2;                 // shots: [1] <psi|psi> = m_0 + m_1 of site 0
    unsigned long long lane;       // the position of the state in the call: part of the Philox counter
};
struct MpsSampleArgs {
    int n;
    long long shots;               // rows of the call
    unsigned long long first_shot, seed;
    const MpsSampleState* states;
    const unsigned char* bits_in;  // amplitudes: [shots][n], shared by the states
};
hipError_t launch_mps_sample_fused(const MpsSampleArgs& a, int nstates, bool amplitudes, hipStream_t s);   // grid (ceil(shots / 64), states)
struct MpsSampleRowArgs {          // gemm route, site q of a chunk of `rows` shots that begins at shot `shot0` of the call
    int q, n, chi;                 // chi = dims[q + 1]
    long long rows, shot0;
    unsigned long long first_shot, seed, lane;
    const double2 *w0, *w1, *g0, *g1;   // [rows][chi]; g: shots only
    double2* v;                    // [rows][chi] <- the chosen w
    const unsigned char* bits_in;  // amplitudes: [shots of the call][n]
    unsigned char* bits;           // the remaining fields as in MpsSampleState, for all shots of the call
    double2* amps;
    unsigned char* status;
    double* norm2;
};
hipError_t launch_mps_sample_rows(const MpsSampleRowArgs& a, bool amplitudes, hipStream_t s);
hipError_t launch_mps_sample_ones(void* v, long long rows, hipStream_t s);   // v[0 .. rows) = 1

// aqc_mps_pauli.hip (Pauli strings between MPS states; rules: aqc_mps_pauli_rule.h)
struct MpsPauliState {             // one state of a fused launch
    const double2* const* sites;   // [n] site tensors [2][dims[q]][dims[q+1]]
    const int* dims;               // [n + 1], every one <= kMpsPauliFusedCap
    const size_t* env_off;         // [n + 1] element offset of L_q in env_l and of R_q in env_r (expectation mode)
    const double2* env_l;
    const double2* env_r;
};
struct MpsPauliFusedArgs {
    int n, nstrings, expectation;
    const MpsPauliState* kets;     // [pairs]
    const MpsPauliState* bras;     // [pairs]; expectation mode: unused
    const unsigned char* strings;  // [nstrings][n]
    const int* first;              // [nstrings] the support of each string (expectation mode)
    const int* last;
    double2* const* out;           // [pairs] -> [nstrings]
};
hipError_t launch_mps_pauli_fused(const MpsPauliFusedArgs& a, int npairs, hipStream_t s);   // grid (strings, pairs)
// the three dressed copies D[c] = conj(ph(c)) B[c ^ f] of every site of a bra: out [3 (X, Y, Z)][total], site q at site_off[q]
hipError_t launch_mps_pauli_dress(const double2* const* sites, const int* dims, const size_t* site_off, int n, size_t total, int max_site_elems,
                                  void* out, hipStream_t s);
// out[idx[k]] = sum_uv M_k[u][v] R_k[v][u] over chi x chi, one workgroup per job k (m_tab, r_tab: `count` device pointers each)
hipError_t launch_mps_pauli_close(const void* const* m_tab, const void* const* r_tab, const int* idx, int count, int chi, void* out, hipStream_t s);

// aqc_mps_melem.hip (matrix elements of operators between MPS states; rules: aqc_mps_melem_rule.h)
struct MpsMelemEntry;
struct MpsMelemOp {                // one operator of a call (the identity is one of them), its sites as the lists of the rule header
    const int* dims;               // [n + 1]
    const int* ent_off;            // [n + 1] the entries of site q: ent[ent_off[q] .. ent_off[q + 1]), in the order a, s', b, s
    const MpsMelemEntry* ent;
    const int* slot_off;           // site q: 2 D_{q+1} + 1 offsets into ent_by_slot from slot_off[2 mask_off[q] + q] on (slot 2 b + s)
    const MpsMelemEntry* ent_by_slot;   // the same entries, those of a slot together, in the order of the list
    const int* mask_off;           // [n + 1] the masks of site q: mask[mask_off[q] + b], bit s: G_{b,s} exists
    const int* mask;
};
struct MpsMelemJob {
    const double2* const* bra_sites;   // [n] site tensors [2][dims[q]][dims[q+1]]
    const int* bra_dims;               // [n + 1]
    const double2* const* ket_sites;
    const int* ket_dims;
    const MpsMelemOp* op;
    int out;                           // index of the job's value in the call's output
};
struct MpsMelemFusedArgs {
    int n;
    const MpsMelemJob* jobs;       // [grid]
    double2* scratch;              // [grid][job_elems]: E | E' | G, the E sets e_elems each
    size_t e_elems, job_elems;
    double2* out;
};
hipError_t launch_mps_melem_fused(const MpsMelemFusedArgs& a, int njobs, hipStream_t s);   // grid (jobs)
// gemm route, one site of a group of jobs that share bonds and operator: G_{b,s} = its entries' w F_{a,s'} in the order of the list
// (F, G: slots 2 a + s' / 2 b + s of x * v elements at f, g + job * stride); E'[b] = 0 (u * v elements at e_next + job * stride) for
// every b without a G
hipError_t launch_mps_melem_combine(const MpsMelemOp* op, int q, const double2* f, double2* g, double2* e_next, size_t stride, int x, int u, int v,
                                    int slots, int njobs, hipStream_t s);

// aqc_mps_ent.hip (Schmidt spectra of MPS states, fused route; rules: aqc_mps_ent_rule.h)
struct MpsEntState {               // one distinct state of a call
    const double2* const* sites;   // [n] site tensors [2][dims[q]][dims[q+1]]
    const int* dims;               // [n + 1], every one <= kMpsEntFusedCap
    const size_t* fac_off;         // [n + 1] element offset of the factor of bond q = 1 .. n - 1 in a block, entry n: the size of a block
    double2* factors;              // the block of C_1 .. C_{n-1}, then the block of D_1 .. D_{n-1}
};
struct MpsEntChainArgs {
    int n;
    const MpsEntState* states;     // [states]
    int walk0;                     // the walk of block x = 0: 0 left (then x = 1 walks right), 1 right
};
hipError_t launch_mps_ent_chain(const MpsEntChainArgs& a, int nstates, hipStream_t s);   // grid (2 walks, states)
hipError_t launch_mps_ent_chain_right(const MpsEntChainArgs& a, int nstates, hipStream_t s);   // grid (1, states): D_{n-1} .. D_1 only
struct MpsEntCutArgs {
    int n, k, first;               // k: leading dimension of a matrix of the SVD batch; first: the chunk's first entry of state / cut
    const int* state;              // per matrix of the call: index into states ...
    const int* cut;                // ... and the cut q = 1 .. n - 1
    const MpsEntState* states;
    double2* a;                    // [count][k][k] <- S_q = C_q D_q^T in the leading chi_q x chi_q
    int* rows;                     // [count] <- chi_q
    int* cols;
};
hipError_t launch_mps_ent_cut(const MpsEntCutArgs& a, int count, hipStream_t s);         // grid (matrices of the chunk)

// aqc_mps_compress.hip (MPS compression, fused route; rules: aqc_mps_compress_rule.h)
struct MpsCompressState {          // one distinct state of a call
    MpsEntState in;                // the input and its right factors (the D block of in.factors)
    const size_t* site_off;        // [n] element offset of the new site q in out_sites (sized by the input's bonds, packed at the new ranks)
    const size_t* lam_off;         // [n - 1] offset of the new bond vector q in out_lam
    double2* out_sites;
    double* out_lam;
    int* ranks;                    // [n - 1] <- r_{q+1}, zero from a failed cut on
    double* dropped;               // [n - 1] <- total - kept of the cut
    int* sweeps;                   // [n - 1] <- sweeps of the cut's SVD
    int* status;                   // [1] <- kMpsCompress*: set once, by the state's own workgroup, at the cut that fails
};
struct MpsCompressArgs {
    int n, q, k, first;            // the step; k: columns of a matrix of the SVD batch (2 k rows); first: the chunk's first state
    const MpsCompressState* states;
    double2* carry;                // [chunk][kCap * kCap]      W_q, r_q x chi_q packed
    double2* m;                    // [chunk][2 * kCap * kCap]  M, 2 r_q x chi_{q+1} packed
    double2* a;                    // [chunk][2 k][k]           B
    int* rows;                     // [chunk] <- 2 r_q (0: the state has failed, its SVD is skipped)
    int* cols;                     // [chunk] <- chi_{q+1}
    const double2* u;              // [chunk][2 k][k]
    const double* s;               // [chunk][k]
    const int* svd_sweeps;
    const int* svd_status;
    double trunc_thr;
    int max_bond;
};
hipError_t launch_mps_compress_form(const MpsCompressArgs& a, int count, hipStream_t s);    // grid (states of the chunk); q = n - 1: the last site
hipError_t launch_mps_compress_split(const MpsCompressArgs& a, int count, hipStream_t s);

// aqc_mps_fromvec.hip (dense vectors into MPS states, fused route; rules: aqc_mps_fromvec_rule.h).  A lane is one vector; the lanes of a
// chunk share two ping-pong work buffers of 2^n complex numbers per lane; the bond dimensions live on the device.  Every store of a
// lane of the call is at (first + lane of the chunk) x the per-lane size; the stores of a chunk at the lane of the chunk.
struct MpsFromVecArgs {
    int n, q, first, kc;           // qubits; the site; the chunk's first lane; the side of a matrix of the SVD batch (2 x the largest bound)
    size_t lane_elems, nr;         // 2^n; N_r = 2^(n-1-q), the rows of A_q
    const double2* src;            // [chunk][2^n] A_q of every lane, [N_r][2 r_q] row-major
    double2* dst;                  // [chunk][2^n] <- A_{q+1} = Y, [N_r][r_{q+1}] row-major
    int* bonds;                    // [lanes][n + 1] r_0 = 1, r_{q+1} <- the split of site q, zero from a failed site on
    int* status;                   // [lanes] kMpsCompress*, set once by the lane's own workgroup
    int* failed_at;                // [lanes] the site (-1: none)
    int* sweeps;                   // [lanes][n - 1]
    double* dropped;               // [lanes][n - 1] total - kept of every cut
    double2* sites;                // [lanes][site_total] the new site q at site_off[q], packed at the ranks decided
    double* lam;                   // [lanes][lam_total] the new bond vector q at lam_off[q]
    const size_t* site_off;        // [n + 1], sized by the bounds of the bonds
    const size_t* lam_off;         // [n]
    // partial factors: level 0 reads A_q in blocks of 64 rows, level > 0 the factors of the level before, one factor a block
    int level, blocks_per_part, max_parts, last;   // last: the level that leaves one factor per lane
    size_t in_blocks;              // blocks of the level's input (level > 0: the factors of the level before)
    const double2* fac_in;         // [chunk][max_parts][64 x 64] factor p of a lane packed at p c^2, c = 2 r_q
    double2* fac_out;
    double2* a;                    // [chunk][kc][kc] <- R^T in the leading 2 r_q x min(2 r_q, N_r) (the last level)
    int* rows;                     // [chunk] <- 2 r_q (0: the lane has failed, its SVD is skipped)
    int* cols;                     // [chunk] <- min(2 r_q, N_r)
    const double2* u;              // [chunk][kc][kc]
    const double* s;               // [chunk][kc]
    const int* svd_sweeps;
    const int* svd_status;
    double2* w;                    // [chunk][64 x 32] W = rescale conj(U[:, :r]), 2 r_q x r_{q+1} packed
    double trunc_thr;
    int max_bond;
};
hipError_t launch_mps_fromvec_qr(const MpsFromVecArgs& a, int parts, int count, hipStream_t s);       // grid (parts, lanes of the chunk)
hipError_t launch_mps_fromvec_split(const MpsFromVecArgs& a, int count, hipStream_t s);                // grid (lanes of the chunk)
hipError_t launch_mps_fromvec_project(const MpsFromVecArgs& a, int count, hipStream_t s);              // grid (row groups, lanes of the chunk)
hipError_t launch_mps_fromvec_last(const MpsFromVecArgs& a, int count, hipStream_t s);                 // grid (lanes of the chunk); q = n - 1

// aqc_mps_tovec.hip (MPS states into dense vectors and blocks of amplitudes, fused route; rules: aqc_mps_tovec_rule.h).  A lane is one
// distinct state; lane z of a launch is state first + z of the call's table, whose record holds sites [n] | bufs [5]: low store 0, 1,
// high store 0, 1, output | dims [n + 1] and the route.  A state of another route is skipped by every workgroup.
struct MpsToVecArgs {
    const unsigned long long* table;   // a record of `per` words per state
    int per, at_sites, at_bufs, at_dims;
    int first;                     // the chunk's first state
    int n, k;                      // qubits; the low sites 0 .. k - 1
    int low_len, high_len;         // sites of each half that the grow steps walk (blocks: high_len = 0, the rows are walked instead)
    int step;                      // grow step: the factors of 2^step rows become those of 2^(step+1)
    int low_store, high_store;     // outer product: which store of each half holds L and H
    long long high_rows;           // rows of H: 2^(n-k), or the listed rows of a block call
    const unsigned char* high_bits;   // blocks: [high_rows][n - k], entry i the bit of site k + i
};
hipError_t launch_mps_tovec_head(const MpsToVecArgs& a, int count, hipStream_t s);    // grid (halves, lanes): the first steps of each half
hipError_t launch_mps_tovec_step(const MpsToVecArgs& a, int count, hipStream_t s);    // grid (tiles of 64 rows, halves, lanes)
hipError_t launch_mps_tovec_rows(const MpsToVecArgs& a, int count, hipStream_t s);    // grid (tiles of 64 listed rows, lanes)
hipError_t launch_mps_tovec_outer(const MpsToVecArgs& a, int count, hipStream_t s);   // grid (column groups, row tiles, lanes)

// aqc_mps_combine.hip (linear combinations of MPS states: the direct sum of an output's terms; rules: aqc_mps_combine_rule.h).  The terms
// are read through the table of the call's distinct states, whose record holds sites [n] | dims [n + 1]; every output writes its own
// stretch of one flat store.
struct MpsCombineOutput {          // one output of a call
    const int* term_state;         // [nterms] the record of each term's state in the table
    const double2* coeffs;         // [nterms]
    const int* block_off;          // [nterms + 1][n + 1] mps_combine_block_offsets
    const size_t* site_off;        // [n + 1] element offset of assembled site q in `sites`; entry n: the elements of the output
    double2* sites;                // <- S_0 .. S_{n-1}, every element written once
    int nterms;
};
struct MpsCombineArgs {
    const unsigned long long* table;   // a record of `per` words per distinct state
    int per, at_sites, at_dims;
    int nstates;                   // records of the table
    int n, first;                  // qubits; the launch's first output
    const MpsCombineOutput* outputs;
};
hipError_t launch_mps_combine_assemble(const MpsCombineArgs& a, int count, size_t largest_site, hipStream_t s);   // grid (tiles, sites, outputs)

// aqc_mps_opsum.hip (operator sums on MPS states: the direct sum of an output's terms c_t O_t psi_t; rules: aqc_mps_opsum_rule.h).  The
// states are read through the table of the call's distinct states as above, the operators through one packed buffer of 8-byte words:
// site offsets [nops][n + 1] (elements of the data) | dims [nops][n + 1] (ints) | the data (complex elements, 16-byte aligned).
struct MpsOpsumOutput {            // one output of a call
    const int* term_state;         // [nterms] the record of each term's state in the table
    const int* term_op;            // [nterms] the term's operator in the packed buffer, -1: none
    const double2* coeffs;         // [nterms]
    const int* block_off;          // [nterms + 1][n + 1] mps_combine_block_offsets of the product bonds
    const int* chi;                // [nterms][n + 1] the bonds of each term's state
    const size_t* site_off;        // [n + 1] element offset of assembled site q in `sites`; entry n: the elements of the output
    double2* sites;                // <- S_0 .. S_{n-1}, every element written once
    int nterms;
};
struct MpsOpsumArgs {
    const unsigned long long* table;   // a record of `per` words per distinct state
    int per, at_sites, at_dims;
    int nstates;                   // records of the table
    int n, first;                  // qubits; the launch's first output
    const unsigned long long* ops;     // the packed operators
    int nops;
    size_t at_op_dims, at_op_data;     // word offsets of the dims and of the data
    size_t op_elems;               // complex elements of the data
    const MpsOpsumOutput* outputs;
};
hipError_t launch_mps_opsum_assemble(const MpsOpsumArgs& a, int count, size_t largest_site, hipStream_t s);   // grid (tiles, sites, outputs)

// aqc_mps_layers.hip (gate layers on MPS states, fused route; rules: aqc_mps_layers_rule.h).  A unit is one evolved state: its working
// copy lives in the call's flat stores, every unit at the same offsets (sized by the call's bounds), the bond dimensions on the device.
// Matrix i of a layer is (unit i / gates, gate i % gates); a chunk takes the matrices [first, first + count).
struct MpsLayersArgs {
    int n, m;                      // qubits; the side of a matrix of the SVD batch (2 K, K the largest bound)
    int layer, gates, first;       // the layer, its number of gates, the chunk's first matrix
    int ngates;                    // folded gates of the whole program (stride of mats and sweeps)
    const int* gate_q;             // [gates] site of each gate of the layer
    const int* gate_id;            // [gates] its index in the program
    const double2* mats;           // [sets][ngates][16] the folded 4 x 4 matrices, row-major on 2 a + b
    const int* unit_set;           // [units] the set of matrices a unit takes
    const unsigned long long* table;   // the input states: per unit `per` words, site pointers at at_sites, bond vectors at at_lams, dims at at_dims
    size_t per, at_sites, at_lams, at_dims;
    const size_t* site_off;        // [n + 1] element offset of site q in a unit's block of `sites`
    const size_t* lam_off;         // [n] offset of bond vector q in a unit's block of `lam`
    const int* bounds;             // [n + 1]
    size_t site_total, lam_total;
    double2* sites;                // [units][site_total] sites packed at the current dims
    double* lam;                   // [units][lam_total]
    int* dims;                     // [units][n + 1]
    double* dropped;               // [units][n - 1] total - kept, summed per bond layer by layer
    int* sweeps;                   // [units][ngates]
    int* failed;                   // [units] 1 + the layer that failed the unit (0: none): skipped in every later layer
    int* fail_code;                // [units][n - 1] kMpsLayers* of the gate on bond q that failed the state ...
    int* fail_layer;               // [units][n - 1] ... and its layer
    double2* a;                    // [chunk][m][m] theta
    int* rows;                     // [chunk] <- 2 chi_q (0: the unit has failed, its SVD is skipped)
    int* cols;                     // [chunk] <- 2 chi_{q+2}
    const double2* u;              // [chunk][m][m]
    const double* s;               // [chunk][m]
    const double2* vh;             // [chunk][m][m]
    const int* svd_sweeps;
    const int* svd_status;
    double trunc_thr;
    int max_bond;
};
hipError_t launch_mps_layer_load(const MpsLayersArgs& a, int units, hipStream_t s);    // grid (units, n)
hipError_t launch_mps_layer_form(const MpsLayersArgs& a, int count, hipStream_t s);    // grid (matrices of the chunk)
hipError_t launch_mps_layer_split(const MpsLayersArgs& a, int count, hipStream_t s);

// aqc_api.cpp: thread-local message behind aqc_last_error(); returns 1
int set_error(const std::string& msg);

// aqc_svd.hip (one-sided Jacobi SVD + the pieces of a truncated 2-qubit MPS gate)
hipError_t launch_svd_identity(void* V, int cols, hipStream_t s);
hipError_t launch_jacobi_round(void* W, int rows, void* V, int cols, const void* pairs, int npairs, double tol, const double* fro2, int* rotations,
                               hipStream_t s);
hipError_t launch_svd_fro2(const void* W, size_t n, double* out, hipStream_t s);   // out[0] = Frobenius norm squared (fixed-order sum)
hipError_t launch_svd_load(const void* a, int m, int n, int mode, void* work, hipStream_t s);
hipError_t launch_svd_assemble(const void* W, const void* V, const int* ord, const double* sigma, int m, int n, int k, int mode, void* u, void* vh,
                               double* s_sorted, hipStream_t s);
bool svd_fits_small(int rows, int cols);
hipError_t launch_jacobi_small(void* W, int rows, void* V, int cols, double tol, int max_sweeps, int* sweeps_out, double* sigma_out,
                               hipStream_t s);   // sigma_out (may be null): the column norms at the end
bool svd_fits_block(int rows, int cols);
int svd_block_size();
hipError_t launch_jacobi_block(void* W, int rows, void* V, int cols, const void* bpairs, int rounds, int per_round, double tol, int max_sweeps,
                               const double* fro2, int* rot, unsigned* bar, int* status, hipStream_t s, int debug = 0);   // debug: tuning builds
hipError_t launch_svd_norms(const void* W, int rows, int cols, double* sigma, hipStream_t s);
hipError_t launch_mps_theta(const void* theta0, const double* lam_left, int chil, int chir, const double* g16, int mode, void* work, hipStream_t s);
// aqc_svd_batch.hip: block Jacobi on the matrix cores, a workgroup per matrix.  The device-pointer core behind aqc_svd_batch: a [count][m][n],
// u [count][m][k], s [count][k], vh [count][k][n] (zeroed here, then the leading parts written), d_rows / d_cols / d_sweeps may be null;
// work and vmat hold svd_batch_work_elems and svd_batch_v_elems complex numbers.  Enqueues on s; synchronises nothing.
size_t svd_batch_work_elems(int count, int m, int n);
size_t svd_batch_v_elems(int count, int m, int n);
hipError_t launch_svd_batch(int count, int m, int n, const int* d_rows, const int* d_cols, const void* d_a, void* d_u, double* d_s, void* d_vh,
                            int* d_sweeps, int* d_status, void* work, void* vmat, hipStream_t s);
// ---- device-resident lanes (aqc_mps_batch.cpp): L MPS in flat storage whose bond dimensions live on the device.  A launch takes only
// lane-independent arguments (site, gate kind, parameter indices); a lane's workgroup reads its own bond dimensions and thetas, so the
// host never waits for a rank decision and the whole walk of an evaluation is one uninterrupted sequence of launches.
constexpr int kLaneCap = 32;                        // largest bond dimension of a lane
constexpr int kLaneSite = 2 * kLaneCap * kLaneCap;  // complex elements reserved per site tensor
constexpr int kLaneEnv = kLaneCap * kLaneCap;       // ... per environment
constexpr int kLaneNoConv = 1, kLaneOverflow = 2, kLaneZero = 4, kLaneLdsShort = 8;   // status bits of a lane
struct LaneMps { void* T; double* lam; int* dims; double* discarded; int n, pad; };   // T[L][n][kLaneSite], lam[L][max(n-1,1)][kLaneCap], dims[L][n+1]
// (gate notation LaneRot / LaneGate1 / LaneGate2 / LaneOp1 / LaneOp2: aqc_mps_walk.h)
// One gate (`one`), or -- ops != null -- `nops` gates on pairwise disjoint sites from a table in device memory, all in one launch (gates of
// one layer of the circuit touch disjoint tensors and bond dimensions: any order, and so also "at once", gives the same bits).
// b / m2 (may be null): a second state that takes the same gates.
hipError_t launch_lanes_gate1(const LaneMps& a, const LaneMps* b, const LaneOp1* ops, int nops, const LaneOp1& one, const double* thetas, int T, int lanes,
                              int bond_hint, hipStream_t s);
// jstats (may be null): [0] += fp64 flops of the Jacobi rotations actually run (per column pair and sweep: 3 inner products and the
// rotation of the pair over the rows of the work matrix, 36 flop a row, + the rotation of V, 20 flop a row), [1] += SVDs,
// [2] += sweeps, [3] += rotations
hipError_t launch_lanes_gate2(const LaneMps& m, const LaneMps* m2, const LaneOp2* ops, int nops, const LaneOp2& one, const double* thetas, int T,
                              double trunc_thr, int max_bond, int* status, int* peak, int lanes, int bond_hint, hipStream_t s,
                              unsigned long long* jstats = nullptr);
hipError_t launch_lanes_env_left(const LaneMps& w, const LaneMps& z, int p, const void* in, size_t in_stride, void* out, size_t out_stride,
                                 const double* gh8, int lanes, hipStream_t s);
hipError_t launch_lanes_env_right(const LaneMps& w, const LaneMps& z, int p, const void* in, size_t in_stride, void* out, size_t out_stride, int lanes,
                                  hipStream_t s);
hipError_t launch_lanes_env_dot(const LaneMps& w, const LaneMps& z, int hi, const void* e, size_t e_stride, const void* rc, size_t rc_stride, void* vals,
                                int nvals, int slot, int lanes, hipStream_t s);
// up to three parameters on the SAME site: per parameter k the rotation g[k] on site q of both operands, then vals[lane][slot + k] = <P_k w|z>
// (gh[k] = P_k^H, 2 x 2 row-major c128) from the environments L[q] and R[q]
struct LaneSteps { LaneGate1 g[3]; double gh[3][8]; int count, pad; };
hipError_t launch_lanes_grad_step(const LaneMps& w, const LaneMps& z, int q, const LaneSteps& steps, const double* thetas, int T, const void* env_l,
                                  size_t l_stride, const void* env_r, size_t r_stride, void* scratch, void* vals, int nvals, int slot, int lanes, hipStream_t s);
hipError_t launch_lanes_basis(const LaneMps& m, const unsigned char* bits /* [lanes][n] */, int lanes, hipStream_t s);   // product basis states
// vals[lane][slot0 + k] = <bank_k|vh_lane> for k < count and the first `lanes` lanes, one workgroup per (k, lane), the environments in LDS sized
// for bonds <= bond_hint (a lane beyond raises kLaneLdsShort in status[lane])
hipError_t launch_lanes_bank_dot(const LaneMps& bank, int count, const LaneMps& vh, int lanes, void* vals, int nvals, int slot0, int* status,
                                 int bond_hint, hipStream_t s);
hipError_t launch_lanes_env_init(void* env_l, size_t l_stride, void* env_r_last, size_t r_stride, int lanes, hipStream_t s);
// environment steps of <(ops) w|z> for small bonds, one launch per site (aqc_svd.hip); gh8: 2x2 (row-major, 4 c128) applied to z's site or null
bool mps_env_fits_small(int xa, int ua, int yb, int vb);
hipError_t launch_mps_env_left(const void* in, const void* A, const void* B, int xa, int ua, int yb, int vb, const double* gh8, void* out, hipStream_t s);
hipError_t launch_mps_env_right(const void* rc, const void* A, const void* B, int xa, int ua, int yb, int vb, void* out, hipStream_t s);
hipError_t launch_mps_theta_fused(const void* tq, const void* tq1, const double* lam_left, int chil, int chim, int chir, const double* g16, int mode,
                                  void* work, hipStream_t s);   // the same from the two site tensors (small bonds: no zgemm launches)
hipError_t launch_mps_split(const void* W, const void* V, const int* ord, const double* sigma, const double* lam_left, int chil, int chir,
                            int k, int mode, double rescale, void* tq, void* tq1, const double* lam_new, double* lam_dst, hipStream_t s);   // lam_new (device, may be null) -> lam_dst[0..k)
hipError_t launch_mps_colscale(void* t, const double* lam, size_t rows, int cols, int mul, hipStream_t s);

// aqc_sketch.hip (sketched AQC on the device: generators, tall-skinny QR, ADAM)
// CholeskyQR2 of `batch` (d x k) c128 matrices (row-major, leading dimension lda, lane_stride elements apart): a <- Q; k a power of
// two <= 64, k <= d.  scratch: the first pass's Q, laid out like a (overwritten); partial: [batch][sk_qr_slabs(d)][k][k] c128,
// rinv: [batch][k][k] c128, status: [batch] ints (lanes with a non-zero word are skipped; a pivot <= abs_floor or negligible against its
// column, or a first pass whose Q is not orthonormal to 1e-4, sets AQC_QR_RANK_DEFICIENT and leaves the lane of a untouched)
int sk_qr_slabs(int d);
hipError_t launch_sk_qr(void* a, void* scratch, size_t lane_stride, int lda, int d, int k, int batch, double abs_floor, void* partial, void* rinv, int* status,
                        hipStream_t s);
// x <- one-hot columns idx[lane][k], y <- u[:, idx]; u: [batch or 1][d][d] (u_stride 0: one target for all lanes)
hipError_t launch_sk_alt(void* x, void* y, size_t lane_stride, int pitch, int d, int k, const void* u, size_t u_stride, const int* idx, int batch,
                         hipStream_t s);
// the (d x k) draw of every lane by the rule of aqc_philox.h: uniform + i uniform, or (normal != 0) Box-Muller normals
hipError_t launch_sk_omega(void* out, size_t lane_stride, int pitch, int d, int k, unsigned long long seed, unsigned long long stream,
                           unsigned long long iteration, int normal, int batch, hipStream_t s);
hipError_t launch_sk_sub(void* a, const void* b, size_t lane_stride, int pitch, int d, int k, int batch, hipStream_t s);
// One evaluation's bookkeeping and (do_update) one ADAM step per lane.  fobj = 1 - Re trace / k goes to profile[lane][col]; a lane that
// has not finished (flag < 2) records the best value and its thetas; flag 0 -> the m / v / theta update of optimizer.py:178-189 with
// g = -Re grads / k, t and nit advance, and a step norm below tol turns the flag to 1 (converged: thetas stay); flag 1 -> 2 (the
// evaluation at the final point has been taken).
struct SkAdam {
    int B, T, k, profile_stride;
    double* thetas;            // [B][T], updated in place
    const double2* trace;      // [B]
    const double2* grads;      // [B][T]
    double *m, *v, *best_x;    // [B][T]
    double *best_f, *profile;  // [B], [B][profile_stride]
    const double* lr;          // [B]
    int *t, *nit, *flag;       // [B]
    double beta1, beta2, eps, tol;
};
hipError_t launch_sk_adam(const SkAdam& st, int col, int do_update, hipStream_t s);

}  // namespace aqc
