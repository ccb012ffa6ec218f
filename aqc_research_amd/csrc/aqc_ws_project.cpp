// The dense stages of the sparse-lhs sweep on a VIRTUAL register (grad_of_dot_product, core_operations.py:823-1019, for the
// lhs states every surrogate objective sweeps from: objective_base.py:42-255).
//
// After its first stage (local address bits L0) the lhs state of a lane is  w = psi (x) |e>:  psi = the stage's gates applied to the
// basis index on L0 (one tile of W), e = the basis index on the other bits F.  Let T be the qubits the gates of the LATER stages
// touch, Cb = T n L0, Us = L0 \ T.  Those gates act on T alone, so for every sub-stage k of theirs
//     w_k[u, i_T] = sum_c M_k[i_T, c] psi[u, c],        M_k = U_k ... U_1 M_0,   M_0[i_T, c] = [i_T = (c on Cb, e on T n F)]
// and the 16 x 16 matrix the gradient walk needs,  R_k = sum z_k w_k^H  over everything but the sub-stage's register bits, is
//     R_k = sum_{rest of i_T, c} Y_k M_k^H,             Y_k = U_k ... U_1 Y_0,   Y_0[i_T, c] = sum_u conj(psi[u, c]) z_0[u, i_T]
// (z_0: z as it enters those stages = the checkpoint the mirrored V^H keeps in ZW).  M and Y are states of |T| + |Cb| virtual
// qubits -- T, plus one spectator per qubit of Cb -- and R_k is exactly what the sweep kernels form from a (w, z) pair: the later
// stages become an ordinary sweep of the gates' sub-circuit on that small register, after ONE pass over z (aqc_project.hip).
// At the headline (16 qubits, L0 = 0..11, T = 8..15) the register has 12 qubits: 1/16 of the elements, and the second stage of
// the sweep -- more than half of an evaluation on the sparse route -- becomes one memory-bound pass plus a tile per lane.
// Exact: the same sums in another order.  Two basis states per lane: one item (M, Y pair) per tile of the first stage they occupy.
#include "aqc_ws.h"

#include <algorithm>

using namespace aqc;

namespace aqc {

namespace {
int popc(uint64_t v) { return __builtin_popcountll(v); }
unsigned deposit_bits(unsigned v, const std::vector<int>& bits) {
    unsigned o = 0;
    for (size_t j = 0; j < bits.size(); ++j)
        if (v >> j & 1) o |= 1u << bits[j];
    return o;
}
}  // namespace

void proj_plan(aqc_ws* ws, int low_bits) {
    ProjRoute& pr = ws->proj;
    pr.ok = false;
    const Program& prog = ws->ctx->prog;
    const DevPlan& p = ws->sweep;
    if (!ws->sw.projected || !ws->sw.sparse_sweep || !ws->inv_mirrored || !p.v3 || ws->col_bits != 0 || ws->ncols != 1 ||
        p.plan.stages.size() < 2 || prog.n > 30 || !list_launches_allowed(ws))
        return;
    const int n = prog.n;
    uint64_t L0 = 0, T = 0;
    for (int b : p.plan.stages[0].bits) L0 |= 1ull << b;
    pr.rest.clear();
    for (size_t s = 1; s < p.plan.stages.size(); ++s)
        for (int gi : p.plan.stages[s].ops) {
            const GateGroup& g = prog.groups[gi];
            pr.rest.push_back(gi);
            T |= 1ull << g.q0;
            if (g.q1 >= 0) T |= 1ull << g.q1;
        }
    if (pr.rest.empty()) return;
    const uint64_t all = (1ull << n) - 1, F = all & ~L0, Cb = T & L0, Us = L0 & ~T;
    pr.t = popc(T); pr.cb = popc(Cb); pr.us = popc(Us);
    pr.nv = pr.t + pr.cb;
    // the pass over z reads runs of 16 elements (address bits 0..3 among the summed ones); the register must be worth it
    if ((Us & 15) != 15 || pr.t < 4 || pr.cb > 6 || pr.nv + 2 > n || pr.nv > 20) return;
    pr.nvp = std::max(pr.nv, 8);
    pr.kv = std::min(pr.nvp, p.k);
    pr.ntiles_v = 1 << (pr.nvp - pr.kv);
    pr.first_subs = p.h_stages[0].nsubs;
    std::vector<int> tbits, cbits, usbits;
    std::vector<int> vq(n, -1);
    for (int b = 0; b < n; ++b) {
        if (T >> b & 1) { vq[b] = (int)tbits.size(); tbits.push_back(b); }
        if (Cb >> b & 1) cbits.push_back(b);
        if (Us >> b & 1) usbits.push_back(b);
    }
    pr.vprog = prog;   // group indices, thetas and slots stay the real ones; only the qubits move
    for (int gi : pr.rest) {
        GateGroup& g = pr.vprog.groups[gi];
        g.q0 = vq[g.q0];
        if (g.q1 >= 0) g.q1 = vq[g.q1];
    }
    Plan best;
    for (int lb = std::max(low_bits, 2); lb >= 2; --lb) {
        Plan cand = make_plan(pr.vprog, 0, pr.kv, lb, false, &pr.rest, pr.nvp);
        if (best.stages.empty() || cand.stages.size() < best.stages.size()) best = cand;
    }
    // (a narrow sub-stage search: the virtual stages are a small share of an evaluation, planning them must not cost what planning the real ones does)
    lower_plan(pr.vprog, best, pr.vsw, 4, true, true, false, (int)ws->sw.projected_beam);
    if (!pr.vsw.v3 || !check_plan(pr.vprog, pr.vsw.plan, &pr.rest).empty()) return;
    lower_plan(pr.vprog, mirror_plan(pr.vsw.plan), pr.vinv, 4, false, true, true);
    if (!pr.vinv.v3 || pr.vinv.h_subs3.size() != pr.vsw.h_subs3.size()) return;
    for (DevPlan* q : {&pr.vsw, &pr.vinv})
        for (DevStage& ds : q->h_stages) {   // one more non-local bit: the item (first or second tile of the lane's lhs state)
            if (ds.nub >= 32) return;
            ds.ubits[ds.nub++] = pr.nvp;
            ds.ntiles *= 2;
        }
    pr.l0_mask = (unsigned)L0;
    pr.ff_mask = (unsigned)(F & ~T);
    pr.cb_mask = (unsigned)Cb;
    pr.tf_mask = (unsigned)(T & F);
    pr.h_tab.clear();
    for (unsigned i = 0; i < (1u << pr.t); ++i) pr.h_tab.push_back(deposit_bits(i, tbits));
    for (unsigned k = 0; k < (1u << pr.us); ++k) pr.h_tab.push_back(deposit_bits(k, usbits));
    for (unsigned c = 0; c < (1u << pr.cb); ++c) pr.h_tab.push_back(deposit_bits(c, cbits));
    for (unsigned c = 0; c < (1u << pr.cb); ++c) {   // the same as an index on the T bits
        const unsigned addr = deposit_bits(c, cbits);
        unsigned it = 0;
        for (size_t j = 0; j < tbits.size(); ++j)
            if (addr >> tbits[j] & 1) it |= 1u << j;
        pr.h_tab.push_back(it);
    }
    pr.ok = true;
    if (ws->sw.verbose)
        fprintf(stderr, "aqc_hip: projected route: the sweep's stages after the first run on %d virtual qubits (%d touched, %d shared with the first "
                "stage) instead of %d: %zu stage(s) of 2^%d tiles, %zu sub-stages\n", pr.nv, pr.t, pr.cb, n, pr.vsw.h_stages.size(), pr.kv,
                pr.vsw.h_subs3.size());
}

int proj_alloc(aqc_ws* ws) {
    ProjRoute& pr = ws->proj;
    if (!pr.ok) return 0;
    const size_t B = (size_t)ws->batch;
    if (upload_plan(pr.vsw) || upload_plan(pr.vinv)) return 1;
    const size_t nsubs = std::max<size_t>(pr.vsw.h_subs3.size(), 1);
    if (pr.vsw.d_umat.alloc(B * nsubs * 12 * 64) || pr.vinv.d_umat.alloc(B * nsubs * 12 * 64)) return 1;
    if (pr.vsw.d_rpart.alloc(B * nsubs * (2 * (size_t)pr.ntiles_v) * 256)) return 1;
    const size_t velems = B * (2ull << pr.nvp), vbytes = sizeof(double2) * velems;
    pr.vy_copies = pr.us > 8 && pr.us <= 10 && pr.cb <= 4 ? 1 << (pr.us - 8) : 1;
    if (pr.vm.alloc(velems) || pr.vy.alloc(velems * pr.vy_copies)) return 1;
    HIP_OK(hipMemsetAsync(pr.vm, 0, vbytes, ws->stream));   // (entries beyond 2^nv -- a register padded to 8 qubits -- stay zero for good)
    HIP_OK(hipMemsetAsync(pr.vy, 0, vbytes * pr.vy_copies, ws->stream));
    pr.cpart_shares = 0;
    const long want_wgs = ws->sw.projected_fused_wgs;
    if (pr.us <= 10 && pr.cb <= 4 && (long)B < want_wgs) {   // the fused pass of a small batch splits its walk over the touched bits (launch_project_fused)
        int shares = 1;
        const long cap = ws->sw.projected_fused_max_shares;   // (1: never split -- what large batches run; tests)
        while ((long)B * pr.vy_copies * shares < want_wgs && 2 * shares <= (1 << (pr.t - 4)) && 2 * shares <= cap) shares *= 2;
        if (shares > 1) {
            if (pr.cpart.alloc((size_t)shares * 2 * B * (16ull << pr.us))) return 1;
            pr.cpart_shares = shares;
        }
    }
    if (pr.vme.alloc(velems)) return 1;
    HIP_OK(hipMemsetAsync(pr.vme, 0, vbytes, ws->stream));
    if (pr.d_tab.upload(pr.h_tab) || pr.d_items.alloc(2 * B * pr.ntiles_v) || pr.d_count.alloc(1) || pr.d_lane_parts.alloc(B)) return 1;
    HIP_OK(hipMemsetAsync(pr.d_count, 0, sizeof(int), ws->stream));
    HIP_OK(hipMemsetAsync(pr.d_lane_parts, 0, sizeof(int) * B, ws->stream));
    return 0;
}

bool list_launches_allowed(const aqc_ws* ws) { return ws->sweep.k < 12 || ws->sw.apply_persist > 0; }   // (mirrored V^H: the sweep's tile size)
bool sweep_route_projected(const aqc_ws* ws, bool sparse) { return sparse && ws->proj.ok; }

static ProjArgs proj_args(aqc_ws* ws);
// the virtual lhs pattern and the item list of the virtual launches: rebuilt when the first-stage list changed (always inside a
// captured graph, whose replays follow a support the host does not see; always with several virtual stages, which work in place on vm)
static int ensure_pattern(aqc_ws* ws, const ProjArgs& a) {
    ProjRoute& pr = ws->proj;
    if (pr.vsw.h_stages.size() == 1 && built_for(ws, pr.init_key, ws->sw_items_key)) return 0;
    ProfScope ps(ws, AQC_K_MISC);
    HIP_OK(launch_project_init(a, ws->stream));
    record_key(ws, pr.init_key, ws->sw_items_key);
    return 0;
}

// what every launch of the route shares: the first-stage items, the bit masks, the virtual buffers' bookkeeping
static ProjArgs proj_args(aqc_ws* ws) {
    ProjRoute& pr = ws->proj;
    ProjArgs a;
    memset(&a, 0, sizeof a);
    a.lane_stride = ws->lane_elems;
    a.items = ws->d_sw_items;
    a.nitems = ws->d_sw_counts;
    a.lane_parts = ws->d_sw_lane_parts;
    const DevStage& s0 = ws->sweep.h_stages[0];
    a.nub0 = s0.nub;
    for (int i = 0; i < s0.nub; ++i) a.ubits0[i] = s0.ubits[i];
    a.ff_mask = pr.ff_mask; a.cb_mask = pr.cb_mask; a.tf_mask = pr.tf_mask;
    a.nvp = pr.nvp;
    a.off_t = pr.d_tab;
    a.off_cb = pr.d_tab + (1u << pr.t) + (1u << pr.us);
    a.it_of_c = a.off_cb + (1u << pr.cb);
    a.off_us = pr.d_tab + (1u << pr.t);
    a.us_bits = pr.us;
    a.t = pr.t; a.cb = pr.cb; a.ntiles_v = pr.ntiles_v;
    a.vm = pr.vm;
    a.vitems = pr.d_items; a.vcount = pr.d_count; a.vlane_parts = pr.d_lane_parts;
    a.batch = ws->batch;
    return a;
}

// The product of the route,  Y[i_T, c] = sum_u conj(psi[u, c]) y[u, i_T]  per first-stage item, into the virtual z:  Y = the full-size
// operand y, k = u, keep = i_T, S = psi in W
static ProjArgs y_product(aqc_ws* ws, ProjArgs a, const double2* y) {
    const ProjRoute& pr = ws->proj;
    a.y = y;
    a.s = ws->bufs[AQC_BUF_W];
    a.out = pr.vy;
    a.s_virtual = 0; a.out_virtual = 1;
    a.staged = 1;   // (proj_plan: address bits 0..3 are among the summed ones)
    a.keep_bits = pr.t; a.k_bits = pr.us;
    a.y_keep = ProjMap{a.off_t, 0};
    a.y_k = ProjMap{a.off_us, 0};
    a.s_k = ProjMap{a.off_us, 0};
    a.s_c = ProjMap{a.off_cb, 0};
    a.o_keep = ProjMap{nullptr, 0};
    a.o_c = ProjMap{nullptr, pr.t};
    return a;
}

// after the sweep's first stage (W holds psi on the listed tiles, ZW the checkpoint): the projection, then the virtual stages
int run_projected_stages(aqc_ws* ws) {
    ProjRoute& pr = ws->proj;
    if (!ws->proj_y0_ready) {   // (else run_vdag_projected of this call has left M_0 and Y_0, from the target, on the virtual register)
        const ProjArgs a = proj_args(ws);
        if (ensure_pattern(ws, a)) return 1;
        ProfScope ps(ws, AQC_K_PROJECT);
        HIP_OK(launch_project(y_product(ws, a, ws->bufs[AQC_BUF_ZW]), ws->stream));   // Y_0, from the checkpoint
    }
    for (size_t s = 0; s < pr.vsw.h_stages.size(); ++s) {
        const Stage3Args a = projected_sweep_stage(ws, s);
        ProfScope ps(ws, AQC_K_SWEEP_VIRTUAL);
        HIP_OK(launch_sweep3(pr.kv, ws->stream, a, ws->sw));
    }
    return 0;
}

// Stage s of a virtual plan (vsw, vinv) on the virtual register.  Its geometry: two items per lane (the tiles of the first stage that
// the lhs state occupies), each a register of nvp qubits in ntiles_v tiles, walked by the item list that project_init_kernel writes.
Stage3Args virtual_stage3_args(aqc_ws* ws, const DevPlan& v, size_t s) {
    const ProjRoute& pr = ws->proj;
    Stage3Args a = stage3_args(ws, v, s);
    a.lane_stride = 2ull << pr.nvp;
    a.ntiles = 2 * pr.ntiles_v;
    a.items = pr.d_items; a.nitems = pr.d_count; a.max_items = 2 * ws->batch * pr.ntiles_v;
    return a;
}
// stage s of the virtual sweep plan on (vm, vy); every item writes the partial-R slot its list entry names
Stage3Args projected_sweep_stage(aqc_ws* ws, size_t s) {
    const ProjRoute& pr = ws->proj;
    Stage3Args a = virtual_stage3_args(ws, pr.vsw, s);
    a.in0 = pr.vm; a.in1 = pr.vy; a.out0 = pr.vm; a.out1 = pr.vy;
    a.store_out = s + 1 < pr.vsw.h_stages.size() ? 3 : 0;
    stage3_sweep_fields(a, pr.vsw, a.ntiles, 0);
    return a;
}

// Objective by projection: its six tile launches are three pairs of independent launches over disjoint buffers (psi with M_end, V^H's
// last stage with Y_0 -- Y_0 alone where the sweep walks backwards, projected_backwalk --, the sweep's first stage with the virtual stage), and each pair runs as ONE launch (launch_apply3_pair /
// launch_sweep3_pair) when the virtual plan has a single stage of the real plans' tile size (unless switched off).  Where the virtual
// stage walks backwards too (projected_virtual_backwalk) the third pair dissolves: its virtual member has become the Y_0 launch, and
// the sweep's first stage -- the real walk back -- is launched alone.  psi with M_end stays a pair.
static bool plan_has_pairs(const aqc_ws* ws) {   // the plans allow them: one virtual stage of the real plans' tile size
    const ProjRoute& pr = ws->proj;
    return pr.ok && pr.vsw.h_stages.size() == 1 && pr.vinv.h_stages.size() == 1 && ws->sweep.k == pr.kv && ws->inv.k == pr.kv;
}
bool projected_pairs(const aqc_ws* ws) { return plan_has_pairs(ws) && ws->sw.projected_pairs && !ws->capturing; }

// Objective by projection: the sweep's first stage walks BACK from (psi, C) -- the states V^H's last stage on the lhs tiles would start
// from and the forward walk would end in -- over the mirrored plan's last stage: one walk instead of two, every R from the sub-stage's
// inputs (sweep_mfma_body<..., BACK>).  run_vdag_projected then does not launch V^H's last stage and the sweep writes the Z tile, so
// both ask here, and the gather follows the sweep.  Static per workspace: the plans mirror each other sub-stage by sub-stage, the tile
// size has the form (aqc_backwalk.h), the stage has a first and a last sub-stage, and the R of its first one may arrive in the "inputs"
// form that the gradient walk conjugates (the R-only sub-stage's mechanism and switch).
bool projected_backwalk(const aqc_ws* ws) {
    const DevPlan& p = ws->sweep;
    const DevPlan& iv = ws->inv;
    return ws->proj.ok && ws->inv_mirrored && p.v3 && iv.v3 && ws->sw.r_only_last && iv.k == p.k && backwalk_tile(p.k) &&
           iv.h_subs3.size() == p.h_subs3.size() && !iv.h_stages.empty() && p.h_stages[0].nsubs >= 2 &&
           iv.h_stages.back().nsubs == p.h_stages[0].nsubs && iv.h_stages.back().sub_begin + iv.h_stages.back().nsubs == (int)iv.h_subs3.size();
}

// AQC_PROJECTED_PAIRS=0 on a plan that has pairs splits every pair into the single launches it was made of, V^H's last stage on the
// lhs tiles among them (tests/test_hip_pairs.py pins their kinds): that launch writes the Z tile and the walk -- the same body, the
// same R -- stores nothing.  A plan without pairs has nothing to split, and neither has a captured graph of a workspace whose pairs
// are on: there the stage is not launched and the walk writes the tile.
bool backwalk_keeps_vdag_stage(const aqc_ws* ws) { return projected_backwalk(ws) && plan_has_pairs(ws) && ws->sw.projected_pairs == 0; }

// ... and the VIRTUAL register is walked once as well.  The launch that takes Y_end down to Y_0 through the mirrored virtual plan starts
// from the states the forward virtual stage would end in -- (w, z) = (M_end, Y_end), both in HBM by then (vme, vy) -- so it is that
// stage's backward walk: the same body forms every R of the virtual plan from its sub-stage's inputs on the way down and leaves Y_0 in
// place; its w ends as the 0/1 pattern M_0, which nobody reads.  No virtual stage is launched behind the real walk then.  Static per
// workspace: the real member walks back, the virtual plans have ONE stage each (the gradient walk conjugates one sub-stage per plan) of
// at least two sub-stages, they mirror each other sub-stage by sub-stage, and the virtual tile size has the form.
bool projected_virtual_backwalk(const aqc_ws* ws) {
    const DevPlan& v = ws->proj.vsw;
    const DevPlan& vi = ws->proj.vinv;
    return projected_backwalk(ws) && v.v3 && vi.v3 && v.h_stages.size() == 1 && vi.h_stages.size() == 1 && vi.k == v.k && v.k == ws->proj.kv && backwalk_tile(ws->proj.kv) &&
           vi.h_subs3.size() == v.h_subs3.size() && v.h_stages[0].nsubs >= 2 && vi.h_stages[0].nsubs == v.h_stages[0].nsubs &&
           vi.h_stages[0].sub_begin + vi.h_stages[0].nsubs == (int)vi.h_subs3.size();
}
// Single launches (AQC_PROJECTED_PAIRS=0 on a plan that has pairs), as for the real member: the plain Y_0 launch stays and writes Y_0,
// the walk is a launch of its own kind (K_SWEEP_VIRTUAL) in front of it -- the apply overwrites Y_end in place -- and stores nothing.
static bool virtual_backwalk_keeps_y0_launch(const aqc_ws* ws) { return projected_virtual_backwalk(ws) && backwalk_keeps_vdag_stage(ws); }

// The virtual stage walked back from (M_end, Y_end): the mirrored virtual plan's stage on (vme, vy), every R to the row of the forward
// sub-stage it mirrors in the virtual sweep plan's partial-R buffer (aqc_backwalk.h), z = Y_0 in place unless a plain launch writes it.
static Stage3Args virtual_backwalk_stage(aqc_ws* ws, bool store_y0) {
    const ProjRoute& pr = ws->proj;
    Stage3Args a = virtual_stage3_args(ws, pr.vinv, 0);
    a.in0 = pr.vme; a.in1 = pr.vy; a.out0 = nullptr; a.out1 = pr.vy;
    a.store_out = store_y0 ? 2 : 0;
    a.backwalk = 1;
    stage3_sweep_fields(a, pr.vinv, a.ntiles, 0);   // (the first sub-stage's operand offsets: the persistent 2^12 form reads them)
    a.rpart = pr.vsw.d_rpart;
    return a;
}

// the gradient entries of the virtual plan's gate groups: its walk rides in the launch of the real plan's (which stops after its first stage)
RgradSecond projected_rgrad_plan(aqc_ws* ws, bool walked_back) {
    ProjRoute& pr = ws->proj;
    DevPlan& v = pr.vsw;
    RgradSecond r;
    memset(&r, 0, sizeof r);
    r.subs = v.d_subs3; r.grps = v.d_grps; r.rpart = v.d_rpart; r.lane_parts = pr.d_lane_parts; r.umat = v.d_umat;
    r.nparts = 2 * pr.ntiles_v;
    r.nsubs_total = r.count = (int)v.h_subs3.size();
    // walked back: the R of the mirrored stage's first sub-stage -- the forward stage's last -- arrives in the "inputs" form (aqc_backwalk.h)
    r.conj_sub = walked_back ? backwalk_conj_sub(r.nsubs_total, pr.vinv.h_stages[0].sub_begin) : -1;
    return r;
}

// ---- the objective's V^H by projection ------------------------------------------------------------------------------------------
// One-call evaluations whose lhs state is ONE basis state per lane with coefficient 1, known to the host (aqc_ws_set_basis), and
// whose gather indices lie in the lane's first-stage tile or differ from the basis index only on the other bits (the flip states
// of the surrogate objectives): nothing of Z = V^H y is read outside the lhs tile, so the stages of V^H are not run at all.
//     C[tile e][u, c] = sum_{i_T} conj(M_end[i_T, c]) y[u, i_T]      M_end = (later stages' gates) M_0: the tile of (later stages)^H y
//     Y_end[i_T, c]   = sum_u conj(psi[u, c]) y[u, i_T]              psi = (first stage's gates)|e_L0>:  Y_0 = (later stages)^H Y_end
// -- two passes over y (the target is read twice, V^H's first stage read and wrote the whole state and ran 4 sub-stages over it) --,
// then V^H's last stage on the lhs tile alone (Z there), the sweep's first stage as ever, the virtual stages from (M_0, Y_0), and
// <g|V^H y> = sum_c Y_0[(c, g on T n F), c] for the gather indices outside the tile.
// Where projected_backwalk holds, V^H's last stage and the sweep's first stage are ONE launch: the sweep walks back from (psi, C), writes
// the Z tile on its way and enqueues the gather itself.  Where projected_virtual_backwalk holds as well, the launch Y_end -> Y_0 here is
// the virtual stage's walk back from (M_end, Y_end): it leaves the virtual plan's R, and the sweep launches no virtual stage.
bool vdag_route_projected(aqc_ws* ws, int x_buf) {
    ProjRoute& pr = ws->proj;
    if (!pr.ok || !ws->sw.projected_vdag || ws->capturing || (long long)ws->lane_elems * ws->batch < ws->sw.projected_vdag_min_elems) return false;
    const ListKey key = key_of(ws, x_buf, true);
    if (ws->projb_key == key) return ws->projb_ok;
    ws->projb_key = key;
    ws->projb_ok = false;
    const std::vector<long long>& el = ws->combo_last_elem[x_buf];
    const std::vector<double>& cf = ws->combo_last_coef[x_buf];
    const size_t B = (size_t)ws->batch;
    if (el.size() != 2 * B || cf.size() != 4 * B || (ws->gather_count > 0 && ws->h_gather.size() != (size_t)ws->gather_count)) return false;
    const unsigned fmask = ~pr.l0_mask & (unsigned)((1ull << ws->ctx->prog.n) - 1);
    for (size_t b = 0; b < B; ++b) {
        if (el[2 * b] < 0 || el[2 * b + 1] >= 0 || cf[4 * b] != 1.0 || cf[4 * b + 1] != 0.0) return false;
        const unsigned e = (unsigned)el[2 * b];
        for (long long gl : ws->h_gather) {
            const unsigned d = e ^ (unsigned)gl;
            if ((d & fmask) == 0) continue;                                // inside the lane's tile
            if ((d & pr.l0_mask) != 0 || (d & pr.ff_mask) != 0) return false;   // another psi, or another slice of y
        }
    }
    ws->projb_ok = true;
    return true;
}

// One member of a couple of independent launches: a list stage on the full-size register (real), or the stages of a virtual plan
// from src into dst (in place after the first).  enqueue_couple runs the members it is given -- both: as ONE launch
// (projected_pairs: the virtual plan has a single stage then, of the real stage's tile size k).
struct VirtualRun { const DevPlan& plan; const double2* src; double2* dst; };
static Stage3Args virtual_apply_stage(aqc_ws* ws, const VirtualRun& v, size_t s) {
    Stage3Args a = virtual_stage3_args(ws, v.plan, s);
    a.in0 = s == 0 ? v.src : v.dst;
    a.out0 = v.dst;
    return a;
}
static int enqueue_couple(aqc_ws* ws, int k, const Stage3Args* real, const VirtualRun* v) {
    if (real && v) {
        ProfScope ps(ws, AQC_K_APPLY_VIRTUAL);
        HIP_OK(launch_apply3_pair(k, ws->stream, *real, virtual_apply_stage(ws, *v, 0), ws->sw));
    } else if (real) {
        ProfScope ps(ws, AQC_K_APPLY_LIST);
        HIP_OK(launch_apply3(k, ws->stream, *real, ws->sw));
    } else {
        for (size_t s = 0; s < v->plan.h_stages.size(); ++s) {
            ProfScope ps(ws, AQC_K_APPLY_VIRTUAL);
            HIP_OK(launch_apply3(ws->proj.kv, ws->stream, virtual_apply_stage(ws, *v, s), ws->sw));
        }
    }
    return 0;
}

int run_vdag_projected(aqc_ws* ws, int x_buf) {   // for a route eval_route has decided (vdag_route_projected) and prepared
    ProjRoute& pr = ws->proj;
    const DevPlan& p = ws->sweep;
    const DevPlan& iv = ws->inv;
    if (ensure_umat(ws, ws->inv, kURoute)) return 1;   // V^H's last stage, the sweep's first, the virtual plans: nothing else is read
    if (!ws->d_sw_items || !ws->w_clean) return fail("objective by projection without the sparse route's preparation");
    if (ensure_sweep_items(ws, x_buf)) return 1;
    Stage3Args psi = stage3_args(ws, p, 0);   // the first stage's gates on the basis index, on the listed tiles: x -> W
    psi.in0 = ws->bufs[x_buf];
    psi.out0 = ws->bufs[AQC_BUF_W];
    stage3_first_list(ws, psi);
    Stage3Args last = stage3_args(ws, iv, iv.h_stages.size() - 1);   // V^H's last stage on the lhs tiles: ZW -> Z
    last.in0 = ws->bufs[AQC_BUF_ZW];
    last.out0 = ws->bufs[AQC_BUF_Z];
    stage3_first_list(ws, last);
    const VirtualRun mend{pr.vsw, pr.vm, pr.vme};   // M_end = (later stages' gates) M_0
    const VirtualRun y0{pr.vinv, pr.vy, pr.vy};     // Y_0 = (later stages)^H Y_end
    const ProjArgs a = proj_args(ws);
    const bool pairs = projected_pairs(ws);
    const bool back = projected_backwalk(ws);   // the sweep of this call takes C -> Z on the lhs tiles along its walk back from (psi, C)

    if (!pairs && enqueue_couple(ws, p.k, &psi, nullptr)) return 1;          // psi
    if (ensure_pattern(ws, a)) return 1;                                      // M_0
    if (enqueue_couple(ws, p.k, pairs ? &psi : nullptr, &mend)) return 1;     // M_end (pairs: with psi)
    if (ws->sw.projected_fused && pr.us <= 10 && pr.cb <= 4 && (pr.us <= 8 || pr.vy_copies == 1 << (pr.us - 8))) {   // both products from one fetch of the target
        ProjArgs q = a;
        q.part_stride = (size_t)ws->batch * (2ull << pr.nvp);
        q.cpart = pr.cpart; q.cpart_shares = pr.cpart_shares;
        q.y = ws->bufs[AQC_BUF_Y]; q.s = ws->bufs[AQC_BUF_W];
        ProfScope ps(ws, AQC_K_PROJECT);
        HIP_OK(launch_project_fused(q, pr.vme, ws->bufs[AQC_BUF_ZW], pr.vy, ws->stream, ws->sw.projected_fused_qb == 4 ? 4 : 2));
    } else {
        {   // Y_end = proj(y)
            ProfScope ps(ws, AQC_K_PROJECT);
            HIP_OK(launch_project(y_product(ws, a, ws->bufs[AQC_BUF_Y]), ws->stream));
        }
        ProjArgs q = a;   // the lhs tile of (later stages)^H y, into ZW
        q.y = ws->bufs[AQC_BUF_Y]; q.s = pr.vme; q.out = ws->bufs[AQC_BUF_ZW];
        q.s_virtual = 1; q.out_virtual = 0; q.staged = 0;
        q.keep_bits = pr.us; q.k_bits = pr.t;
        q.y_keep = ProjMap{a.off_us, 0}; q.y_k = ProjMap{a.off_t, 0};
        q.s_k = ProjMap{nullptr, 0}; q.s_c = ProjMap{nullptr, pr.t};
        q.o_keep = ProjMap{a.off_us, 0}; q.o_c = ProjMap{a.off_cb, 0};
        ProfScope ps(ws, AQC_K_PROJECT);
        HIP_OK(launch_project(q, ws->stream));
    }
    // Y_0.  projected_virtual_backwalk: the launch that leaves it is the virtual stage's walk back from (M_end, Y_end) -- still ONE launch
    // of the kind of the plain one, the same U^H products on Y_end, and the virtual plan's R on the way.  Single launches keep the
    // plain launch behind a walk that stores nothing (the apply overwrites Y_end in place, so the walk goes first).
    const bool vback = projected_virtual_backwalk(ws), keep_y0 = virtual_backwalk_keeps_y0_launch(ws);
    if (vback) {
        ProfScope ps(ws, keep_y0 ? AQC_K_SWEEP_VIRTUAL : AQC_K_APPLY_VIRTUAL);
        HIP_OK(launch_sweep3(pr.kv, ws->stream, virtual_backwalk_stage(ws, !keep_y0), ws->sw));
    }
    if ((!pairs || back) && (!vback || keep_y0) && enqueue_couple(ws, iv.k, nullptr, &y0)) return 1;
    if ((!back || backwalk_keeps_vdag_stage(ws)) && enqueue_couple(ws, iv.k, &last, pairs && !back ? &y0 : nullptr)) return 1;   // V^H's last stage (pairs: with Y_0)
    vdag_projected_state_after(ws, x_buf);
    return 0;
}

// the registered gather of a Z that run_vdag_projected (projected_backwalk: and the sweep behind it) has left: the indices inside the lhs tiles from Z, the others from the virtual z
int proj_fix_amplitudes(aqc_ws* ws, int x_buf) {
    ProjRoute& pr = ws->proj;
    if (results_guard(ws)) return 1;
    ProfScope ps(ws, AQC_K_MISC);
    ProjArgs a = proj_args(ws);
    HIP_OK(launch_project_amps(a, ws->d_index, ws->gather_count, ws->d_combo_prev[x_buf], ws->d_small, pr.vy, ws->bufs[AQC_BUF_Z], ws->stream));
    return 0;
}

}  // namespace aqc
