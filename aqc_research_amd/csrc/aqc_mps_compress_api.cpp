// C ABI (include/aqc_hip.h): compression of single-lane MPS states: canonical form and truncation of every bond, many states per call.
// Rules: aqc_mps_compress_rule.h; kernels: aqc_mps_compress.hip, the right factors by aqc_mps_ent.hip, the SVDs of a step by the
// device-pointer core of aqc_svd_batch.hip.  The skeleton of the call: aqc_mps_call.h; the sweep of both routes: aqc_mps_sweep.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "aqc_mps_compress_rule.h"
#include "aqc_mps_sweep.h"

using namespace aqc;

namespace {

std::atomic<size_t> g_svd_budget{kMpsCallBudget};   // aqc_mps_compress_svd_budget: tests lower it to run many chunks on few states

// what the call adds to the view of one distinct state
struct StateWork : SweepWork {
    int route = 0;
    aqc_mps* made = nullptr;   // canonical route: the compressed clone, handed to the state's first lane
};

struct Call {
    int n = 0, cuts = 0;
    std::vector<MpsView> views;       // distinct, in order of first appearance
    std::vector<StateWork> states;    // one per view
    std::vector<int> lane_state;      // per lane: index into views / states
    FusedSweep sweep;                 // of the states on the fused route (aqc_mps_sweep.h)
};

// a failed call: the outputs and the canonical route's clones that no lane has taken
void drop_outputs(Call& c, aqc_mps** out, int nstates) {
    drop_outputs(out, nstates);
    for (StateWork& w : c.states) {
        if (w.made) (void)aqc_mps_destroy(w.made);
        w.made = nullptr;
    }
}

}  // namespace

extern "C" {

int aqc_mps_compress_route(int n, const int32_t* dims) {
    if (!dims || n < 1) return -1;
    for (int q = 0; q <= n; ++q)
        if (dims[q] < 1) return -1;
    return mps_compress_route(n, dims);
}

int64_t aqc_mps_compress_svd_budget(int64_t bytes) {
    return swap_budget(g_svd_budget, bytes, kMpsCallBudget);
}

int aqc_mps_compress(aqc_mps* const* states, int nstates, double trunc_thr, int max_bond, int method, aqc_mps** out, int32_t* ranks,
                     double* dropped, int32_t* sweeps, int32_t* status) {
    if (check_truncating_call(states, out, nstates, trunc_thr, max_bond, "state", mps_ent_method_ok(method), method)) return 1;
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    Call c;
    c.n = c.sweep.n = n;
    c.cuts = c.sweep.cuts = n - 1;
    c.sweep.trunc_thr = trunc_thr;
    c.sweep.max_bond = max_bond;
    if ((size_t)nstates * (size_t)std::max(c.cuts, 1) > (size_t)1 << 28) return failf("too many cuts in one call: %d states x %d cuts", nstates, c.cuts);
    HIP_OK(hipSetDevice(device));
    if (n == 1) {   // nothing to cut: copies
        for (int i = 0; i < nstates; ++i) {
            if (aqc_mps_clone(states[i], &out[i])) { drop_outputs(c, out, nstates); return 1; }
            if (status) status[i] = kMpsCompressOk;
        }
        return 0;
    }
    if (view_states(states, (size_t)nstates, n, c.views, c.lane_state)) return 1;
    c.states.resize(c.views.size());
    std::vector<int> fused;
    for (int i = 0; i < nstates; ++i) {
        const int k = c.lane_state[i];
        StateWork& w = c.states[k];
        if (w.route) continue;   // (not the state's first lane)
        const MpsView& v = c.views[k];
        if ((w.route = resolve_route(method, mps_compress_route(n, v.dims.data()), v.max_bond, kMpsEntFusedCap, "state", i)) < 0) return 1;
        w.size(n, v.dims.data());
        if (w.route == kMpsEntFused) {
            fused.push_back(k);
            c.sweep.k = std::max(c.sweep.k, v.max_bond);
        }
    }
    if (!fused.empty()) {
        hipStream_t st = mps_stream(states[0]);
        std::vector<SweepInput> in;
        std::vector<SweepWork*> work;
        for (int k : fused) {
            in.push_back({c.views[k].t.data(), c.views[k].dims.data()});
            work.push_back(&c.states[k]);
        }
        if (finish_call(st, c.sweep.run(in, work, g_svd_budget.load(), st), "compression")) return 1;   // the one synchronisation of the sweep
        for (size_t i = 0; i < fused.size(); ++i) c.sweep.collect(i, c.states[fused[i]]);
    }
    for (size_t k = 0; k < c.states.size(); ++k)
        if (c.states[k].route != kMpsEntFused && sweep_canonical(c.views[k], trunc_thr, max_bond, c.states[k], &c.states[k].made)) { drop_outputs(c, out, nstates); return 1; }
    for (int i = 0; i < nstates; ++i) {
        StateWork& w = c.states[c.lane_state[i]];
        if (w.status == kMpsCompressOk) {
            int rc = 0;
            if (w.route == kMpsEntFused) rc = c.sweep.adopt(w, device, aqc_mps_discarded_weight(c.views[c.lane_state[i]].h), &out[i]);
            else if (w.made) { out[i] = w.made; w.made = nullptr; }
            else {   // a later listing of a canonical state: a copy of the lane that took the clone
                for (int j = 0; j < i && !out[i] && !rc; ++j)
                    if (c.lane_state[j] == c.lane_state[i]) rc = aqc_mps_clone(out[j], &out[i]);
            }
            if (rc || !out[i]) { drop_outputs(c, out, nstates); return rc ? 1 : failf("compression lost a state"); }
        }
        for (int q = 0; q < c.cuts; ++q) {
            const size_t at = (size_t)i * c.cuts + q;
            if (ranks) ranks[at] = w.ranks[q];
            if (dropped) dropped[at] = w.dropped[q];
            if (sweeps) sweeps[at] = w.sweeps[q];
        }
        if (status) status[i] = w.status;
    }
    return 0;
}

}  // extern "C"
