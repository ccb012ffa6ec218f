// C ABI (include/aqc_hip.h): compression of single-lane MPS states: canonical form and truncation of every bond, many states per call.
// Rules: aqc_mps_compress_rule.h; kernels: aqc_mps_compress.hip, the right factors by aqc_mps_ent.hip, the SVDs of a step by the
// device-pointer core of aqc_svd_batch.hip.  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_compress_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsEntByRule == kMpsByRule && kMpsEntFused == kMpsFused, "resolve_route");
std::atomic<size_t> g_svd_budget{kMpsCallBudget};   // aqc_mps_compress_svd_budget: tests lower it to run many chunks on few states
constexpr int kPlaneElems = kMpsEntFusedCap * kMpsEntFusedCap;
enum { kSites, kFacOff, kSiteOff, kLamOff, kDims };   // the sections of a fused state's record in Call::table

// what the call adds to the view of one distinct state
struct StateWork {
    int route = 0, status = kMpsCompressOk;
    std::vector<int> ranks, sweeps;
    std::vector<double> dropped;
    std::vector<size_t> fac_off, site_off, lam_off;
    size_t fac_at = 0, site_at = 0, lam_at = 0;   // element offsets of this state's blocks in the call's stores
    aqc_mps* made = nullptr;                      // canonical route: the compressed clone, handed to the state's first lane
};

struct Call {
    int n = 0, cuts = 0, k = 1;
    double trunc_thr = 0.0;
    int max_bond = 0;
    std::vector<MpsView> views;       // distinct, in order of first appearance
    std::vector<StateWork> states;    // one per view
    std::vector<int> lane_state;      // per lane: index into views / states
    MpsTable table;                        // per fused state: site pointers | factor offsets | site offsets | bond offsets | dims
    DevBuf<MpsEntState> d_in;
    DevBuf<MpsCompressState> d_states;
    DevBuf<double2> d_factors, d_sites, d_carry, d_m;
    DevBuf<double> d_lam, d_dropped;
    DevBuf<int> d_results;                 // per fused state: ranks | sweeps | status
    SvdChunk svd;                          // of 2 k x k matrices, one per state of a chunk
    std::vector<int> h_results;
    std::vector<double> h_dropped;
};

int run_fused(Call& c, const std::vector<int>& fused, hipStream_t st) {
    const size_t n = (size_t)c.n, cuts = (size_t)c.cuts, res = 2 * cuts + 1;
    c.table = MpsTable({mps_table_words(n), mps_table_words(n + 1), mps_table_words(n), mps_table_words(n), mps_table_ints(n + 1)}, fused.size());
    size_t fac_total = 0, site_total = 0, lam_total = 0;
    for (size_t i = 0; i < fused.size(); ++i) {
        StateWork& w = c.states[fused[i]];
        const MpsView& v = c.views[fused[i]];
        c.table.put(i, kSites, v.t, n);
        c.table.put(i, kFacOff, w.fac_off, n + 1);
        c.table.put(i, kSiteOff, w.site_off, n);
        c.table.put(i, kLamOff, w.lam_off, w.lam_off.size());
        c.table.put(i, kDims, v.dims, n + 1);
        w.fac_at = fac_total; w.site_at = site_total; w.lam_at = lam_total;
        fac_total += 2 * w.fac_off[n];
        site_total += w.site_off[n];
        for (size_t q = 1; q < n; ++q) lam_total += (size_t)v.dims[q];
    }
    const int K = c.k, chunk = mps_compress_chunk(K, fused.size(), g_svd_budget.load());
    if (c.table.upload() || c.d_factors.alloc(std::max<size_t>(fac_total, 1)) || c.d_sites.alloc(site_total) ||
        c.d_lam.alloc(std::max<size_t>(lam_total, 1)) || c.d_results.alloc(res * fused.size()) || c.d_dropped.alloc(cuts * fused.size()) ||
        c.d_carry.alloc((size_t)chunk * kPlaneElems) || c.d_m.alloc((size_t)chunk * 2 * kPlaneElems) || c.svd.alloc(chunk, 2 * K, K)) return 1;
    std::vector<MpsEntState> hin(fused.size());
    std::vector<MpsCompressState> hs(fused.size());
    for (size_t i = 0; i < fused.size(); ++i) {
        const StateWork& w = c.states[fused[i]];
        hin[i].sites = c.table.at<const double2*>(i, kSites);
        hin[i].fac_off = c.table.at<size_t>(i, kFacOff);
        hin[i].dims = c.table.at<int>(i, kDims);
        hin[i].factors = c.d_factors + w.fac_at;
        hs[i].in = hin[i];
        hs[i].site_off = c.table.at<size_t>(i, kSiteOff);
        hs[i].lam_off = c.table.at<size_t>(i, kLamOff);
        hs[i].out_sites = c.d_sites + w.site_at;
        hs[i].out_lam = c.d_lam + w.lam_at;
        hs[i].ranks = c.d_results + i * res;
        hs[i].sweeps = hs[i].ranks + cuts;
        hs[i].status = hs[i].sweeps + cuts;
        hs[i].dropped = c.d_dropped + i * cuts;
    }
    if (c.d_in.upload(hin) || c.d_states.upload(hs)) return 1;
    HIP_OK(hipMemsetAsync(c.d_results, 0, sizeof(int) * res * fused.size(), st));
    HIP_OK(hipMemsetAsync(c.d_dropped, 0, sizeof(double) * cuts * fused.size(), st));
    for (size_t s0 = 0; s0 < fused.size(); s0 += kMaxGridY) {
        MpsEntChainArgs a{c.n, c.d_in + s0, 1};
        HIP_OK(launch_mps_ent_chain_right(a, (int)std::min<size_t>(kMaxGridY, fused.size() - s0), st));
    }
    for (size_t first = 0; first < fused.size(); first += chunk) {   // the chunks share the step's stores: one stream orders them
        const int count = (int)std::min<size_t>(chunk, fused.size() - first);
        MpsCompressArgs a{c.n, 0, K, (int)first, c.d_states, c.d_carry, c.d_m, c.svd.a, c.svd.rows(), c.svd.cols(), c.svd.u, c.svd.s, c.svd.sweeps(), c.svd.status(), c.trunc_thr, c.max_bond};
        for (int q = 0; q + 1 < c.n; ++q) {
            a.q = q;
            HIP_OK(launch_mps_compress_form(a, count, st));
            HIP_OK(c.svd.launch(count, st));
            HIP_OK(launch_mps_compress_split(a, count, st));
        }
        a.q = c.n - 1;
        HIP_OK(launch_mps_compress_form(a, count, st));
    }
    c.h_results.resize(res * fused.size());
    c.h_dropped.resize(std::max<size_t>(cuts * fused.size(), 1));
    HIP_OK(hipMemcpyAsync(c.h_results.data(), c.d_results, sizeof(int) * res * fused.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.h_dropped.data(), c.d_dropped, sizeof(double) * cuts * fused.size(), hipMemcpyDeviceToHost, st));
    return 0;
}

// a fused state's lane: a new engine state from the tensors the sweep left on the device
int adopt_fused(const Call& c, const MpsView& v, const StateWork& w, int device, aqc_mps** out) {
    const int n = c.n;
    std::vector<int> dims(n + 1, 1);
    double discarded = aqc_mps_discarded_weight(v.h);
    for (int q = 1; q < n; ++q) { dims[q] = w.ranks[q - 1]; discarded += w.dropped[q - 1]; }
    return adopt_flat(device, n, dims.data(), c.d_sites + w.site_at, w.site_off.data(), c.d_lam + w.lam_at, w.lam_off.data(), discarded, out);
}

// canonical route: on a clone, the identity sweeps of the engine, then its truncating sweep left to right.  The engine reports an SVD at
// its sweep limit as an error of the gate, and so does this route: of the statuses it gives only 0 and 2.  A state that is not finite
// (or has a zero site) gets the status of the fused route
int run_canonical(const Call& c, const MpsView& v, StateWork& w) {
    const int n = c.n;
    bool finite = true, zero = false;
    aqc_mps* m = nullptr;
    if (canonical_clone(v, true, &finite, &zero, &m)) return 1;
    if (!m) { w.status = kMpsCompressNonFinite; return 0; }
    int rc = 0;
    for (int q = 0; q + 1 < n && !rc; ++q) {
        const double before = aqc_mps_discarded_weight(m);
        rc = aqc_mps_gate2(m, q, q + 1, kIdentityGate2, c.trunc_thr, c.max_bond);
        w.dropped[q] = aqc_mps_discarded_weight(m) - before;
    }
    std::vector<int> dims(n + 1);
    if (!rc) rc = aqc_mps_dims(m, dims.data());
    if (rc) { (void)aqc_mps_destroy(m); return 1; }
    for (int q = 1; q < n; ++q) w.ranks[q - 1] = dims[q];
    w.made = m;
    return 0;
}

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
    c.n = n;
    c.cuts = n - 1;
    c.trunc_thr = trunc_thr;
    c.max_bond = max_bond;
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
        w.fac_off = mps_ent_factor_offsets(n, v.dims.data());
        w.site_off = mps_site_offsets(n, v.dims.data());
        w.lam_off = mps_compress_lam_offsets(n, v.dims.data());
        w.ranks.assign(c.cuts, 0);
        w.sweeps.assign(c.cuts, 0);
        w.dropped.assign(c.cuts, 0.0);
        if (w.route == kMpsEntFused) {
            fused.push_back(k);
            c.k = std::max(c.k, v.max_bond);
        }
    }
    if (!fused.empty()) {
        hipStream_t st = mps_stream(states[0]);
        if (finish_call(st, run_fused(c, fused, st), "compression")) return 1;   // the one synchronisation of the sweep
        const size_t cuts = (size_t)c.cuts, res = 2 * cuts + 1;
        for (size_t i = 0; i < fused.size(); ++i) {
            StateWork& w = c.states[fused[i]];
            const int* r = c.h_results.data() + i * res;
            w.ranks.assign(r, r + cuts);
            w.sweeps.assign(r + cuts, r + 2 * cuts);
            w.status = r[2 * cuts];
            w.dropped.assign(c.h_dropped.begin() + i * cuts, c.h_dropped.begin() + (i + 1) * cuts);
        }
    }
    for (size_t k = 0; k < c.states.size(); ++k)
        if (c.states[k].route != kMpsEntFused && run_canonical(c, c.views[k], c.states[k])) { drop_outputs(c, out, nstates); return 1; }
    for (int i = 0; i < nstates; ++i) {
        StateWork& w = c.states[c.lane_state[i]];
        if (w.status == kMpsCompressOk) {
            int rc = 0;
            if (w.route == kMpsEntFused) rc = adopt_fused(c, c.views[c.lane_state[i]], w, device, &out[i]);
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
