// C ABI (include/aqc_hip.h): Schmidt spectra of every cut of single-lane MPS states.  Rules: aqc_mps_ent_rule.h; kernels: aqc_mps_ent.hip,
// the cuts' SVDs by the device-pointer core of aqc_svd_batch.hip.  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <limits>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_ent_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsEntByRule == kMpsByRule && kMpsEntFused == kMpsFused, "resolve_route");
enum { kSites, kFacOff, kDims };      // the sections of a fused state's record in Call::table

// what the call adds to the view of one distinct state
struct StateWork {
    int route = 0, fused_index = -1;
    std::vector<size_t> fac_off;      // mps_ent_factor_offsets
    size_t fac_at = 0;                // element offset of this state's two blocks in Call::d_factors
    std::vector<double> values;       // canonical route: [cuts][kmax]
    bool finite = true;
};

struct Call {
    int n = 0, cuts = 0, kmax = 0;
    std::vector<MpsView> views;       // distinct, in order of first appearance
    std::vector<StateWork> states;    // one per view
    std::vector<int> lane_state;      // per lane: index into views / states
    // fused route
    std::vector<int> item_state, item_cut, item_lane;   // per matrix: fused index of its state, the cut, the lane it is written to
    std::vector<double> h_s;
    std::vector<int> h_sweeps, h_status;
    int k = 1;
    MpsTable table;                        // per fused state: site pointers | factor offsets | dims
    DevBuf<MpsEntState> d_states;
    DevBuf<double2> d_factors;
    DevBuf<double> d_s;                    // the spectra of every matrix of the call
    DevBuf<int> d_items, d_ints;           // state | cut of every matrix; sweeps | status of every matrix
    SvdChunk svd;                          // of k x k matrices, one per (state, cut) of a chunk; s, sweeps and status are the call's
};

int run_fused(Call& c, const std::vector<int>& fused, double* factors_out, const std::vector<size_t>& lane_factor_at, hipStream_t st) {
    const size_t n = (size_t)c.n;
    c.table = MpsTable({mps_table_words(n), mps_table_words(n + 1), mps_table_ints(n + 1)}, fused.size());
    size_t fac_total = 0;
    for (size_t i = 0; i < fused.size(); ++i) {
        StateWork& w = c.states[fused[i]];
        c.table.put(i, kSites, c.views[fused[i]].t, n);
        c.table.put(i, kFacOff, w.fac_off, n + 1);
        c.table.put(i, kDims, c.views[fused[i]].dims, n + 1);
        w.fac_at = fac_total;
        fac_total += 2 * w.fac_off[n];
    }
    if (c.table.upload() || c.d_factors.alloc(std::max<size_t>(fac_total, 1))) return 1;
    std::vector<MpsEntState> hs(fused.size());
    for (size_t i = 0; i < fused.size(); ++i) {
        hs[i].sites = c.table.at<const double2*>(i, kSites);
        hs[i].fac_off = c.table.at<size_t>(i, kFacOff);
        hs[i].dims = c.table.at<int>(i, kDims);
        hs[i].factors = c.d_factors + c.states[fused[i]].fac_at;
    }
    if (c.d_states.upload(hs)) return 1;
    for (size_t s0 = 0; s0 < fused.size(); s0 += kMaxGridY) {
        MpsEntChainArgs a{c.n, c.d_states + s0};
        HIP_OK(launch_mps_ent_chain(a, (int)std::min<size_t>(kMaxGridY, fused.size() - s0), st));
    }
    const size_t total = c.item_state.size();
    if (total) {
        const int K = c.k, chunk = mps_ent_chunk(K, total, kMpsCallBudget);
        std::vector<int> items(c.item_state);
        items.insert(items.end(), c.item_cut.begin(), c.item_cut.end());
        if (c.d_items.upload(items) || c.d_ints.alloc(2 * total) || c.d_s.alloc(total * K) || c.svd.alloc(chunk, K, K, false)) return 1;
        int* d_sweeps = c.d_ints;
        int* d_status = d_sweeps + total;
        for (size_t first = 0; first < total; first += chunk) {   // the chunks share the SVD's stores: one stream orders them
            const int count = (int)std::min<size_t>(chunk, total - first);
            MpsEntCutArgs a{c.n, K, (int)first, c.d_items, c.d_items + total, c.d_states, c.svd.a, c.svd.rows(), c.svd.cols()};
            HIP_OK(launch_mps_ent_cut(a, count, st));
            HIP_OK(c.svd.launch(count, c.d_s + first * K, d_sweeps + first, d_status + first, st));
        }
        c.h_s.resize(total * K);
        c.h_sweeps.resize(total);
        c.h_status.resize(total);
        HIP_OK(hipMemcpyAsync(c.h_s.data(), c.d_s, sizeof(double) * total * K, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(c.h_sweeps.data(), d_sweeps, sizeof(int) * total, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(c.h_status.data(), d_status, sizeof(int) * total, hipMemcpyDeviceToHost, st));
    }
    if (factors_out)
        for (size_t lane = 0; lane < c.lane_state.size(); ++lane) {
            const StateWork& w = c.states[c.lane_state[lane]];
            if (w.fac_off[n])
                HIP_OK(hipMemcpyAsync(factors_out + 2 * lane_factor_at[lane], c.d_factors + w.fac_at, sizeof(double2) * 2 * w.fac_off[n], hipMemcpyDeviceToHost, st));
        }
    return 0;
}

// canonical route: the identity sweeps of the engine on a clone; the bond vectors are the Schmidt values.  A state that is not finite
// gives NaN rows, as on the fused route
int run_canonical(Call& c, const MpsView& v, StateWork& w) {
    const int n = c.n;
    w.values.assign((size_t)c.cuts * c.kmax, 0.0);
    bool has_zero_site = false;
    aqc_mps* m = nullptr;
    if (canonical_clone(v, false, &w.finite, &has_zero_site, &m)) return 1;
    if (!w.finite) return 0;
    std::vector<int> dims(n + 1);
    int rc = aqc_mps_dims(m, dims.data());
    for (int q = 1; q < n && !rc; ++q) {
        const void* site = nullptr;
        const double* lam = nullptr;
        rc = mps_peek(m, q - 1, &site, &lam);
        const int count = std::min(dims[q], v.dims[q]);   // (the sweeps never grow a bond)
        if (!rc && hipMemcpy(w.values.data() + (size_t)(q - 1) * c.kmax, lam, sizeof(double) * count, hipMemcpyDeviceToHost) != hipSuccess)
            rc = failf("download of a bond vector failed");
    }
    (void)aqc_mps_destroy(m);
    return rc;
}

}  // namespace

extern "C" {

int aqc_mps_ent_route(int n, const int32_t* dims) {
    if (!dims || n < 1) return -1;
    for (int q = 0; q <= n; ++q)
        if (dims[q] < 1) return -1;
    return mps_ent_route(n, dims);
}

int aqc_mps_rank_rule(int count, const double* s, double trunc_thr, int max_bond, int32_t* rank, double* dropped) {
    if (!s || !rank || !dropped) return failf("null argument");
    if (count < 1) return failf("a spectrum has at least one value");
    if (!(trunc_thr >= 0.0)) return failf("trunc_thr must be non-negative");
    for (int j = 0; j + 1 < count; ++j)
        if (!(s[j] >= s[j + 1])) return failf("the spectrum must be descending: value %d", j + 1);
    int k = 0;
    if (!mps_rank_rule(count, s, trunc_thr, max_bond, &k, dropped)) return failf("zero or non-finite spectrum");
    *rank = k;
    return 0;
}

int aqc_mps_ent_schmidt(aqc_mps* const* states, int nstates, int method, int kmax, double* s, int32_t* sweeps, int32_t* status, double* factors) {
    if (!states || !s) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    if (!mps_ent_method_ok(method)) return failf("unknown method %d", method);
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    Call c;
    c.n = n;
    c.cuts = mps_ent_cuts(n);
    c.kmax = kmax;
    const int rows = std::max(c.cuts, 1);
    if ((size_t)nstates * (size_t)rows > (size_t)1 << 28) return failf("too many cuts in one call: %d states x %d cuts", nstates, c.cuts);
    HIP_OK(hipSetDevice(device));
    if (view_states(states, (size_t)nstates, n, c.views, c.lane_state)) return 1;
    c.states.resize(c.views.size());
    std::vector<size_t> lane_factor_at(nstates, 0);
    std::vector<int> fused;
    size_t factor_total = 0;
    int need = 1;
    for (int i = 0; i < nstates; ++i) {
        const int k = c.lane_state[i];
        StateWork& w = c.states[k];
        if (!w.route) {   // the state's first lane
            const MpsView& v = c.views[k];
            w.fac_off = mps_ent_factor_offsets(n, v.dims.data());
            if ((w.route = resolve_route(method, mps_ent_route(n, v.dims.data()), v.max_bond, kMpsEntFusedCap, "state", i)) < 0) return 1;
            if (factors && w.route != kMpsEntFused) return failf("the factors are those of the fused route; state %d takes the canonical one", i);
            need = std::max(need, v.max_bond);
            if (w.route == kMpsEntFused) {
                w.fused_index = (int)fused.size();
                fused.push_back(k);
                for (int q = 1; q < n; ++q) c.k = std::max(c.k, v.dims[q]);
            }
        }
        lane_factor_at[i] = factor_total;
        factor_total += 2 * w.fac_off[n];
    }
    if (kmax < need) return failf("kmax = %d is below the largest bond dimension %d", kmax, need);
    for (int i = 0; i < nstates; ++i) {
        const StateWork& w = c.states[c.lane_state[i]];
        if (w.route != kMpsEntFused) continue;
        for (int q = 1; q < n; ++q) {
            c.item_state.push_back(w.fused_index);
            c.item_cut.push_back(q);
            c.item_lane.push_back(i);
        }
    }
    const size_t out_count = (size_t)nstates * rows;
    std::fill(s, s + out_count * kmax, 0.0);
    if (sweeps) std::fill(sweeps, sweeps + out_count, 0);
    if (status) std::fill(status, status + out_count, (int32_t)kMpsEntConverged);
    if (!fused.empty()) {
        hipStream_t st = mps_stream(states[0]);
        if (finish_call(st, run_fused(c, fused, factors, lane_factor_at, st), "Schmidt values")) return 1;
        for (size_t item = 0; item < c.item_state.size(); ++item) {
            const int lane = c.item_lane[item], q = c.item_cut[item], chi = c.views[c.lane_state[lane]].dims[q];
            const size_t row = (size_t)lane * rows + (q - 1);
            const bool bad = c.h_status[item] == kMpsEntNonFinite;
            for (int k = 0; k < (bad ? kmax : chi); ++k) s[row * kmax + k] = bad ? std::numeric_limits<double>::quiet_NaN() : c.h_s[item * c.k + k];
            if (sweeps) sweeps[row] = c.h_sweeps[item];
            if (status) status[row] = c.h_status[item];
            else if (c.h_status[item] == kMpsEntSweepLimit) return failf("state %d, cut %d: the SVD reached its sweep limit", lane, q);
        }
    }
    for (size_t k = 0; k < c.states.size(); ++k) {
        if (c.states[k].route == kMpsEntFused || c.cuts == 0) continue;
        if (run_canonical(c, c.views[k], c.states[k])) return 1;
    }
    for (int i = 0; i < nstates; ++i) {
        const StateWork& w = c.states[c.lane_state[i]];
        if (w.route == kMpsEntFused || c.cuts == 0) continue;
        for (int q = 1; q < n; ++q) {
            const size_t row = (size_t)i * rows + (q - 1);
            for (int k = 0; k < kmax; ++k) s[row * kmax + k] = w.finite ? w.values[(size_t)(q - 1) * kmax + k] : std::numeric_limits<double>::quiet_NaN();
            if (status) status[row] = w.finite ? kMpsEntConverged : kMpsEntNonFinite;
        }
    }
    return 0;
}

}  // extern "C"
