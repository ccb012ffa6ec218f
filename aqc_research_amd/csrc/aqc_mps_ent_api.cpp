// C ABI (include/aqc_hip.h): Schmidt spectra of every cut of single-lane MPS states.  Rules: aqc_mps_ent_rule.h; kernels: aqc_mps_ent.hip,
// the cuts' SVDs by the device-pointer core of aqc_svd_batch.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "aqc_devbuf.h"
#include "aqc_mps_ent_rule.h"
#include "aqc_mps_host.h"

using namespace aqc;

namespace {

constexpr size_t kSvdBudget = (size_t)256 << 20;   // bytes the SVD's stores (a, u, vh, work, vmat) of a chunk may take
constexpr int kMaxGridY = 65535;

// one distinct state of the call
struct StateWork {
    aqc_mps* h = nullptr;
    int route = 0, fused_index = -1;
    std::vector<int> dims;
    std::vector<const double2*> t;
    std::vector<size_t> fac_off;      // mps_ent_factor_offsets
    size_t fac_at = 0;                // element offset of this state's two blocks in Call::d_factors
    std::vector<double> values;       // canonical route: [cuts][kmax]
    bool finite = true;
};

struct Call {
    int n = 0, cuts = 0, kmax = 0;
    std::vector<StateWork> states;    // distinct, in order of first appearance
    std::vector<int> lane_state;      // per lane: index into states
    // fused route
    std::vector<int> item_state, item_cut, item_lane;   // per matrix: fused index of its state, the cut, the lane it is written to
    std::vector<double> h_s;
    std::vector<int> h_sweeps, h_status;
    int k = 1;
    DevBuf<unsigned long long> d_tables;   // per fused state: site pointers | factor offsets | dims, 8-byte words
    DevBuf<MpsEntState> d_states;
    DevBuf<double2> d_factors, d_a, d_u, d_vh, d_work, d_vmat;
    DevBuf<double> d_s;
    DevBuf<int> d_items, d_ints;           // state | cut of every matrix; sweeps | status of every matrix, rows | cols of a chunk
};

int run_fused(Call& c, const std::vector<int>& fused, double* factors_out, const std::vector<size_t>& lane_factor_at, hipStream_t st) {
    static_assert(sizeof(unsigned long long) == sizeof(size_t) && sizeof(unsigned long long) == sizeof(const double2*), "8-byte words");
    const size_t n = (size_t)c.n, per = n + (n + 1) + (n + 2) / 2;
    std::vector<unsigned long long> words(per * fused.size(), 0);
    size_t fac_total = 0;
    for (size_t i = 0; i < fused.size(); ++i) {
        StateWork& w = c.states[fused[i]];
        unsigned long long* p = words.data() + i * per;
        memcpy(p, w.t.data(), n * 8);
        memcpy(p + n, w.fac_off.data(), (n + 1) * 8);
        memcpy(p + 2 * n + 1, w.dims.data(), (n + 1) * sizeof(int));
        w.fac_at = fac_total;
        fac_total += 2 * w.fac_off[n];
    }
    if (c.d_tables.upload(words) || c.d_factors.alloc(std::max<size_t>(fac_total, 1))) return 1;
    std::vector<MpsEntState> hs(fused.size());
    for (size_t i = 0; i < fused.size(); ++i) {
        const unsigned long long* p = c.d_tables + i * per;
        hs[i].sites = reinterpret_cast<const double2* const*>(p);
        hs[i].fac_off = reinterpret_cast<const size_t*>(p + n);
        hs[i].dims = reinterpret_cast<const int*>(p + 2 * n + 1);
        hs[i].factors = c.d_factors + c.states[fused[i]].fac_at;
    }
    if (c.d_states.upload(hs)) return 1;
    for (size_t s0 = 0; s0 < fused.size(); s0 += kMaxGridY) {
        MpsEntChainArgs a{c.n, c.d_states + s0};
        HIP_OK(launch_mps_ent_chain(a, (int)std::min<size_t>(kMaxGridY, fused.size() - s0), st));
    }
    const size_t total = c.item_state.size();
    if (total) {
        const int K = c.k, chunk = mps_ent_chunk(K, total, kSvdBudget);
        std::vector<int> items(c.item_state);
        items.insert(items.end(), c.item_cut.begin(), c.item_cut.end());
        const size_t mat = (size_t)K * K;
        if (c.d_items.upload(items) || c.d_ints.alloc(2 * total + 2 * (size_t)chunk) || c.d_s.alloc(total * K) || c.d_a.alloc(chunk * mat) ||
            c.d_u.alloc(chunk * mat) || c.d_vh.alloc(chunk * mat) || c.d_work.alloc(svd_batch_work_elems(chunk, K, K)) ||
            c.d_vmat.alloc(svd_batch_v_elems(chunk, K, K))) return 1;
        int* d_sweeps = c.d_ints;
        int* d_status = d_sweeps + total;
        int* d_rows = d_status + total;
        int* d_cols = d_rows + chunk;
        for (size_t first = 0; first < total; first += chunk) {   // the chunks share the SVD's stores: one stream orders them
            const int count = (int)std::min<size_t>(chunk, total - first);
            MpsEntCutArgs a{c.n, K, (int)first, c.d_items, c.d_items + total, c.d_states, c.d_a, d_rows, d_cols};
            HIP_OK(launch_mps_ent_cut(a, count, st));
            HIP_OK(launch_svd_batch(count, K, K, d_rows, d_cols, c.d_a, c.d_u, c.d_s + first * K, c.d_vh, d_sweeps + first, d_status + first, c.d_work,
                                    c.d_vmat, st));
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

// canonical route: the identity sweeps of the engine on a clone; the bond vectors are the Schmidt values
int run_canonical(Call& c, StateWork& w) {
    const int n = c.n;
    w.values.assign((size_t)c.cuts * c.kmax, 0.0);
    std::vector<double2> host;
    for (int q = 0; q < n && w.finite; ++q) {   // a state that is not finite gives NaN rows, as on the fused route
        host.resize((size_t)2 * w.dims[q] * w.dims[q + 1]);
        HIP_OK(hipMemcpy(host.data(), w.t[q], sizeof(double2) * host.size(), hipMemcpyDeviceToHost));
        for (const double2& x : host)
            if (!(std::isfinite(x.x) && std::isfinite(x.y))) { w.finite = false; break; }
    }
    if (!w.finite) return 0;
    aqc_mps* m = nullptr;
    if (aqc_mps_clone(w.h, &m)) return 1;
    static const double eye[32] = {1, 0, 0, 0, 0, 0, 0, 0,  0, 0, 1, 0, 0, 0, 0, 0,  0, 0, 0, 0, 1, 0, 0, 0,  0, 0, 0, 0, 0, 0, 1, 0};
    int rc = 0;
    for (int q = n - 2; q >= 0 && !rc; --q) rc = aqc_mps_gate2(m, q, q + 1, eye, 0.0, 0);
    for (int q = 0; q + 1 < n && !rc; ++q) rc = aqc_mps_gate2(m, q, q + 1, eye, 0.0, 0);
    std::vector<int> dims(n + 1);
    if (!rc) rc = aqc_mps_dims(m, dims.data());
    for (int q = 1; q < n && !rc; ++q) {
        const void* site = nullptr;
        const double* lam = nullptr;
        rc = mps_peek(m, q - 1, &site, &lam);
        const int count = std::min(dims[q], w.dims[q]);   // (the sweeps never grow a bond)
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
    for (int i = 0; i < nstates; ++i)
        if (!states[i]) return failf("null state");
    const int n = aqc_mps_num_qubits(states[0]), device = aqc_mps_device(states[0]);
    if (n < 1) return failf("a state needs at least 1 qubit");
    for (int i = 0; i < nstates; ++i)
        if (aqc_mps_num_qubits(states[i]) != n || aqc_mps_device(states[i]) != device) return failf("MPS states differ in size or device");
    Call c;
    c.n = n;
    c.cuts = mps_ent_cuts(n);
    c.kmax = kmax;
    const int rows = std::max(c.cuts, 1);
    if ((size_t)nstates * (size_t)rows > (size_t)1 << 28) return failf("too many cuts in one call: %d states x %d cuts", nstates, c.cuts);
    std::map<const aqc_mps*, int> seen;
    std::vector<size_t> lane_factor_at(nstates, 0);
    size_t factor_total = 0;
    int need = 1;
    for (int i = 0; i < nstates; ++i) {
        auto it = seen.find(states[i]);
        if (it == seen.end()) {
            it = seen.emplace(states[i], (int)c.states.size()).first;
            c.states.emplace_back();
            StateWork& w = c.states.back();
            w.h = states[i];
            w.dims.resize(n + 1);
            if (aqc_mps_dims(states[i], w.dims.data())) return 1;
            w.fac_off = mps_ent_factor_offsets(n, w.dims.data());
            w.route = method == kMpsEntByRule ? mps_ent_route(n, w.dims.data()) : method;
            const int maxb = mps_ent_max_bond(n, w.dims.data());
            if (w.route == kMpsEntFused && maxb > kMpsEntFusedCap)
                return failf("the fused route takes bond dimensions up to %d; state %d has %d", (int)kMpsEntFusedCap, i, maxb);
            if (factors && w.route != kMpsEntFused) return failf("the factors are those of the fused route; state %d takes the canonical one", i);
            need = std::max(need, maxb);
        }
        c.lane_state.push_back(it->second);
        lane_factor_at[i] = factor_total;
        factor_total += 2 * c.states[it->second].fac_off[n];
    }
    if (kmax < need) return failf("kmax = %d is below the largest bond dimension %d", kmax, need);
    HIP_OK(hipSetDevice(device));
    for (StateWork& w : c.states) {   // (mps_peek drains the state's own stream: what aqc_mps_dot_ops does for its second operand)
        w.t.resize(n);
        for (int q = 0; q < n; ++q) {
            const void* site = nullptr;
            const double* lam = nullptr;
            if (mps_peek(w.h, q, &site, &lam)) return 1;
            w.t[q] = static_cast<const double2*>(site);
        }
    }
    std::vector<int> fused;
    for (size_t k = 0; k < c.states.size(); ++k)
        if (c.states[k].route == kMpsEntFused) {
            c.states[k].fused_index = (int)fused.size();
            fused.push_back((int)k);
            for (int q = 1; q < n; ++q) c.k = std::max(c.k, c.states[k].dims[q]);
        }
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
        const int rc = run_fused(c, fused, factors, lane_factor_at, st);
        const hipError_t e = hipStreamSynchronize(st);   // before any buffer goes, also after a failure
        if (rc) return 1;
        if (e != hipSuccess) return failf("Schmidt values failed: %s", hipGetErrorString(e));
        for (size_t item = 0; item < c.item_state.size(); ++item) {
            const int lane = c.item_lane[item], q = c.item_cut[item], chi = c.states[c.lane_state[lane]].dims[q];
            const size_t row = (size_t)lane * rows + (q - 1);
            const bool bad = c.h_status[item] == kMpsEntNonFinite;
            for (int k = 0; k < (bad ? kmax : chi); ++k) s[row * kmax + k] = bad ? std::numeric_limits<double>::quiet_NaN() : c.h_s[item * c.k + k];
            if (sweeps) sweeps[row] = c.h_sweeps[item];
            if (status) status[row] = c.h_status[item];
            else if (c.h_status[item] == kMpsEntSweepLimit) return failf("state %d, cut %d: the SVD reached its sweep limit", lane, q);
        }
    }
    for (StateWork& w : c.states) {
        if (w.route == kMpsEntFused || c.cuts == 0) continue;
        if (run_canonical(c, w)) return 1;
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
