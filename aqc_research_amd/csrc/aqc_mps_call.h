// The skeleton of a call that reads single-lane MPS states (aqc_mps_obs_api.cpp, aqc_mps_sample_api.cpp, aqc_mps_pauli_api.cpp,
// aqc_mps_ent_api.cpp, aqc_mps_compress_api.cpp, aqc_mps_combine_api.cpp, aqc_mps_opsum_api.cpp, aqc_mps_layers_api.cpp, aqc_mps_tovec_api.cpp): check the handles, view the distinct states, pack what the kernels read
// of them into one table, launch on the first state's stream, synchronise once, assemble.  Each of those files keeps its own plan,
// launches and results; what they share about their input states is here and in the HIP-free aqc_mps_states_rule.h.  The second
// half holds the host scaffolding of a truncating sweep (aqc_mps_compress_api.cpp, aqc_mps_layers_api.cpp, aqc_mps_fromvec_api.cpp;
// DESIGN.md 6w, "Sweep calls"): the argument checks, the chunk budget, the stores of a chunk of the batched SVD (those also in aqc_mps_ent_api.cpp),
// flat stores sized by static bounds, and the adoption of the new states from them; the device side of the cut is aqc_mps_cut.h; the
// sweep over whole states that compression, linear combinations and operator sums share is aqc_mps_sweep.h (the two that sweep a direct
// sum share aqc_mps_sum_call.h on top of it).
// Private to csrc/ (everything has internal linkage).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "aqc_devbuf.h"
#include "aqc_mps_compress_rule.h"
#include "aqc_mps_host.h"
#include "aqc_mps_states_rule.h"

namespace {

constexpr int kMaxGridY = 65535;
enum { kMpsByRule = 0, kMpsFused = 1 };                // what the method / route numbers of all five calls have in common

// ---- check: no null handle, one size and one device in `a` and (where given) `b`; n and the device are those of a[0]
[[maybe_unused]] int check_states(aqc_mps* const* a, aqc_mps* const* b, int count, int min_qubits, int* n_out, int* device_out) {
    for (int i = 0; i < count; ++i)
        if (!a[i] || (b && !b[i])) return failf("null state");
    const int n = aqc_mps_num_qubits(a[0]), device = aqc_mps_device(a[0]);
    if (n < min_qubits) return min_qubits > 1 ? failf("pair density matrices need at least %d qubits", min_qubits) : failf("a state needs at least 1 qubit");
    for (int i = 0; i < count; ++i)
        for (const aqc_mps* h : {(const aqc_mps*)a[i], (const aqc_mps*)(b ? b[i] : a[i])})
            if (aqc_mps_num_qubits(h) != n || aqc_mps_device(h) != device) return failf("MPS states differ in size or device");
    *n_out = n;
    *device_out = device;
    return 0;
}

// ---- view: what a call reads of one distinct state, after one drain of the state's own stream (what aqc_mps_dot_ops does for its
// second operand).  views: the distinct states of the list in order of first appearance; lane_state[i]: the view of handles[i]
struct MpsView {
    aqc_mps* h = nullptr;
    int max_bond = 1;
    std::vector<int> dims;
    std::vector<const double2*> t;
};
[[maybe_unused]] int view_states(aqc_mps* const* handles, size_t count, int n, std::vector<MpsView>& views, std::vector<int>& lane_state) {
    MpsDistinct<aqc_mps*> distinct = mps_distinct(handles, count);
    lane_state.swap(distinct.lane_state);
    views.resize(distinct.items.size());
    for (size_t k = 0; k < views.size(); ++k) {
        MpsView& v = views[k];
        v.h = distinct.items[k];
        v.dims.resize(n + 1);
        v.t.resize(n);
        if (mps_view(v.h, v.dims.data(), v.t.data())) return 1;
        v.max_bond = mps_max_bond(n, v.dims.data());
    }
    return 0;
}

// ---- route: the method of the call, or the rule's choice; the fused route refuses bonds beyond its cap.  -1 with the message set
[[maybe_unused]] int resolve_route(int method, int rule_route, int max_bond, int cap, const char* what, int index) {
    const int route = method == kMpsByRule ? rule_route : method;
    if (route == kMpsFused && max_bond > cap) {
        failf("the fused route takes bond dimensions up to %d; %s %d has %d", cap, what, index, max_bond);
        return -1;
    }
    return route;
}

// ---- table: one record per state in the layout of aqc_mps_states_rule.h, one upload per call (a table that was never uploaded hands
// out null pointers: a call whose states all take the gemm route of the observables or of sampling needs none)
struct MpsTable {
    static_assert(sizeof(unsigned long long) == sizeof(size_t) && sizeof(unsigned long long) == sizeof(const double2*), "8-byte words");
    MpsTableLayout layout;
    std::vector<unsigned long long> words;
    DevBuf<unsigned long long> dev;
    MpsTable() = default;
    MpsTable(std::initializer_list<MpsTableSection> sections, size_t nstates) : layout(sections), words(layout.per * nstates, 0) {}
    template <class T>
    void put(size_t state, int section, const std::vector<T>& v, size_t count) { memcpy(words.data() + layout.word(state, section), v.data(), count * sizeof(T)); }
    int upload() { return dev.upload(words); }
    template <class T>
    const T* at(size_t state, int section) const { return dev ? reinterpret_cast<const T*>(dev + layout.word(state, section)) : nullptr; }
};

// ---- L_0 .. L_{n-1} and R_n .. R_1 of <psi|psi>, once per state and call.  Fused (d_sites, d_dims, d_off: the state's sections of
// the call's table): both halves by the sweep of the observables on the matrix cores; else the engine's environment steps on the
// pair (psi, psi), the halves asked for
enum { kEnvLeft = 1, kEnvRight = 2 };
struct NormEnvs { DevBuf<double2> l, r, tmp; };
[[maybe_unused]] int norm_environments(NormEnvs& e, const MpsView& v, const std::vector<size_t>& off, hipStream_t st, bool fused, int halves,
                                       const double2* const* d_sites = nullptr, const int* d_dims = nullptr, const size_t* d_off = nullptr) {
    if (e.r) return 0;
    const int n = (int)v.t.size();
    const size_t total = off[n + 1];
    static const double one[2] = {1.0, 0.0};
    if (fused) halves = kEnvLeft | kEnvRight;
    if (((halves & kEnvLeft) && e.l.alloc(total)) || e.r.alloc(total)) return 1;
    if (halves & kEnvLeft) HIP_OK(hipMemcpyAsync(e.l + off[0], one, sizeof one, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(e.r + off[n], one, sizeof one, hipMemcpyHostToDevice, st));
    if (fused) {
        MpsObsFusedArgs a{};
        a.n = n;
        a.sites = d_sites;
        a.dims = d_dims;
        a.env_off = d_off;
        a.env_l = e.l;
        a.env_r = e.r;
        HIP_OK(launch_mps_obs_env(a, st));
        return 0;
    }
    const int* dims = v.dims.data();
    size_t tmax = 1;
    for (int q = 0; q < n; ++q) tmax = std::max(tmax, (size_t)dims[q] * dims[q + 1]);
    if (e.tmp.alloc(tmax)) return 1;
    for (int q = 0; (halves & kEnvLeft) && q + 1 < n; ++q)
        if (env_left(st, e.l + off[q], v.t[q], v.t[q], site_dims(dims, dims, q), nullptr, nullptr, e.tmp, e.l + off[q + 1])) return 1;
    for (int q = n - 1; q >= 1; --q)
        if (env_right(st, e.r + off[q + 1], v.t[q], v.t[q], site_dims(dims, dims, q), e.tmp, e.r + off[q])) return 1;
    return 0;
}

// ---- the canonical route's start: the sites are scanned on the host; a state that is not finite (or, where the caller says so, has a
// site of zeros) is left alone and *m stays null; else *m is a clone after the engine's two identity sweeps, the caller's to destroy
[[maybe_unused]] const double kIdentityGate2[32] = {1, 0, 0, 0, 0, 0, 0, 0,  0, 0, 1, 0, 0, 0, 0, 0,  0, 0, 0, 0, 1, 0, 0, 0,  0, 0, 0, 0, 0, 0, 1, 0};
[[maybe_unused]] int canonical_clone(const MpsView& v, bool stop_at_zero_site, bool* finite, bool* has_zero_site, aqc_mps** m) {
    const int n = (int)v.t.size();
    std::vector<double2> host;
    *finite = true;
    *has_zero_site = false;
    *m = nullptr;
    for (int q = 0; q < n && *finite; ++q) {
        host.resize((size_t)2 * v.dims[q] * v.dims[q + 1]);
        HIP_OK(hipMemcpy(host.data(), v.t[q], sizeof(double2) * host.size(), hipMemcpyDeviceToHost));
        bool all_zero = true;
        for (const double2& x : host) {
            if (!(std::isfinite(x.x) && std::isfinite(x.y))) { *finite = false; break; }
            if (x.x != 0.0 || x.y != 0.0) all_zero = false;
        }
        *has_zero_site = *has_zero_site || all_zero;
    }
    if (!*finite || (stop_at_zero_site && *has_zero_site)) return 0;
    if (aqc_mps_clone(v.h, m)) return 1;
    int rc = 0;
    for (int q = n - 2; q >= 0 && !rc; --q) rc = aqc_mps_gate2(*m, q, q + 1, kIdentityGate2, 0.0, 0);
    for (int q = 0; q + 1 < n && !rc; ++q) rc = aqc_mps_gate2(*m, q, q + 1, kIdentityGate2, 0.0, 0);
    if (rc) {
        (void)aqc_mps_destroy(*m);
        *m = nullptr;
    }
    return rc;
}

// ======== sweep calls: compression, gate layers, conversion of dense vectors (and, for its SVDs alone, the Schmidt spectra).  A sweep
// forms a matrix per lane, runs launch_svd_batch over a chunk of lanes and cuts (aqc_mps_cut.h on the device); the new states are
// adopted from flat stores after the call's one synchronisation.

// ---- check: what every truncating call refuses, in one order; out[] is nulled first: whatever follows, the caller finds null or a
// state it owns.  what: "state" or "vector"; method_ok: the call's own verdict on its method number
[[maybe_unused]] int check_truncating_call(const void* in, aqc_mps** out, int count, double trunc_thr, int max_bond, const char* what, bool method_ok,
                                           int method) {
    if (!in || !out) return failf("null argument");
    if (count < 1) return failf("at least one %s is needed", what);
    for (int i = 0; i < count; ++i) out[i] = nullptr;
    if (!method_ok) return failf("unknown method %d", method);
    if (!(trunc_thr >= 0.0) || !std::isfinite(trunc_thr)) return failf("trunc_thr must be a non-negative number");
    if (max_bond < 0) return failf("max_bond must be non-negative");
    return 0;
}

// ---- budget: the bytes a call sizes its chunks by, behind the *_budget entry points (tests lower it to run many chunks on few lanes):
// bytes > 0 sets it, else the default comes back; returns the value before
[[maybe_unused]] int64_t swap_budget(std::atomic<size_t>& budget, int64_t bytes, size_t dflt) {
    return (int64_t)budget.exchange(bytes > 0 ? (size_t)bytes : dflt);
}

// ---- the stores of one chunk of the batched SVD of m x n matrices (m >= n): a, u [chunk][m][n], s [chunk][n], vh [chunk][n][n], the
// work stores of aqc_svd_batch.hip, and per matrix rows | cols | sweeps | status in one block.  results = false: s, sweeps and status
// are the caller's, for the whole call (aqc_mps_ent_api.cpp), and go to the second launch()
struct SvdChunk {
    int chunk = 0, m = 0, n = 0;
    DevBuf<double2> a, u, vh, work, vmat;
    DevBuf<double> s;
    DevBuf<int> ints;
    int alloc(int chunk_, int m_, int n_, bool results = true) {
        chunk = chunk_; m = m_; n = n_;
        const size_t c = (size_t)chunk, mat = (size_t)m * n;
        return a.alloc(c * mat) || u.alloc(c * mat) || vh.alloc(c * n * n) || work.alloc(svd_batch_work_elems(chunk, m, n)) ||
               vmat.alloc(svd_batch_v_elems(chunk, m, n)) || ints.alloc((results ? 4 : 2) * c) || (results && s.alloc(c * n));
    }
    int* rows() const { return ints; }
    int* cols() const { return ints + chunk; }
    int* sweeps() const { return ints + 2 * (size_t)chunk; }
    int* status() const { return ints + 3 * (size_t)chunk; }
    hipError_t launch(int count, double* d_s, int* d_sweeps, int* d_status, hipStream_t st) const {
        return launch_svd_batch(count, m, n, rows(), cols(), a, u, d_s, vh, d_sweeps, d_status, work, vmat, st);
    }
    hipError_t launch(int count, hipStream_t st) const { return launch(count, s, sweeps(), status(), st); }
};

// ---- adopt: a new engine state from site tensors and bond vectors that the sweep left in flat device stores, site q at
// site_base + site_off[q], bond vector q at lam_base + lam_off[q]
[[maybe_unused]] int adopt_flat(int device, int n, const int* dims, const double2* site_base, const size_t* site_off, const double* lam_base,
                                const size_t* lam_off, double discarded, aqc_mps** out) {
    std::vector<const void*> sites(n);
    std::vector<const double*> lams(std::max(n - 1, 1), nullptr);
    for (int q = 0; q < n; ++q) {
        sites[q] = site_base + site_off[q];
        if (q < n - 1) lams[q] = lam_base + lam_off[q];
    }
    return mps_adopt(device, n, dims, sites.data(), lams.data(), discarded, out);
}

// ---- flat stores sized by static bounds of the bonds, every lane at the same offsets (gate layers, dense vectors; compression sizes
// its stores per state): site_off (n + 1 entries) | lam_off (n entries) on the device in one upload
struct BoundedStores {
    std::vector<size_t> site_off, lam_off;
    size_t site_total = 0, lam_total = 1;
    DevBuf<double2> sites;
    DevBuf<double> lam;
    DevBuf<size_t> off;
    int alloc(int n, const int* bounds, size_t lanes) {
        site_off = mps_site_offsets(n, bounds);
        lam_off = mps_compress_lam_offsets(n, bounds);
        site_total = site_off[n];
        lam_total = std::max<size_t>(lam_off[n - 1], 1);
        std::vector<size_t> both(site_off);
        both.insert(both.end(), lam_off.begin(), lam_off.end());
        return off.upload(both) || sites.alloc(lanes * site_total) || lam.alloc(lanes * lam_total);
    }
    const size_t* d_site_off() const { return off; }
    const size_t* d_lam_off() const { return off + site_off.size(); }
    double2* site(size_t lane, int q) const { return sites + lane * site_total + site_off[q]; }
    int adopt(int device, int n, size_t lane, const int* dims, double discarded, aqc_mps** out) const {
        return adopt_flat(device, n, dims, sites + lane * site_total, site_off.data(), lam + lane * lam_total, lam_off.data(), discarded, out);
    }
};

// ---- a failed call gives back every state it has made
[[maybe_unused]] void drop_outputs(aqc_mps** out, int count) {
    for (int i = 0; i < count; ++i) {
        if (out[i]) (void)aqc_mps_destroy(out[i]);
        out[i] = nullptr;
    }
}

// ---- the end of the launches: the one synchronisation of the call, before any buffer goes, also after a failure (rc != 0)
[[maybe_unused]] int finish_call(hipStream_t st, int rc, const char* what) {
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return 1;
    if (e != hipSuccess) return failf("%s failed: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace
