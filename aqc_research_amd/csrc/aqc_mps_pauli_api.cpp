// C ABI (include/aqc_hip.h): Pauli strings between single-lane MPS states.  Rules: aqc_mps_pauli_rule.h; kernels: aqc_mps_pauli.hip.
// The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <map>
#include <memory>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_obs_rule.h"
#include "aqc_mps_pauli_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsPauliByRule == kMpsByRule && kMpsPauliFused == kMpsFused, "resolve_route");
enum { kSites, kEnvOff, kSiteOff, kDims };            // the sections of a state's record in Call::table

// what the call adds to the view of one distinct state; alive until the call's last synchronisation
struct StateWork {
    const MpsView* v = nullptr;
    std::vector<size_t> off;                          // env offsets, n + 2 entries (the last = total)
    std::vector<size_t> site_off;                     // element offset of site q in one dressed copy, n + 1 entries (the last = total)
    NormEnvs env;                                     // expectation mode: of the kets, built once
    DevBuf<double2> dressed;
    // the same on the device, inside the call's one table
    const double2* const* d_sites = nullptr;
    const size_t* d_off = nullptr;
    const size_t* d_site_off = nullptr;
    const int* d_dims = nullptr;
};

// one walk of the gemm route: the pairs of the call that share their bond dimensions
struct WalkWork {
    DevBuf<double2> scratch;
    DevBuf<void*> d_ptrs;
    DevBuf<int> d_ints;
};

struct Call {
    int n = 0, npairs = 0, nstrings = 0;
    bool expectation = false;
    const uint8_t* strings = nullptr;
    std::vector<int> first, last;
    std::vector<MpsView> views;                       // distinct, in order of first appearance
    std::vector<StateWork> states;                    // one per view
    std::vector<std::unique_ptr<WalkWork>> walks;
    DevBuf<double2> d_out, d_one;
    MpsTable table;                                   // per distinct state: site pointers | env offsets | site offsets | dims
    DevBuf<unsigned char> d_strings;
    DevBuf<int> d_support;
    DevBuf<MpsPauliState> d_kets, d_bras;
    DevBuf<double2*> d_outs;
};

// what the kernels read of every distinct state, in one upload for the call
int tables(Call& c) {
    const size_t n = (size_t)c.n;
    c.table = MpsTable({mps_table_words(n), mps_table_words(n + 2), mps_table_words(n + 1), mps_table_ints(n + 1)}, c.states.size());
    for (size_t k = 0; k < c.states.size(); ++k) {
        c.table.put(k, kSites, c.views[k].t, n);
        c.table.put(k, kEnvOff, c.states[k].off, n + 2);
        c.table.put(k, kSiteOff, c.states[k].site_off, n + 1);
        c.table.put(k, kDims, c.views[k].dims, n + 1);
    }
    if (c.table.upload()) return 1;
    for (size_t k = 0; k < c.states.size(); ++k) {
        StateWork& w = c.states[k];
        w.d_sites = c.table.at<const double2*>(k, kSites);
        w.d_off = c.table.at<size_t>(k, kEnvOff);
        w.d_site_off = c.table.at<size_t>(k, kSiteOff);
        w.d_dims = c.table.at<int>(k, kDims);
    }
    return 0;
}

int dress(StateWork& w, hipStream_t st) {   // the X, Y, Z copies of every site, once per bra and call
    if (w.dressed) return 0;
    const int n = (int)w.v->t.size();
    const size_t total = w.site_off[n];
    size_t smax = 1;
    for (int q = 0; q < n; ++q) smax = std::max(smax, 2 * (size_t)w.v->dims[q] * w.v->dims[q + 1]);
    if (w.dressed.alloc(3 * total)) return 1;
    HIP_OK(launch_mps_pauli_dress(w.d_sites, w.d_dims, w.d_site_off, n, total, (int)smax, w.dressed, st));
    return 0;
}

// One walk for the pairs `pairs`, which share the bond dimensions of bra and ket: a job is one string of one pair (job k: pair
// pairs[k / S], string k % S); the jobs are walked site by site in groups, F = [M T_0; M T_1] stacked, M' = D^H F.
int run_gemm(Call& c, const std::vector<int>& pairs, const std::vector<StateWork*>& bras, const std::vector<StateWork*>& kets, hipStream_t st) {
    const int n = c.n, S = c.nstrings;
    const size_t njobs = pairs.size() * (size_t)S;
    const int* bd = bras[pairs[0]]->v->dims.data();
    const int* kd = kets[pairs[0]]->v->dims.data();
    const size_t melems = mps_pauli_m_elems(n, bd, kd), felems = mps_pauli_f_elems(n, bd, kd);
    const size_t gsize = (size_t)mps_pauli_group_size(melems + felems, (int)std::min<size_t>(njobs, (size_t)kMpsPauliGroupMax), kMpsCallBudget);
    c.walks.emplace_back(new WalkWork());
    WalkWork& w = *c.walks.back();
    if (w.scratch.alloc(gsize * (melems + felems))) return 1;
    for (int p : pairs)
        if (dress(*bras[p], st) || (c.expectation && norm_environments(kets[p]->env, *kets[p]->v, kets[p]->off, st, false, kEnvLeft | kEnvRight))) return 1;
    double2* m_base = w.scratch;
    double2* f_base = m_base + gsize * melems;
    // the tables of every group and site, built first and uploaded once: pointers (7 per job that crosses the site, 2 per job that ends
    // there) and ints (the output index of every job that ends there)
    struct SiteJob { int q; size_t ptr_at; int nstep; size_t close_at, int_at; int nclose; };
    std::vector<SiteJob> jobs;
    std::vector<void*> ptrs;
    std::vector<int> ints;
    auto first_of = [&](size_t k) { return c.expectation ? c.first[k % S] : 0; };
    auto last_of = [&](size_t k) { return c.expectation ? c.last[k % S] : n - 1; };
    for (size_t g0 = 0; g0 < njobs; g0 += gsize) {
        const size_t g1 = std::min(njobs, g0 + gsize);
        for (int q = 0; q < n; ++q) {
            std::vector<size_t> active, closing;
            for (size_t k = g0; k < g1; ++k) {
                if (first_of(k) <= q && q <= last_of(k)) active.push_back(k);
                if (q == last_of(k)) closing.push_back(k);
            }
            if (active.empty()) continue;
            SiteJob job{q, ptrs.size(), (int)active.size(), 0, ints.size(), (int)closing.size()};
            const size_t half = (size_t)bd[q] * kd[q + 1], tsize = (size_t)kd[q] * kd[q + 1];
            auto m_slot = [&](size_t k) { return m_base + (k - g0) * melems; };
            auto f_slot = [&](size_t k) { return f_base + (k - g0) * felems; };
            auto ket_of = [&](size_t k) -> const StateWork& { return *kets[pairs[k / S]]; };
            // tables [7][nstep]: M in | T_q[0] | T_q[1] | F | F + one product | D | M out
            for (size_t k : active) {
                const double2* in = q > first_of(k) ? m_slot(k) : c.expectation ? ket_of(k).env.l + ket_of(k).off[q] : (double2*)c.d_one;
                ptrs.push_back(const_cast<double2*>(in));
            }
            for (size_t k : active) ptrs.push_back(const_cast<double2*>(ket_of(k).v->t[q]));
            for (size_t k : active) ptrs.push_back(const_cast<double2*>(ket_of(k).v->t[q] + tsize));
            for (size_t k : active) ptrs.push_back(f_slot(k));
            for (size_t k : active) ptrs.push_back(f_slot(k) + half);
            for (size_t k : active) {
                const StateWork& bra = *bras[pairs[k / S]];
                const int letter = c.strings[(k % S) * n + q];
                const double2* d = letter == kMpsPauliI ? bra.v->t[q] : bra.dressed + (size_t)(letter - 1) * bra.site_off[n] + bra.site_off[q];
                ptrs.push_back(const_cast<double2*>(d));
            }
            for (size_t k : active) ptrs.push_back(m_slot(k));
            job.close_at = ptrs.size();
            for (size_t k : closing) ptrs.push_back(m_slot(k));
            for (size_t k : closing) {
                ptrs.push_back(c.expectation ? ket_of(k).env.r + ket_of(k).off[q + 1] : (double2*)c.d_one);
                ints.push_back((int)((size_t)pairs[k / S] * S + k % S));
            }
            jobs.push_back(job);
        }
    }
    if (w.d_ptrs.upload(ptrs) || w.d_ints.upload(ints)) return 1;
    for (const SiteJob& job : jobs) {
        const int q = job.q, x = bd[q], u = bd[q + 1], y = kd[q], v = kd[q + 1], m = job.nstep;
        void* const* tab = w.d_ptrs + job.ptr_at;
        auto ctab = [&](size_t at) { return reinterpret_cast<const void* const*>(tab + at); };
        HIP_OK(launch_zgemm_tables_op(false, false, x, v, y, ctab(0), y, ctab((size_t)m), v, tab + 3 * (size_t)m, v, 0, 0, 0, m, 1, st));
        HIP_OK(launch_zgemm_tables_op(false, false, x, v, y, ctab(0), y, ctab(2 * (size_t)m), v, tab + 4 * (size_t)m, v, 0, 0, 0, m, 1, st));
        HIP_OK(launch_zgemm_tables_op(true, false, u, v, 2 * x, ctab(5 * (size_t)m), u, ctab(3 * (size_t)m), v, tab + 6 * (size_t)m, v, 0, 0, 0, m, 1, st));
        if (job.nclose) {
            const void* const* close = reinterpret_cast<const void* const*>(w.d_ptrs + job.close_at);
            HIP_OK(launch_mps_pauli_close(close, close + job.nclose, w.d_ints + job.int_at, job.nclose, c.expectation ? v : 1, c.d_out, st));
        }
    }
    return 0;
}

// every pair of the fused route in one launch per kMaxGridY pairs
int run_fused(Call& c, const std::vector<int>& fused, const std::vector<StateWork*>& bras, const std::vector<StateWork*>& kets, hipStream_t st) {
    std::vector<int> support(c.first);
    support.insert(support.end(), c.last.begin(), c.last.end());
    if (c.d_strings.upload(std::vector<unsigned char>(c.strings, c.strings + (size_t)c.nstrings * c.n)) || c.d_support.upload(support)) return 1;
    std::vector<MpsPauliState> hk, hb;
    std::vector<double2*> outs;
    auto entry = [](const StateWork& w) {
        MpsPauliState e{};
        e.sites = w.d_sites; e.dims = w.d_dims; e.env_off = w.d_off; e.env_l = w.env.l; e.env_r = w.env.r;
        return e;
    };
    for (int p : fused) {
        StateWork& k = *kets[p];
        if (c.expectation && norm_environments(k.env, *k.v, k.off, st, true, kEnvLeft | kEnvRight, k.d_sites, k.d_dims, k.d_off)) return 1;
        hk.push_back(entry(k));
        hb.push_back(entry(*bras[p]));
        outs.push_back(c.d_out + (size_t)p * c.nstrings);
    }
    if (c.d_kets.upload(hk) || c.d_bras.upload(hb) || c.d_outs.upload(outs)) return 1;
    for (size_t p0 = 0; p0 < fused.size(); p0 += kMaxGridY) {
        MpsPauliFusedArgs a{};
        a.n = c.n; a.nstrings = c.nstrings; a.expectation = c.expectation;
        a.kets = c.d_kets + p0; a.bras = c.d_bras + p0;
        a.strings = c.d_strings;
        a.first = c.d_support; a.last = c.d_support + c.nstrings;
        a.out = c.d_outs + p0;
        HIP_OK(launch_mps_pauli_fused(a, (int)std::min<size_t>(kMaxGridY, fused.size() - p0), st));
    }
    return 0;
}

int run(Call& c, aqc_mps* const* bras, aqc_mps* const* kets, int method, double* out, hipStream_t st) {
    const int n = c.n;
    std::vector<aqc_mps*> listed;   // bra and ket of every pair (expectation mode: the ket twice)
    for (int p = 0; p < c.npairs; ++p) listed.insert(listed.end(), {bras ? bras[p] : kets[p], kets[p]});
    std::vector<int> listed_state;
    if (view_states(listed.data(), listed.size(), n, c.views, listed_state)) return 1;
    c.states.resize(c.views.size());
    for (size_t k = 0; k < c.states.size(); ++k) {
        StateWork& w = c.states[k];
        w.v = &c.views[k];
        w.off = mps_obs_env_offsets(n, w.v->dims.data());
        w.site_off = mps_site_offsets(n, w.v->dims.data());
    }
    std::vector<StateWork*> wb(c.npairs), wk(c.npairs);
    std::vector<int> fused, gemm;
    for (int p = 0; p < c.npairs; ++p) {
        wb[p] = &c.states[listed_state[2 * p]];
        wk[p] = &c.states[listed_state[2 * p + 1]];
        const int* bd = wb[p] == wk[p] ? nullptr : wb[p]->v->dims.data();
        const int* kd = wk[p]->v->dims.data();
        const int route = resolve_route(method, mps_pauli_route(n, bd, kd), mps_pauli_max_bond(n, bd, kd), kMpsPauliFusedCap, "pair", p);
        if (route < 0) return 1;
        (route == kMpsPauliFused ? fused : gemm).push_back(p);
    }
    if (tables(c) || c.d_out.alloc((size_t)c.npairs * c.nstrings)) return 1;
    if (!gemm.empty()) {
        if (c.d_one.alloc(1)) return 1;
        static const double one[2] = {1.0, 0.0};
        HIP_OK(hipMemcpyAsync(c.d_one, one, sizeof one, hipMemcpyHostToDevice, st));
    }
    if (!fused.empty() && run_fused(c, fused, wb, wk, st)) return 1;
    std::map<std::pair<std::vector<int>, std::vector<int>>, std::vector<int>> walks;   // pairs with the same bonds share a walk
    for (int p : gemm) walks[{wb[p]->v->dims, wk[p]->v->dims}].push_back(p);
    for (const auto& walk : walks)
        if (run_gemm(c, walk.second, wb, wk, st)) return 1;
    HIP_OK(hipMemcpyAsync(out, c.d_out, sizeof(double2) * (size_t)c.npairs * c.nstrings, hipMemcpyDeviceToHost, st));
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_pauli_route(int n, const int32_t* bra_dims, const int32_t* ket_dims) {
    if (!ket_dims || n < 1) return -1;
    for (int q = 0; q <= n; ++q)
        if (ket_dims[q] < 1 || (bra_dims && bra_dims[q] < 1)) return -1;
    return mps_pauli_route(n, bra_dims, ket_dims);
}

int aqc_mps_pauli_support(int n, int nstrings, const uint8_t* strings, int32_t* first, int32_t* last) {
    if (!strings || !first || !last) return failf("null argument");
    if (n < 1) return failf("a string needs at least 1 qubit");
    if (nstrings < 1) return failf("at least one string is needed");
    const int64_t bad = mps_pauli_bad_letter(strings, (size_t)nstrings * n);
    if (bad >= 0) return failf("string %lld, qubit %lld: a letter is 0, 1, 2 or 3 (I, X, Y, Z), not %d", (long long)(bad / n), (long long)(bad % n), (int)strings[bad]);
    for (int s = 0; s < nstrings; ++s) mps_pauli_support(n, strings + (size_t)s * n, first + s, last + s);
    return 0;
}

int aqc_mps_pauli(aqc_mps* const* bras, aqc_mps* const* kets, int npairs, int nstrings, const uint8_t* strings, int method, double* out) {
    if (!kets || !strings || !out) return failf("null argument");
    if (npairs < 1) return failf("at least one pair of states is needed");
    if (nstrings < 1) return failf("at least one string is needed");
    if (!mps_pauli_method_ok(method)) return failf("unknown method %d", method);
    int n = 0, device = 0;
    if (check_states(kets, bras, npairs, 1, &n, &device)) return 1;
    if ((size_t)npairs * (size_t)nstrings > (size_t)1 << 30) return failf("too many values in one call: %d pairs x %d strings", npairs, nstrings);
    Call c;
    c.n = n;
    c.npairs = npairs;
    c.nstrings = nstrings;
    c.expectation = bras == nullptr;
    c.strings = strings;
    c.first.resize(nstrings);
    c.last.resize(nstrings);
    if (aqc_mps_pauli_support(n, nstrings, strings, c.first.data(), c.last.data())) return 1;
    HIP_OK(hipSetDevice(device));
    hipStream_t st = mps_stream(kets[0]);
    return finish_call(st, run(c, bras, kets, method, out, st), "Pauli strings");
}

}  // extern "C"
