// C ABI (include/aqc_hip.h): pair density matrices of single-lane MPS states.  Rules: aqc_mps_obs_rule.h; kernels: aqc_mps_obs.hip.
// The skeleton of the call: aqc_mps_call.h.
#include <memory>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_obs_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsObsByRule == kMpsByRule && kMpsObsFused == kMpsFused, "resolve_route");
enum { kSites, kEnvOff, kDims };                      // the sections of a state's record in the call's table

// everything one lane's launches read or write; alive until the call's last synchronisation
struct StateWork {
    int n = 0;
    const MpsView* v = nullptr;                       // the lane's state
    std::vector<size_t> off;                          // env offsets, n + 2 entries (the last = total)
    NormEnvs env;
    DevBuf<double2> chains, close, sums;
    DevBuf<int> d_ints;
    DevBuf<void*> d_ptrs;
    std::vector<double2> h_sums;
};

// the chains after the environments (norm_environments: the copies of one, then the sweep on the matrix cores)
int run_fused(StateWork& w, const MpsObsPlan& plan, const MpsTable& table, size_t state, hipStream_t st) {
    const int n = w.n;
    std::vector<int> ints;                                   // chain_start | chain_last | emit_of
    std::vector<int> chain_of(n, -1), starts;
    for (int i = 0; i < n; ++i)
        if (plan.last[i] >= 0) { chain_of[i] = (int)starts.size(); starts.push_back(i); }
    const int nchains = (int)starts.size();
    ints.insert(ints.end(), starts.begin(), starts.end());
    for (int i : starts) ints.push_back(plan.last[i]);
    const size_t emit_at = ints.size();
    ints.resize(emit_at + (size_t)nchains * n, -1);
    for (size_t e = 0; e < plan.emits.size(); ++e) ints[emit_at + (size_t)chain_of[plan.emits[e].chain] * n + plan.emits[e].site] = (int)e;
    if (w.d_ints.upload(ints)) return 1;
    MpsObsFusedArgs a;
    a.n = n;
    a.sites = table.at<const double2*>(state, kSites);
    a.dims = table.at<int>(state, kDims);
    a.env_off = table.at<size_t>(state, kEnvOff);
    a.env_l = w.env.l;
    a.env_r = w.env.r;
    a.chain_start = w.d_ints;
    a.chain_last = w.d_ints + nchains;
    a.emit_of = w.d_ints + emit_at;
    a.sums = w.sums;
    HIP_OK(launch_mps_obs_fused(a, nchains, st));
    return 0;
}

int run_gemm(StateWork& w, const MpsObsPlan& plan, hipStream_t st) {
    const int n = w.n;
    const int* dims = w.v->dims.data();
    const size_t S = mps_obs_slot_elems(n, dims);
    std::vector<int> starts;
    for (int i = 0; i < n; ++i)
        if (plan.last[i] >= 0) starts.push_back(i);
    const int nchains = (int)starts.size();
    const int gsize = mps_obs_group_size(n, dims, nchains, kMpsCallBudget);
    // per chain: E [3][S] and F [3][2 S]; closing: H [2][S] and K [3][S]
    if (w.chains.alloc((size_t)gsize * 3 * kMpsObsComps * S) || w.close.alloc(5 * S)) return 1;
    double2* e_base = w.chains;
    double2* f_base = e_base + (size_t)gsize * kMpsObsComps * S;
    double2* hbuf = w.close;
    double2* kbuf = hbuf + 2 * S;
    auto e_slot = [&](int slot) { return e_base + (size_t)slot * kMpsObsComps * S; };
    auto f_slot = [&](int slot) { return f_base + (size_t)slot * kMpsObsComps * 2 * S; };
    // the tables of every group and site, built first and uploaded once: pointers (5 per stepping chain) and ints (2 per emission)
    struct SiteJob { int q; size_t ptr_at; int nstep; size_t int_at; int nemit; int open_slot; };
    std::vector<std::vector<SiteJob>> jobs;
    std::vector<void*> ptrs;
    std::vector<int> ints;
    std::vector<std::vector<int>> emits_at(n);
    for (size_t e = 0; e < plan.emits.size(); ++e) emits_at[plan.emits[e].site].push_back((int)e);
    for (int g0 = 0; g0 < nchains; g0 += gsize) {
        const int g1 = std::min(nchains, g0 + gsize);
        int q_last = 0;
        for (int c = g0; c < g1; ++c) q_last = std::max(q_last, plan.last[starts[c]]);
        std::vector<SiteJob> group;
        for (int q = starts[g0]; q <= q_last; ++q) {
            SiteJob job{q, ptrs.size(), 0, ints.size(), 0, -1};
            const size_t lr = (size_t)dims[q] * dims[q + 1];
            std::vector<int> stepping;
            for (int c = g0; c < g1; ++c) {
                if (starts[c] == q) job.open_slot = c - g0;
                if (starts[c] < q && q < plan.last[starts[c]]) stepping.push_back(c - g0);
            }
            job.nstep = (int)stepping.size();
            // tables [5][nstep]: E slots | T_q[0] | T_q[1] | F slots | F slots + one site matrix
            for (int s : stepping) ptrs.push_back(e_slot(s));
            for (int k = 0; k < job.nstep; ++k) ptrs.push_back(const_cast<double2*>(w.v->t[q]));
            for (int k = 0; k < job.nstep; ++k) ptrs.push_back(const_cast<double2*>(w.v->t[q] + lr));
            for (int s : stepping) ptrs.push_back(f_slot(s));
            for (int s : stepping) ptrs.push_back(f_slot(s) + lr);
            std::vector<int> slots, idx;
            for (int e : emits_at[q]) {
                const int c = plan.emits[e].chain;
                int pos = -1;
                for (int k = g0; k < g1; ++k) if (starts[k] == c) pos = k - g0;
                if (pos >= 0) { slots.push_back(pos); idx.push_back(e); }
            }
            job.nemit = (int)slots.size();
            ints.insert(ints.end(), slots.begin(), slots.end());
            ints.insert(ints.end(), idx.begin(), idx.end());
            group.push_back(job);
        }
        jobs.push_back(group);
    }
    if (w.d_ptrs.upload(ptrs) || w.d_ints.upload(ints)) return 1;
    for (const std::vector<SiteJob>& group : jobs)
        for (const SiteJob& job : group) {
            const int q = job.q, x = dims[q], u = dims[q + 1];
            const size_t lr = (size_t)x * u;
            const double2* t0 = w.v->t[q];
            const double2* t1 = t0 + lr;
            if (job.nemit) {   // K^{cd} = T_c (R_{q+1} T_d^H), components 00, 01, 11; then the sums of every chain that emits here
                const double2* r = w.env.r + w.off[q + 1];
                HIP_OK(launch_zgemm_bh(false, false, u, x, u, r, u, t0, u, hbuf, x, st));
                HIP_OK(launch_zgemm_bh(false, false, u, x, u, r, u, t1, u, hbuf + S, x, st));
                HIP_OK(launch_zgemm(false, false, x, x, u, t0, u, hbuf, x, kbuf, x, st));
                HIP_OK(launch_zgemm(false, false, x, x, u, t0, u, hbuf + S, x, kbuf + S, x, st));
                HIP_OK(launch_zgemm(false, false, x, x, u, t1, u, hbuf + S, x, kbuf + 2 * S, x, st));
                HIP_OK(launch_mps_obs_sums(e_base, w.d_ints + job.int_at, w.d_ints + job.int_at + job.nemit, job.nemit, S, kbuf, S, x, w.sums, st));
            }
            if (job.nstep) {   // F = [E T_0; E T_1] stacked, E <- [T_0; T_1]^H F, for the 3 components of every chain that crosses the site
                void* const* tab = w.d_ptrs + job.ptr_at;
                const int m = job.nstep;
                auto ctab = [&](int k) { return reinterpret_cast<const void* const*>(tab + (size_t)k * m); };
                HIP_OK(launch_zgemm_tables_op(false, false, x, u, x, ctab(0), x, ctab(1), u, tab + 3 * (size_t)m, u, S, 0, 2 * S, m, kMpsObsComps, st));
                HIP_OK(launch_zgemm_tables_op(false, false, x, u, x, ctab(0), x, ctab(2), u, tab + 4 * (size_t)m, u, S, 0, 2 * S, m, kMpsObsComps, st));
                HIP_OK(launch_zgemm_tables_op(true, false, u, u, 2 * x, ctab(1), u, ctab(3), u, tab, u, 0, 2 * S, S, m, kMpsObsComps, st));
            }
            if (job.open_slot >= 0) {   // G_a = L_q T_a into the chain's F; E^{00} = T_0^H G_0, E^{01} = T_1^H G_0, E^{11} = T_1^H G_1
                const double2* l = w.env.l + w.off[q];
                double2* g = f_slot(job.open_slot);
                double2* e = e_slot(job.open_slot);
                HIP_OK(launch_zgemm(false, false, x, u, x, l, x, t0, u, g, u, st));
                HIP_OK(launch_zgemm(false, false, x, u, x, l, x, t1, u, g + lr, u, st));
                HIP_OK(launch_zgemm(true, false, u, u, x, t0, u, g, u, e, u, st));
                HIP_OK(launch_zgemm(true, false, u, u, x, t1, u, g, u, e + S, u, st));
                HIP_OK(launch_zgemm(true, false, u, u, x, t1, u, g + lr, u, e + 2 * S, u, st));
            }
        }
    return 0;
}

// the 4 x 4 of an emission from its sums [3][4]: the upper triangle, mirrored; the diagonal's imaginary parts are dropped
void assemble(const double2* sums, double* m /* [4][4] complex */) {
    for (int e = 0; e < kMpsObsUpper; ++e) {
        const MpsObsEntry en = mps_obs_upper(e);
        const double2 v = sums[en.ecomp * 4 + (en.eadj ? 3 : en.kcomp)];
        m[2 * (4 * en.row + en.col)] = v.x;
        m[2 * (4 * en.row + en.col) + 1] = en.row == en.col ? 0.0 : v.y;
        if (en.row != en.col) {
            m[2 * (4 * en.col + en.row)] = v.x;
            m[2 * (4 * en.col + en.row) + 1] = -v.y;
        }
    }
}

}  // namespace

extern "C" {

int aqc_mps_obs_plan(int n, int npairs, const int32_t* pairs, int32_t* chain_last, int32_t* nemits, int32_t* serves) {
    if (!pairs || !chain_last || !nemits || !serves) return failf("null argument");
    if (n < 2) return failf("pair density matrices need at least 2 qubits");
    if (npairs < 1) return failf("at least one pair is needed");
    MpsObsPlan plan;
    if (!mps_obs_plan(n, npairs, pairs, plan)) return failf("a pair needs two different qubits below %d", n);
    for (int i = 0; i < n; ++i) chain_last[i] = plan.last[i];
    *nemits = (int32_t)plan.emits.size();
    for (int p = 0; p < npairs; ++p) {
        const MpsObsEmit& e = plan.emits[plan.pair_emit[p]];
        serves[3 * p] = e.chain;
        serves[3 * p + 1] = e.site;
        serves[3 * p + 2] = plan.pair_transposed[p];
    }
    return 0;
}

int aqc_mps_obs_route(int n, const int32_t* dims) {
    if (!dims || n < 1) return -1;
    return mps_obs_route(n, dims);
}

int aqc_mps_obs_pairs(aqc_mps* const* states, int nstates, int npairs, const int32_t* pairs, int method, double* out) {
    if (!states || !pairs || !out) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    if (npairs < 1) return failf("at least one pair is needed");
    if (method != kMpsObsByRule && method != kMpsObsFused && method != kMpsObsGemm) return failf("unknown method %d", method);
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 2, &n, &device)) return 1;
    MpsObsPlan plan;
    if (!mps_obs_plan(n, npairs, pairs, plan)) return failf("a pair needs two different qubits below %d", n);
    HIP_OK(hipSetDevice(device));
    hipStream_t st = mps_stream(states[0]);
    const size_t nemit = plan.emits.size();
    std::vector<MpsView> views;
    std::vector<int> lane_state;
    if (view_states(states, (size_t)nstates, n, views, lane_state)) return 1;
    std::vector<int> routes(views.size(), 0);
    bool any_fused = false;
    for (int s = 0; s < nstates; ++s) {
        const MpsView& v = views[lane_state[s]];
        int& route = routes[lane_state[s]];
        if (!route && (route = resolve_route(method, mps_obs_route(n, v.dims.data()), v.max_bond, kMpsObsFusedCap, "state", s)) < 0) return 1;
        any_fused = any_fused || route == kMpsObsFused;
    }
    MpsTable table;   // what the fused route reads of the states
    if (any_fused) {
        table = MpsTable({mps_table_words((size_t)n), mps_table_words((size_t)n + 2), mps_table_ints((size_t)n + 1)}, views.size());
        for (size_t k = 0; k < views.size(); ++k) {
            table.put(k, kSites, views[k].t, n);
            table.put(k, kEnvOff, mps_obs_env_offsets(n, views[k].dims.data()), n + 2);
            table.put(k, kDims, views[k].dims, n + 1);
        }
        if (table.upload()) return 1;
    }
    std::vector<std::unique_ptr<StateWork>> work;
    int rc = 0;
    for (int s = 0; s < nstates && !rc; ++s) {   // the work is per lane: a state listed twice is walked twice, its block written twice
        const size_t k = (size_t)lane_state[s];
        const MpsView& v = views[k];
        work.emplace_back(new StateWork());
        StateWork& w = *work.back();
        w.n = n;
        w.v = &v;
        w.off = mps_obs_env_offsets(n, v.dims.data());
        if (w.sums.alloc(nemit * kMpsObsComps * 4)) { rc = 1; break; }
        const bool fused = routes[k] == kMpsObsFused;
        rc = norm_environments(w.env, v, w.off, st, fused, kEnvLeft | kEnvRight, table.at<const double2*>(k, kSites), table.at<int>(k, kDims),
                               table.at<size_t>(k, kEnvOff)) ||
             (fused ? run_fused(w, plan, table, k, st) : run_gemm(w, plan, st));
        if (rc) break;
        w.h_sums.resize(nemit * kMpsObsComps * 4);
        if (hipMemcpyAsync(w.h_sums.data(), w.sums, sizeof(double2) * w.h_sums.size(), hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = failf("download of the sums failed");
    }
    if (finish_call(st, rc, "pair density matrices")) return 1;
    for (int s = 0; s < nstates; ++s)
        for (int p = 0; p < npairs; ++p) {
            double m[32];
            assemble(work[s]->h_sums.data() + (size_t)plan.pair_emit[p] * kMpsObsComps * 4, m);
            mps_obs_place(m, plan.pair_transposed[p], out + 32 * ((size_t)s * npairs + p));
        }
    return 0;
}

}  // extern "C"
