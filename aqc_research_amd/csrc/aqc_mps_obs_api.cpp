// C ABI (include/aqc_hip.h): pair density matrices of single-lane MPS states.  Rules: aqc_mps_obs_rule.h; kernels: aqc_mps_obs.hip.
#include <memory>
#include <vector>

#include "aqc_devbuf.h"
#include "aqc_mps_host.h"
#include "aqc_mps_obs_rule.h"

using namespace aqc;

namespace {

constexpr size_t kGroupBudget = (size_t)256 << 20;   // bytes of chain scratch a group of chains of the gemm route may take

// everything one state's launches read or write; alive until the call's last synchronisation
struct StateWork {
    int n = 0;
    std::vector<int> dims;
    std::vector<const double2*> t;
    std::vector<size_t> off;                          // env offsets, n + 2 entries (the last = total)
    DevBuf<double2> env_l, env_r, tmp, chains, close, sums;
    DevBuf<const double2*> d_sites;
    DevBuf<int> d_ints;
    DevBuf<size_t> d_off;
    DevBuf<void*> d_ptrs;
    std::vector<double2> h_sums;
};

// L_0 .. L_{n-1} and R_n .. R_1 of <psi|psi>; gemm route: with the engine's environment steps on the pair (psi, psi) (env_left / env_right of aqc_mps_host.h)
int environments(StateWork& w, hipStream_t st, bool fused) {
    const int n = w.n;
    const size_t total = w.off[n + 1];
    size_t tmax = 1;
    for (int q = 0; q < n; ++q) tmax = std::max(tmax, (size_t)w.dims[q] * w.dims[q + 1]);
    if (w.env_l.alloc(total) || w.env_r.alloc(total) || w.tmp.alloc(tmax)) return 1;
    static const double one[2] = {1.0, 0.0};
    HIP_OK(hipMemcpyAsync(w.env_l + w.off[0], one, sizeof one, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(w.env_r + w.off[n], one, sizeof one, hipMemcpyHostToDevice, st));
    if (fused) return 0;   // the fused route sweeps them on the matrix cores (run_fused)
    const int* dims = w.dims.data();
    for (int q = 0; q + 1 < n; ++q)
        if (env_left(st, w.env_l + w.off[q], w.t[q], w.t[q], site_dims(dims, dims, q), nullptr, nullptr, w.tmp, w.env_l + w.off[q + 1])) return 1;
    for (int q = n - 1; q >= 1; --q)
        if (env_right(st, w.env_r + w.off[q + 1], w.t[q], w.t[q], site_dims(dims, dims, q), w.tmp, w.env_r + w.off[q])) return 1;
    return 0;
}

int run_fused(StateWork& w, const MpsObsPlan& plan, hipStream_t st) {
    const int n = w.n;
    std::vector<int> ints;                                   // dims | chain_start | chain_last | emit_of
    ints.insert(ints.end(), w.dims.begin(), w.dims.end());
    std::vector<int> chain_of(n, -1), starts;
    for (int i = 0; i < n; ++i)
        if (plan.last[i] >= 0) { chain_of[i] = (int)starts.size(); starts.push_back(i); }
    const int nchains = (int)starts.size();
    ints.insert(ints.end(), starts.begin(), starts.end());
    for (int i : starts) ints.push_back(plan.last[i]);
    const size_t emit_at = ints.size();
    ints.resize(emit_at + (size_t)nchains * n, -1);
    for (size_t e = 0; e < plan.emits.size(); ++e) ints[emit_at + (size_t)chain_of[plan.emits[e].chain] * n + plan.emits[e].site] = (int)e;
    std::vector<const double2*> sites(w.t.begin(), w.t.end());
    if (w.d_ints.upload(ints) || w.d_sites.upload(sites) || w.d_off.upload(w.off)) return 1;
    MpsObsFusedArgs a;
    a.n = n;
    a.sites = w.d_sites;
    a.dims = w.d_ints;
    a.env_off = w.d_off;
    a.env_l = w.env_l;
    a.env_r = w.env_r;
    a.chain_start = w.d_ints + (n + 1);
    a.chain_last = w.d_ints + (n + 1) + nchains;
    a.emit_of = w.d_ints + emit_at;
    a.sums = w.sums;
    HIP_OK(launch_mps_obs_env(a, st));
    HIP_OK(launch_mps_obs_fused(a, nchains, st));
    return 0;
}

int run_gemm(StateWork& w, const MpsObsPlan& plan, hipStream_t st) {
    const int n = w.n;
    const int* dims = w.dims.data();
    const size_t S = mps_obs_slot_elems(n, dims);
    std::vector<int> starts;
    for (int i = 0; i < n; ++i)
        if (plan.last[i] >= 0) starts.push_back(i);
    const int nchains = (int)starts.size();
    const int gsize = mps_obs_group_size(n, dims, nchains, kGroupBudget);
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
            for (int k = 0; k < job.nstep; ++k) ptrs.push_back(const_cast<double2*>(w.t[q]));
            for (int k = 0; k < job.nstep; ++k) ptrs.push_back(const_cast<double2*>(w.t[q] + lr));
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
            const double2* t0 = w.t[q];
            const double2* t1 = t0 + lr;
            if (job.nemit) {   // K^{cd} = T_c (R_{q+1} T_d^H), components 00, 01, 11; then the sums of every chain that emits here
                const double2* r = w.env_r + w.off[q + 1];
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
                const double2* l = w.env_l + w.off[q];
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
    for (int s = 0; s < nstates; ++s)
        if (!states[s]) return failf("null state");
    const int n = aqc_mps_num_qubits(states[0]), device = aqc_mps_device(states[0]);
    if (n < 2) return failf("pair density matrices need at least 2 qubits");
    for (int s = 1; s < nstates; ++s)
        if (aqc_mps_num_qubits(states[s]) != n || aqc_mps_device(states[s]) != device) return failf("MPS states differ in size or device");
    MpsObsPlan plan;
    if (!mps_obs_plan(n, npairs, pairs, plan)) return failf("a pair needs two different qubits below %d", n);
    HIP_OK(hipSetDevice(device));
    hipStream_t st = mps_stream(states[0]);
    const size_t nemit = plan.emits.size();
    std::vector<std::unique_ptr<StateWork>> work;
    int rc = 0;
    for (int s = 0; s < nstates && !rc; ++s) {
        work.emplace_back(new StateWork());
        StateWork& w = *work.back();
        w.n = n;
        w.dims.resize(n + 1);
        w.t.resize(n);
        if (aqc_mps_dims(states[s], w.dims.data())) { rc = 1; break; }
        for (int q = 0; q < n && !rc; ++q) {   // (mps_peek drains the state's own stream: what aqc_mps_dot_ops does for its second operand)
            const void* site = nullptr;
            const double* lam = nullptr;
            rc = mps_peek(states[s], q, &site, &lam);
            w.t[q] = static_cast<const double2*>(site);
        }
        if (rc) break;
        w.off = mps_obs_env_offsets(n, w.dims.data());
        int route = method == kMpsObsByRule ? mps_obs_route(n, w.dims.data()) : method;
        if (route == kMpsObsFused && mps_obs_max_bond(n, w.dims.data()) > kMpsObsFusedCap) {
            rc = failf("the fused route takes bond dimensions up to %d; state %d has %d", (int)kMpsObsFusedCap, s, mps_obs_max_bond(n, w.dims.data()));
            break;
        }
        if (w.sums.alloc(nemit * kMpsObsComps * 4)) { rc = 1; break; }
        rc = environments(w, st, route == kMpsObsFused) || (route == kMpsObsFused ? run_fused(w, plan, st) : run_gemm(w, plan, st));
        if (rc) break;
        w.h_sums.resize(nemit * kMpsObsComps * 4);
        if (hipMemcpyAsync(w.h_sums.data(), w.sums, sizeof(double2) * w.h_sums.size(), hipMemcpyDeviceToHost, st) != hipSuccess)
            rc = failf("download of the sums failed");
    }
    const hipError_t e = hipStreamSynchronize(st);   // before any buffer goes, also after a failure
    if (rc) return 1;
    if (e != hipSuccess) return failf("pair density matrices failed: %s", hipGetErrorString(e));
    for (int s = 0; s < nstates; ++s)
        for (int p = 0; p < npairs; ++p) {
            double m[32];
            assemble(work[s]->h_sums.data() + (size_t)plan.pair_emit[p] * kMpsObsComps * 4, m);
            mps_obs_place(m, plan.pair_transposed[p], out + 32 * ((size_t)s * npairs + p));
        }
    return 0;
}

}  // extern "C"
