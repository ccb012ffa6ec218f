// C ABI (include/aqc_hip.h): linear combinations of single-lane MPS states, sum_k c_k psi_k compressed, many outputs per call.
// Rules: aqc_mps_combine_rule.h; the direct sums are assembled by aqc_mps_combine.hip, swept by what compression uses on both routes
// (aqc_mps_sweep.h).  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "aqc_mps_combine_rule.h"
#include "aqc_mps_sweep.h"

using namespace aqc;

namespace {

std::atomic<size_t> g_svd_budget{kMpsCallBudget};   // aqc_mps_combine_svd_budget: tests lower it to run many chunks on few outputs
constexpr long long kMaxSummedBond = 1 << 20;        // (block offsets are ints, a site of 2 Sigma^2 elements must fit the device)
enum { kSites, kDims };                              // the sections of a distinct state's record in Call::table

// one output: its terms as views of the call, the direct sum's shape, where it lies in the call's stores, what the sweep decides
struct Output : SweepWork {
    int route = 0, first = 0, nterms = 0;   // its terms: [first, first + nterms) of the call's term arrays
    std::vector<int> dims;                  // Sigma_0 .. Sigma_n
    std::vector<int> block_off;             // mps_combine_block_offsets
    std::vector<size_t> asm_off;            // mps_combine_site_offsets
    size_t asm_at = 0, block_at = 0, off_at = 0;
    std::vector<const double2*> sites;      // device pointers of the assembled sites
};

struct Call {
    int n = 0, cuts = 0;
    std::vector<MpsView> views;       // the distinct states, in order of first appearance
    std::vector<int> state_view;      // per listed state: index into views
    std::vector<Output> outputs;
    MpsTable table;                   // per distinct state: site pointers | dims
    DevBuf<int> d_term_view, d_block_off;
    DevBuf<double2> d_coeffs, d_sums;
    DevBuf<size_t> d_site_off;
    DevBuf<MpsCombineOutput> d_outputs;
    DevBuf<double> d_ones;            // canonical route: the unit bond vector of every bond
    FusedSweep sweep;                 // of the outputs on the fused route
};

// the direct sums of all outputs into c.d_sums: uploads and ONE launch
int assemble(Call& c, const int32_t* term_state, const double* coeffs, hipStream_t st) {
    const size_t n = (size_t)c.n, nout = c.outputs.size();
    c.table = MpsTable({mps_table_words(n), mps_table_ints(n + 1)}, c.views.size());
    for (size_t k = 0; k < c.views.size(); ++k) {
        c.table.put(k, kSites, c.views[k].t, n);
        c.table.put(k, kDims, c.views[k].dims, n + 1);
    }
    const size_t terms = (size_t)c.outputs.back().first + c.outputs.back().nterms;
    std::vector<int> term_view(terms), block_off;
    std::vector<double2> cf(terms);
    std::vector<size_t> site_off;
    size_t total = 0, largest = 1;
    for (size_t t = 0; t < terms; ++t) {
        term_view[t] = c.state_view[term_state[t]];
        cf[t] = make_double2(coeffs[2 * t], coeffs[2 * t + 1]);
    }
    for (Output& o : c.outputs) {
        o.block_at = block_off.size();
        block_off.insert(block_off.end(), o.block_off.begin(), o.block_off.end());
        o.off_at = site_off.size();
        site_off.insert(site_off.end(), o.asm_off.begin(), o.asm_off.end());
        o.asm_at = total;
        total += o.asm_off[n];
        for (size_t q = 0; q < n; ++q) largest = std::max(largest, o.asm_off[q + 1] - o.asm_off[q]);
    }
    if (c.table.upload() || c.d_term_view.upload(term_view) || c.d_coeffs.upload(cf) || c.d_block_off.upload(block_off) ||
        c.d_site_off.upload(site_off) || c.d_sums.alloc(total)) return 1;
    std::vector<MpsCombineOutput> ho(nout);
    for (size_t j = 0; j < nout; ++j) {
        Output& o = c.outputs[j];
        ho[j] = MpsCombineOutput{c.d_term_view + o.first, c.d_coeffs + o.first, c.d_block_off + o.block_at, c.d_site_off + o.off_at, c.d_sums + o.asm_at, o.nterms};
        o.sites.resize(n);
        for (size_t q = 0; q < n; ++q) o.sites[q] = c.d_sums + o.asm_at + o.asm_off[q];
    }
    if (c.d_outputs.upload(ho)) return 1;
    MpsCombineArgs a{c.table.dev, (int)c.table.layout.per, (int)c.table.layout.at[kSites], (int)c.table.layout.at[kDims], (int)c.views.size(), c.n, 0, c.d_outputs};
    HIP_OK(launch_mps_combine_assemble(a, (int)nout, largest, st));
    return 0;
}

// canonical route: the assembled sum as an engine state with unit bond vectors, then compression's canonical route on it
int run_canonical(Call& c, Output& o, int device, double trunc_thr, int max_bond, aqc_mps** made) {
    std::vector<const void*> sites(o.sites.begin(), o.sites.end());
    std::vector<const double*> lams(std::max(c.n - 1, 1), c.d_ones);
    aqc_mps* sum = nullptr;
    if (mps_adopt(device, c.n, o.dims.data(), sites.data(), lams.data(), 0.0, &sum)) return 1;
    MpsView v;
    v.h = sum;
    v.dims.resize(c.n + 1);
    v.t.resize(c.n);
    int rc = mps_view(sum, v.dims.data(), v.t.data());
    if (!rc) rc = sweep_canonical(v, trunc_thr, max_bond, o, made);
    (void)aqc_mps_destroy(sum);
    return rc;
}

// n = 1: the assembled site is the result; a sum that is zero or not finite fails as a spectrum would
int adopt_one_qubit(Call& c, int device, aqc_mps** out) {
    std::vector<double2> host(2 * c.outputs.size());
    HIP_OK(hipMemcpy(host.data(), c.d_sums, sizeof(double2) * host.size(), hipMemcpyDeviceToHost));
    const int dims[2] = {1, 1};
    for (size_t j = 0; j < c.outputs.size(); ++j) {
        Output& o = c.outputs[j];
        const double2 a = host[2 * j], b = host[2 * j + 1];
        const double norm2 = a.x * a.x + a.y * a.y + b.x * b.x + b.y * b.y;
        if (!(norm2 > 0.0) || !std::isfinite(norm2)) { o.status = kMpsCompressNonFinite; continue; }
        const void* site = o.sites[0];
        const double* none = nullptr;
        if (mps_adopt(device, 1, dims, &site, &none, 0.0, &out[j])) return 1;
    }
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_combine_route(int n, int nterms, const int32_t* dims) {
    if (!dims || n < 1 || nterms < 1) return -1;
    for (size_t i = 0; i < (size_t)nterms * (n + 1); ++i)
        if (dims[i] < 1) return -1;
    return mps_combine_route(n, nterms, dims);
}

int64_t aqc_mps_combine_svd_budget(int64_t bytes) {
    return swap_budget(g_svd_budget, bytes, kMpsCallBudget);
}

int aqc_mps_combine(aqc_mps* const* states, int nstates, int nout, const int32_t* term_off, const int32_t* term_state, const double* coeffs,
                    double trunc_thr, int max_bond, int method, aqc_mps** out, int32_t* ranks, double* dropped, int32_t* sweeps, int32_t* status) {
    if (check_truncating_call(states, out, nout, trunc_thr, max_bond, "output", mps_ent_method_ok(method), method)) return 1;
    if (!term_off || !term_state || !coeffs) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    switch (mps_combine_check_terms(nstates, nout, term_off, term_state)) {
        case 0: break;
        case 1: return failf("term_off must start at 0");
        case 2: return failf("every output needs at least one term (term_off must grow)");
        default: return failf("a term names a state outside the %d of the call", nstates);
    }
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    Call c;
    c.n = c.sweep.n = n;
    c.cuts = c.sweep.cuts = n - 1;
    c.sweep.trunc_thr = trunc_thr;
    c.sweep.max_bond = max_bond;
    if ((size_t)nout * (size_t)std::max(c.cuts, 1) > (size_t)1 << 28) return failf("too many cuts in one call: %d outputs x %d cuts", nout, c.cuts);
    HIP_OK(hipSetDevice(device));
    if (view_states(states, (size_t)nstates, n, c.views, c.state_view)) return 1;
    c.outputs.resize(nout);
    std::vector<SweepInput> in;
    std::vector<SweepWork*> work;
    std::vector<int> fused;
    bool canonical = false;
    int widest = 1;
    for (int j = 0; j < nout; ++j) {
        Output& o = c.outputs[j];
        o.first = term_off[j];
        o.nterms = term_off[j + 1] - term_off[j];
        std::vector<int> dims;
        for (int k = 0; k < o.nterms; ++k) {
            const std::vector<int>& d = c.views[c.state_view[term_state[o.first + k]]].dims;
            dims.insert(dims.end(), d.begin(), d.end());
        }
        const long long bond = mps_combine_max_bond(n, o.nterms, dims.data());
        if (bond > kMaxSummedBond) return failf("output %d: a summed bond dimension of %lld is beyond %lld", j, bond, kMaxSummedBond);
        if ((o.route = resolve_route(method, mps_combine_route(n, o.nterms, dims.data()), (int)bond, kMpsEntFusedCap, "output", j)) < 0) return 1;
        o.dims = mps_combine_dims(n, o.nterms, dims.data());
        o.block_off = mps_combine_block_offsets(n, o.nterms, dims.data());
        o.asm_off = mps_combine_site_offsets(n, o.nterms, dims.data());
        o.size(n, o.dims.data());
        widest = std::max(widest, (int)bond);
        if (o.route == kMpsEntFused && n > 1) {
            fused.push_back(j);
            c.sweep.k = std::max(c.sweep.k, (int)bond);
        } else if (n > 1) {
            canonical = true;
        }
    }
    hipStream_t st = mps_stream(states[0]);
    int rc = assemble(c, term_state, coeffs, st);
    if (!rc && !fused.empty()) {
        for (int j : fused) {
            in.push_back({c.outputs[j].sites.data(), c.outputs[j].dims.data()});
            work.push_back(&c.outputs[j]);
        }
        rc = c.sweep.run(in, work, g_svd_budget.load(), st);
    }
    if (finish_call(st, rc, "the linear combination")) return 1;   // the one synchronisation of the call
    for (size_t i = 0; i < fused.size(); ++i) c.sweep.collect(i, c.outputs[fused[i]]);
    if (n == 1) {
        if (adopt_one_qubit(c, device, out)) { drop_outputs(out, nout); return 1; }
    } else if (canonical && c.d_ones.upload(std::vector<double>(widest, 1.0))) {
        return 1;
    }
    for (int j = 0; j < nout; ++j) {
        Output& o = c.outputs[j];
        if (n > 1) {
            int bad = 0;
            if (o.route != kMpsEntFused) bad = run_canonical(c, o, device, trunc_thr, max_bond, &out[j]);
            else if (o.status == kMpsCompressOk) bad = c.sweep.adopt(o, device, 0.0, &out[j]);
            if (bad || (o.status == kMpsCompressOk && !out[j])) { drop_outputs(out, nout); return bad ? 1 : failf("the linear combination lost a state"); }
        }
        for (int q = 0; q < c.cuts; ++q) {
            const size_t at = (size_t)j * c.cuts + q;
            if (ranks) ranks[at] = o.ranks[q];
            if (dropped) dropped[at] = o.dropped[q];
            if (sweeps) sweeps[at] = o.sweeps[q];
        }
        if (status) status[j] = o.status;
    }
    return 0;
}

}  // extern "C"
