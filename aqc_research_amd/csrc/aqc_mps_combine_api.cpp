// C ABI (include/aqc_hip.h): linear combinations of single-lane MPS states, sum_k c_k psi_k compressed, many outputs per call.
// Rules: aqc_mps_combine_rule.h; the direct sums are assembled by aqc_mps_combine.hip, swept by what compression uses on both routes
// (aqc_mps_sweep.h).  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "aqc_mps_sum_call.h"

using namespace aqc;

namespace {

std::atomic<size_t> g_svd_budget{kMpsCallBudget};   // aqc_mps_combine_svd_budget: tests lower it to run many chunks on few outputs
enum { kSites, kDims };                              // the sections of a distinct state's record in Call::table

struct Call : SumCall {
    std::vector<MpsView> views;       // the distinct states, in order of first appearance
    std::vector<int> state_view;      // per listed state: index into views
    MpsTable table;                   // per distinct state: site pointers | dims
    DevBuf<int> d_term_view, d_block_off;
    DevBuf<double2> d_coeffs;
    DevBuf<size_t> d_site_off;
    DevBuf<MpsCombineOutput> d_outputs;
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
    for (size_t t = 0; t < terms; ++t) {
        term_view[t] = c.state_view[term_state[t]];
        cf[t] = make_double2(coeffs[2 * t], coeffs[2 * t + 1]);
    }
    size_t largest = 1;
    const size_t total = c.pack(block_off, site_off, &largest);
    if (c.table.upload() || c.d_term_view.upload(term_view) || c.d_coeffs.upload(cf) || c.d_block_off.upload(block_off) ||
        c.d_site_off.upload(site_off) || c.d_sums.alloc(total)) return 1;
    c.point_sites();
    std::vector<MpsCombineOutput> ho(nout);
    for (size_t j = 0; j < nout; ++j) {
        const SumOutput& o = c.outputs[j];
        ho[j] = MpsCombineOutput{c.d_term_view + o.first, c.d_coeffs + o.first, c.d_block_off + o.block_at, c.d_site_off + o.off_at, c.d_sums + o.asm_at, o.nterms};
    }
    if (c.d_outputs.upload(ho)) return 1;
    MpsCombineArgs a{c.table.dev, (int)c.table.layout.per, (int)c.table.layout.at[kSites], (int)c.table.layout.at[kDims], (int)c.views.size(), c.n, 0, c.d_outputs};
    HIP_OK(launch_mps_combine_assemble(a, (int)nout, largest, st));
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
    c.start(n, trunc_thr, max_bond);
    if ((size_t)nout * (size_t)std::max(c.cuts, 1) > (size_t)1 << 28) return failf("too many cuts in one call: %d outputs x %d cuts", nout, c.cuts);
    HIP_OK(hipSetDevice(device));
    if (view_states(states, (size_t)nstates, n, c.views, c.state_view)) return 1;
    c.outputs.resize(nout);
    for (int j = 0; j < nout; ++j) {
        const int nterms = term_off[j + 1] - term_off[j];
        std::vector<int> dims;
        for (int k = 0; k < nterms; ++k) {
            const std::vector<int>& d = c.views[c.state_view[term_state[term_off[j] + k]]].dims;
            dims.insert(dims.end(), d.begin(), d.end());
        }
        if (c.shape(j, term_off[j], nterms, dims.data(), mps_combine_max_bond(n, nterms, dims.data()), method, mps_combine_route(n, nterms, dims.data()))) return 1;
    }
    hipStream_t st = mps_stream(states[0]);
    const int rc = assemble(c, term_state, coeffs, st);
    return sum_sweep_and_adopt(c, rc, g_svd_budget.load(), st, device, trunc_thr, max_bond, "the linear combination", out, ranks, dropped, sweeps, status);
}

}  // extern "C"
