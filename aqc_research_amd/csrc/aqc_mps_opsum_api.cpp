// C ABI (include/aqc_hip.h): operator sums on single-lane MPS states, sum_t c_t O_t psi_t compressed (O_t an MPO or absent), many
// outputs per call.  Rules: aqc_mps_opsum_rule.h; the direct sums of the product terms are assembled by aqc_mps_opsum.hip, swept by
// what compression uses on both routes (aqc_mps_sweep.h); the call shares its scaffolding with linear combinations
// (aqc_mps_sum_call.h).  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "aqc_mps_opsum_rule.h"
#include "aqc_mps_sum_call.h"

using namespace aqc;

namespace {

std::atomic<size_t> g_svd_budget{kMpsCallBudget};   // aqc_mps_opsum_svd_budget: tests lower it to run many chunks on few outputs
enum { kSites, kDims };                              // the sections of a distinct state's record in Call::table

struct Call : SumCall {
    std::vector<MpsView> views;       // the distinct states, in order of first appearance
    std::vector<int> state_view;      // per listed state: index into views
    std::vector<int> term_chi;        // [terms][n + 1] the bonds of every term's state
    MpsTable table;                   // per distinct state: site pointers | dims
    DevBuf<unsigned long long> d_ops; // site offsets | dims | data of the call's operators
    DevBuf<int> d_term_view, d_term_op, d_block_off, d_term_chi;
    DevBuf<double2> d_coeffs;
    DevBuf<size_t> d_site_off;
    DevBuf<MpsOpsumOutput> d_outputs;
};

// the direct sums of all outputs into c.d_sums: uploads and ONE launch
int assemble(Call& c, int nops, const int32_t* op_dims, const int64_t* op_site_off, const double* op_data, size_t op_elems, const int32_t* term_state,
             const int32_t* term_op, const double* coeffs, hipStream_t st) {
    const size_t n = (size_t)c.n, nout = c.outputs.size();
    c.table = MpsTable({mps_table_words(n), mps_table_ints(n + 1)}, c.views.size());
    for (size_t k = 0; k < c.views.size(); ++k) {
        c.table.put(k, kSites, c.views[k].t, n);
        c.table.put(k, kDims, c.views[k].dims, n + 1);
    }
    // the operators: site offsets (words) | dims (ints) | data from an even word on (16-byte aligned complex elements)
    const size_t entries = (size_t)nops * (n + 1), at_dims = entries, at_data = (at_dims + (entries + 1) / 2 + 1) & ~(size_t)1;
    std::vector<unsigned long long> ops(at_data + 2 * op_elems, 0);
    for (size_t i = 0; i < entries; ++i) ops[i] = (unsigned long long)op_site_off[i];
    if (entries) memcpy(ops.data() + at_dims, op_dims, entries * sizeof(int32_t));
    if (op_elems) memcpy(ops.data() + at_data, op_data, op_elems * 2 * sizeof(double));
    const size_t terms = (size_t)c.outputs.back().first + c.outputs.back().nterms;
    std::vector<int> term_view(terms), ops_of(term_op, term_op + terms), block_off;
    std::vector<double2> cf(terms);
    std::vector<size_t> site_off;
    for (size_t t = 0; t < terms; ++t) {
        term_view[t] = c.state_view[term_state[t]];
        cf[t] = make_double2(coeffs[2 * t], coeffs[2 * t + 1]);
    }
    size_t largest = 1;
    const size_t total = c.pack(block_off, site_off, &largest);
    if (c.table.upload() || c.d_ops.upload(ops, 2) || c.d_term_view.upload(term_view) || c.d_term_op.upload(ops_of) || c.d_coeffs.upload(cf) ||
        c.d_block_off.upload(block_off) || c.d_term_chi.upload(c.term_chi) || c.d_site_off.upload(site_off) || c.d_sums.alloc(total)) return 1;
    c.point_sites();
    std::vector<MpsOpsumOutput> ho(nout);
    for (size_t j = 0; j < nout; ++j) {
        const SumOutput& o = c.outputs[j];
        ho[j] = MpsOpsumOutput{c.d_term_view + o.first, c.d_term_op + o.first, c.d_coeffs + o.first, c.d_block_off + o.block_at,
                               c.d_term_chi + (size_t)o.first * (n + 1), c.d_site_off + o.off_at, c.d_sums + o.asm_at, o.nterms};
    }
    if (c.d_outputs.upload(ho)) return 1;
    MpsOpsumArgs a{c.table.dev, (int)c.table.layout.per, (int)c.table.layout.at[kSites], (int)c.table.layout.at[kDims], (int)c.views.size(), c.n, 0,
                   c.d_ops, nops, at_dims, at_data, op_elems, c.d_outputs};
    HIP_OK(launch_mps_opsum_assemble(a, (int)nout, largest, st));
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_opsum_route(int n, int nterms, const int32_t* state_dims, const int32_t* op_dims) {
    if (!state_dims || !op_dims || n < 1 || nterms < 1) return -1;
    for (size_t i = 0; i < (size_t)nterms * (n + 1); ++i)
        if (state_dims[i] < 1 || op_dims[i] < 1) return -1;
    return mps_opsum_route(n, nterms, state_dims, op_dims);
}

int64_t aqc_mps_opsum_svd_budget(int64_t bytes) {
    return swap_budget(g_svd_budget, bytes, kMpsCallBudget);
}

int aqc_mps_opsum(aqc_mps* const* states, int nstates, int nops, const int32_t* op_dims, const int64_t* op_site_off, const double* op_data, int nout,
                  const int32_t* term_off, const int32_t* term_state, const int32_t* term_op, const double* coeffs, double trunc_thr, int max_bond, int method,
                  aqc_mps** out, int32_t* ranks, double* dropped, int32_t* sweeps, int32_t* status) {
    if (check_truncating_call(states, out, nout, trunc_thr, max_bond, "output", mps_ent_method_ok(method), method)) return 1;
    if (!term_off || !term_state || !term_op || !coeffs) return failf("null argument");
    if (nops < 0 || (nops > 0 && (!op_dims || !op_site_off || !op_data))) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    switch (mps_opsum_check_terms(nstates, nops, nout, term_off, term_state, term_op)) {
        case 0: break;
        case 1: return failf("term_off must start at 0");
        case 2: return failf("every output needs at least one term (term_off must grow)");
        case 3: return failf("a term names a state outside the %d of the call", nstates);
        default: return failf("a term names an operator outside the %d of the call", nops);
    }
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    long long op_elems = 0;
    for (int o = 0; o < nops; ++o) {
        const std::vector<long long> off(op_site_off + (size_t)o * (n + 1), op_site_off + (size_t)(o + 1) * (n + 1));
        const int bad = mps_opsum_check_op(n, op_dims + (size_t)o * (n + 1), off.data());
        if (bad == 1) return failf("operator %d: the bond dimensions of an operator on %d qubits are at least 1, the first and the last 1", o, n);
        if (bad) return failf("operator %d: the site offsets are not the packed layout of its bond dimensions", o);
        op_elems = std::max(op_elems, (long long)op_site_off[(size_t)o * (n + 1) + n]);
    }
    Call c;
    c.start(n, trunc_thr, max_bond);
    if ((size_t)nout * (size_t)std::max(c.cuts, 1) > (size_t)1 << 28) return failf("too many cuts in one call: %d outputs x %d cuts", nout, c.cuts);
    HIP_OK(hipSetDevice(device));
    if (view_states(states, (size_t)nstates, n, c.views, c.state_view)) return 1;
    c.outputs.resize(nout);
    const std::vector<int> ones(n + 1, 1);
    for (int j = 0; j < nout; ++j) {
        const int nterms = term_off[j + 1] - term_off[j];
        std::vector<int> chi, dop;
        for (int k = 0; k < nterms; ++k) {
            const int t = term_off[j] + k;
            const std::vector<int>& d = c.views[c.state_view[term_state[t]]].dims;
            const int* w = term_op[t] < 0 ? ones.data() : op_dims + (size_t)term_op[t] * (n + 1);
            chi.insert(chi.end(), d.begin(), d.end());
            dop.insert(dop.end(), w, w + n + 1);
        }
        const long long bond = mps_opsum_max_bond(n, nterms, chi.data(), dop.data());
        if (bond > kMaxSummedBond) return failf("output %d: a summed product bond dimension of %lld is beyond %lld", j, bond, kMaxSummedBond);
        std::vector<int> widths(chi.size());   // (every product bond is at most their sum: it fits an int)
        for (int k = 0; k < nterms; ++k) {
            const size_t at = (size_t)k * (n + 1);
            mps_opsum_term_dims(n, chi.data() + at, dop.data() + at, nullptr, widths.data() + at);
        }
        if (c.shape(j, term_off[j], nterms, widths.data(), bond, method, mps_opsum_route(n, nterms, chi.data(), dop.data()))) return 1;
        c.term_chi.insert(c.term_chi.end(), chi.begin(), chi.end());
    }
    hipStream_t st = mps_stream(states[0]);
    const int rc = assemble(c, nops, op_dims, op_site_off, op_data, (size_t)op_elems, term_state, term_op, coeffs, st);
    return sum_sweep_and_adopt(c, rc, g_svd_budget.load(), st, device, trunc_thr, max_bond, "the operator sum", out, ranks, dropped, sweeps, status);
}

}  // extern "C"
