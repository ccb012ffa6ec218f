// C ABI (include/aqc_hip.h): whole programs of gates on single-lane MPS states, layer by layer, many states per call.
// Rules: aqc_mps_layers_rule.h; kernels: aqc_mps_layers.hip, the SVDs of a layer by the device-pointer core of aqc_svd_batch.hip.  The
// skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_layers_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsLayersByRule == kMpsByRule && kMpsLayersFused == kMpsFused, "resolve_route");
std::atomic<size_t> g_svd_budget{kMpsCallBudget};   // aqc_mps_apply_svd_budget: tests lower it to run many chunks on few states
enum { kSites, kLams, kDims };                      // the sections of a unit's record in Call::table

// a program after routing, with the numbers of every set of matrices (one set for all states, or one per listing)
struct Program {
    int n = 0, nsets = 1;
    std::vector<MpsLayersRouted> ops;
    MpsLayersPlan plan;
    std::vector<cd> opmats;   // [nsets][ops][16]
    std::vector<cd> gates;    // [nsets][folded gates][16]
    std::vector<cd> singles;  // [nsets][n][4]
    size_t ngates() const { return plan.gates.size(); }
    void fold() {
        gates.assign((size_t)nsets * std::max<size_t>(ngates(), 1) * 16, cd(0.0, 0.0));
        singles.assign((size_t)nsets * n * 4, cd(0.0, 0.0));
        for (int s = 0; s < nsets; ++s)
            mps_layers_fold(plan, ops, opmats.data() + (size_t)s * ops.size() * 16, gates.data() + (size_t)s * ngates() * 16, singles.data() + (size_t)s * n * 4);
    }
    const double* gate(int set, int g) const { return reinterpret_cast<const double*>(gates.data() + ((size_t)set * ngates() + g) * 16); }
    const double* single(int set, int q) const { return reinterpret_cast<const double*>(singles.data() + ((size_t)set * n + q) * 4); }
};

// one evolved state: a distinct input with one set of matrices
struct Unit {
    int view = 0, set = 0;
    int code = kMpsLayersOk, layer = -1, site = -1;
    std::vector<int> dims, sweeps;
    double dropped = 0.0;
    aqc_mps* made = nullptr;   // gatewise route: the evolved clone, handed to the unit's first lane
    int first_lane = -1;
};

struct Call {
    int n = 0, route = 0, max_bond = 0;
    double trunc_thr = 0.0;
    std::vector<MpsView> views;
    std::vector<int> lane_state, lane_unit;
    std::vector<Unit> units;
    std::vector<int> bounds;
    MpsTable table;
    BoundedStores stores;                  // the working copy of every unit, sized by the bounds
    DevBuf<double2> d_mats;
    DevBuf<double> d_dropped;
    DevBuf<int> d_plan, d_unit_set, d_bounds, d_dims, d_sweeps, d_fail;   // d_fail: failed | fail_code | fail_layer
    SvdChunk svd;                          // of 2 K x 2 K matrices, one per (gate, unit) of a chunk
    std::vector<int> h_dims, h_sweeps, h_fail;
    std::vector<double> h_dropped;
};

bool finite_matrix(const double* m, int count) {
    for (int i = 0; i < 2 * count; ++i)
        if (!std::isfinite(m[i])) return false;
    return true;
}

int run_fused(Call& c, const Program& p, hipStream_t st) {
    const size_t n = (size_t)c.n, units = c.units.size(), ngates = p.ngates(), bonds = std::max<size_t>(n - 1, 1);
    const int K = *std::max_element(c.bounds.begin(), c.bounds.end()), M = 2 * K;
    c.table = MpsTable({mps_table_words(n), mps_table_words(n), mps_table_ints(n + 1)}, units);
    std::vector<std::vector<const double*>> view_lams(c.views.size());
    for (size_t k = 0; k < c.views.size(); ++k) {
        view_lams[k].assign(n, nullptr);
        for (int q = 0; q + 1 < c.n; ++q) {
            const void* site = nullptr;
            if (mps_peek(c.views[k].h, q, &site, &view_lams[k][q])) return 1;
        }
    }
    std::vector<int> unit_set(units);
    for (size_t u = 0; u < units; ++u) {
        const MpsView& v = c.views[c.units[u].view];
        c.table.put(u, kSites, v.t, n);
        c.table.put(u, kLams, view_lams[c.units[u].view], n);
        c.table.put(u, kDims, v.dims, n + 1);
        unit_set[u] = c.units[u].set;
    }
    // the plan on the device: per layer the sites of its gates, then their indices in the program
    std::vector<int> plan_words;
    std::vector<size_t> layer_at;
    for (const std::vector<int>& layer : p.plan.layers) {
        layer_at.push_back(plan_words.size());
        for (int g : layer) plan_words.push_back(p.plan.gates[g].q);
        for (int g : layer) plan_words.push_back(g);
    }
    const size_t widest = p.plan.widest();
    const int chunk = widest ? mps_layers_chunk(K, widest * units, g_svd_budget.load()) : 0;
    std::vector<double2> mats(p.gates.size());
    memcpy(mats.data(), p.gates.data(), sizeof(double2) * mats.size());
    if (c.table.upload() || c.d_plan.upload(plan_words) || c.d_unit_set.upload(unit_set) || c.d_bounds.upload(c.bounds) || c.d_mats.upload(mats) ||
        c.stores.alloc(c.n, c.bounds.data(), units) || c.d_dims.alloc(units * (n + 1)) ||
        c.d_dropped.alloc(units * bonds) || c.d_sweeps.alloc(units * std::max<size_t>(ngates, 1)) || c.d_fail.alloc(units * (1 + 2 * bonds))) return 1;
    if (chunk && c.svd.alloc(chunk, M, M)) return 1;
    HIP_OK(hipMemsetAsync(c.d_dropped, 0, sizeof(double) * units * bonds, st));
    HIP_OK(hipMemsetAsync(c.d_sweeps, 0, sizeof(int) * units * std::max<size_t>(ngates, 1), st));
    HIP_OK(hipMemsetAsync(c.d_fail, 0, sizeof(int) * units * (1 + 2 * bonds), st));
    MpsLayersArgs a{};
    a.n = c.n; a.m = M; a.ngates = (int)ngates;
    a.mats = c.d_mats; a.unit_set = c.d_unit_set;
    a.table = c.table.dev; a.per = c.table.layout.per;
    a.at_sites = c.table.layout.at[kSites]; a.at_lams = c.table.layout.at[kLams]; a.at_dims = c.table.layout.at[kDims];
    a.site_off = c.stores.d_site_off(); a.lam_off = c.stores.d_lam_off(); a.bounds = c.d_bounds;
    a.site_total = c.stores.site_total; a.lam_total = c.stores.lam_total;
    a.sites = c.stores.sites; a.lam = c.stores.lam; a.dims = c.d_dims; a.dropped = c.d_dropped; a.sweeps = c.d_sweeps;
    a.failed = c.d_fail; a.fail_code = c.d_fail + units; a.fail_layer = c.d_fail + units * (1 + bonds);
    a.a = c.svd.a; a.u = c.svd.u; a.s = c.svd.s; a.vh = c.svd.vh;
    a.rows = c.svd.rows(); a.cols = c.svd.cols(); a.svd_sweeps = c.svd.sweeps(); a.svd_status = c.svd.status();
    a.trunc_thr = c.trunc_thr; a.max_bond = c.max_bond;
    HIP_OK(launch_mps_layer_load(a, (int)units, st));
    for (size_t l = 0; l < p.plan.layers.size(); ++l) {   // the chunks share the layer's stores: one stream orders them
        a.layer = (int)l;
        a.gates = (int)p.plan.layers[l].size();
        a.gate_q = c.d_plan + layer_at[l];
        a.gate_id = a.gate_q + a.gates;
        const size_t total = (size_t)a.gates * units;
        for (size_t first = 0; first < total; first += chunk) {
            const int count = (int)std::min<size_t>(chunk, total - first);
            a.first = (int)first;
            HIP_OK(launch_mps_layer_form(a, count, st));
            HIP_OK(c.svd.launch(count, st));
            HIP_OK(launch_mps_layer_split(a, count, st));
        }
    }
    for (size_t u = 0; u < units; ++u)   // the qubits that no 2-qubit op touches: their bonds are the input's
        for (int q = 0; q < c.n; ++q)
            if (p.plan.has_single[q]) {
                const MpsView& v = c.views[c.units[u].view];
                double2* site = c.stores.site(u, q);
                HIP_OK(launch_gate1q(site, site, 1, (size_t)v.dims[q] * v.dims[q + 1], 0, p.single(c.units[u].set, q), st));
            }
    c.h_dims.resize(units * (n + 1));
    c.h_sweeps.resize(units * std::max<size_t>(ngates, 1));
    c.h_fail.resize(units * (1 + 2 * bonds));
    c.h_dropped.resize(units * bonds);
    HIP_OK(hipMemcpyAsync(c.h_dims.data(), c.d_dims, sizeof(int) * c.h_dims.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.h_sweeps.data(), c.d_sweeps, sizeof(int) * c.h_sweeps.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.h_fail.data(), c.d_fail, sizeof(int) * c.h_fail.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.h_dropped.data(), c.d_dropped, sizeof(double) * c.h_dropped.size(), hipMemcpyDeviceToHost, st));
    return 0;
}

// what the one synchronisation brought back, per unit
int read_fused(Call& c, const Program& p) {
    const size_t n = (size_t)c.n, units = c.units.size(), ngates = p.ngates(), bonds = std::max<size_t>(n - 1, 1);
    for (size_t u = 0; u < units; ++u) {
        Unit& w = c.units[u];
        w.sweeps.assign(c.h_sweeps.begin() + u * std::max<size_t>(ngates, 1), c.h_sweeps.begin() + u * std::max<size_t>(ngates, 1) + ngates);
        const int failed = c.h_fail[u];
        if (failed) {   // the gates of the layer that failed it, the lowest site first
            const int* code = c.h_fail.data() + units + u * bonds;
            const int* layer = c.h_fail.data() + units * (1 + bonds) + u * bonds;
            for (size_t q = 0; q + 1 < n && w.code == kMpsLayersOk; ++q)
                if (code[q] && layer[q] == failed - 1) { w.code = code[q]; w.layer = layer[q]; w.site = (int)q; }
            if (w.code == kMpsLayersOk) return failf("a state failed without a reason");
            continue;
        }
        w.dims.assign(c.h_dims.begin() + u * (n + 1), c.h_dims.begin() + (u + 1) * (n + 1));
        if (!mps_layers_ranks_fit(c.n, c.bounds.data(), w.dims.data())) return failf("a rank passed its static bound");
        for (size_t q = 0; q + 1 < n; ++q) w.dropped += c.h_dropped[u * bonds + q];   // bond by bond, each summed layer by layer
    }
    return 0;
}

int adopt_fused(const Call& c, size_t u, int device, aqc_mps** out) {
    const Unit& w = c.units[u];
    return c.stores.adopt(device, c.n, u, w.dims.data(), aqc_mps_discarded_weight(c.views[w.view].h) + w.dropped, out);
}

// gatewise route: gate_adjacent in layer order on a clone, with the folded matrices; the engine reports an SVD at its sweep limit as an
// error of the gate, and so does this route: of the statuses it gives only 0 and 2
int run_gatewise(const Call& c, const Program& p, Unit& w) {
    const MpsView& v = c.views[w.view];
    const int n = c.n;
    std::vector<double2> host;
    for (int q = 0; q < n; ++q) {
        host.resize((size_t)2 * v.dims[q] * v.dims[q + 1]);
        HIP_OK(hipMemcpy(host.data(), v.t[q], sizeof(double2) * host.size(), hipMemcpyDeviceToHost));
        for (const double2& x : host)
            if (!(std::isfinite(x.x) && std::isfinite(x.y))) { w.code = kMpsLayersNonFinite; w.layer = 0; w.site = std::min(q, std::max(n - 2, 0)); return 0; }
    }
    aqc_mps* m = nullptr;
    if (aqc_mps_clone(v.h, &m)) return 1;
    const double before = aqc_mps_discarded_weight(m);
    for (size_t l = 0; l < p.plan.layers.size(); ++l)
        for (int g : p.plan.layers[l]) {
            const int q = p.plan.gates[g].q;
            if (!aqc_mps_gate2(m, q, q + 1, p.gate(w.set, g), c.trunc_thr, c.max_bond)) continue;
            (void)aqc_mps_destroy(m);
            if (!strstr(aqc_last_error(), "zero or non-finite")) return 1;
            w.code = kMpsLayersNonFinite; w.layer = (int)l; w.site = q;
            return 0;
        }
    for (int q = 0; q < n; ++q)
        if (p.plan.has_single[q] && aqc_mps_gate1(m, q, p.single(w.set, q))) { (void)aqc_mps_destroy(m); return 1; }
    w.dims.resize(n + 1);
    if (aqc_mps_dims(m, w.dims.data())) { (void)aqc_mps_destroy(m); return 1; }
    w.dropped = aqc_mps_discarded_weight(m) - before;
    w.sweeps.assign(p.ngates(), 0);
    w.made = m;
    return 0;
}

// a failed call: the outputs and the gatewise route's clones that no lane has taken
void drop_outputs(Call& c, aqc_mps** out, int nstates) {
    drop_outputs(out, nstates);
    for (Unit& w : c.units) {
        if (w.made) (void)aqc_mps_destroy(w.made);
        w.made = nullptr;
    }
}

int check_call(aqc_mps* const* states, int nstates, aqc_mps** out, double trunc_thr, int max_bond, int method) {
    return check_truncating_call(states, out, nstates, trunc_thr, max_bond, "state", mps_layers_method_ok(method), method);
}

// the route of the call: the method, or the rule's choice; the fused route refuses what the rule does not allow
int call_route(const Call& c, int method) {
    int rule = kMpsLayersFused;
    for (size_t k = 0; k < c.views.size(); ++k) {
        if (mps_layers_route(c.n, c.views[k].dims.data(), c.max_bond) == kMpsLayersFused) continue;
        rule = kMpsLayersGatewise;
        if (method != kMpsLayersFused) continue;
        if (resolve_route(method, rule, c.views[k].max_bond, kMpsLayersCap, "state", (int)k) < 0) return -1;
        failf("the fused route takes bond dimensions up to %d; with max_bond %d a bond of %d qubits can reach %d", (int)kMpsLayersCap, c.max_bond, c.n,
              mps_layers_natural(c.n, c.n / 2, c.max_bond));
        return -1;
    }
    return method == kMpsLayersByRule ? rule : method;
}

// the program is set (ops, plan, opmats); states checked by check_call
int run_program(Program& p, aqc_mps* const* states, int nstates, int n, int device, double trunc_thr, int max_bond, int method, aqc_mps** out,
                int32_t* ranks, double* dropped, int32_t* sweeps, int32_t* status) {
    Call c;
    c.n = n;
    c.trunc_thr = trunc_thr;
    c.max_bond = max_bond;
    if ((size_t)nstates * std::max<size_t>(p.ngates(), 1) > (size_t)1 << 28) return failf("too many gates in one call: %d states x %zu gates", nstates, p.ngates());
    if (p.plan.widest() * (size_t)nstates > (size_t)1 << 30) return failf("too many gates in one layer");
    HIP_OK(hipSetDevice(device));
    if (view_states(states, (size_t)nstates, n, c.views, c.lane_state)) return 1;
    if ((c.route = call_route(c, method)) < 0) return 1;
    c.lane_unit.resize(nstates);
    for (int i = 0; i < nstates; ++i) {
        if (p.nsets > 1) {   // matrices per state: every listing is its own lane
            c.lane_unit[i] = (int)c.units.size();
            c.units.push_back(Unit{});
            c.units.back().view = c.lane_state[i];
            c.units.back().set = i;
        } else {
            if ((size_t)c.lane_state[i] == c.units.size()) {
                c.units.push_back(Unit{});
                c.units.back().view = c.lane_state[i];
            }
            c.lane_unit[i] = c.lane_state[i];
        }
    }
    p.fold();
    if (c.route == kMpsLayersFused) {
        c.bounds = mps_layers_bounds(n, max_bond, nullptr);
        for (const MpsView& v : c.views) {
            const std::vector<int> b = mps_layers_bounds(n, max_bond, v.dims.data());
            for (int q = 0; q <= n; ++q) c.bounds[q] = std::max(c.bounds[q], b[q]);
        }
        hipStream_t st = mps_stream(states[0]);
        if (finish_call(st, run_fused(c, p, st), "gate layers")) return 1;   // the one synchronisation of the call
        if (read_fused(c, p)) return 1;
    } else {
        for (Unit& w : c.units)
            if (run_gatewise(c, p, w)) { drop_outputs(c, out, nstates); return 1; }
    }
    const size_t ngates = p.ngates();
    for (int i = 0; i < nstates; ++i) {
        Unit& w = c.units[c.lane_unit[i]];
        if (w.code == kMpsLayersOk) {
            int rc = 0;
            if (c.route == kMpsLayersFused) rc = adopt_fused(c, (size_t)c.lane_unit[i], device, &out[i]);
            else if (w.made) { out[i] = w.made; w.made = nullptr; w.first_lane = i; }
            else rc = aqc_mps_clone(out[w.first_lane], &out[i]);   // a later listing of the unit: a copy of the lane that took the clone
            if (rc || !out[i]) { drop_outputs(c, out, nstates); return rc ? 1 : failf("gate layers lost a state"); }
        }
        for (int q = 0; q <= n && ranks; ++q) ranks[(size_t)i * (n + 1) + q] = w.code == kMpsLayersOk ? w.dims[q] : 0;
        if (dropped) dropped[i] = w.dropped;
        for (size_t g = 0; g < ngates && sweeps; ++g) sweeps[(size_t)i * ngates + g] = g < w.sweeps.size() ? w.sweeps[g] : 0;
        if (status) { status[3 * i] = w.code; status[3 * i + 1] = w.layer; status[3 * i + 2] = w.site; }
    }
    return 0;
}

// the ops of the ABI, checked: -1 after a message
int read_ops(int n, int nops, const int32_t* qubits, const int32_t* kinds, std::vector<MpsLayersOp>& ops) {
    if (nops < 0 || (nops > 0 && (!qubits || !kinds))) return failf("null argument");
    ops.resize(nops);
    for (int i = 0; i < nops; ++i) {
        const int a = qubits[2 * i], b = qubits[2 * i + 1];
        if (kinds[i] != 1 && kinds[i] != 2) return failf("op %d: kind must be 1 or 2", i);
        if (a < 0 || a >= n || (kinds[i] == 2 && (b < 0 || b >= n))) return failf("op %d: qubit out of range", i);
        if (kinds[i] == 2 && a == b) return failf("op %d: invalid qubit pair", i);
        ops[i] = {kinds[i] == 2, a, kinds[i] == 2 ? b : a};
    }
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_apply_route(int n, const int32_t* dims, int max_bond) {
    if (n < 1 || max_bond < 0) return -1;
    for (int q = 0; dims && q <= n; ++q)
        if (dims[q] < 1) return -1;
    return mps_layers_route(n, dims, max_bond);
}

int64_t aqc_mps_apply_svd_budget(int64_t bytes) {
    return swap_budget(g_svd_budget, bytes, kMpsCallBudget);
}

int aqc_mps_apply_plan(int n, int nops, const int32_t* qubits, const int32_t* kinds, int32_t* counts, int32_t* gate_sites, int32_t* gate_layers) {
    if (n < 1 || !counts) return failf("null argument");
    std::vector<MpsLayersOp> ops;
    if (read_ops(n, nops, qubits, kinds, ops)) return 1;
    const MpsLayersPlan plan = mps_layers_plan(n, mps_layers_route_ops(ops));
    counts[0] = (int32_t)plan.layers.size();
    counts[1] = (int32_t)plan.gates.size();
    for (size_t g = 0; g < plan.gates.size(); ++g) {
        if (gate_sites) gate_sites[g] = plan.gates[g].q;
        if (gate_layers) gate_layers[g] = plan.gates[g].layer;
    }
    return 0;
}

int aqc_mps_apply_gates(aqc_mps* const* states, int nstates, int nops, const int32_t* qubits, const int32_t* kinds, const double* mats, int per_state,
                        double trunc_thr, int max_bond, int method, aqc_mps** out, int32_t* ranks, double* dropped, int32_t* sweeps, int32_t* status) {
    if (check_call(states, nstates, out, trunc_thr, max_bond, method)) return 1;
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    std::vector<MpsLayersOp> ops;
    if (read_ops(n, nops, qubits, kinds, ops)) return 1;
    if (nops > 0 && !mats) return failf("null argument");
    Program p;
    p.n = n;
    p.nsets = per_state ? nstates : 1;
    p.ops = mps_layers_route_ops(ops);
    p.plan = mps_layers_plan(n, p.ops);
    std::vector<size_t> at(nops + 1, 0);   // doubles in front of op i in a set of the caller's matrices
    for (int i = 0; i < nops; ++i) at[i + 1] = at[i] + (ops[i].two ? 32 : 8);
    if ((size_t)p.nsets * p.ops.size() > (size_t)1 << 26) return failf("too many ops in one call");
    p.opmats.assign((size_t)p.nsets * p.ops.size() * 16, cd(0.0, 0.0));
    static const double swap_gate[32] = {1, 0, 0, 0, 0, 0, 0, 0,  0, 0, 0, 0, 1, 0, 0, 0,  0, 0, 1, 0, 0, 0, 0, 0,  0, 0, 0, 0, 0, 0, 1, 0};
    for (int s = 0; s < p.nsets; ++s) {
        const double* set = mats + (size_t)s * at[nops];
        for (int i = 0; i < nops; ++i)
            if (!finite_matrix(set + at[i], ops[i].two ? 16 : 4)) return failf("op %d: the matrix is not finite", i);
        for (size_t r = 0; r < p.ops.size(); ++r) {
            const MpsLayersRouted& op = p.ops[r];
            double* dst = reinterpret_cast<double*>(p.opmats.data() + ((size_t)s * p.ops.size() + r) * 16);
            if (!op.two) memcpy(dst, set + at[op.src], sizeof(double) * 8);
            else if (op.swap) memcpy(dst, swap_gate, sizeof swap_gate);
            else permute_gate(set + at[op.src], op.flip != 0, dst);
        }
    }
    return run_program(p, states, nstates, n, device, trunc_thr, max_bond, method, out, ranks, dropped, sweeps, status);
}

int aqc_mps_apply_circuit_many(const aqc_circuit* circ, const double* thetas, int num_thetas, int per_state, aqc_mps* const* states, int nstates, int inverse,
                               double trunc_thr, int max_bond, int method, aqc_mps** out, int32_t* ranks, double* dropped, int32_t* sweeps, int32_t* status) {
    if (check_call(states, nstates, out, trunc_thr, max_bond, method)) return 1;
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    if (!thetas || num_thetas < 0) return failf("null argument");
    if (check_circuit(circ, n)) return 1;
    const int sets = per_state ? nstates : 1;
    for (size_t i = 0; i < (size_t)sets * num_thetas; ++i)
        if (!std::isfinite(thetas[i])) return failf("theta %zu is not finite", i);
    const std::vector<CircuitOp> cops = circuit_ops(circ, n, inverse != 0);
    Program p;
    p.n = n;
    p.nsets = sets;
    for (size_t i = 0; i < cops.size(); ++i) p.ops.push_back(cops[i].two ? MpsLayersRouted{1, cops[i].op2.q, (int)i, cops[i].op2.g.kind == 0, cops[i].op2.g.flip} : MpsLayersRouted{0, cops[i].op1.q, (int)i, 0, 0});
    p.plan = mps_layers_plan(n, p.ops);
    if ((size_t)p.nsets * p.ops.size() > (size_t)1 << 26) return failf("too many ops in one call");
    p.opmats.assign((size_t)p.nsets * p.ops.size() * 16, cd(0.0, 0.0));
    for (int s = 0; s < sets; ++s) {
        const double* th = thetas + (size_t)s * num_thetas;
        for (size_t i = 0; i < cops.size(); ++i) {
            double* dst = reinterpret_cast<double*>(p.opmats.data() + ((size_t)s * cops.size() + i) * 16);
            if (cops[i].two) gate2_matrix(cops[i].op2.g, th, dst);
            else pack(gate1_matrix(cops[i].op1.g, th), dst);
        }
    }
    return run_program(p, states, nstates, n, device, trunc_thr, max_bond, method, out, ranks, dropped, sweeps, status);
}

int aqc_mps_apply_circuit_plan(const aqc_circuit* circ, int inverse, int32_t* counts) {
    if (!circ || !counts) return failf("null argument");
    const int n = circ->num_qubits;
    if (n < 1 || check_circuit(circ, n)) return n < 1 ? failf("number of qubits out of range") : 1;
    std::vector<MpsLayersRouted> ops;
    for (const CircuitOp& op : circuit_ops(circ, n, inverse != 0)) ops.push_back(op.two ? MpsLayersRouted{1, op.op2.q, 0, 0, 0} : MpsLayersRouted{0, op.op1.q, 0, 0, 0});
    const MpsLayersPlan plan = mps_layers_plan(n, ops);
    counts[0] = (int32_t)plan.layers.size();
    counts[1] = (int32_t)plan.gates.size();
    return 0;
}

}  // extern "C"
