// C ABI (include/aqc_hip.h): matrix elements of operators between single-lane MPS states, <phi|O|psi> for many (bra, operator, ket)
// jobs per call.  Rules: aqc_mps_melem_rule.h; kernels: aqc_mps_melem.hip.  The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_melem_rule.h"
#include "aqc_mps_opsum_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsMelemByRule == kMpsByRule && kMpsMelemFused == kMpsFused, "resolve_route");
std::atomic<size_t> g_budget{kMpsMelemBudget};   // aqc_mps_melem_budget: tests lower it to run many groups on few jobs
enum { kSites, kDims };                          // the sections of a distinct state's record in Call::table
constexpr int kMaxOpBond = 16384;                // (2 D slots are one grid dimension of the combining kernel)

// the lists of the rule header for every site of one operator (the call's last operator is the identity)
struct OpLists {
    std::vector<int> dims, ent_off, mask_off, mask, slot_off;
    std::vector<MpsMelemEntry> ent, by_slot;
    // what the host reads per site on the gemm route: the (a, s') that have entries, in order
    std::vector<std::vector<std::pair<int, int>>> pairs;
};
OpLists op_lists(int n, const int* dims, const double* data, const int64_t* site_off) {
    OpLists o;
    o.dims.assign(n + 1, 1);
    if (dims) o.dims.assign(dims, dims + n + 1);
    o.ent_off.assign(n + 1, 0);
    o.mask_off.assign(n + 1, 0);
    o.pairs.resize(n);
    for (int q = 0; q < n; ++q) {
        std::vector<int> mask;
        const size_t at = o.ent.size();
        mps_melem_entries(o.dims[q], o.dims[q + 1], data ? data + 2 * site_off[q] : nullptr, o.ent, mask);
        o.mask.insert(o.mask.end(), mask.begin(), mask.end());
        o.ent_off[q + 1] = (int)o.ent.size();
        o.mask_off[q + 1] = (int)o.mask.size();
        const int slots = 2 * o.dims[q + 1];
        for (int slot = 0; slot < slots; ++slot) {   // those of a slot together, in the order of the list
            o.slot_off.push_back((int)o.by_slot.size());
            for (size_t e = at; e < o.ent.size(); ++e)
                if (2 * o.ent[e].b + o.ent[e].s == slot) o.by_slot.push_back(o.ent[e]);
        }
        o.slot_off.push_back((int)o.by_slot.size());
        for (size_t e = at; e < o.ent.size(); ++e)
            if (o.pairs[q].empty() || o.pairs[q].back() != std::make_pair(o.ent[e].a, o.ent[e].sp)) o.pairs[q].emplace_back(o.ent[e].a, o.ent[e].sp);
    }
    return o;
}

struct Job { int bra, ket, op, index; };   // views of bra and ket, the operator (nops: the identity), the job's place in the output

// one walk of the gemm route: the jobs of the call that share bonds and operator
struct WalkWork {
    DevBuf<void*> d_ptrs;
};

struct Call {
    int n = 0, njobs = 0;
    std::vector<MpsView> views;       // distinct, in order of first appearance
    std::vector<OpLists> ops;         // the call's operators, then the identity
    std::vector<Job> jobs;
    std::vector<std::unique_ptr<WalkWork>> walks;
    MpsTable table;                   // per distinct state: site pointers | dims
    DevBuf<int> d_ints;               // per operator: dims | ent_off | mask_off | mask | slot_off
    DevBuf<MpsMelemEntry> d_ent;      // per operator: ent | by_slot
    DevBuf<MpsMelemOp> d_ops;
    DevBuf<MpsMelemJob> d_jobs;
    DevBuf<double2> d_out, d_one, d_scratch;
};

int upload_ops(Call& c) {
    std::vector<int> ints;
    std::vector<MpsMelemEntry> ent;
    std::vector<size_t> int_at, ent_at;
    for (const OpLists& o : c.ops) {
        int_at.push_back(ints.size());
        ent_at.push_back(ent.size());
        for (const std::vector<int>* v : {&o.dims, &o.ent_off, &o.mask_off, &o.mask, &o.slot_off}) ints.insert(ints.end(), v->begin(), v->end());
        ent.insert(ent.end(), o.ent.begin(), o.ent.end());
        ent.insert(ent.end(), o.by_slot.begin(), o.by_slot.end());
    }
    if (c.d_ints.upload(ints) || c.d_ent.upload(ent)) return 1;
    std::vector<MpsMelemOp> ho;
    for (size_t k = 0; k < c.ops.size(); ++k) {
        const OpLists& o = c.ops[k];
        const int* base = c.d_ints + int_at[k];
        const size_t w = (size_t)c.n + 1;
        MpsMelemOp d{};
        d.dims = base;
        d.ent_off = base + w;
        d.mask_off = base + 2 * w;
        d.mask = base + 3 * w;
        d.slot_off = d.mask + o.mask.size();
        d.ent = c.d_ent + ent_at[k];
        d.ent_by_slot = d.ent + o.ent.size();
        ho.push_back(d);
    }
    return c.d_ops.upload(ho);
}

const int* dims_of(const Call& c, int view) { return c.views[view].dims.data(); }

// The scratch of a call: ONE buffer (Call::d_scratch) that the groups of the fused launch and of every gemm walk use one after the
// other -- the stream is in order -- so a call holds at most `budget` bytes of it whatever the number of walks.  A plan is the slice
// of one job and the jobs of a group; the fused launch sizes its slices by the largest E set and G set among its jobs
struct ScratchPlan { size_t e_elems = 1, g_elems = 1, job_elems = 1, gsize = 1; };
ScratchPlan plan_fused(const Call& c, const std::vector<int>& fused, size_t budget) {
    ScratchPlan p;
    for (int j : fused) {
        const Job& job = c.jobs[j];
        const int* od = c.ops[job.op].dims.data();
        p.e_elems = std::max(p.e_elems, mps_melem_e_elems(c.n, dims_of(c, job.bra), dims_of(c, job.ket), od));
        p.g_elems = std::max(p.g_elems, mps_melem_g_elems(c.n, dims_of(c, job.bra), dims_of(c, job.ket), od));
    }
    p.job_elems = 2 * p.e_elems + p.g_elems;   // (within the caps: at most 4 * 32 * 64 * 64)
    p.gsize = (size_t)mps_melem_group_size(p.job_elems, fused.size(), budget);
    return p;
}
ScratchPlan plan_gemm(const Call& c, const std::vector<int>& members, size_t budget) {
    const Job& head = c.jobs[members[0]];
    const int* od = c.ops[head.op].dims.data();
    ScratchPlan p;
    p.e_elems = mps_melem_e_elems(c.n, dims_of(c, head.bra), dims_of(c, head.ket), od);
    p.g_elems = mps_melem_g_elems(c.n, dims_of(c, head.bra), dims_of(c, head.ket), od);
    p.job_elems = mps_melem_job_elems(c.n, dims_of(c, head.bra), dims_of(c, head.ket), od, true);
    p.gsize = (size_t)mps_melem_group_size(p.job_elems, members.size(), budget);
    return p;
}

// the fused jobs in groups whose scratch stays below the budget, one launch per group
int run_fused(Call& c, const std::vector<int>& fused, const ScratchPlan& plan, hipStream_t st) {
    std::vector<MpsMelemJob> hj;
    const size_t e_elems = plan.e_elems, job_elems = plan.job_elems, gsize = plan.gsize;
    for (int j : fused) {
        const Job& job = c.jobs[j];
        hj.push_back(MpsMelemJob{c.table.at<const double2*>(job.bra, kSites), c.table.at<int>(job.bra, kDims), c.table.at<const double2*>(job.ket, kSites),
                                 c.table.at<int>(job.ket, kDims), c.d_ops + job.op, job.index});
    }
    if (c.d_jobs.upload(hj)) return 1;
    for (size_t g0 = 0; g0 < fused.size(); g0 += gsize) {
        MpsMelemFusedArgs a{};
        a.n = c.n;
        a.jobs = c.d_jobs + g0;
        a.scratch = c.d_scratch;
        a.e_elems = e_elems;
        a.job_elems = job_elems;
        a.out = c.d_out;
        HIP_OK(launch_mps_melem_fused(a, (int)std::min(gsize, fused.size() - g0), st));
    }
    return 0;
}

// zgemm table launches of `count` products whose tables lie at tab: [A][B][C], `count` entries each
int table_products(bool conj_t, bool accum, int M, int N, int K, int lda, int ldb, int ldc, void* const* tab, size_t count, hipStream_t st) {
    for (size_t c0 = 0; c0 < count; c0 += kMaxGridY) {
        const int m = (int)std::min<size_t>(kMaxGridY, count - c0);
        auto ctab = [&](size_t block) { return reinterpret_cast<const void* const*>(tab + block * count + c0); };
        HIP_OK(launch_zgemm_tables_op(conj_t, accum, M, N, K, ctab(0), lda, ctab(1), ldb, tab + 2 * count + c0, ldc, 0, 0, 0, m, 1, st));
    }
    return 0;
}

// One walk for the jobs `members`, which share the bond dimensions of bra and ket and the operator; a job's slice of the scratch is
// E | E' | G | F, and E_q lies in the E set q & 1.  Per site: one batch for the F, the combining kernel, one batch for B^H G
int run_gemm(Call& c, const std::vector<int>& members, const ScratchPlan& plan, hipStream_t st) {
    const int n = c.n;
    const Job& head = c.jobs[members[0]];
    const int* bd = dims_of(c, head.bra);
    const int* kd = dims_of(c, head.ket);
    const OpLists& op = c.ops[head.op];
    const int* od = op.dims.data();
    const size_t e_elems = plan.e_elems, g_elems = plan.g_elems, job_elems = plan.job_elems, gsize = plan.gsize;
    c.walks.emplace_back(new WalkWork());
    WalkWork& w = *c.walks.back();
    double2* base = c.d_scratch;
    auto e_set = [&](size_t k, int q) { return base + k * job_elems + (size_t)(q & 1) * e_elems; };
    auto g_of = [&](size_t k) { return base + k * job_elems + 2 * e_elems; };
    auto f_of = [&](size_t k) { return base + k * job_elems + 2 * e_elems + g_elems; };
    struct Step { int q; size_t jobs, f_at, nf, first_at, nfirst, second_at, nsecond; };
    std::vector<Step> steps;
    std::vector<void*> ptrs;
    for (size_t g0 = 0; g0 < members.size(); g0 += gsize) {
        const size_t count = std::min(gsize, members.size() - g0);
        for (int q = 0; q < n; ++q) {
            const int x = bd[q], u = bd[q + 1], y = kd[q], v = kd[q + 1];
            const size_t esize = (size_t)x * y, gs = (size_t)x * v, nsize = (size_t)u * v, tsize = (size_t)y * v, bsize = (size_t)x * u;
            Step s{q, count, ptrs.size(), 0, 0, 0, 0, 0};
            // F_{a,s'} = E_q[a] T_q[s']: tables [A][B][C]
            std::vector<void*> ta, tb, tc;
            for (size_t k = 0; k < count; ++k) {
                const Job& job = c.jobs[members[g0 + k]];
                for (const auto& p : op.pairs[q]) {
                    ta.push_back(q == 0 ? (double2*)c.d_one : e_set(k, q) + (size_t)p.first * esize);
                    tb.push_back(const_cast<double2*>(c.views[job.ket].t[q] + (size_t)p.second * tsize));
                    tc.push_back(f_of(k) + (size_t)(2 * p.first + p.second) * gs);
                }
            }
            s.nf = ta.size();
            for (const auto* t : {&ta, &tb, &tc}) ptrs.insert(ptrs.end(), t->begin(), t->end());
            // E_{q+1}[b] = B_q[s]^H G_{b,s}: the first G of every b stores, the second one adds
            const int* mask = op.mask.data() + op.mask_off[q];
            for (int pass = 0; pass < 2; ++pass) {
                ta.clear(); tb.clear(); tc.clear();
                for (size_t k = 0; k < count; ++k) {
                    const Job& job = c.jobs[members[g0 + k]];
                    for (int b = 0; b < od[q + 1]; ++b) {
                        if (mask[b] == 0 || (pass == 1 && mask[b] != 3)) continue;
                        const int sx = pass == 1 ? 1 : (mask[b] & 1) ? 0 : 1;
                        ta.push_back(const_cast<double2*>(c.views[job.bra].t[q] + (size_t)sx * bsize));
                        tb.push_back(g_of(k) + (size_t)(2 * b + sx) * gs);
                        tc.push_back(q + 1 < n ? e_set(k, q + 1) + (size_t)b * nsize : (double2*)c.d_out + job.index);
                    }
                }
                (pass ? s.second_at : s.first_at) = ptrs.size();
                (pass ? s.nsecond : s.nfirst) = ta.size();
                for (const auto* t : {&ta, &tb, &tc}) ptrs.insert(ptrs.end(), t->begin(), t->end());
            }
            steps.push_back(s);
        }
    }
    if (w.d_ptrs.upload(ptrs)) return 1;
    for (const Step& s : steps) {
        const int q = s.q, x = bd[q], u = bd[q + 1], y = kd[q], v = kd[q + 1];
        if (table_products(false, false, x, v, y, y, v, v, w.d_ptrs + s.f_at, s.nf, st)) return 1;
        HIP_OK(launch_mps_melem_combine(c.d_ops + head.op, q, f_of(0), g_of(0), e_set(0, q + 1), job_elems, x, u, v, 2 * od[q + 1], (int)s.jobs, st));
        if (table_products(true, false, u, v, x, u, v, v, w.d_ptrs + s.first_at, s.nfirst, st)) return 1;
        if (table_products(true, true, u, v, x, u, v, v, w.d_ptrs + s.second_at, s.nsecond, st)) return 1;
    }
    return 0;
}

// routes: per job, decided by the caller from the states' bond dimensions as the host holds them, before any device work
int run(Call& c, aqc_mps* const* states, int nstates, const int32_t* job_bra, const int32_t* job_op, const int32_t* job_ket, int nops,
        const std::vector<int>& routes, double* out, hipStream_t st) {
    const int n = c.n;
    std::vector<int> state_view;
    if (view_states(states, (size_t)nstates, n, c.views, state_view)) return 1;
    std::vector<int> fused;
    std::map<std::tuple<std::vector<int>, std::vector<int>, int>, std::vector<int>> walks;   // jobs with the same bonds and operator share a walk
    for (int j = 0; j < c.njobs; ++j) {
        const Job job{state_view[job_bra[j]], state_view[job_ket[j]], job_op[j] < 0 ? nops : job_op[j], j};
        c.jobs.push_back(job);
        if (routes[j] == kMpsMelemFused) fused.push_back(j);
        else walks[std::make_tuple(c.views[job.bra].dims, c.views[job.ket].dims, job.op)].push_back(j);
    }
    const size_t ns = (size_t)n;
    c.table = MpsTable({mps_table_words(ns), mps_table_ints(ns + 1)}, c.views.size());
    for (size_t k = 0; k < c.views.size(); ++k) {
        c.table.put(k, kSites, c.views[k].t, ns);
        c.table.put(k, kDims, c.views[k].dims, ns + 1);
    }
    const size_t budget = g_budget.load();
    ScratchPlan fused_plan;
    std::vector<ScratchPlan> walk_plans;
    size_t scratch = 0;
    if (!fused.empty()) {
        fused_plan = plan_fused(c, fused, budget);
        scratch = fused_plan.gsize * fused_plan.job_elems;
    }
    for (const auto& walk : walks) {
        const ScratchPlan p = plan_gemm(c, walk.second, budget);
        if (p.job_elems > ((size_t)1 << 40))
            return failf("job %d: its scratch of %zu complex numbers is beyond what one call takes", c.jobs[walk.second[0]].index, p.job_elems);
        walk_plans.push_back(p);
        scratch = std::max(scratch, p.gsize * p.job_elems);
    }
    if (c.table.upload() || upload_ops(c) || c.d_out.alloc((size_t)c.njobs) || c.d_one.alloc(1) || c.d_scratch.alloc(scratch)) return 1;
    static const double one[2] = {1.0, 0.0};
    HIP_OK(hipMemcpyAsync(c.d_one, one, sizeof one, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(c.d_out, 0, sizeof(double2) * (size_t)c.njobs, st));   // (a chain whose last site has no entry is an exact 0)
    if (!fused.empty() && run_fused(c, fused, fused_plan, st)) return 1;
    size_t at = 0;
    for (const auto& walk : walks)
        if (run_gemm(c, walk.second, walk_plans[at++], st)) return 1;
    HIP_OK(hipMemcpyAsync(out, c.d_out, sizeof(double2) * (size_t)c.njobs, hipMemcpyDeviceToHost, st));
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_melem_route(int n, const int32_t* bra_dims, const int32_t* ket_dims, const int32_t* op_dims) {
    if (!ket_dims || n < 1) return -1;
    for (int q = 0; q <= n; ++q)
        if (ket_dims[q] < 1 || (bra_dims && bra_dims[q] < 1) || (op_dims && op_dims[q] < 1)) return -1;
    if (op_dims && (op_dims[0] != 1 || op_dims[n] != 1)) return -1;
    return mps_melem_route(n, bra_dims, ket_dims, op_dims);
}

int aqc_mps_melem_entries(int dl, int dr, const double* w, int32_t* out, int32_t* mask) {
    if (!out || !mask || (w && (dl < 1 || dr < 1 || dl > kMaxOpBond || dr > kMaxOpBond))) return -1;
    std::vector<MpsMelemEntry> ent;
    std::vector<int> m;
    mps_melem_entries(dl, dr, w, ent, m);
    for (size_t e = 0; e < ent.size(); ++e) {
        const int32_t row[5] = {ent[e].a, ent[e].sp, ent[e].b, ent[e].s, ent[e].first};
        memcpy(out + 5 * e, row, sizeof row);
    }
    for (size_t b = 0; b < m.size(); ++b) mask[b] = m[b];
    return (int)ent.size();
}

int64_t aqc_mps_melem_budget(int64_t bytes) {
    return swap_budget(g_budget, bytes, kMpsMelemBudget);
}

int aqc_mps_melem(aqc_mps* const* states, int nstates, int nops, const int32_t* op_dims, const int64_t* op_site_off, const double* op_data, int njobs,
                  const int32_t* job_bra, const int32_t* job_op, const int32_t* job_ket, int method, double* out) {
    if (!states || !job_bra || !job_op || !job_ket || !out) return failf("null argument");
    if (nops < 0 || (nops > 0 && (!op_dims || !op_site_off || !op_data))) return failf("null argument");
    if (nstates < 1) return failf("at least one state is needed");
    if (njobs < 1) return failf("at least one job is needed");
    if (njobs > 1 << 28) return failf("too many jobs in one call: %d", njobs);
    if (!mps_melem_method_ok(method)) return failf("unknown method %d", method);
    for (int j = 0; j < njobs; ++j) {
        if (job_bra[j] < 0 || job_bra[j] >= nstates || job_ket[j] < 0 || job_ket[j] >= nstates) return failf("job %d names a state outside the %d of the call", j, nstates);
        if (job_op[j] < -1 || job_op[j] >= nops) return failf("job %d names an operator outside the %d of the call", j, nops);
    }
    int n = 0, device = 0;
    if (check_states(states, nullptr, nstates, 1, &n, &device)) return 1;
    Call c;
    c.n = n;
    c.njobs = njobs;
    for (int o = 0; o < nops; ++o) {
        const std::vector<long long> off(op_site_off + (size_t)o * (n + 1), op_site_off + (size_t)(o + 1) * (n + 1));
        const int bad = mps_opsum_check_op(n, op_dims + (size_t)o * (n + 1), off.data());
        if (bad == 1) return failf("operator %d: the bond dimensions of an operator on %d qubits are at least 1, the first and the last 1", o, n);
        if (bad) return failf("operator %d: the site offsets are not the packed layout of its bond dimensions", o);
        const int dmax = mps_melem_max_op_bond(n, op_dims + (size_t)o * (n + 1));
        if (dmax > kMaxOpBond) return failf("operator %d: a bond dimension of %d is beyond %d", o, dmax, kMaxOpBond);
    }
    for (int o = 0; o < nops; ++o) c.ops.push_back(op_lists(n, op_dims + (size_t)o * (n + 1), op_data, op_site_off + (size_t)o * (n + 1)));
    c.ops.push_back(op_lists(n, nullptr, nullptr, nullptr));
    // the route of every job from the bond dimensions as the host holds them: a refused call has touched no device
    std::vector<int> state_dims((size_t)nstates * (n + 1)), routes(njobs);
    for (int k = 0; k < nstates; ++k)
        if (aqc_mps_dims(states[k], state_dims.data() + (size_t)k * (n + 1))) return 1;
    for (int j = 0; j < njobs; ++j) {
        const int* bd = state_dims.data() + (size_t)job_bra[j] * (n + 1);
        const int* kd = state_dims.data() + (size_t)job_ket[j] * (n + 1);
        const int* od = c.ops[job_op[j] < 0 ? nops : job_op[j]].dims.data();
        const int dmax = mps_melem_max_op_bond(n, od);
        routes[j] = resolve_route(method, mps_melem_route(n, bd, kd, od), mps_melem_max_bond(n, bd, kd), kMpsMelemFusedCap, "job", j);
        if (routes[j] < 0) return 1;
        if (routes[j] == kMpsMelemFused && dmax > kMpsMelemOpCap)
            return failf("the fused route takes operator bond dimensions up to %d; job %d has %d", (int)kMpsMelemOpCap, j, dmax);
    }
    HIP_OK(hipSetDevice(device));
    hipStream_t st = mps_stream(states[0]);
    return finish_call(st, run(c, states, nstates, job_bra, job_op, job_ket, nops, routes, out, st), "operator matrix elements");
}

}  // extern "C"
