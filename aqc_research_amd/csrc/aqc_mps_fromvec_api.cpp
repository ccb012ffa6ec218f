// C ABI (include/aqc_hip.h): dense vectors into single-lane MPS states, every bond truncated, many vectors per call.
// Rules: aqc_mps_fromvec_rule.h; kernels: aqc_mps_fromvec.hip, the SVD of a site by the device-pointer core of aqc_svd_batch.hip.  The call
// has no input states: it orders its work on a stream of its own and ends as the calls of aqc_mps_call.h do, with one synchronisation.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_fromvec_rule.h"

using namespace aqc;

namespace {

std::atomic<size_t> g_budget{kMpsFromVecBudget};   // aqc_mps_from_vec_budget: tests lower it to run many chunks on few lanes

struct Call {
    int n = 0, cuts = 0, lanes = 0, kc = 2, chunk = 1, max_parts = 1;
    double trunc_thr = 0.0;
    int max_bond = 0;
    std::vector<int> bounds;                 // n + 1
    BoundedStores stores;                    // the new sites and bond vectors of every lane, sized by the bounds
    DevBuf<double2> d_ping, d_pong, d_fac0, d_fac1, d_w;
    DevBuf<double> d_dropped;
    DevBuf<int> d_lane_ints;                 // bonds [lanes][n + 1] | status [lanes] | failed_at [lanes] | sweeps [lanes][cuts]
    SvdChunk svd;                            // of kc x kc matrices, one per lane of a chunk
    std::vector<int> h_lane_ints;
    std::vector<double> h_dropped;
};

int run_fused(Call& c, const double2* vecs, hipStream_t st) {
    const size_t n = (size_t)c.n, cuts = (size_t)c.cuts, lanes = (size_t)c.lanes, chunk = (size_t)c.chunk, elems = (size_t)1 << c.n;
    const size_t ints = (n + 1) + 2 + cuts, fac = (size_t)c.max_parts * 64 * 64;
    c.h_lane_ints.assign(lanes * ints, 0);
    int* h_bonds = c.h_lane_ints.data();
    int* h_failed = h_bonds + lanes * (n + 1) + lanes;
    for (size_t i = 0; i < lanes; ++i) { h_bonds[i * (n + 1)] = 1; h_failed[i] = -1; }
    if (c.d_ping.alloc(chunk * elems) || c.d_pong.alloc(chunk * elems) || c.d_fac0.alloc(chunk * fac) || c.d_fac1.alloc(chunk * fac) ||
        c.svd.alloc(c.chunk, c.kc, c.kc) || c.d_w.alloc(chunk * 64 * kMpsFromVecCap) || c.stores.alloc(c.n, c.bounds.data(), lanes) ||
        c.d_dropped.alloc(lanes * cuts) || c.d_lane_ints.upload(c.h_lane_ints)) return 1;
    HIP_OK(hipMemsetAsync(c.d_dropped, 0, sizeof(double) * lanes * cuts, st));
    MpsFromVecArgs a{};
    a.n = c.n;
    a.kc = c.kc;
    a.lane_elems = elems;
    a.bonds = c.d_lane_ints;
    a.status = a.bonds + lanes * (n + 1);
    a.failed_at = a.status + lanes;
    a.sweeps = a.failed_at + lanes;
    a.dropped = c.d_dropped;
    a.sites = c.stores.sites;
    a.lam = c.stores.lam;
    a.site_off = c.stores.d_site_off();
    a.lam_off = c.stores.d_lam_off();
    a.max_parts = c.max_parts;
    a.a = c.svd.a;
    a.rows = c.svd.rows();
    a.cols = c.svd.cols();
    a.u = c.svd.u;
    a.s = c.svd.s;
    a.svd_sweeps = c.svd.sweeps();
    a.svd_status = c.svd.status();
    a.w = c.d_w;
    a.trunc_thr = c.trunc_thr;
    a.max_bond = c.max_bond;
    for (size_t first = 0; first < lanes; first += chunk) {   // the chunks share the work buffers: one stream orders them
        const int count = (int)std::min(chunk, lanes - first);
        a.first = (int)first;
        HIP_OK(hipMemcpyAsync(c.d_ping, vecs + first * elems, sizeof(double2) * (size_t)count * elems, hipMemcpyHostToDevice, st));
        double2* bufs[2] = {c.d_ping, c.d_pong};
        for (int q = 0; q + 1 < c.n; ++q) {
            a.q = q;
            a.nr = (size_t)1 << (c.n - 1 - q);
            a.src = bufs[q & 1];
            a.dst = bufs[(q + 1) & 1];
            int parts = mps_fromvec_parts(a.nr);
            double2* facs[2] = {c.d_fac0, c.d_fac1};
            a.in_blocks = mps_fromvec_blocks(a.nr);
            a.blocks_per_part = (int)mps_fromvec_blocks_per_part(a.nr);
            for (int level = 0;; ++level) {
                a.level = level;
                a.last = parts == 1;
                a.fac_in = facs[(level + 1) & 1];
                a.fac_out = facs[level & 1];
                HIP_OK(launch_mps_fromvec_qr(a, parts, count, st));
                if (parts == 1) break;
                a.in_blocks = (size_t)parts;
                a.blocks_per_part = kMpsFromVecFanIn;
                parts = mps_fromvec_fold(parts);
            }
            HIP_OK(c.svd.launch(count, st));
            HIP_OK(launch_mps_fromvec_split(a, count, st));
            HIP_OK(launch_mps_fromvec_project(a, count, st));
        }
        a.q = c.n - 1;
        a.nr = 1;
        a.src = bufs[(c.n - 1) & 1];
        HIP_OK(launch_mps_fromvec_last(a, count, st));
    }
    c.h_dropped.assign(std::max<size_t>(lanes * cuts, 1), 0.0);
    HIP_OK(hipMemcpyAsync(c.h_lane_ints.data(), c.d_lane_ints, sizeof(int) * lanes * ints, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(c.h_dropped.data(), c.d_dropped, sizeof(double) * lanes * cuts, hipMemcpyDeviceToHost, st));
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_from_vec_route(int n, int max_bond) {
    if (n < 1 || max_bond < 0) return -1;
    return mps_fromvec_route(n, max_bond);
}

int64_t aqc_mps_from_vec_budget(int64_t bytes) {
    return swap_budget(g_budget, bytes, kMpsFromVecBudget);
}

int aqc_mps_from_vec(int device, int n, int lanes, const double* vecs, double trunc_thr, int max_bond, int method, aqc_mps** out, int32_t* bonds,
                     double* dropped, int32_t* sweeps, int32_t* status, int32_t* failed_at, int32_t* parts) {
    if (check_truncating_call(vecs, out, lanes, trunc_thr, max_bond, "vector", mps_fromvec_method_ok(method), method)) return 1;
    if (n < kMpsFromVecMinQubits) return failf("a vector needs at least %d qubits", (int)kMpsFromVecMinQubits);
    const int route = method == kMpsFromVecByRule ? mps_fromvec_route(n, max_bond) : method;
    if (route == kMpsFromVecHost) return failf("the host route of the conversion (%d qubits, max_bond %d) is the caller's: vector_to_canonical_mps", n, max_bond);
    if (mps_fromvec_route(n, max_bond) != kMpsFromVecFused)
        return failf("the fused route takes 2 .. %d qubits and bonds up to %d; %d qubits with max_bond %d can reach %d", (int)kMpsFromVecMaxQubits,
                     (int)kMpsFromVecCap, n, max_bond, n <= kMpsFromVecMaxQubits ? mps_fromvec_bound(n, n / 2, max_bond) : 0);
    Call c;
    c.n = n;
    c.cuts = n - 1;
    c.lanes = lanes;
    c.trunc_thr = trunc_thr;
    c.max_bond = max_bond;
    const size_t budget = g_budget.load();
    c.chunk = mps_fromvec_chunk(n, (size_t)lanes, budget);
    if (c.chunk < 1)
        return failf("one vector of %d qubits needs %zu bytes of work buffers, the budget is %zu (aqc_mps_from_vec_budget)", n, mps_fromvec_lane_bytes(n), budget);
    if ((size_t)lanes * (size_t)c.cuts > (size_t)1 << 28) return failf("too many cuts in one call: %d vectors x %d cuts", lanes, c.cuts);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return failf("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return failf("device out of range");
    HIP_OK(hipSetDevice(device));
    c.bounds = mps_fromvec_bounds(n, max_bond);
    c.kc = 2 * mps_max_bond(n, c.bounds.data());
    for (int q = 0; q + 1 < n; ++q) {
        const int p = mps_fromvec_parts((size_t)1 << (n - 1 - q));
        c.max_parts = std::max(c.max_parts, p);
        if (parts) parts[q] = p;
    }
    hipStream_t st = nullptr;
    HIP_OK(hipStreamCreate(&st));
    const int rc = finish_call(st, run_fused(c, reinterpret_cast<const double2*>(vecs), st), "conversion");   // the one synchronisation of the call
    (void)hipStreamDestroy(st);
    if (rc) return 1;
    const size_t np1 = (size_t)n + 1, cuts = (size_t)c.cuts, L = (size_t)lanes;
    const int* h_bonds = c.h_lane_ints.data();
    const int* h_status = h_bonds + L * np1;
    const int* h_failed = h_status + L;
    const int* h_sweeps = h_failed + L;
    for (size_t i = 0; i < L; ++i) {
        const int* b = h_bonds + i * np1;
        if (h_status[i] == kMpsCompressOk) {
            double discarded = 0.0;
            for (size_t q = 0; q < cuts; ++q) discarded += c.h_dropped[i * cuts + q];
            if (c.stores.adopt(device, n, i, b, discarded, &out[i])) { drop_outputs(out, lanes); return 1; }
        }
        for (size_t q = 0; q < np1; ++q)
            if (bonds) bonds[i * np1 + q] = b[q];
        for (size_t q = 0; q < cuts; ++q) {
            if (dropped) dropped[i * cuts + q] = c.h_dropped[i * cuts + q];
            if (sweeps) sweeps[i * cuts + q] = h_sweeps[i * cuts + q];
        }
        if (status) status[i] = h_status[i];
        if (failed_at) failed_at[i] = h_failed[i];
    }
    return 0;
}

}  // extern "C"
