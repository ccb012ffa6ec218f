// The truncating sweep over whole states that compression (aqc_mps_compress_api.cpp), linear combinations
// (aqc_mps_combine_api.cpp) and operator sums (aqc_mps_opsum_api.cpp; both through aqc_mps_sum_call.h) share, on both routes (rules: aqc_mps_compress_rule.h; kernels: aqc_mps_compress.hip, the right factors by
// aqc_mps_ent.hip, the SVDs of a step by aqc_svd_batch.hip).  A state to sweep is site pointers and bond dimensions: it need not be an
// engine state (the assembled sites of a direct sum are not).
//   fused      FusedSweep::run enqueues, for all its states together: the right chain, then per chunk of states and per bond form /
//              SVD batch / split, then the last site; the results come back after the caller's one synchronisation (collect), the
//              new states are adopted from the sweep's flat stores (adopt)
//   canonical  sweep_canonical: on a clone of an engine state, the identity sweeps of the engine, then its truncating sweep
// Private to csrc/ (everything has internal linkage).
#pragma once
#include "aqc_mps_call.h"

namespace {

static_assert(kMpsEntByRule == kMpsByRule && kMpsEntFused == kMpsFused, "resolve_route");

// a state to sweep (host arrays that outlive run)
struct SweepInput {
    const double2* const* sites = nullptr;   // [n] device pointers, site q [2][dims[q]][dims[q+1]]
    const int* dims = nullptr;               // [n + 1], every one <= kMpsEntFusedCap on the fused route
};

// what a sweep adds to a state: the decisions of its cuts and where its blocks lie in the stores of a fused sweep
struct SweepWork {
    int status = kMpsCompressOk;
    std::vector<int> ranks, sweeps;
    std::vector<double> dropped;
    std::vector<size_t> fac_off, site_off, lam_off;
    size_t fac_at = 0, site_at = 0, lam_at = 0;   // element offsets of this state's blocks in the sweep's stores
    void size(int n, const int* dims) {
        fac_off = mps_ent_factor_offsets(n, dims);
        site_off = mps_site_offsets(n, dims);
        lam_off = mps_compress_lam_offsets(n, dims);
        ranks.assign(n - 1, 0);
        sweeps.assign(n - 1, 0);
        dropped.assign(n - 1, 0.0);
    }
};

struct FusedSweep {
    static constexpr int kPlaneElems = kMpsEntFusedCap * kMpsEntFusedCap;
    enum { kSites, kFacOff, kSiteOff, kLamOff, kDims };   // the sections of a state's record in the table
    int n = 0, cuts = 0, k = 1;            // k: the largest bond of the swept states
    double trunc_thr = 0.0;
    int max_bond = 0;
    MpsTable table;                        // per state: site pointers | factor offsets | site offsets | bond offsets | dims
    DevBuf<MpsEntState> d_in;
    DevBuf<MpsCompressState> d_states;
    DevBuf<double2> d_factors, d_sites, d_carry, d_m;
    DevBuf<double> d_lam, d_dropped;
    DevBuf<int> d_results;                 // per state: ranks | sweeps | status
    SvdChunk svd;                          // of 2 k x k matrices, one per state of a chunk
    std::vector<int> h_results;
    std::vector<double> h_dropped;

    // in[i] is swept into work[i] (sized by SweepWork::size at in[i]'s bonds); budget: bytes of the SVD stores of a chunk
    int run(const std::vector<SweepInput>& in, const std::vector<SweepWork*>& work, size_t budget, hipStream_t st) {
        const size_t nn = (size_t)n, ncuts = (size_t)cuts, res = 2 * ncuts + 1, count = in.size();
        table = MpsTable({mps_table_words(nn), mps_table_words(nn + 1), mps_table_words(nn), mps_table_words(nn), mps_table_ints(nn + 1)}, count);
        size_t fac_total = 0, site_total = 0, lam_total = 0;
        for (size_t i = 0; i < count; ++i) {
            SweepWork& w = *work[i];
            table.put(i, kSites, std::vector<const double2*>(in[i].sites, in[i].sites + nn), nn);
            table.put(i, kFacOff, w.fac_off, nn + 1);
            table.put(i, kSiteOff, w.site_off, nn);
            table.put(i, kLamOff, w.lam_off, w.lam_off.size());
            table.put(i, kDims, std::vector<int>(in[i].dims, in[i].dims + nn + 1), nn + 1);
            w.fac_at = fac_total; w.site_at = site_total; w.lam_at = lam_total;
            fac_total += 2 * w.fac_off[nn];
            site_total += w.site_off[nn];
            for (size_t q = 1; q < nn; ++q) lam_total += (size_t)in[i].dims[q];
        }
        const int K = k, chunk = mps_compress_chunk(K, count, budget);
        if (table.upload() || d_factors.alloc(std::max<size_t>(fac_total, 1)) || d_sites.alloc(site_total) ||
            d_lam.alloc(std::max<size_t>(lam_total, 1)) || d_results.alloc(res * count) || d_dropped.alloc(ncuts * count) ||
            d_carry.alloc((size_t)chunk * kPlaneElems) || d_m.alloc((size_t)chunk * 2 * kPlaneElems) || svd.alloc(chunk, 2 * K, K)) return 1;
        std::vector<MpsEntState> hin(count);
        std::vector<MpsCompressState> hs(count);
        for (size_t i = 0; i < count; ++i) {
            const SweepWork& w = *work[i];
            hin[i].sites = table.at<const double2*>(i, kSites);
            hin[i].fac_off = table.at<size_t>(i, kFacOff);
            hin[i].dims = table.at<int>(i, kDims);
            hin[i].factors = d_factors + w.fac_at;
            hs[i].in = hin[i];
            hs[i].site_off = table.at<size_t>(i, kSiteOff);
            hs[i].lam_off = table.at<size_t>(i, kLamOff);
            hs[i].out_sites = d_sites + w.site_at;
            hs[i].out_lam = d_lam + w.lam_at;
            hs[i].ranks = d_results + i * res;
            hs[i].sweeps = hs[i].ranks + ncuts;
            hs[i].status = hs[i].sweeps + ncuts;
            hs[i].dropped = d_dropped + i * ncuts;
        }
        if (d_in.upload(hin) || d_states.upload(hs)) return 1;
        HIP_OK(hipMemsetAsync(d_results, 0, sizeof(int) * res * count, st));
        HIP_OK(hipMemsetAsync(d_dropped, 0, sizeof(double) * ncuts * count, st));
        for (size_t s0 = 0; s0 < count; s0 += kMaxGridY) {
            MpsEntChainArgs a{n, d_in + s0, 1};
            HIP_OK(launch_mps_ent_chain_right(a, (int)std::min<size_t>(kMaxGridY, count - s0), st));
        }
        for (size_t first = 0; first < count; first += chunk) {   // the chunks share the step's stores: one stream orders them
            const int part = (int)std::min<size_t>(chunk, count - first);
            MpsCompressArgs a{n, 0, K, (int)first, d_states, d_carry, d_m, svd.a, svd.rows(), svd.cols(), svd.u, svd.s, svd.sweeps(), svd.status(), trunc_thr, max_bond};
            for (int q = 0; q + 1 < n; ++q) {
                a.q = q;
                HIP_OK(launch_mps_compress_form(a, part, st));
                HIP_OK(svd.launch(part, st));
                HIP_OK(launch_mps_compress_split(a, part, st));
            }
            a.q = n - 1;
            HIP_OK(launch_mps_compress_form(a, part, st));
        }
        h_results.resize(res * count);
        h_dropped.resize(std::max<size_t>(ncuts * count, 1));
        HIP_OK(hipMemcpyAsync(h_results.data(), d_results, sizeof(int) * res * count, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_dropped.data(), d_dropped, sizeof(double) * ncuts * count, hipMemcpyDeviceToHost, st));
        return 0;
    }

    // after the synchronisation: the decisions of state i of run
    void collect(size_t i, SweepWork& w) const {
        const size_t ncuts = (size_t)cuts, res = 2 * ncuts + 1;
        const int* r = h_results.data() + i * res;
        w.ranks.assign(r, r + ncuts);
        w.sweeps.assign(r + ncuts, r + 2 * ncuts);
        w.status = r[2 * ncuts];
        w.dropped.assign(h_dropped.begin() + i * ncuts, h_dropped.begin() + (i + 1) * ncuts);
    }

    // a new engine state from the tensors the sweep left on the device; discarded: the weight it starts from, the cuts' is added
    int adopt(const SweepWork& w, int device, double discarded, aqc_mps** out) const {
        std::vector<int> dims(n + 1, 1);
        for (int q = 1; q < n; ++q) { dims[q] = w.ranks[q - 1]; discarded += w.dropped[q - 1]; }
        return adopt_flat(device, n, dims.data(), d_sites + w.site_at, w.site_off.data(), d_lam + w.lam_at, w.lam_off.data(), discarded, out);
    }
};

// canonical route: on a clone, the identity sweeps of the engine, then its truncating sweep left to right.  The engine reports an SVD at
// its sweep limit as an error of the gate, and so does this route: of the statuses it gives only 0 and 2.  A state that is not finite
// (or has a zero site) gets the status of the fused route.  *made: the new state (null for a failed one), the caller's to destroy
int sweep_canonical(const MpsView& v, double trunc_thr, int max_bond, SweepWork& w, aqc_mps** made) {
    const int n = (int)v.t.size();
    bool finite = true, zero = false;
    aqc_mps* m = nullptr;
    *made = nullptr;
    if (canonical_clone(v, true, &finite, &zero, &m)) return 1;
    if (!m) { w.status = kMpsCompressNonFinite; return 0; }
    int rc = 0;
    for (int q = 0; q + 1 < n && !rc; ++q) {
        const double before = aqc_mps_discarded_weight(m);
        rc = aqc_mps_gate2(m, q, q + 1, kIdentityGate2, trunc_thr, max_bond);
        w.dropped[q] = aqc_mps_discarded_weight(m) - before;
    }
    std::vector<int> dims(n + 1);
    if (!rc) rc = aqc_mps_dims(m, dims.data());
    if (rc) { (void)aqc_mps_destroy(m); return 1; }
    for (int q = 1; q < n; ++q) w.ranks[q - 1] = dims[q];
    *made = m;
    return 0;
}

}  // namespace
