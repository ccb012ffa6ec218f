// The host scaffolding that the two calls which sweep a direct sum share: linear combinations (aqc_mps_combine_api.cpp) and operator
// sums (aqc_mps_opsum_api.cpp).  Each of them assembles the direct sums of its outputs with its own kernel into SumCall::d_sums; the
// shape of an output from the widths of its terms, the packing of the outputs' index arrays, the sweep on both routes
// (aqc_mps_sweep.h) and the adoption of the results are stated here once.
// Private to csrc/ (everything has internal linkage).
#pragma once
#include "aqc_mps_combine_rule.h"
#include "aqc_mps_sweep.h"

namespace {

constexpr long long kMaxSummedBond = 1 << 20;        // (block offsets are ints, a site of 2 Sigma^2 elements must fit the device)

// one output: its terms as a stretch of the call's term arrays, the direct sum's shape, where it lies in the call's stores, what the
// sweep decides
struct SumOutput : SweepWork {
    int route = 0, first = 0, nterms = 0;   // its terms: [first, first + nterms) of the call's term arrays
    std::vector<int> dims;                  // Sigma_0 .. Sigma_n
    std::vector<int> block_off;             // mps_combine_block_offsets
    std::vector<size_t> asm_off;            // mps_combine_site_offsets
    size_t asm_at = 0, block_at = 0, off_at = 0;
    std::vector<const double2*> sites;      // device pointers of the assembled sites
};

struct SumCall {
    int n = 0, cuts = 0, widest = 1;
    bool canonical = false;           // an output of two or more qubits takes the canonical route
    std::vector<SumOutput> outputs;
    std::vector<int> fused;           // the outputs on the fused route
    DevBuf<double2> d_sums;           // the assembled sites of all outputs
    DevBuf<double> d_ones;            // canonical route: the unit bond vector of every bond
    FusedSweep sweep;                 // of the outputs on the fused route

    void start(int n_, double trunc_thr, int max_bond) {
        n = sweep.n = n_;
        cuts = sweep.cuts = n_ - 1;
        sweep.trunc_thr = trunc_thr;
        sweep.max_bond = max_bond;
    }
    // output j from the widths of its terms ([nterms][n + 1]; `bond` their largest sum, in 64 bits); -1 with the message set
    int shape(int j, int first, int nterms, const int* widths, long long bond, int method, int rule_route) {
        SumOutput& o = outputs[j];
        o.first = first;
        o.nterms = nterms;
        if (bond > kMaxSummedBond) return failf("output %d: a summed bond dimension of %lld is beyond %lld", j, bond, kMaxSummedBond), -1;
        if ((o.route = resolve_route(method, rule_route, (int)bond, kMpsEntFusedCap, "output", j)) < 0) return -1;
        o.dims = mps_combine_dims(n, nterms, widths);
        o.block_off = mps_combine_block_offsets(n, nterms, widths);
        o.asm_off = mps_combine_site_offsets(n, nterms, widths);
        o.size(n, o.dims.data());
        widest = std::max(widest, (int)bond);
        if (o.route == kMpsEntFused && n > 1) {
            fused.push_back(j);
            sweep.k = std::max(sweep.k, (int)bond);
        } else if (n > 1) {
            canonical = true;
        }
        return 0;
    }
    // the block offsets and site offsets of all outputs, one after the other; returns the elements of d_sums, *largest the largest site
    size_t pack(std::vector<int>& block_off, std::vector<size_t>& site_off, size_t* largest) {
        size_t total = 0;
        *largest = 1;
        for (SumOutput& o : outputs) {
            o.block_at = block_off.size();
            block_off.insert(block_off.end(), o.block_off.begin(), o.block_off.end());
            o.off_at = site_off.size();
            site_off.insert(site_off.end(), o.asm_off.begin(), o.asm_off.end());
            o.asm_at = total;
            total += o.asm_off[n];
            for (int q = 0; q < n; ++q) *largest = std::max(*largest, o.asm_off[q + 1] - o.asm_off[q]);
        }
        return total;
    }
    // after d_sums is allocated
    void point_sites() {
        for (SumOutput& o : outputs) {
            o.sites.resize(n);
            for (int q = 0; q < n; ++q) o.sites[q] = d_sums + o.asm_at + o.asm_off[q];
        }
    }
};

// canonical route: the assembled sum as an engine state with unit bond vectors, then compression's canonical route on it
[[maybe_unused]] int sum_run_canonical(SumCall& c, SumOutput& o, int device, double trunc_thr, int max_bond, aqc_mps** made) {
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
[[maybe_unused]] int sum_adopt_one_qubit(SumCall& c, int device, aqc_mps** out) {
    std::vector<double2> host(2 * c.outputs.size());
    HIP_OK(hipMemcpy(host.data(), c.d_sums, sizeof(double2) * host.size(), hipMemcpyDeviceToHost));
    const int dims[2] = {1, 1};
    for (size_t j = 0; j < c.outputs.size(); ++j) {
        SumOutput& o = c.outputs[j];
        const double2 a = host[2 * j], b = host[2 * j + 1];
        const double norm2 = a.x * a.x + a.y * a.y + b.x * b.x + b.y * b.y;
        if (!(norm2 > 0.0) || !std::isfinite(norm2)) { o.status = kMpsCompressNonFinite; continue; }
        const void* site = o.sites[0];
        const double* none = nullptr;
        if (mps_adopt(device, 1, dims, &site, &none, 0.0, &out[j])) return 1;
    }
    return 0;
}

// Everything after the assembly was enqueued (rc: its result): the fused sweep of the fused outputs together, the one synchronisation
// of the call, the canonical outputs one by one, the new states and what the cuts decided.  what: the call, for messages
[[maybe_unused]] int sum_sweep_and_adopt(SumCall& c, int rc, size_t budget, hipStream_t st, int device, double trunc_thr, int max_bond, const char* what,
                                        aqc_mps** out, int32_t* ranks, double* dropped, int32_t* sweeps, int32_t* status) {
    const int n = c.n, nout = (int)c.outputs.size();
    std::vector<SweepInput> in;
    std::vector<SweepWork*> work;
    if (!rc && !c.fused.empty()) {
        for (int j : c.fused) {
            in.push_back({c.outputs[j].sites.data(), c.outputs[j].dims.data()});
            work.push_back(&c.outputs[j]);
        }
        rc = c.sweep.run(in, work, budget, st);
    }
    if (finish_call(st, rc, what)) return 1;   // the one synchronisation of the call
    for (size_t i = 0; i < c.fused.size(); ++i) c.sweep.collect(i, c.outputs[c.fused[i]]);
    if (n == 1) {
        if (sum_adopt_one_qubit(c, device, out)) { drop_outputs(out, nout); return 1; }
    } else if (c.canonical && c.d_ones.upload(std::vector<double>(c.widest, 1.0))) {
        return 1;
    }
    for (int j = 0; j < nout; ++j) {
        SumOutput& o = c.outputs[j];
        if (n > 1) {
            int bad = 0;
            if (o.route != kMpsEntFused) bad = sum_run_canonical(c, o, device, trunc_thr, max_bond, &out[j]);
            else if (o.status == kMpsCompressOk) bad = c.sweep.adopt(o, device, 0.0, &out[j]);
            if (bad || (o.status == kMpsCompressOk && !out[j])) { drop_outputs(out, nout); return bad ? 1 : failf("%s lost a state", what); }
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

}  // namespace
