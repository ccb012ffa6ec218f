// C ABI (include/aqc_hip.h): shots and amplitudes of single-lane MPS states.  Rules: aqc_mps_sample_rule.h; kernels: aqc_mps_sample.hip.
// The skeleton of the call: aqc_mps_call.h.
#include <algorithm>
#include <memory>
#include <vector>

#include "aqc_mps_call.h"
#include "aqc_mps_sample_rule.h"

using namespace aqc;

namespace {

static_assert(kMpsSampleByRule == kMpsByRule && kMpsSampleFused == kMpsFused, "resolve_route");
enum { kSites, kEnvOff, kDims };                      // the sections of a state's record in the call's table

// everything one lane's launches read or write; alive until the call's last synchronisation
struct StateWork {
    int n = 0, route = 0;
    const MpsView* v = nullptr;                       // the lane's state
    std::vector<size_t> off;                          // env offsets, n + 2 entries (the last = total)
    NormEnvs env;                                     // shots: R_n .. R_1 (the fused sweep brings the left half with it)
    DevBuf<double2> mats, amps;
    DevBuf<unsigned char> bits, status;
    DevBuf<double> norm2;
    std::vector<unsigned char> h_status;
};

struct Call {
    int n = 0, nstates = 0, device = 0;
    int64_t count = 0;                                // shots, or bit strings
    uint64_t first_shot = 0, seed = 0;
    bool amplitudes = false;
    const unsigned char* d_bits_in = nullptr;         // amplitudes: [count][n] on the device
};

// the shots walked in chunks: per site V T_0, V T_1, W_0 R, W_1 R and the row kernel
int run_gemm(StateWork& w, const Call& c, int lane, hipStream_t st) {
    const int n = w.n;
    const int maxb = w.v->max_bond;
    const int64_t chunk = mps_sample_chunk(maxb, c.count);
    const size_t mat = (size_t)chunk * maxb;
    if (w.mats.alloc(kMpsSampleGemmMats * mat)) return 1;
    double2 *v = w.mats, *w0 = v + mat, *w1 = w0 + mat, *g0 = w1 + mat, *g1 = g0 + mat;
    for (int64_t s0 = 0; s0 < c.count; s0 += chunk) {
        const int rows = (int)std::min<int64_t>(chunk, c.count - s0);
        HIP_OK(launch_mps_sample_ones(v, rows, st));
        for (int q = 0; q < n; ++q) {
            const int x = w.v->dims[q], u = w.v->dims[q + 1];
            const double2* t0 = w.v->t[q];
            const double2* t1 = t0 + (size_t)x * u;
            HIP_OK(launch_zgemm(false, false, rows, u, x, v, x, t0, u, w0, u, st));
            HIP_OK(launch_zgemm(false, false, rows, u, x, v, x, t1, u, w1, u, st));
            if (!c.amplitudes) {
                const double2* r = w.env.r + w.off[q + 1];
                HIP_OK(launch_zgemm(false, false, rows, u, u, w0, u, r, u, g0, u, st));
                HIP_OK(launch_zgemm(false, false, rows, u, u, w1, u, r, u, g1, u, st));
            }
            MpsSampleRowArgs a{};
            a.q = q; a.n = n; a.chi = u;
            a.rows = rows; a.shot0 = s0;
            a.first_shot = c.first_shot; a.seed = c.seed; a.lane = (unsigned long long)lane;
            a.w0 = w0; a.w1 = w1; a.g0 = g0; a.g1 = g1; a.v = v;
            a.bits_in = c.d_bits_in;
            a.bits = w.bits; a.amps = w.amps; a.status = w.status; a.norm2 = w.norm2;
            HIP_OK(launch_mps_sample_rows(a, c.amplitudes, st));
        }
    }
    return 0;
}

// what both entry points do once their arguments have passed; outputs may be null where the entry point allows it
int run(aqc_mps* const* states, const Call& c, int method, const unsigned char* bits_in, unsigned char* bits, double* amps, double* norm2) {
    const int n = c.n, nstates = c.nstates;
    HIP_OK(hipSetDevice(c.device));
    hipStream_t st = mps_stream(states[0]);
    std::vector<MpsView> views;
    std::vector<int> lane_state;
    if (view_states(states, (size_t)nstates, n, views, lane_state)) return 1;
    std::vector<int> routes(views.size(), 0);
    bool any_fused = false;
    for (int s = 0; s < nstates; ++s) {
        const MpsView& v = views[lane_state[s]];
        int& route = routes[lane_state[s]];
        if (!route && (route = resolve_route(method, mps_sample_route(n, v.dims.data()), v.max_bond, kMpsSampleFusedCap, "state", s)) < 0) return 1;
        any_fused = any_fused || route == kMpsSampleFused;
    }
    MpsTable dev;   // what the fused route reads of the states
    if (any_fused) {
        dev = MpsTable({mps_table_words((size_t)n), mps_table_words((size_t)n + 2), mps_table_ints((size_t)n + 1)}, views.size());
        for (size_t k = 0; k < views.size(); ++k) {
            dev.put(k, kSites, views[k].t, n);
            dev.put(k, kEnvOff, mps_obs_env_offsets(n, views[k].dims.data()), n + 2);
            dev.put(k, kDims, views[k].dims, n + 1);
        }
        if (dev.upload()) return 1;
    }
    std::vector<std::unique_ptr<StateWork>> work;
    DevBuf<unsigned char> d_bits_in;
    DevBuf<MpsSampleState> d_table;
    Call call = c;
    int rc = 0;
    if (c.amplitudes) {
        rc = d_bits_in.upload(std::vector<unsigned char>(bits_in, bits_in + (size_t)c.count * n));
        call.d_bits_in = d_bits_in;
    }
    std::vector<MpsSampleState> table;
    for (int s = 0; s < nstates && !rc; ++s) {   // the work is per lane: the lane is part of the Philox counter
        const size_t k = (size_t)lane_state[s];
        const MpsView& v = views[k];
        work.emplace_back(new StateWork());
        StateWork& w = *work.back();
        w.n = n;
        w.v = &v;
        w.off = mps_obs_env_offsets(n, v.dims.data());
        w.route = routes[k];
        if (w.amps.alloc((size_t)c.count)) { rc = 1; break; }
        if (!c.amplitudes) {
            if (w.bits.alloc((size_t)c.count * n) || w.status.alloc((size_t)c.count) || w.norm2.alloc(1)) { rc = 1; break; }
            if (hipMemsetAsync(w.status, 0, (size_t)c.count, st) != hipSuccess) { rc = failf("clearing the status failed"); break; }
        }
        const double2* const* d_sites = dev.at<const double2*>(k, kSites);
        const int* d_dims = dev.at<int>(k, kDims);
        const size_t* d_off = dev.at<size_t>(k, kEnvOff);
        if (!c.amplitudes && (rc = norm_environments(w.env, v, w.off, st, w.route == kMpsSampleFused, kEnvRight, d_sites, d_dims, d_off))) break;
        if (w.route == kMpsSampleFused) {
            MpsSampleState e{};
            e.sites = d_sites; e.dims = d_dims; e.env_off = d_off; e.env_r = w.env.r;
            e.bits = w.bits; e.amps = w.amps; e.status = w.status; e.norm2 = w.norm2;
            e.lane = (unsigned long long)s;
            table.push_back(e);
        } else if ((rc = run_gemm(w, call, s, st))) {
            break;
        }
    }
    if (!rc && !table.empty()) {   // every state of the fused route in one launch
        MpsSampleArgs a{};
        a.n = n; a.shots = c.count; a.first_shot = c.first_shot; a.seed = c.seed;
        a.bits_in = call.d_bits_in;
        if (!(rc = d_table.upload(table))) {
            a.states = d_table;
            const hipError_t e = launch_mps_sample_fused(a, (int)table.size(), c.amplitudes, st);
            if (e != hipSuccess) rc = failf("launch_mps_sample_fused failed: %s", hipGetErrorString(e));
        }
    }
    for (int s = 0; s < nstates && !rc; ++s) {
        StateWork& w = *work[s];
        hipError_t e = hipSuccess;
        if (amps) e = hipMemcpyAsync(amps + 2 * (size_t)s * c.count, w.amps, sizeof(double2) * (size_t)c.count, hipMemcpyDeviceToHost, st);
        if (!c.amplitudes) {
            w.h_status.resize((size_t)c.count);
            if (e == hipSuccess) e = hipMemcpyAsync(bits + (size_t)s * c.count * n, w.bits, (size_t)c.count * n, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(w.h_status.data(), w.status, (size_t)c.count, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && norm2) e = hipMemcpyAsync(norm2 + s, w.norm2, sizeof(double), hipMemcpyDeviceToHost, st);
        }
        if (e != hipSuccess) rc = failf("download of the results failed: %s", hipGetErrorString(e));
    }
    if (finish_call(st, rc, c.amplitudes ? "amplitudes" : "sampling")) return 1;
    for (int s = 0; s < nstates; ++s)
        for (size_t k = 0; k < work[s]->h_status.size(); ++k)
            if (work[s]->h_status[k])
                return failf("lane %d, shot %llu: the weights of the two branches do not add up to a finite positive number", s,
                             (unsigned long long)(c.first_shot + k));
    return 0;
}

}  // namespace

extern "C" {

int aqc_mps_sample_route(int n, const int32_t* dims) {
    if (!dims || n < 1) return -1;
    return mps_sample_route(n, dims);
}

int aqc_mps_sample(aqc_mps* const* states, int nstates, int64_t shots, uint64_t first_shot, uint64_t seed, int method, uint8_t* bits, double* amps,
                   double* norm2) {
    if (!states || !bits) return failf("null argument");
    if (const char* msg = mps_sample_check_counts(nstates, shots)) return failf("%s", msg);
    if (!mps_sample_method_ok(method)) return failf("unknown method %d", method);
    Call c;
    if (check_states(states, nullptr, nstates, 1, &c.n, &c.device)) return 1;
    c.nstates = nstates;
    c.count = shots;
    c.first_shot = first_shot;
    c.seed = seed;
    return run(states, c, method, nullptr, bits, amps, norm2);
}

int aqc_mps_amplitudes(aqc_mps* const* states, int nstates, int64_t count, const uint8_t* bits, int method, double* amps) {
    if (!states || !bits || !amps) return failf("null argument");
    if (const char* msg = mps_sample_check_counts(nstates, count)) return failf("%s", msg);
    if (!mps_sample_method_ok(method)) return failf("unknown method %d", method);
    Call c;
    if (check_states(states, nullptr, nstates, 1, &c.n, &c.device)) return 1;
    const int64_t bad = mps_sample_bad_bit(bits, (size_t)count * c.n);
    if (bad >= 0) return failf("bit string %lld, qubit %lld: a bit is 0 or 1, not %d", (long long)(bad / c.n), (long long)(bad % c.n), (int)bits[bad]);
    c.nstates = nstates;
    c.count = count;
    c.amplitudes = true;
    return run(states, c, method, bits, nullptr, amps, nullptr);
}

}  // extern "C"
