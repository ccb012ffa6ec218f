// C ABI (include/aqc_hip.h): shots and amplitudes of single-lane MPS states.  Rules: aqc_mps_sample_rule.h; kernels: aqc_mps_sample.hip.
#include <algorithm>
#include <memory>
#include <vector>

#include "aqc_devbuf.h"
#include "aqc_mps_host.h"
#include "aqc_mps_sample_rule.h"

using namespace aqc;

namespace {

// everything one state's launches read or write; alive until the call's last synchronisation
struct StateWork {
    int n = 0, route = 0;
    std::vector<int> dims;
    std::vector<const double2*> t;
    std::vector<size_t> off;                          // env offsets, n + 2 entries (the last = total)
    DevBuf<double2> env_l, env_r, tmp, mats, amps;
    DevBuf<unsigned char> bits, status;
    DevBuf<double> norm2;
    DevBuf<const double2*> d_sites;
    DevBuf<int> d_dims;
    DevBuf<size_t> d_off;
    std::vector<unsigned char> h_status;
};

struct Call {
    int n = 0, nstates = 0;
    int64_t count = 0;                                // shots, or bit strings
    uint64_t first_shot = 0, seed = 0;
    bool amplitudes = false;
    const unsigned char* d_bits_in = nullptr;         // amplitudes: [count][n] on the device
};

// R_n .. R_1 of <psi|psi>: fused route on the matrix cores (the sweep of the observables, whose left half comes with it), gemm route
// with the engine's environment step on the pair (psi, psi)
int environments(StateWork& w, hipStream_t st) {
    const int n = w.n;
    const size_t total = w.off[n + 1];
    static const double one[2] = {1.0, 0.0};
    if (w.env_r.alloc(total)) return 1;
    HIP_OK(hipMemcpyAsync(w.env_r + w.off[n], one, sizeof one, hipMemcpyHostToDevice, st));
    const int* dims = w.dims.data();
    if (w.route == kMpsSampleFused) {
        if (w.env_l.alloc(total)) return 1;
        HIP_OK(hipMemcpyAsync(w.env_l + w.off[0], one, sizeof one, hipMemcpyHostToDevice, st));
        MpsObsFusedArgs a{};
        a.n = n;
        a.sites = w.d_sites;
        a.dims = w.d_dims;
        a.env_off = w.d_off;
        a.env_l = w.env_l;
        a.env_r = w.env_r;
        HIP_OK(launch_mps_obs_env(a, st));
        return 0;
    }
    size_t tmax = 1;
    for (int q = 0; q < n; ++q) tmax = std::max(tmax, (size_t)dims[q] * dims[q + 1]);
    if (w.tmp.alloc(tmax)) return 1;
    for (int q = n - 1; q >= 1; --q)
        if (env_right(st, w.env_r + w.off[q + 1], w.t[q], w.t[q], site_dims(dims, dims, q), w.tmp, w.env_r + w.off[q])) return 1;
    return 0;
}

// the shots walked in chunks: per site V T_0, V T_1, W_0 R, W_1 R and the row kernel
int run_gemm(StateWork& w, const Call& c, int lane, hipStream_t st) {
    const int n = w.n;
    const int maxb = mps_obs_max_bond(n, w.dims.data());
    const int64_t chunk = mps_sample_chunk(maxb, c.count);
    const size_t mat = (size_t)chunk * maxb;
    if (w.mats.alloc(kMpsSampleGemmMats * mat)) return 1;
    double2 *v = w.mats, *w0 = v + mat, *w1 = w0 + mat, *g0 = w1 + mat, *g1 = g0 + mat;
    for (int64_t s0 = 0; s0 < c.count; s0 += chunk) {
        const int rows = (int)std::min<int64_t>(chunk, c.count - s0);
        HIP_OK(launch_mps_sample_ones(v, rows, st));
        for (int q = 0; q < n; ++q) {
            const int x = w.dims[q], u = w.dims[q + 1];
            const double2* t0 = w.t[q];
            const double2* t1 = t0 + (size_t)x * u;
            HIP_OK(launch_zgemm(false, false, rows, u, x, v, x, t0, u, w0, u, st));
            HIP_OK(launch_zgemm(false, false, rows, u, x, v, x, t1, u, w1, u, st));
            if (!c.amplitudes) {
                const double2* r = w.env_r + w.off[q + 1];
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
    HIP_OK(hipSetDevice(aqc_mps_device(states[0])));
    hipStream_t st = mps_stream(states[0]);
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
    for (int s = 0; s < nstates && !rc; ++s) {
        work.emplace_back(new StateWork());
        StateWork& w = *work.back();
        w.n = n;
        w.dims.resize(n + 1);
        w.t.resize(n);
        if (aqc_mps_dims(states[s], w.dims.data())) { rc = 1; break; }
        for (int q = 0; q < n && !rc; ++q) {   // (mps_peek drains the state's own stream)
            const void* site = nullptr;
            const double* lam = nullptr;
            rc = mps_peek(states[s], q, &site, &lam);
            w.t[q] = static_cast<const double2*>(site);
        }
        if (rc) break;
        w.off = mps_obs_env_offsets(n, w.dims.data());
        const int maxb = mps_obs_max_bond(n, w.dims.data());
        w.route = method == kMpsSampleByRule ? mps_sample_route(n, w.dims.data()) : method;
        if (w.route == kMpsSampleFused && maxb > kMpsSampleFusedCap) {
            rc = failf("the fused route takes bond dimensions up to %d; state %d has %d", (int)kMpsSampleFusedCap, s, maxb);
            break;
        }
        if (w.amps.alloc((size_t)c.count)) { rc = 1; break; }
        if (!c.amplitudes) {
            if (w.bits.alloc((size_t)c.count * n) || w.status.alloc((size_t)c.count) || w.norm2.alloc(1)) { rc = 1; break; }
            if (hipMemsetAsync(w.status, 0, (size_t)c.count, st) != hipSuccess) { rc = failf("clearing the status failed"); break; }
        }
        if (w.route == kMpsSampleFused) {
            std::vector<const double2*> sites(w.t.begin(), w.t.end());
            if (w.d_sites.upload(sites) || w.d_dims.upload(w.dims) || w.d_off.upload(w.off)) { rc = 1; break; }
        }
        if (!c.amplitudes && (rc = environments(w, st))) break;
        if (w.route == kMpsSampleFused) {
            MpsSampleState e{};
            e.sites = w.d_sites; e.dims = w.d_dims; e.env_off = w.d_off; e.env_r = w.env_r;
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
    const hipError_t e = hipStreamSynchronize(st);   // before any buffer goes, also after a failure
    if (rc) return 1;
    if (e != hipSuccess) return failf("%s failed: %s", c.amplitudes ? "amplitudes" : "sampling", hipGetErrorString(e));
    for (int s = 0; s < nstates; ++s)
        for (size_t k = 0; k < work[s]->h_status.size(); ++k)
            if (work[s]->h_status[k])
                return failf("lane %d, shot %llu: the weights of the two branches do not add up to a finite positive number", s,
                             (unsigned long long)(c.first_shot + k));
    return 0;
}

// the checks on the states that both entry points share; *n_out = the number of qubits
int check_states(aqc_mps* const* states, int nstates, int* n_out) {
    for (int s = 0; s < nstates; ++s)
        if (!states[s]) return failf("null state");
    const int n = aqc_mps_num_qubits(states[0]), device = aqc_mps_device(states[0]);
    if (n < 1) return failf("a state needs at least 1 qubit");
    for (int s = 1; s < nstates; ++s)
        if (aqc_mps_num_qubits(states[s]) != n || aqc_mps_device(states[s]) != device) return failf("MPS states differ in size or device");
    *n_out = n;
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
    if (check_states(states, nstates, &c.n)) return 1;
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
    if (check_states(states, nstates, &c.n)) return 1;
    const int64_t bad = mps_sample_bad_bit(bits, (size_t)count * c.n);
    if (bad >= 0) return failf("bit string %lld, qubit %lld: a bit is 0 or 1, not %d", (long long)(bad / c.n), (long long)(bad % c.n), (int)bits[bad]);
    c.nstates = nstates;
    c.count = count;
    c.amplitudes = true;
    return run(states, c, method, bits, nullptr, amps, nullptr);
}

}  // extern "C"
