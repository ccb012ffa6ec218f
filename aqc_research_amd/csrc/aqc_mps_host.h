// Host-side helpers shared by the single-lane MPS engine (aqc_mps_engine.cpp) and the lockstep lanes (aqc_mps_batch.cpp): error
// reporting, the checks of a circuit description and of a block range.  The gates themselves -- 2 x 2 algebra, entangler matrices, the block list and the walk of
// an ansatz -- are stated in aqc_mps_walk.h (included through aqc_launch.h), the skeleton that executes a gradient walk in
// aqc_mps_gradwalk.h, the site step of a pair of states in aqc_mps_contract.h; its device executor and the small-or-gemm choice of an
// environment step are here.  Private to csrc/ (everything has internal linkage).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/aqc_hip.h"
#include "aqc_launch.h"
#include "aqc_mps_contract.h"
#include "aqc_mps_gradwalk.h"

namespace aqc {
// device pointers of site q of a single-lane MPS (T_q, and the Schmidt vector of bond q when q < n - 1) after its stream has drained:
// how the lockstep lanes take a copy of a state built by the single-lane engine (defined in aqc_mps_engine.cpp)
int mps_peek(const aqc_mps* m, int q, const void** site, const double** lam);
// all of a state at once for the calls that only read it (aqc_mps_call.h): its n + 1 bond dimensions and the device pointers of its n
// sites, after ONE drain of its stream
int mps_view(const aqc_mps* m, int* dims, const double2** sites);
// the reverse: a new single-lane MPS from tensors that live on the device (site q: [2][dims[q]][dims[q+1]] complex, T_q = Gamma_q lambda_q;
// lams[q]: the dims[q+1] Schmidt values of bond q), copied
int mps_adopt(int device, int n, const int* dims, const void* const* sites, const double* const* lams, double discarded, aqc_mps** out);
// the stream a single-lane MPS orders its work on (aqc_mps_obs_api.cpp enqueues on the first state's, as aqc_mps_dot_ops does)
hipStream_t mps_stream(const aqc_mps* m);
}  // namespace aqc

namespace {

[[maybe_unused]] int failf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return aqc::set_error(buf);
}

#define HIP_OK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return failf("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// ---- the site steps of aqc_mps_contract.h on the device: the products on one stream
struct StreamOps {
    hipStream_t st;
    int gemm(bool conj_t, bool accum, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc) {
        HIP_OK(launch_zgemm(conj_t, accum, M, N, K, A, lda, B, ldb, C, ldc, st));
        return 0;
    }
    int gemm_bh(bool conj_t, bool accum, int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc) {
        HIP_OK(launch_zgemm_bh(conj_t, accum, M, N, K, A, lda, B, ldb, C, ldc, st));
        return 0;
    }
};

// An operator G on A's side is read off B's: <G a|b> = <a|G^H b>.  The packed G^H, or null without an operator ...
[[maybe_unused]] const double* adjoint8(const M2* op, double* g8) {
    if (!op) return nullptr;
    pack(adjoint(*op), g8);
    return g8;
}
// ... and site p of B seen through it: B_p itself without an operator, else `scratch` ([2][ne]) after one launch; null after a failure
[[maybe_unused]] const double2* site_through(hipStream_t st, const double2* b_p, size_t ne, const double* gh8, double2* scratch) {
    if (!gh8) return b_p;
    const hipError_t e = launch_gate1q(b_p, scratch, 1, ne, 0, gh8, st);
    if (e == hipSuccess) return scratch;
    failf("launch_gate1q failed: %s", hipGetErrorString(e));
    return nullptr;
}

// An environment step through site p (gh8: an operator on A's side): ONE launch when the bonds are small, the operator folded in;
// else the products of contract_left / contract_right (tmp as they size it), the site of B first taken through G^H into `bsite`.
[[maybe_unused]] int env_left(hipStream_t st, const double2* in, const double2* a_p, const double2* b_p, const SiteDims& d, const double* gh8,
                              double2* bsite, double2* tmp, double2* out) {
    if (mps_env_fits_small(d.xa, d.ua, d.yb, d.vb)) {
        HIP_OK(launch_mps_env_left(in, a_p, b_p, d.xa, d.ua, d.yb, d.vb, gh8, out, st));
        return 0;
    }
    b_p = site_through(st, b_p, (size_t)d.yb * d.vb, gh8, bsite);
    StreamOps ops{st};
    return !b_p || contract_left(ops, in, a_p, b_p, d, tmp, out);
}
[[maybe_unused]] int env_right(hipStream_t st, const double2* rc, const double2* a_p, const double2* b_p, const SiteDims& d, double2* tmp, double2* out) {
    if (mps_env_fits_small(d.xa, d.ua, d.yb, d.vb)) {
        HIP_OK(launch_mps_env_right(rc, a_p, b_p, d.xa, d.ua, d.yb, d.vb, out, st));
        return 0;
    }
    StreamOps ops{st};
    return contract_right(ops, rc, a_p, b_p, d, tmp, out);
}

[[maybe_unused]] int check_circuit(const aqc_circuit* c, int n) {
    if (!c || !c->blocks) return failf("null circuit description");
    if (c->num_qubits != n) return failf("circuit and MPS differ in the number of qubits");
    if (c->entangler != AQC_CX && c->entangler != AQC_CZ && c->entangler != AQC_CP) return failf("unknown entangler");
    if (c->num_blocks < 0) return failf("negative number of blocks");
    for (int b = 0; b < c->num_blocks; ++b) {
        const int ct = c->blocks[b], tg = c->blocks[c->num_blocks + b];
        if (ct < 0 || ct >= n || tg < 0 || tg >= n || ct == tg) return failf("block %d couples invalid qubits", b);
    }
    return 0;
}

// block range of a gradient walk: block_from < 0 stands for all blocks of the circuit
[[maybe_unused]] int check_block_range(const aqc_circuit* c, int& block_from, int& block_to) {
    if (block_from < 0) { block_from = 0; block_to = c->num_blocks; }
    if (block_from > block_to || block_to > c->num_blocks) return failf("invalid block range");
    return 0;
}

}  // namespace
