// Host-side helpers shared by the single-lane MPS engine (aqc_mps_engine.cpp) and the lockstep lanes (aqc_mps_batch.cpp): error
// reporting, the checks of a circuit description and of a block range.  The gates themselves -- 2 x 2 algebra, entangler matrices, the block list and the walk of
// an ansatz -- are stated in aqc_mps_walk.h (included through aqc_launch.h), the skeleton that executes a gradient walk in
// aqc_mps_gradwalk.h.  Private to csrc/ (everything has internal linkage).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/aqc_hip.h"
#include "aqc_launch.h"
#include "aqc_mps_gradwalk.h"

namespace aqc {
// device pointers of site q of a single-lane MPS (T_q, and the Schmidt vector of bond q when q < n - 1) after its stream has drained:
// how the lockstep lanes take a copy of a state built by the single-lane engine (defined in aqc_mps_engine.cpp)
int mps_peek(const aqc_mps* m, int q, const void** site, const double** lam);
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
