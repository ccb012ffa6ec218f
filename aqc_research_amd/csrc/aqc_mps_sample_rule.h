// The rules of measuring MPS states (aqc_mps_sample.hip, aqc_mps_sample_api.cpp), HIP-free: the same text is compiled into the library
// and by a plain C++ compiler (tests/native/mps_sample_rule_selftest.cpp); tests/mps_sample_ref.py states the result in NumPy.
// Notation of aqc_mps_obs_rule.h:
//   state       psi(b) = T_0[b_0] T_1[b_1] ... T_{n-1}[b_{n-1}], site tensors [2][chi_q][chi_{q+1}], any gauge; bits[s][q] = qubit q = site q
//   R_n = [1]   R_q[x][y] = sum_c sum_uv T_q[c][x][u] R_{q+1}[u][v] conj(T_q[c][y][v])
// Shot s of lane l (the position of the state in the call) starts with v = [1] and takes, for q = 0 .. n - 1,
//   w_c = v T_q[c]                                       c = 0, 1     (row vector of length chi_{q+1})
//   m_c = Re sum_uv w_c[u] R_{q+1}[u][v] conj(w_c[v])                 (both weights are computed, none is a difference)
//   u   = uniform(seed, l, s, q)
//   bit = 0 if u (m_0 + m_1) < m_0 else 1                             (mps_sample_decide)
//   v   = w_bit
// without rescaling: after the last site v is the scalar psi(b), and p(b) = |psi(b)|^2 / R_0.  R_0 = <psi|psi> is m_0 + m_1 of site 0,
// which is the same number in every shot.  A branch of exactly zero weight is never taken (u < 1, so u tot < tot; and 0 < 0 is false).
// m_0 + m_1 not finite or <= 0 is an error of that shot (mps_sample_weights_ok), never a quiet bit.
// Draw rule, in the style of the head of aqc_philox.h: uniform(seed, l, s, q) is word q % 4 of the block
//     philox4x64_10(counter = {1 + q / 4, s, l, 0}, key = {seed, AQC_SAMPLE_STREAM})
// through philox_uniform, so np.random.Generator(np.random.Philox(key=[seed, AQC_SAMPLE_STREAM], counter=[0, s, l, 0])).random(n) gives
// the n uniforms of shot s bit for bit: a shot depends on (state, seed, lane, shot number) alone, not on the number of shots in the
// call, on where a chunk of shots begins or on the other states.
// Amplitudes of given bit strings follow the same walk with the bit given; no weights, no environments.
//   route       fused (a workgroup walks the whole chain for 64 shots inside one launch, v in LDS) when every bond dimension of the state
//               is <= kMpsSampleFusedCap, else gemm (shots x chi matrices in memory, four zgemm launches and a row kernel per site, the
//               shots walked in chunks of mps_sample_chunk).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "aqc_mps_obs_rule.h"
#include "aqc_philox.h"

namespace aqc {

enum { kMpsSampleFusedCap = 64, kMpsSampleBlockShots = 64 };
enum { kMpsSampleByRule = 0, kMpsSampleFused = 1, kMpsSampleGemm = 2 };
constexpr uint64_t kMpsSampleStream = 16;                       // AQC_SAMPLE_STREAM of include/aqc_hip.h
constexpr int64_t kMpsSampleMaxShots = (int64_t)1 << 24;        // per call
constexpr size_t kMpsSampleScratch = kMpsCallBudget;            // bytes of shots x chi matrices a chunk of the gemm route may take
constexpr int64_t kMpsSampleMaxChunk = (int64_t)1 << 20;        // rows of one zgemm launch
enum { kMpsSampleGemmMats = 5 };                                // V, W_0, W_1, G_0, G_1

// the four uniforms of sites 4 blk .. 4 blk + 3 of shot `shot` of lane `lane`
AQC_PHILOX_FN void mps_sample_block(uint64_t seed, uint64_t lane, uint64_t shot, uint64_t blk, uint64_t out[4]) {
    const uint64_t ctr[4] = {1 + blk, shot, lane, 0}, key[2] = {seed, kMpsSampleStream};
    philox4x64_10(ctr, key, out);
}
AQC_PHILOX_FN double mps_sample_uniform(uint64_t seed, uint64_t lane, uint64_t shot, uint64_t q) {
    uint64_t out[4];
    mps_sample_block(seed, lane, shot, q >> 2, out);
    return philox_uniform(out[q & 3]);
}

AQC_PHILOX_FN int mps_sample_decide(double u, double m0, double m1) { return u * (m0 + m1) < m0 ? 0 : 1; }
AQC_PHILOX_FN bool mps_sample_weights_ok(double m0, double m1) {
    const double tot = m0 + m1;
    return tot > 0.0 && tot - tot == 0.0;   // positive and finite (NaN fails the first test, +inf the second)
}

// dims: the n + 1 bond dimensions
inline int mps_sample_route(int n, const int* dims) { return mps_max_bond(n, dims) <= kMpsSampleFusedCap ? kMpsSampleFused : kMpsSampleGemm; }

// shots walked together by the gemm route: as many as keep the kMpsSampleGemmMats matrices [chunk][max_bond] within the scratch,
// at least 64, at most what one launch takes and no more than the call has
inline int64_t mps_sample_chunk(int max_bond, int64_t shots) {
    const size_t per_shot = sizeof(double) * 2 * (size_t)kMpsSampleGemmMats * (size_t)(max_bond < 1 ? 1 : max_bond);
    int64_t c = (int64_t)(kMpsSampleScratch / per_shot);
    if (c < kMpsSampleBlockShots) c = kMpsSampleBlockShots;
    if (c > kMpsSampleMaxChunk) c = kMpsSampleMaxChunk;
    if (c > shots) c = shots;
    return c < 1 ? 1 : c;
}

// validity of the arguments that need no state: null where a message is returned
inline const char* mps_sample_check_counts(int nstates, int64_t shots) {
    if (nstates < 1) return "at least one state is needed";
    if (shots < 1) return "at least one shot is needed";
    if (shots > kMpsSampleMaxShots) return "at most 2^24 shots per call";
    return nullptr;
}
inline bool mps_sample_method_ok(int method) { return method == kMpsSampleByRule || method == kMpsSampleFused || method == kMpsSampleGemm; }
// index of the first value other than 0 / 1, -1: none
inline int64_t mps_sample_bad_bit(const uint8_t* bits, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (bits[i] > 1) return (int64_t)i;
    return -1;
}

}  // namespace aqc
