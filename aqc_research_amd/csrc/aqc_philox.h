// Philox4x64-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator behind
// np.random.Philox, for the sketching-vector draws (aqc_sketch.hip).  HIP-free: the same text is compiled for the device
// and by a plain C++ compiler (tests/native/philox_selftest.cpp).
//
// Draw rule of the sketching generators.  A plane is d*k doubles of one lane; element e of plane p, lane l, sketch number
// (iteration) it, is word e % 4 of the block
//     philox4x64_10(counter = {1 + e / 4, it, l, p}, key = {seed, stream})
// turned into a uniform double of [0, 1) by (word >> 11) * 2^-53.  NumPy advances the counter BEFORE its first block, so
//     np.random.Generator(np.random.Philox(key=[seed, stream], counter=[0, it, l, p])).random(d * k)
// is that plane bit for bit.  stream = the generator kind (AQC_SKETCH_RAND / AQC_SKETCH_EIGEN of include/aqc_hip.h).
//   rand : Omega = plane 0 + i plane 1                                                    (sk_core.py:329-356)
//   eigen: Omega = N(planes 0, 1) + i N(planes 2, 3), N(u1, u2) = sqrt(-2 log(1 - u1)) cos(2 pi u2)   (Box-Muller; :404-464)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AQC_PHILOX_FN __host__ __device__ inline
#else
#define AQC_PHILOX_FN inline
#endif

namespace aqc {

AQC_PHILOX_FN uint64_t philox_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// out[4] <- the block of counter ctr[4] (ctr[0] least significant) under key[2]
AQC_PHILOX_FN void philox4x64_10(const uint64_t ctr[4], const uint64_t key[2], uint64_t out[4]) {
    const uint64_t M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    const uint64_t W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
    uint64_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
        const uint64_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ctr <- ctr + n as one 256-bit number (what NumPy's generator does between blocks, with n = 1)
AQC_PHILOX_FN void philox_advance(uint64_t ctr[4], uint64_t n) {
    for (int i = 0; i < 4 && n; ++i) {
        const uint64_t before = ctr[i];
        ctr[i] += n;
        n = ctr[i] < before ? 1 : 0;
    }
}

AQC_PHILOX_FN double philox_uniform(uint64_t word) { return (double)(word >> 11) * (1.0 / 9007199254740992.0); }

// element e of the plane (it, lane, plane) under (seed, stream): see the head of this file
AQC_PHILOX_FN double philox_plane_uniform(uint64_t seed, uint64_t stream, uint64_t it, uint64_t lane, uint64_t plane, uint64_t e) {
    const uint64_t ctr[4] = {1 + (e >> 2), it, lane, plane}, key[2] = {seed, stream};
    uint64_t out[4];
    philox4x64_10(ctr, key, out);
    return philox_uniform(out[e & 3]);
}

}  // namespace aqc
