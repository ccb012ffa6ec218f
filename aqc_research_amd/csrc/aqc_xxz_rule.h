// The rules of exact XXZ time evolution (aqc_xxz.hip), HIP-free: the same text is compiled for the device and by a plain C++
// compiler (tests/native/xxz_rule_selftest.cpp); tests/xxz_ref.py states the same rules in NumPy.
//   H = -1/4 sum_{i=0}^{n-2} (X_i X_{i+1} + Y_i Y_{i+1} + delta Z_i Z_{i+1})      open chain, half-spin convention (trotter.py:183-230)
//   action   (H psi)(s) = diag(s) psi(s) - 1/2 sum_{i : bit i of a(s)} psi(s ^ (3 << i)),  a(s) = (s ^ (s >> 1)) & (2^(n-1) - 1):
//            bit i of a(s) is set where qubits i and i + 1 differ; diag(s) = -(delta / 4) (n - 1 - 2 popcount(a(s)))
//   radius   R = (n - 1) (1/2 + |delta| / 4) >= ||H||
//   series   exp(-i H t) psi = sum_{k=0}^{K} c_k T_k(H / R) psi with x = R t, c_0 = J_0(x), c_k = 2 (-i)^k J_k(x);
//            K = the smallest k >= ceil(|x|) + 20 with |J_k(|x|)| <= 1e-17
//   Bessel   J_0 .. J_K(|x|) by Miller's downward recurrence, normalised with J_0 + 2 sum_m J_2m = 1
// All index arithmetic is 64-bit: n goes up to 30 and lanes << n up to 2^kMaxBits.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define AQC_XXZ_FN __host__ __device__ inline
#else
#define AQC_XXZ_FN inline
#endif

namespace aqc {

enum { kXxzMinQubits = 2, kXxzMaxQubits = 30, kXxzMaxTerms = 1 << 16 };

// anti-alignment mask: bit i is set where qubits i and i + 1 of the basis state s differ
AQC_XXZ_FN uint64_t xxz_anti(uint64_t s, int n) { return (s ^ (s >> 1)) & (((uint64_t)1 << (n - 1)) - 1); }
// the diagonal of H at a state with anti-alignment mask a: aligned bonds count -delta/4, the others +delta/4
AQC_XXZ_FN double xxz_diag(uint64_t a, int n, double delta) { return -(0.25 * delta) * (double)(n - 1 - 2 * __builtin_popcountll(a)); }
// the state bond i couples s to (both qubits flipped; only where bit i of a(s) is set)
AQC_XXZ_FN uint64_t xxz_partner(uint64_t s, int i) { return s ^ ((uint64_t)3 << i); }
AQC_XXZ_FN double xxz_radius(int n, double delta) { return (double)(n - 1) * (0.5 + 0.25 * fabs(delta)); }

// J_0 .. J_K(ax) for ax = |x| >= 0 into J (resized to K + 1) and K, the series length; -1 when K would pass kXxzMaxTerms or ax is
// not finite.  Host only.
inline int xxz_series(double ax, std::vector<double>& J) {
    if (!(ax >= 0.0) || !isfinite(ax) || ax > (double)kXxzMaxTerms) return -1;
    const int kmin = (int)ceil(ax) + 20;
    // the start of the downward recurrence: J_k(x) falls below 1e-17 near k = x + 11.6 x^(1/3) and the error the start leaves
    // in J_k is (J_start / J_k)^2, so 40 + 25 x^(1/3) indices above kmin put it far below one rounding
    int start = kmin + 40 + (int)(25.0 * cbrt(ax));
    start += start & 1;
    std::vector<double> f((size_t)start + 2, 0.0);
    if (ax < 1e-8) {
        // (x/2)^k / k!: the next term of the power series is smaller by x^2 / (4 (k + 1)) < 1e-16
        f[0] = 1.0;
        for (int k = 1; k <= start; ++k) f[k] = f[k - 1] * (0.5 * ax) / (double)k;
    } else {
        f[start + 1] = 0.0;
        f[start] = 1.0;
        for (int k = start; k >= 1; --k) {
            f[k - 1] = (2.0 * (double)k / ax) * f[k] - f[k + 1];
            if (fabs(f[k - 1]) > 1e200)   // rescale what has been computed; entries that underflow are zero at this precision
                for (int m = k - 1; m <= start; ++m) f[m] *= 1e-200;
        }
        double norm = 0.0;   // J_0 + 2 (J_2 + J_4 + ...) = 1, summed from the small end
        for (int m = start; m >= 2; m -= 2) norm += 2.0 * f[m];
        norm += f[0];
        const double inv = 1.0 / norm;
        for (int k = 0; k <= start; ++k) f[k] *= inv;
    }
    int K = kmin;
    while (K <= start && fabs(f[K]) > 1e-17) ++K;
    if (K > start || K > kXxzMaxTerms) return -1;
    J.assign(f.begin(), f.begin() + K + 1);
    return K;
}

// c_k of the series for the signed x = R t from J_k(|x|): J_k(-x) = (-1)^k J_k(x), (-i)^k = 1, -i, -1, i
inline void xxz_coefficient(int k, double jk_abs, bool negative_x, double& re, double& im) {
    const double j = (negative_x && (k & 1)) ? -jk_abs : jk_abs;
    const double m = k == 0 ? j : 2.0 * j;
    switch (k & 3) {
        case 0: re = m; im = 0.0; break;
        case 1: re = 0.0; im = -m; break;
        case 2: re = -m; im = 0.0; break;
        default: re = 0.0; im = m; break;
    }
}

}  // namespace aqc
