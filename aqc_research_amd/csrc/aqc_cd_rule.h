// The two rules of coordinate-descent AQC (aqc_cd.hip), HIP-free: the same text is compiled for the device and by a plain C++
// compiler (tests/native/cd_rule_selftest.cpp).
//   step rule   the Newton / gradient step of one parameter from (grad sum, <w|z>)          core_op_matrix.py:833-850
//   close rule  what the end of a sweep does to a lane of the driver loop                   aqc_coord_descent.py:81-101
// The reference's third exit, the time limit, is not here: the host looks at its clock between chunks of sweeps, so a lane is
// marked AQC_CD_TIMEOUT at chunk granularity (aqc_ws_cd_minimize), never in the middle of a chunk.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define AQC_CD_FN __host__ __device__ inline
#else
#define AQC_CD_FN inline
#endif

namespace aqc {

enum { kCdRunning = 0, kCdNormal = 1, kCdEarly = 2, kCdTimeout = 3 };   // AQC_CD_* of include/aqc_hip.h

// kind: 0 = Y (ry), 1 = Z (rz), 2 = X (rx).  (gr, gi) = sum of the kind's products, (pr, pi) = <w|z>, inv_d2n = 1 / d^2.
AQC_CD_FN void cd_delta(int kind, double gr, double gi, double pr, double pi, double inv_d2n, double& dt_out) {
    // grad = f * S with f = 0.5 (Y) or 0.5j (Z, X)   (core_op_matrix.py:284-389)
    double g_re, g_im;
    if (kind == 0) { g_re = 0.5 * gr; g_im = 0.5 * gi; } else { g_re = -0.5 * gi; g_im = 0.5 * gr; }
    // _delta_theta (core_op_matrix.py:833-850); d^2 is a power of two: multiplying by its reciprocal IS the division
    double d1 = (-2.0 * (pr * g_re + pi * g_im)) * inv_d2n;
    const double d2 = (-2.0 * (g_re * g_re + g_im * g_im) + 0.5 * (pr * pr + pi * pi)) * inv_d2n;
    const double tol = 1.4901161193847656e-08, lr = 0.19634954084936207, maxdt = 0.78539816339744831;
    double dt;
    if (d2 < tol) { d1 /= fmax(fabs(d1), 1.0); dt = -lr * d1; } else { dt = -d1 / d2; }
    // |dt| <= max_delta_theta: dt / |dt / maxdt| is maxdt with the sign of dt (:849-850); NaN steps are left alone like there
    if (fabs(dt) > maxdt) dt = copysign(maxdt, dt);
    dt_out = dt;
}

// One lane at the end of a sweep, in the reference's order: the profile entry and the sweep count, the best value so far, then the
// exits -- a small objective ends the lane as "early" before a small step or the last sweep end it as "normal".  Returns true when
// the sweep's thetas are the best so far: the caller copies them (that part is parallel work on the device).
AQC_CD_FN bool cd_close(double fobj, double dtheta_max, double fobj_thr, double dtheta_thr, int maxiter, double* profile, int& nit,
                        double& best_f, int& status) {
    profile[nit] = fobj;
    ++nit;
    const bool improved = fobj < best_f;
    if (improved) best_f = fobj;
    if (fobj < fobj_thr) status = kCdEarly;
    else if (dtheta_max < dtheta_thr) status = kCdNormal;
    else if (nit == maxiter) status = kCdNormal;
    return improved;
}

}  // namespace aqc
