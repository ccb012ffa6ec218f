// Coordinate-descent sweep (core_op_matrix.py:765-917).  Parameters are strictly sequential (Gauss-Seidel); each needs
// grad = 0.5j<P w|z> and prod = <w|z>, the Newton / gradient step from them (cd_delta, aqc_cd_rule.h), and the rotation with the
// OLD angle on z and the NEW angle on w.  Two routes, both driven by the host's segment list: one persistent launch where the
// operands fit LDS, and a walk of plain launches (one per parameter, one per segment) where they do not.  No host round trip
// inside a sweep on either.
#include <hip/hip_runtime.h>

#include "aqc_cd_rule.h"
#include "aqc_lanes.h"
#include "aqc_launch.h"

namespace aqc {

typedef double2 cplx;

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ size_t pair_index(size_t g, int hbit) {
    const size_t lo = g & (((size_t)1 << hbit) - 1);
    return ((g >> hbit) << (hbit + 1)) | lo;
}

// kind: 0 = Y (ry), 1 = Z (rz), 2 = X (rx)
__device__ __forceinline__ void rot_pair(int kind, cplx& a0, cplx& a1, double c, double s) {
    if (kind == 0) {  // Ry
        const cplx t0 = make_double2(c * a0.x - s * a1.x, c * a0.y - s * a1.y);
        const cplx t1 = make_double2(s * a0.x + c * a1.x, s * a0.y + c * a1.y);
        a0 = t0; a1 = t1;
    } else if (kind == 1) {  // Rz
        a0 = make_double2(c * a0.x + s * a0.y, c * a0.y - s * a0.x);
        a1 = make_double2(c * a1.x - s * a1.y, c * a1.y + s * a1.x);
    } else {  // Rx
        const cplx t0 = make_double2(c * a0.x + s * a1.y, c * a0.y - s * a1.x);
        const cplx t1 = make_double2(s * a0.y + c * a1.x, c * a1.y - s * a0.x);
        a0 = t0; a1 = t1;
    }
}

// ---- the whole sweep -- or many sweeps -- as ONE persistent launch ------------------------------------------------------
// Up to 6 qubits the two d x d operands of the walk fit one workgroup's LDS (2 x 16 KiB at d = 32, 2 x 64 KiB at d = 64), so a
// workgroup per lane holds w and z for the whole walk: no launch per parameter, no HBM round trip between parameters.  Lanes
// are independent problems (random restarts of one ansatz, different targets).  Per sweep and lane:
//   theta -> (cos, sin) of every half angle (all threads in parallel);
//   z <- target (HBM -> LDS), z <- V(theta)^H z in LDS (v_dagger_mul_mat, core_op_matrix.py:562-642), w <- I;
//   the Gauss-Seidel walk of core_op_matrix.py:852-912;
//   fobj = 1 - |<w|z>|^2 / d^2 (:917).
// The walk is cut into SEGMENTS: a front-layer qubit (3 parameters) or a unit block (entangler + 4 parameters).  All gates of a
// segment act on two address bits (a, b), so a thread takes the 4 elements of w and of z that differ in exactly those bits into
// registers ONCE per segment: the entangler is a register permutation, each parameter is
//   partial inner products on the thread's two pairs -> wave reduction (4 sums in 7 exchange steps: the butterfly transposes
//   while it adds) -> the waves' partials through LDS, one barrier -> the Newton / gradient step worked out by EVERY thread from
//   the same numbers in the same order (identical arithmetic, nothing to broadcast) -> z rotated by the old angle, w by the new
//   one, in registers;
// and the group goes back to LDS when the segment ends (first version: every parameter read both operands from LDS twice and
// wrote them once -- 96 KiB of LDS traffic per parameter and lane at d = 32; now 64 KiB per SEGMENT).
struct CdSeg {
    int32_t ha, hb;       // address bits of the segment's two qubits: a = control / the front-layer qubit, b = target / any other qubit
    int32_t ent;          // 0 none (front layer), 1 CX, 2 CZ -- applied to both operands before the rotations
    int32_t nrot;         // parameters of the segment (3 or 4)
    int32_t kind[4];      // 0 Ry, 1 Rz, 2 Rx
    int32_t on_b[4];      // rotated qubit: 0 = a, 1 = b
    int32_t tindex[4];    // index of the parameter
};

// (the step rule, cd_delta, lives in aqc_cd_rule.h: the driver's close rule sits next to it and a host program tests both)

// cos / sin of x for |x| <= pi / 8 (half of a step that is clamped to pi / 4): Taylor polynomials in x^2, remainders < 1e-20
__device__ __forceinline__ void sincos_small(double x, double& s, double& c) {
    const double x2 = x * x;
    double ps = -7.6471637318198164759e-13;           // -1/15!
    double pc = -1.1470745597729724714e-11;           // -1/14!
    ps = fma(ps, x2, 1.6059043836821614599e-10);      //  1/13!
    pc = fma(pc, x2, 2.0876756987868098979e-09);      //  1/12!
    ps = fma(ps, x2, -2.5052108385441718775e-08);     // -1/11!
    pc = fma(pc, x2, -2.7557319223985890653e-07);     // -1/10!
    ps = fma(ps, x2, 2.7557319223985890653e-06);      //  1/9!
    pc = fma(pc, x2, 2.4801587301587301587e-05);      //  1/8!
    ps = fma(ps, x2, -1.9841269841269841270e-04);     // -1/7!
    pc = fma(pc, x2, -1.3888888888888888889e-03);     // -1/6!
    ps = fma(ps, x2, 8.3333333333333333333e-03);      //  1/5!
    pc = fma(pc, x2, 4.1666666666666666667e-02);      //  1/4!
    ps = fma(ps, x2, -1.6666666666666666667e-01);     // -1/3!
    pc = fma(pc, x2, -0.5);                           // -1/2!
    s = fma(ps * x2, x, x);
    c = fma(pc, x2, 1.0);
}

// rotation of the thread's two pairs: (0,1),(2,3) for a gate on bit a, (0,2),(1,3) on bit b
template <int KIND, bool ON_B>
__device__ __forceinline__ void rot_group(cplx (&e)[4], double c, double s) {
    if (ON_B) { rot_pair(KIND, e[0], e[2], c, s); rot_pair(KIND, e[1], e[3], c, s); }
    else      { rot_pair(KIND, e[0], e[1], c, s); rot_pair(KIND, e[2], e[3], c, s); }
}

struct CdShared {          // what a parameter step needs besides the thread's registers
    double* th;            // LDS: thetas of the lane
    const double2* cs;     // LDS: (cos, sin) of every half angle at the start of the sweep
    double* red;           // LDS: [2 parities][4 waves][4] partial sums
    double inv_d2n;
    int tid, wave, wl;
    unsigned parity;
};

// One parameter of the walk (core_op_matrix.py:855-912) with the gate kind and the rotated bit known at compile time.
template <int KIND, bool ON_B, int G>
__device__ __forceinline__ void cd_param(cplx (&ww)[G][4], cplx (&zz)[G][4], const bool (&live)[G], int tix, CdShared& sh) {
    double gr = 0, gi = 0, pr = 0, pi = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        if (!live[j]) continue;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int i0 = ON_B ? p : 2 * p, i1 = ON_B ? p + 2 : 2 * p + 1;
            const cplx w0 = ww[j][i0], w1 = ww[j][i1], z0 = zz[j][i0], z1 = zz[j][i1];
            const double c00r = w0.x * z0.x + w0.y * z0.y, c00i = w0.x * z0.y - w0.y * z0.x;
            const double c11r = w1.x * z1.x + w1.y * z1.y, c11i = w1.x * z1.y - w1.y * z1.x;
            pr += c00r + c11r;
            pi += c00i + c11i;
            if (KIND == 1) {
                gr += c00r - c11r;
                gi += c00i - c11i;
            } else {
                const double c01r = w0.x * z1.x + w0.y * z1.y, c01i = w0.x * z1.y - w0.y * z1.x;
                const double c10r = w1.x * z0.x + w1.y * z0.y, c10i = w1.x * z0.y - w1.y * z0.x;
                if (KIND == 0) { gr += c01r - c10r; gi += c01i - c10i; } else { gr += c01r + c10r; gi += c01i + c10i; }
            }
        }
    }
    const double v = wave_sum4(gr, gi, pr, pi, sh.wl);
    double* rd = sh.red + 16 * (sh.parity & 1);   // double-buffered: the next parameter's partials never overtake a reader
    ++sh.parity;
    if (sh.wl < 4) rd[4 * sh.wave + sh.wl] = v;   // [wave][0 gr, 1 pr, 2 gi, 3 pi]
    const double2 co = sh.cs[tix];
#pragma unroll
    for (int j = 0; j < G; ++j) rot_group<KIND, ON_B>(zz[j], co.x, co.y);   // z <- R(theta_old) z: does not wait for the sums
    __syncthreads();
    gr = (rd[0] + rd[4]) + (rd[8] + rd[12]);
    pr = (rd[1] + rd[5]) + (rd[9] + rd[13]);
    gi = (rd[2] + rd[6]) + (rd[10] + rd[14]);
    pi = (rd[3] + rd[7]) + (rd[11] + rd[15]);
    double dt;
    cd_delta(KIND, gr, gi, pr, pi, sh.inv_d2n, dt);
    double sd, cd;
    sincos_small(0.5 * dt, sd, cd);
    const double cn = co.x * cd - co.y * sd, sn = co.y * cd + co.x * sd;   // half angle of theta_old + dt
#pragma unroll
    for (int j = 0; j < G; ++j) rot_group<KIND, ON_B>(ww[j], cn, sn);       // w <- R(theta_new) w
    if (sh.tid == 0) sh.th[tix] += dt;   // (read again at the start of the next sweep only)
}

// RULE: the driver's stop rules (CdRule, aqc_launch.h; aqc_ws_cd_minimize) at the end of every sweep.  They are compiled in or out:
// the instance without them is the plain "nsweeps sweeps, one objective value per sweep" of aqc_ws_cd_sweeps, the code it was before
// the rules existed.  With them a lane that has ended is skipped, a sweep's largest step is max |theta - theta at its start| (the
// lane's thetas in HBM are brought up to date after every sweep, so they are that start), and a lane leaves its loop when it ends.
__device__ __forceinline__ double cd_max_nan(double a, double b) { return (b > a || b != b) ? b : a; }   // a NaN stays (np.amax)

template <int G, bool RULE>
__device__ __forceinline__ void cd_persistent_body(const CdSeg* __restrict__ prog, int nsegs, int nbits, int col_bits,
                                                   const cplx* __restrict__ target, size_t lane_stride, double* thetas, int T,
                                                   double* fobj, int nsweeps, int max_steps, const CdRule& rule) {
    extern __shared__ double cd_lds[];
    if (RULE && rule.status[blockIdx.x] != kCdRunning) return;   // a finished lane (workgroup-uniform, before any barrier)
    const int N = 1 << nbits, ngroups = N >> 2;
    cplx* w = reinterpret_cast<cplx*>(cd_lds);
    cplx* z = w + N;
    double* th = reinterpret_cast<double*>(z + N);
    double2* cs = reinterpret_cast<double2*>(th + ((T + 1) & ~1));
    const int tid = threadIdx.x, lane = blockIdx.x;
    const double dim = (double)(1 << (nbits - col_bits));
    CdShared sh{th, cs, reinterpret_cast<double*>(cs + T), 1.0 / (dim * dim), tid, tid >> 6, tid & 63, 0u};
    const int cmask = (1 << col_bits) - 1;
    double* my_thetas = thetas + (size_t)lane * T;
    const cplx* y = target + (size_t)lane * lane_stride;
    for (int t = tid; t < T; t += 256) th[t] = my_thetas[t];
    __syncthreads();
    for (int sweep = 0; sweep < nsweeps; ++sweep) {
        for (int t = tid; t < T; t += 256) { double s, c; sincos(0.5 * th[t], &s, &c); cs[t] = make_double2(c, s); }
        for (int e = tid; e < N; e += 256) {
            z[e] = y[e];
            w[e] = make_double2(((e >> col_bits) == (e & cmask)) ? 1.0 : 0.0, 0.0);
        }
        __syncthreads();
        // ---- z <- V^H z: the segments in reverse order, inside a segment the rotations in reverse order with inverted angles,
        // then the (self-inverse) entangler; one LDS round trip and one barrier per segment
        for (int sg = nsegs - 1; sg >= 0; --sg) {
            const CdSeg& seg = prog[sg];
            const int ha = __builtin_amdgcn_readfirstlane(seg.ha), hb = __builtin_amdgcn_readfirstlane(seg.hb);
            const int ent = __builtin_amdgcn_readfirstlane(seg.ent);
            const int t0 = __builtin_amdgcn_readfirstlane(seg.tindex[0]), t1 = __builtin_amdgcn_readfirstlane(seg.tindex[1]);
            const int t2 = __builtin_amdgcn_readfirstlane(seg.tindex[2]), t3 = __builtin_amdgcn_readfirstlane(seg.tindex[3]);
            const int lo = min(ha, hb), hi = max(ha, hb), ia = 1 << ha, ib = 1 << hb;
            cplx zz[G][4];
            int base[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int g = tid + 256 * j;
                base[j] = (int)pair_index(pair_index((size_t)(g < ngroups ? g : 0), lo), hi);
                zz[j][0] = z[base[j]]; zz[j][1] = z[base[j] + ia]; zz[j][2] = z[base[j] + ib]; zz[j][3] = z[base[j] + ia + ib];
            }
            const double2 c0 = cs[t0], c1 = cs[t1], c2 = cs[t2], c3 = cs[ent ? t3 : t0];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (ent == 0) {          // front layer: Rz(t0)^-1 ... after Ry(t1)^-1 after Rz(t2)^-1 in reverse order of the walk
                    rot_group<1, false>(zz[j], c2.x, -c2.y); rot_group<0, false>(zz[j], c1.x, -c1.y); rot_group<1, false>(zz[j], c0.x, -c0.y);
                } else {
                    if (ent == 1) rot_group<2, true>(zz[j], c3.x, -c3.y); else rot_group<1, true>(zz[j], c3.x, -c3.y);
                    rot_group<0, true>(zz[j], c2.x, -c2.y); rot_group<1, false>(zz[j], c1.x, -c1.y); rot_group<0, false>(zz[j], c0.x, -c0.y);
                    if (ent == 1) { const cplx t = zz[j][1]; zz[j][1] = zz[j][3]; zz[j][3] = t; }
                    else zz[j][3] = make_double2(-zz[j][3].x, -zz[j][3].y);
                }
                if (tid + 256 * j < ngroups) {
                    z[base[j]] = zz[j][0]; z[base[j] + ia] = zz[j][1]; z[base[j] + ib] = zz[j][2]; z[base[j] + ia + ib] = zz[j][3];
                }
            }
            __syncthreads();
        }
        // ---- the walk
        int left = max_steps >= 0 ? max_steps : 0x7fffffff;   // (tests: stop after a given number of parameter steps)
        for (int sg = 0; sg < nsegs && left > 0; ++sg) {
            const CdSeg& seg = prog[sg];
            const int ha = __builtin_amdgcn_readfirstlane(seg.ha), hb = __builtin_amdgcn_readfirstlane(seg.hb);
            const int ent = __builtin_amdgcn_readfirstlane(seg.ent);
            const int t0 = __builtin_amdgcn_readfirstlane(seg.tindex[0]), t1 = __builtin_amdgcn_readfirstlane(seg.tindex[1]);
            const int t2 = __builtin_amdgcn_readfirstlane(seg.tindex[2]), t3 = __builtin_amdgcn_readfirstlane(seg.tindex[3]);
            const int lo = min(ha, hb), hi = max(ha, hb), ia = 1 << ha, ib = 1 << hb;
            cplx ww[G][4], zz[G][4];
            int base[G];
            bool live[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int g = tid + 256 * j;
                live[j] = g < ngroups;
                base[j] = (int)pair_index(pair_index((size_t)(live[j] ? g : 0), lo), hi);
                ww[j][0] = w[base[j]]; ww[j][1] = w[base[j] + ia]; ww[j][2] = w[base[j] + ib]; ww[j][3] = w[base[j] + ia + ib];
                zz[j][0] = z[base[j]]; zz[j][1] = z[base[j] + ia]; zz[j][2] = z[base[j] + ib]; zz[j][3] = z[base[j] + ia + ib];
            }
            if (ent == 0) {                       // front layer of one qubit: Rz(t2), Ry(t1), Rz(t0)  (tindex = t2, t1, t0 in walk order)
                cd_param<1, false, G>(ww, zz, live, t0, sh);
                if (--left > 0) { cd_param<0, false, G>(ww, zz, live, t1, sh);
                if (--left > 0) { cd_param<1, false, G>(ww, zz, live, t2, sh); --left; } }
            } else {
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    if (ent == 1) {
                        cplx t = zz[j][1]; zz[j][1] = zz[j][3]; zz[j][3] = t;
                        t = ww[j][1]; ww[j][1] = ww[j][3]; ww[j][3] = t;
                    } else {
                        zz[j][3] = make_double2(-zz[j][3].x, -zz[j][3].y);
                        ww[j][3] = make_double2(-ww[j][3].x, -ww[j][3].y);
                    }
                }
                cd_param<0, false, G>(ww, zz, live, t0, sh);
                if (--left > 0) { cd_param<1, false, G>(ww, zz, live, t1, sh);
                if (--left > 0) { cd_param<0, true, G>(ww, zz, live, t2, sh);
                if (--left > 0) { if (ent == 1) cd_param<2, true, G>(ww, zz, live, t3, sh); else cd_param<1, true, G>(ww, zz, live, t3, sh); --left; } } }
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (live[j]) {
                    w[base[j]] = ww[j][0]; w[base[j] + ia] = ww[j][1]; w[base[j] + ib] = ww[j][2]; w[base[j] + ia + ib] = ww[j][3];
                    z[base[j]] = zz[j][0]; z[base[j] + ia] = zz[j][1]; z[base[j] + ib] = zz[j][2]; z[base[j] + ia + ib] = zz[j][3];
                }
            }
            __syncthreads();
        }
        // ---- fobj = 1 - |<w|z> / d|^2
        double pr = 0, pi = 0;
        for (int e = tid; e < N; e += 256) {
            const cplx a = w[e], b = z[e];
            pr += a.x * b.x + a.y * b.y;
            pi += a.x * b.y - a.y * b.x;
        }
        pr = wsum(pr); pi = wsum(pi);
        double dm = 0.0;
        if (RULE) {
            for (int t = tid; t < T; t += 256) dm = cd_max_nan(dm, fabs(th[t] - my_thetas[t]));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dm = cd_max_nan(dm, __shfl_xor(dm, o, 64));
        }
        double* rd = sh.red + 16 * (sh.parity & 1);
        ++sh.parity;
        if (sh.wl == 0) { rd[4 * sh.wave] = pr; rd[4 * sh.wave + 1] = pi; if (RULE) rd[4 * sh.wave + 2] = dm; }
        __syncthreads();
        if (tid == 0) {
            const double a = (rd[0] + rd[4]) + (rd[8] + rd[12]), b = (rd[1] + rd[5]) + (rd[9] + rd[13]);
            const double f = 1.0 - (a * a + b * b) * sh.inv_d2n;
            if (!RULE) fobj[(size_t)lane * nsweeps + sweep] = f;
            else {               // the close rule; its verdict goes to the other threads through two words of this parity's slots
                const double dmax = cd_max_nan(cd_max_nan(rd[2], rd[6]), cd_max_nan(rd[10], rd[14]));
                int nit = rule.nit[lane], status = kCdRunning;
                double best = rule.best_f[lane];
                const bool improved = cd_close(f, dmax, rule.fobj_thr, rule.dtheta_thr, rule.maxiter, rule.profile + (size_t)lane * rule.maxiter,
                                               nit, best, status);
                rule.nit[lane] = nit; rule.best_f[lane] = best; rule.status[lane] = status;
                rd[2] = improved ? 1.0 : 0.0;
                rd[3] = (double)status;
            }
        }
        __syncthreads();
        if (RULE) {              // (rd is written again two parameters later at the earliest: after the next sweep's barriers)
            const bool improved = rd[2] != 0.0, done = rd[3] != 0.0;
            for (int t = tid; t < T; t += 256) {   // (a thread reads and writes its own entries of my_thetas only)
                my_thetas[t] = th[t];
                if (improved) rule.best_thetas[(size_t)lane * T + t] = th[t];
            }
            if (done) break;
        }
    }
    for (int t = tid; t < T; t += 256) my_thetas[t] = th[t];
}

// up to 5 qubits: one 4-element group per thread; three workgroups per CU (50 KiB of LDS each at 5 qubits and 735 parameters),
// i.e. three waves per SIMD: the register budget is set accordingly.  6 qubits: four groups per thread, one workgroup per CU
// (128 KiB of LDS).  Each with and without the driver's rules.
#define AQC_CD_PERSISTENT_ARGS                                                                                                        \
    const CdSeg* __restrict__ prog, int nsegs, int nbits, int col_bits, const cplx* __restrict__ target, size_t lane_stride, double* thetas, \
        int T, double* fobj, int nsweeps, int max_steps, CdRule rule
__global__ __launch_bounds__(256, 3) void cd_persistent_kernel_g1(AQC_CD_PERSISTENT_ARGS) {
    cd_persistent_body<1, false>(prog, nsegs, nbits, col_bits, target, lane_stride, thetas, T, fobj, nsweeps, max_steps, rule);
}
__global__ __launch_bounds__(256) void cd_persistent_kernel_g4(AQC_CD_PERSISTENT_ARGS) {
    cd_persistent_body<4, false>(prog, nsegs, nbits, col_bits, target, lane_stride, thetas, T, fobj, nsweeps, max_steps, rule);
}
__global__ __launch_bounds__(256, 3) void cd_persistent_rule_kernel_g1(AQC_CD_PERSISTENT_ARGS) {
    cd_persistent_body<1, true>(prog, nsegs, nbits, col_bits, target, lane_stride, thetas, T, fobj, nsweeps, max_steps, rule);
}
__global__ __launch_bounds__(256) void cd_persistent_rule_kernel_g4(AQC_CD_PERSISTENT_ARGS) {
    cd_persistent_body<4, true>(prog, nsegs, nbits, col_bits, target, lane_stride, thetas, T, fobj, nsweeps, max_steps, rule);
}
#undef AQC_CD_PERSISTENT_ARGS

size_t cd_persistent_lds_bytes(int nbits, int T) {
    return ((size_t)2 << nbits) * sizeof(cplx) + (size_t)((T + 1) & ~1) * sizeof(double) + (size_t)T * sizeof(double2) + 32 * sizeof(double);
}

hipError_t launch_cd_persistent(const void* prog, int nsegs, int nbits, int col_bits, const void* target, size_t lane_stride, double* thetas,
                                int T, double* fobj, int nsweeps, int max_steps, int batch, hipStream_t s, const CdRule* rule_in) {
    const CdRule rule = rule_in ? *rule_in : CdRule{};
    const size_t lds = cd_persistent_lds_bytes(nbits, T);
    const bool big = ((size_t)1 << nbits) / 4 > 256;    // more than one 4-element group per thread (6 qubits: 4)
    typedef void (*Kernel)(const CdSeg*, int, int, int, const cplx*, size_t, double*, int, double*, int, int, CdRule);
    static const Kernel kernels[4] = {cd_persistent_kernel_g1, cd_persistent_kernel_g4, cd_persistent_rule_kernel_g1, cd_persistent_rule_kernel_g4};
    const int which = (big ? 1 : 0) + (rule_in ? 2 : 0);
    static size_t granted_all[64][4] = {};   // hipFuncSetAttribute applies to the current device: one record per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    size_t (&granted)[4] = granted_all[dev];
    if (lds > granted[which] || dev == 0) {   // (device 0 doubles as the catch-all slot: always set there -- the call is cheap)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernels[which]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        granted[which] = lds;
    }
    kernels[which]<<<batch, 256, lds, s>>>(static_cast<const CdSeg*>(prog), nsegs, nbits, col_bits, static_cast<const cplx*>(target), lane_stride, thetas,
                                           T, fobj, nsweeps, max_steps, rule);
    return hipGetLastError();
}

// ---- the walk for operands that do not fit LDS: plain launches, grid (nparts, lanes) ----------------------------------------------
// Beyond 6 qubits w and z live in HBM.  The walk keeps the persistent kernel's segments: a thread takes the 4-element groups of w and
// of z on the segment's two address bits into registers, and
//   the OPENER (one launch per segment) applies the entangler as the same register permutation, writes the elements it moved and
//     leaves the partial sums (grad, prod) of the segment's first parameter, one set of four doubles per workgroup;
//   a STEP (one launch per parameter) has every workgroup add the lane's nparts partial sets in one fixed order (thread t takes sets
//     t, t + 256, ... in index order, then the wave and workgroup sums of cd_param), derive the step with cd_delta, rotate z by the old
//     angle and w by the new one, and -- unless the parameter closes the segment -- form the next parameter's partials from the same
//     registers: one read and one write of w and z per parameter.
// Workgroup 0 of a lane stores the new theta and folds |theta_new - theta_old| into the lane's running maximum.  The old angle is read
// from theta_in, which no launch of the walk writes (the close kernel copies theta_out over it when the sweep ends), and the partial
// sets alternate between two buffers by the parity of the parameter: inside one launch some workgroups still read set p while others
// already write set p + 1.  nparts depends on the lane's size alone, never on the batch, and no sum is atomic: a lane of a batch goes
// through the same arithmetic as the same problem alone.  A lane whose status is not kCdRunning is skipped by every launch.
int cd_wide_parts(size_t lane_elems) { return (int)std::min<size_t>(512, std::max<size_t>(1, ((lane_elems >> 2) + 255) / 256)); }

template <int KIND, bool ON_B>
__device__ __forceinline__ void cd_group_sums(const cplx (&ww)[4], const cplx (&zz)[4], double& gr, double& gi, double& pr, double& pi) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int i0 = ON_B ? p : 2 * p, i1 = ON_B ? p + 2 : 2 * p + 1;
        const cplx w0 = ww[i0], w1 = ww[i1], z0 = zz[i0], z1 = zz[i1];
        const double c00r = w0.x * z0.x + w0.y * z0.y, c00i = w0.x * z0.y - w0.y * z0.x;
        const double c11r = w1.x * z1.x + w1.y * z1.y, c11i = w1.x * z1.y - w1.y * z1.x;
        pr += c00r + c11r;
        pi += c00i + c11i;
        if (KIND == 1) {
            gr += c00r - c11r;
            gi += c00i - c11i;
        } else {
            const double c01r = w0.x * z1.x + w0.y * z1.y, c01i = w0.x * z1.y - w0.y * z1.x;
            const double c10r = w1.x * z0.x + w1.y * z0.y, c10i = w1.x * z0.y - w1.y * z0.x;
            if (KIND == 0) { gr += c01r - c10r; gi += c01i - c10i; } else { gr += c01r + c10r; gi += c01i + c10i; }
        }
    }
}
// (kind, on_b) are launch arguments: uniform branches to the five combinations a segment has
__device__ __forceinline__ void cd_group_sums_rt(int kind, int on_b, const cplx (&ww)[4], const cplx (&zz)[4], double& gr, double& gi,
                                                 double& pr, double& pi) {
    if (!on_b) { if (kind == 0) cd_group_sums<0, false>(ww, zz, gr, gi, pr, pi); else cd_group_sums<1, false>(ww, zz, gr, gi, pr, pi); }
    else if (kind == 0) cd_group_sums<0, true>(ww, zz, gr, gi, pr, pi);
    else if (kind == 1) cd_group_sums<1, true>(ww, zz, gr, gi, pr, pi);
    else cd_group_sums<2, true>(ww, zz, gr, gi, pr, pi);
}
__device__ __forceinline__ void cd_group_rot_rt(int kind, int on_b, cplx (&e)[4], double c, double s) {
    if (on_b) { rot_pair(kind, e[0], e[2], c, s); rot_pair(kind, e[1], e[3], c, s); }
    else      { rot_pair(kind, e[0], e[1], c, s); rot_pair(kind, e[2], e[3], c, s); }
}
// the workgroup's four sums -> out[0 gr, 1 pr, 2 gi, 3 pi]; red: 16 doubles of LDS.  Reached by all 256 threads.
__device__ __forceinline__ void cd_wide_put(double gr, double gi, double pr, double pi, double* red, double* out) {
    const int tid = threadIdx.x, wl = tid & 63;
    const double v = wave_sum4(gr, gi, pr, pi, wl);
    if (wl < 4) red[4 * (tid >> 6) + wl] = v;
    __syncthreads();
    if (tid < 4) out[tid] = (red[tid] + red[4 + tid]) + (red[8 + tid] + red[12 + tid]);
}

__global__ __launch_bounds__(256) void cd_wide_open_kernel(CdWide a) {
    __shared__ double red[16];
    const int lane = blockIdx.y;
    if (a.status[lane] != kCdRunning) return;   // (workgroup-uniform, before the barrier)
    cplx* w = static_cast<cplx*>(a.w) + (size_t)lane * a.lane_stride;
    cplx* z = static_cast<cplx*>(a.z) + (size_t)lane * a.lane_stride;
    const int lo = min(a.ha, a.hb), hi = max(a.ha, a.hb);
    const size_t ia = (size_t)1 << a.ha, ib = (size_t)1 << a.hb;
    double gr = 0, gi = 0, pr = 0, pi = 0;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < (size_t)a.ngroups; g += (size_t)a.nparts * 256) {
        const size_t base = pair_index(pair_index(g, lo), hi);
        cplx ww[4] = {w[base], w[base + ia], w[base + ib], w[base + ia + ib]};
        cplx zz[4] = {z[base], z[base + ia], z[base + ib], z[base + ia + ib]};
        if (a.ent == 1) {          // CX: the control's 1-half swaps along the target
            cplx t = zz[1]; zz[1] = zz[3]; zz[3] = t;
            t = ww[1]; ww[1] = ww[3]; ww[3] = t;
            w[base + ia] = ww[1]; w[base + ia + ib] = ww[3];
            z[base + ia] = zz[1]; z[base + ia + ib] = zz[3];
        } else if (a.ent == 2) {   // CZ
            zz[3] = make_double2(-zz[3].x, -zz[3].y);
            ww[3] = make_double2(-ww[3].x, -ww[3].y);
            w[base + ia + ib] = ww[3];
            z[base + ia + ib] = zz[3];
        }
        cd_group_sums_rt(a.next_kind, a.next_on_b, ww, zz, gr, gi, pr, pi);
    }
    cd_wide_put(gr, gi, pr, pi, red, a.part_out + 4 * ((size_t)lane * a.nparts + blockIdx.x));
}

__global__ __launch_bounds__(256) void cd_wide_step_kernel(CdWide a) {
    __shared__ double red_in[16], red_out[16];
    const int lane = blockIdx.y, tid = threadIdx.x, wl = tid & 63;
    if (a.status[lane] != kCdRunning) return;   // (workgroup-uniform, before any barrier)
    double gr = 0, gi = 0, pr = 0, pi = 0;
    const double* part = a.part_in + 4 * (size_t)lane * a.nparts;
    for (int i = tid; i < a.nparts; i += 256) { gr += part[4 * i]; pr += part[4 * i + 1]; gi += part[4 * i + 2]; pi += part[4 * i + 3]; }
    const double v = wave_sum4(gr, gi, pr, pi, wl);
    if (wl < 4) red_in[4 * (tid >> 6) + wl] = v;
    __syncthreads();
    gr = (red_in[0] + red_in[4]) + (red_in[8] + red_in[12]);
    pr = (red_in[1] + red_in[5]) + (red_in[9] + red_in[13]);
    gi = (red_in[2] + red_in[6]) + (red_in[10] + red_in[14]);
    pi = (red_in[3] + red_in[7]) + (red_in[11] + red_in[15]);
    double dt;
    cd_delta(a.kind, gr, gi, pr, pi, a.inv_d2n, dt);   // every thread of every workgroup: the same numbers in the same order
    const double t_old = a.theta_in[(size_t)lane * a.T + a.tindex], t_new = t_old + dt;
    double so, co, sn, cn;
    sincos(0.5 * t_old, &so, &co);
    sincos(0.5 * t_new, &sn, &cn);
    if (blockIdx.x == 0 && tid == 0) {
        a.theta_out[(size_t)lane * a.T + a.tindex] = t_new;
        a.dmax[lane] = cd_max_nan(a.dmax[lane], fabs(t_new - t_old));   // (launches of one stream: nobody else touches the word)
    }
    cplx* w = static_cast<cplx*>(a.w) + (size_t)lane * a.lane_stride;
    cplx* z = static_cast<cplx*>(a.z) + (size_t)lane * a.lane_stride;
    const int lo = min(a.ha, a.hb), hi = max(a.ha, a.hb);
    const size_t ia = (size_t)1 << a.ha, ib = (size_t)1 << a.hb;
    gr = gi = pr = pi = 0;
    for (size_t g = (size_t)blockIdx.x * 256 + tid; g < (size_t)a.ngroups; g += (size_t)a.nparts * 256) {
        const size_t base = pair_index(pair_index(g, lo), hi);
        cplx ww[4] = {w[base], w[base + ia], w[base + ib], w[base + ia + ib]};
        cplx zz[4] = {z[base], z[base + ia], z[base + ib], z[base + ia + ib]};
        cd_group_rot_rt(a.kind, a.on_b, zz, co, so);   // z <- R(theta_old) z
        cd_group_rot_rt(a.kind, a.on_b, ww, cn, sn);   // w <- R(theta_new) w
        if (a.next_kind >= 0) cd_group_sums_rt(a.next_kind, a.next_on_b, ww, zz, gr, gi, pr, pi);
        w[base] = ww[0]; w[base + ia] = ww[1]; w[base + ib] = ww[2]; w[base + ia + ib] = ww[3];
        z[base] = zz[0]; z[base + ia] = zz[1]; z[base + ib] = zz[2]; z[base + ia + ib] = zz[3];
    }
    if (a.next_kind >= 0) cd_wide_put(gr, gi, pr, pi, red_out, a.part_out + 4 * ((size_t)lane * a.nparts + blockIdx.x));
}

// The end of a sweep on the wide route, one small workgroup per lane: fobj = 1 - |<w|z>|^2 / d^2 from the vdot launch's result, the
// close rule (aqc_cd_rule.h), the sweep's thetas copied over the ones the next V^H reads -- and over the best ones when they are.
__global__ __launch_bounds__(64) void cd_close_kernel(CdClose a) {
    __shared__ int improved_s;
    const int lane = blockIdx.x, tid = threadIdx.x;
    if (a.rule.status[lane] != kCdRunning) return;
    if (tid == 0) {
        const double2 tr = a.trace[lane];
        int nit = a.rule.nit[lane], status = kCdRunning;
        double best = a.rule.best_f[lane];
        improved_s = cd_close(1.0 - (tr.x * tr.x + tr.y * tr.y) * a.inv_d2n, a.dmax[lane], a.rule.fobj_thr, a.rule.dtheta_thr, a.rule.maxiter,
                              a.rule.profile + (size_t)lane * a.rule.maxiter, nit, best, status) ? 1 : 0;
        a.rule.nit[lane] = nit; a.rule.best_f[lane] = best; a.rule.status[lane] = status;
        a.dmax[lane] = 0.0;
    }
    __syncthreads();
    const bool improved = improved_s != 0;
    for (int t = tid; t < a.T; t += 64) {
        const double c = a.theta_cur[(size_t)lane * a.T + t];
        a.theta_own[(size_t)lane * a.T + t] = c;
        if (improved) a.rule.best_thetas[(size_t)lane * a.T + t] = c;
    }
}

// lanes still running -> one int word, what the host reads between chunks; mark != 0: the time limit has passed, they become that first
__global__ __launch_bounds__(256) void cd_count_kernel(int* status, int batch, int mark, int* running) {
    __shared__ int cnt[4];
    int c = 0;
    for (int b = threadIdx.x; b < batch; b += 256)
        if (status[b] == kCdRunning) { if (mark) status[b] = mark; else ++c; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) *running = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
}

hipError_t launch_cd_wide_open(const CdWide& a, int batch, hipStream_t s) {
    cd_wide_open_kernel<<<dim3(a.nparts, batch), 256, 0, s>>>(a);
    return hipGetLastError();
}
hipError_t launch_cd_wide_step(const CdWide& a, int batch, hipStream_t s) {
    cd_wide_step_kernel<<<dim3(a.nparts, batch), 256, 0, s>>>(a);
    return hipGetLastError();
}
hipError_t launch_cd_close(const CdClose& a, int batch, hipStream_t s) {
    cd_close_kernel<<<batch, 64, 0, s>>>(a);
    return hipGetLastError();
}
hipError_t launch_cd_count(int* status, int batch, int mark, int* running, hipStream_t s) {
    cd_count_kernel<<<1, 256, 0, s>>>(status, batch, mark, running);
    return hipGetLastError();
}

}  // namespace aqc
