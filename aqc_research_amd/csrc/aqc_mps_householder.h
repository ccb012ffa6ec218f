// The R-only Householder of a stacked matrix held in the four LDS planes of aqc_mps_planes.h (rules: mps_ent_reflection and
// mps_ent_stacked_row of aqc_mps_ent_rule.h): the step the factor walks of aqc_mps_ent.hip and the partial factors of aqc_mps_fromvec.hip
// share.  Device code, internal linkage.
#pragma once
#include "aqc_mps_ent_rule.h"
#include "aqc_mps_planes.h"

namespace aqc {
namespace {

constexpr int kEntRows = 2 * kCap;                       // rows of the largest stacked matrix

// element (logical row r, column c) of the stacked matrix: offset of its real part from the planes' base, the imaginary part kPlane on
__device__ __forceinline__ int stacked_at(int r, int c, int chi_in) {
    const MpsEntRow at = mps_ent_stacked_row(r, chi_in);
    return (at.plane == 0 ? 2 * kPlane : 0) + at.row * kLd + c;   // < 4 kPlane: at.row < kCap, c < kCap
}

// R factor of the stacked 2 chi_in x chi_out matrix held in the four planes, in place.  v: the reflection vector (2 x kEntRows doubles),
// wp: the partial inner products (2 x 4 x kCap), np: the partial norms of the next column (4)
__device__ __forceinline__ void householder_lds(double* smem, int chi_in, int chi_out, double* v, double* wp, double* np) {
    const int tid = threadIdx.x, c = tid & (kCap - 1), part = tid >> 6;
    const int rows = 2 * chi_in, nref = mps_ent_reflections(rows, chi_out);
    if (c == 0) {   // the norm of column 0, by the four threads that own it
        double s = 0.0;
        for (int r = part; r < rows; r += 4) {
            const int at = stacked_at(r, 0, chi_in);
            s += smem[at] * smem[at] + smem[at + kPlane] * smem[at + kPlane];
        }
        np[part] = s;
    }
    __syncthreads();
    for (int j = 0; j < nref; ++j) {
        const double norm2 = (np[0] + np[1]) + (np[2] + np[3]);
        const bool reflect = mps_ent_reflects(norm2);   // the same for every thread; a NaN reflects
        const int jj = stacked_at(j, j, chi_in);
        const MpsEntReflection h = mps_ent_reflection(smem[jj], smem[jj + kPlane], norm2);
        if (tid < rows - j) {   // rows - j <= kEntRows <= the workgroup
            const int at = stacked_at(j + tid, j, chi_in);
            v[tid] = tid == 0 ? h.v0r : smem[at];
            v[kEntRows + tid] = tid == 0 ? h.v0i : smem[at + kPlane];
        }
        __syncthreads();   // v is whole; np and the diagonal entry have been read
        const bool mine = reflect && c > j && c < chi_out;
        if (mine) {   // this thread's share of w_c = v^H M[j.., c]
            double wr = 0.0, wi = 0.0;
            for (int r = j + part; r < rows; r += 4) {
                const int at = stacked_at(r, c, chi_in);
                const double vr = v[r - j], vi = v[kEntRows + r - j], mr = smem[at], mi = smem[at + kPlane];
                wr += vr * mr + vi * mi;
                wi += vr * mi - vi * mr;
            }
            wp[part * kCap + c] = wr;
            wp[(4 + part) * kCap + c] = wi;
        }
        __syncthreads();
        double next = 0.0;   // this thread's share of the norm of column j + 1 below row j
        if (mine) {
            const double wr = h.tau * ((wp[c] + wp[kCap + c]) + (wp[2 * kCap + c] + wp[3 * kCap + c]));
            const double wi = h.tau * ((wp[4 * kCap + c] + wp[5 * kCap + c]) + (wp[6 * kCap + c] + wp[7 * kCap + c]));
            for (int r = j + part; r < rows; r += 4) {
                const int at = stacked_at(r, c, chi_in);
                const double vr = v[r - j], vi = v[kEntRows + r - j];
                const double mr = smem[at] - (vr * wr - vi * wi), mi = smem[at + kPlane] - (vr * wi + vi * wr);
                smem[at] = mr;
                smem[at + kPlane] = mi;
                if (r > j) next += mr * mr + mi * mi;
            }
        } else if (c == j + 1 && c < chi_out) {   // no reflection: the column is as it was
            for (int r = j + part; r < rows; r += 4) {
                const int at = stacked_at(r, c, chi_in);
                if (r > j) next += smem[at] * smem[at] + smem[at + kPlane] * smem[at + kPlane];
            }
        }
        if (c == j + 1) np[part] = next;
        if (reflect && c == j) {   // column j is alpha e_0
            for (int r = j + part; r < rows; r += 4) {
                const int at = stacked_at(r, j, chi_in);
                smem[at] = r == j ? h.alphar : 0.0;
                smem[at + kPlane] = r == j ? h.alphai : 0.0;
            }
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace aqc
