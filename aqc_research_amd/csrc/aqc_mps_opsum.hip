// Operator sums on MPS states: the direct sum of every output's terms c_t O_t psi_t, the product sites of an operator term formed on
// the way (rules and notation: aqc_mps_opsum_rule.h; host side: aqc_mps_opsum_api.cpp).
//
// mps_opsum_assemble_kernel     ONE launch over all sites of all outputs of a call.  Workgroup (tile, q, output) walks the elements of
//                               assembled site S_q of its output at a stride of the tiles; element e is, by mps_opsum_source (the
//                               host's text), a zero, an element of a state's site (a term without operator), or the two complex
//                               products W_q[a][b][s][0] T_q[0][i][j] + W_q[a][b][s][1] T_q[1][i][j] of an operator term -- times the
//                               term's coefficient on site 0.  n = 1: the two sums over the terms, in their order.
// Every element of every assembled site is written exactly once, the zeros included: nothing is cleared beforehand.  No atomics, no
// shared memory, no loop other than over elements and over the terms of the output.  An element is written only inside its site by
// the output's own offsets.  A term is read only when its state index and its operator index are records of the call, the state's
// elements lie inside the state's site by the state's own bond dimensions, and (a, b) and the addressed elements lie inside the
// operator's site by the operator's own dims and inside the packed data -- anything else is a zero, which the sweep then reports as
// it would any state.  An operator's site is a few hundred bytes that every thread of a workgroup reads: it stays in the caches, and
// the launch is bound by its writes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aqc_launch.h"
#include "aqc_mps_opsum_rule.h"

namespace aqc {

namespace {
constexpr int kOpsumThreads = 256, kOpsumMaxTiles = 64;

struct TermSite { const double2* t; size_t elems; };
// site q of the state of term k, and its size by the state's own dims; null when the index is no record of the table
__device__ inline TermSite term_site(const MpsOpsumArgs& a, const MpsOpsumOutput& o, int k, int q) {
    const int state = o.term_state[k];
    if (state < 0 || state >= a.nstates) return {nullptr, 0};
    const unsigned long long* rec = a.table + (size_t)state * a.per;
    const int* dims = reinterpret_cast<const int*>(rec + a.at_dims);
    return {reinterpret_cast<const double2* const*>(rec + a.at_sites)[q], (size_t)2 * dims[q] * dims[q + 1]};
}
// W_q[a][b][s][0 .. 1] of operator `op`, null when op is no record of the call or (a, b) or the elements lie outside its site
__device__ inline const double2* op_row(const MpsOpsumArgs& a, int op, int q, int ia, int ib, int s) {
    if (op < 0 || op >= a.nops || ia < 0 || ib < 0) return nullptr;
    const size_t* site_off = reinterpret_cast<const size_t*>(a.ops) + (size_t)op * (a.n + 1);
    const int* dims = reinterpret_cast<const int*>(a.ops + a.at_op_dims) + (size_t)op * (a.n + 1);
    if (ia >= dims[q] || ib >= dims[q + 1]) return nullptr;
    const size_t at = site_off[q] + ((size_t)ia * dims[q + 1] + ib) * 4 + 2 * s;
    if (at + 2 > a.op_elems || at + 2 > site_off[q + 1]) return nullptr;
    return reinterpret_cast<const double2*>(a.ops + a.at_op_data) + at;
}
// The complex products with their roundings stated, not left to the compiler's contraction: a term without operator must give the
// bits of mps_combine_assemble_kernel, whose products are compiled as written here (site 0: cmul; n = 1: cmul_first).  Both round
// one product of each part and fuse the other; they differ in which product of the imaginary part is the rounded one.
__device__ inline double2 cmul(double2 c, double2 v) {
#pragma clang fp contract(off)
    return make_double2(__builtin_fma(c.x, v.x, -(c.y * v.y)), __builtin_fma(c.x, v.y, c.y * v.x));
}
__device__ inline double2 cmul_first(double2 c, double2 v) {
#pragma clang fp contract(off)
    return make_double2(__builtin_fma(c.x, v.x, -(c.y * v.y)), __builtin_fma(c.y, v.x, c.x * v.y));
}
// w[0] x0 + w[1] x1: the two complex products of the statement, s' = 0 then s' = 1
__device__ inline double2 apply_row(const double2* w, double2 x0, double2 x1) {
#pragma clang fp contract(off)
    const double2 p = cmul(w[0], x0), r = cmul(w[1], x1);
    return make_double2(p.x + r.x, p.y + r.y);
}
}  // namespace

// grid (tiles, n, outputs of the launch); 256 threads
__global__ __launch_bounds__(256) void mps_opsum_assemble_kernel(MpsOpsumArgs a) {
    const MpsOpsumOutput o = a.outputs[a.first + blockIdx.z];
    const int q = blockIdx.y, n = a.n, nterms = o.nterms;
    const size_t count = o.site_off[q + 1] - o.site_off[q];   // 2 Sigma_q Sigma_{q+1}
    double2* out = o.sites + o.site_off[q];
    const size_t stride = (size_t)gridDim.x * kOpsumThreads;
    if (n == 1) {
        for (size_t e = (size_t)blockIdx.x * kOpsumThreads + threadIdx.x; e < count && e < 2; e += stride) {
            double2 acc = make_double2(0.0, 0.0);
            for (int k = 0; k < nterms; ++k) {
                const TermSite ts = term_site(a, o, k, 0);
                if (ts.elems < 2) continue;
                double2 x = ts.t[e];
                const int op = o.term_op[k];
                if (op != -1) {
                    const double2* w = op_row(a, op, 0, 0, 0, (int)e);
                    if (!w) continue;
                    x = apply_row(w, ts.t[0], ts.t[1]);
                }
                const double2 p = cmul_first(o.coeffs[k], x);
                acc.x += p.x;
                acc.y += p.y;
            }
            out[e] = acc;
        }
        return;
    }
    for (size_t e = (size_t)blockIdx.x * kOpsumThreads + threadIdx.x; e < count; e += stride) {
        const MpsOpsumSource src = mps_opsum_source(n, nterms, o.block_off, o.chi, o.term_op, q, e);
        double2 v = make_double2(0.0, 0.0);
        bool read = false;
        if (src.kind != kMpsOpsumZero) {
            const TermSite ts = term_site(a, o, src.term, q);
            if (src.kind == kMpsOpsumCopy) {
                if (src.x0 < ts.elems) {
                    v = ts.t[src.x0];
                    read = true;
                }
            } else if (src.x0 < ts.elems && src.x1 < ts.elems) {
                const double2* w = op_row(a, o.term_op[src.term], q, src.a, src.b, src.s);
                if (w) {
                    v = apply_row(w, ts.t[src.x0], ts.t[src.x1]);
                    read = true;
                }
            }
        }
        if (read && q == 0) v = cmul(o.coeffs[src.term], v);
        out[e] = v;
    }
}

hipError_t launch_mps_opsum_assemble(const MpsOpsumArgs& a, int count, size_t largest_site, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (a.n > 65535) return hipErrorInvalidValue;
    size_t tiles = (largest_site + kOpsumThreads - 1) / kOpsumThreads;
    tiles = tiles < 1 ? 1 : tiles > (size_t)kOpsumMaxTiles ? kOpsumMaxTiles : tiles;
    // one launch unless the grid would pass 2^31 threads or 65535 outputs (more than 2^23 / (tiles n) outputs in a call)
    const size_t most = std::max<size_t>(1, std::min<size_t>(65535, ((size_t)1 << 23) / (tiles * (size_t)a.n)));
    MpsOpsumArgs part = a;
    for (size_t done = 0; done < (size_t)count; done += most) {
        part.first = a.first + (int)done;
        const dim3 grid((unsigned)tiles, (unsigned)a.n, (unsigned)std::min<size_t>(most, (size_t)count - done));
        mps_opsum_assemble_kernel<<<grid, kOpsumThreads, 0, s>>>(part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace aqc
