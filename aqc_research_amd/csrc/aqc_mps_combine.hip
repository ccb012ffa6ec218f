// Linear combinations of MPS states: the direct sum of every output's terms (rules and notation: aqc_mps_combine_rule.h; host side:
// aqc_mps_combine_api.cpp).
//
// mps_combine_assemble_kernel   ONE launch over all sites of all outputs of a call.  Workgroup (tile, q, output) walks the elements of
//                               assembled site S_q of its output at a stride of the tiles; element e is, by mps_combine_source (the
//                               host's text), an element of one term's site -- times the term's coefficient on site 0 -- or a zero.
//                               n = 1: the two sums over the terms, in their order.
// Every element of every assembled site is written exactly once, the zeros included: nothing is cleared beforehand.  No atomics, no
// shared memory, no loop bound that depends on data other than bond dimensions and term counts.  An element is written only inside
// its site by the output's own offsets; a term is read only when its state index is a record of the table and the element lies inside
// that state's site by the state's own bond dimensions -- anything else is a zero, which the sweep then reports as it would any state.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aqc_launch.h"
#include "aqc_mps_combine_rule.h"

namespace aqc {

namespace {
constexpr int kCombineThreads = 256, kCombineMaxTiles = 64;

struct TermSite { const double2* t; size_t elems; };
// site q of the state of term k, and its size by the state's own dims; null when the index is no record of the table
__device__ inline TermSite term_site(const MpsCombineArgs& a, const MpsCombineOutput& o, int k, int q) {
    const int state = o.term_state[k];
    if (state < 0 || state >= a.nstates) return {nullptr, 0};
    const unsigned long long* rec = a.table + (size_t)state * a.per;
    const int* dims = reinterpret_cast<const int*>(rec + a.at_dims);
    return {reinterpret_cast<const double2* const*>(rec + a.at_sites)[q], (size_t)2 * dims[q] * dims[q + 1]};
}
}  // namespace

// grid (tiles, n, outputs of the launch); 256 threads
__global__ __launch_bounds__(256) void mps_combine_assemble_kernel(MpsCombineArgs a) {
    const MpsCombineOutput o = a.outputs[a.first + blockIdx.z];
    const int q = blockIdx.y, n = a.n, nterms = o.nterms;
    const size_t count = o.site_off[q + 1] - o.site_off[q];   // 2 Sigma_q Sigma_{q+1}
    double2* out = o.sites + o.site_off[q];
    const size_t stride = (size_t)gridDim.x * kCombineThreads;
    if (n == 1) {
        for (size_t e = (size_t)blockIdx.x * kCombineThreads + threadIdx.x; e < count && e < 2; e += stride) {
            double2 acc = make_double2(0.0, 0.0);
            for (int k = 0; k < nterms; ++k) {
                const TermSite ts = term_site(a, o, k, 0);
                if (e >= ts.elems) continue;
                const double2 c = o.coeffs[k], x = ts.t[e];
                acc.x += c.x * x.x - c.y * x.y;
                acc.y += c.x * x.y + c.y * x.x;
            }
            out[e] = acc;
        }
        return;
    }
    for (size_t e = (size_t)blockIdx.x * kCombineThreads + threadIdx.x; e < count; e += stride) {
        const MpsCombineSource src = mps_combine_source(n, nterms, o.block_off, q, e);
        double2 v = make_double2(0.0, 0.0);
        if (src.term >= 0) {
            const TermSite ts = term_site(a, o, src.term, q);
            if (src.elem < ts.elems) {
                v = ts.t[src.elem];
                if (q == 0) {
                    const double2 c = o.coeffs[src.term];
                    v = make_double2(c.x * v.x - c.y * v.y, c.x * v.y + c.y * v.x);
                }
            }
        }
        out[e] = v;
    }
}

hipError_t launch_mps_combine_assemble(const MpsCombineArgs& a, int count, size_t largest_site, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (a.n > 65535) return hipErrorInvalidValue;
    size_t tiles = (largest_site + kCombineThreads - 1) / kCombineThreads;
    tiles = tiles < 1 ? 1 : tiles > (size_t)kCombineMaxTiles ? kCombineMaxTiles : tiles;
    // one launch unless the grid would pass 2^31 threads or 65535 outputs (more than 2^23 / (tiles n) outputs in a call)
    const size_t most = std::max<size_t>(1, std::min<size_t>(65535, ((size_t)1 << 23) / (tiles * (size_t)a.n)));
    MpsCombineArgs part = a;
    for (size_t done = 0; done < (size_t)count; done += most) {
        part.first = a.first + (int)done;
        const dim3 grid((unsigned)tiles, (unsigned)a.n, (unsigned)std::min<size_t>(most, (size_t)count - done));
        mps_combine_assemble_kernel<<<grid, kCombineThreads, 0, s>>>(part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace aqc
