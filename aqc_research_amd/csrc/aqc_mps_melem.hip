// Matrix elements of operators between MPS states: <phi|O|psi> for many (bra, operator, ket) jobs per call, by a walk that carries the
// operator's bond (rules and notation: aqc_mps_melem_rule.h; host side: aqc_mps_melem_api.cpp).
//
// fused route (every bond of bra and ket <= kMpsMelemFusedCap = 64, every operator bond <= kMpsMelemOpCap = 32): one workgroup per job
// walks its whole chain inside one launch.  The four planes of aqc_mps_planes.h fill the LDS, so the D_q matrices E_q[a] and the
// G_{b,s} of a site live in the workgroup's slice of one global scratch buffer (E | E' | G) and pass through the planes one at a time.
// The step across site q, in the order of the rule's list of entries (a, then s'):
//     for each a that has an entry:   E_q[a] -> E planes
//         for each s' of a's entries: F = E_q[a] T_q[s']           (MFMA, A operand from LDS, B operand streamed from memory)
//             for each entry (a, s', b, s): G_{b,s} (=, +=) w F    the thread that owns an accumulator element owns that element of
//                                                                   every G: a read-modify-write without atomics or barriers, the
//                                                                   first entry of a G stores, so no G is read before it is written
//     for each b:  for s = 0, 1 where G_{b,s} exists:  G_{b,s} -> F planes,  acc (=, +=) B_q[s]^H G_{b,s}     (MFMA, B operand from LDS)
//                  E_{q+1}[b] = acc -> E' (exact zeros when no G_{b,s} exists); E and E' swap per site
// a outermost: an E matrix is staged once per site and an F never leaves the accumulators; with b outermost every F would be formed
// once per b that reads it, or be kept in memory like G.  Operand tiles are zero-filled beyond the bonds (plane_fill writes the
// whole tiles a product reads), so accumulators there are exact zeros.  Every sum runs in a fixed order that depends on the bonds and
// the operator only: no atomics, and a value does not depend on which other jobs are in the call.
//
// gemm route (any bond): the products are zgemm table launches (aqc_mps.hip); here is the elementwise kernel that combines the F of a
// site into its G.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_mps_melem_rule.h"
#include "aqc_mps_planes.h"

namespace aqc {

static_assert((int)kMpsMelemFusedCap == (int)kMpsObsFusedCap, "the planes of aqc_mps_planes.h are sized by the observables' cap");

namespace {

__device__ __forceinline__ int up_to(int x, int step) { return (x + step - 1) / step * step; }

}  // namespace

// grid (jobs); 256 threads; dynamic LDS kFusedLds
__global__ __launch_bounds__(256) void mps_melem_fused_kernel(MpsMelemFusedArgs a) {
    extern __shared__ __attribute__((aligned(16))) double melem_smem[];
    double* er = melem_smem;
    double* ei = er + kPlane;
    double* fr = ei + kPlane;
    double* fi = fr + kPlane;
    const int tid = threadIdx.x;
    const MpsMelemJob job = a.jobs[blockIdx.x];
    const MpsMelemOp op = *job.op;
    cplx* e_cur = a.scratch + (size_t)blockIdx.x * a.job_elems;
    cplx* e_next = e_cur + a.e_elems;
    cplx* g = e_next + a.e_elems;
    planes_zero(melem_smem);
    if (tid == 0) e_cur[0] = make_double2(1.0, 0.0);
    __syncthreads();
    Acc acc, tot;
    acc_zero(tot);
    for (int q = 0; q < a.n; ++q) {
        const int bl = job.bra_dims[q], br = job.bra_dims[q + 1], kl = job.ket_dims[q], kr = job.ket_dims[q + 1], dr = op.dims[q + 1];
        const cplx* T = job.ket_sites[q];
        const cplx* B = job.bra_sites[q];
        const size_t esize = (size_t)bl * kl, gsize = (size_t)bl * kr, nsize = (size_t)br * kr;
        const MpsMelemEntry* ent = op.ent;
        int e = op.ent_off[q];
        const int e1 = op.ent_off[q + 1];
        while (e < e1) {
            const int ea = ent[e].a;
            plane_fill(e_cur + (size_t)ea * esize, bl, kl, up_to(bl, 16), up_to(kl, 4), er, ei);
            __syncthreads();
            while (e < e1 && ent[e].a == ea) {
                const int sp = ent[e].sp;
                prod_lds_mem(er, ei, T + (size_t)sp * kl * kr, bl, kl, kr, acc);   // F_{a,s'}
                while (e < e1 && ent[e].a == ea && ent[e].sp == sp) {
                    const MpsMelemEntry t = ent[e];
                    acc_axpy(acc, t.wr, t.wi, g + (size_t)(2 * t.b + t.s) * gsize, bl, kr, t.first != 0);
                    ++e;
                }
            }
            __syncthreads();   // every wave is done with the E planes (after the last a: the G are complete)
        }
        const int* mask = op.mask + op.mask_off[q];
        for (int b = 0; b < dr; ++b) {
            const int m = mask[b];
            bool have = false;
            for (int s = 0; s < 2; ++s) {
                if (!((m >> s) & 1)) continue;
                plane_fill(g + (size_t)(2 * b + s) * gsize, bl, kr, up_to(bl, 4), up_to(kr, 16), fr, fi);
                __syncthreads();
                prod_memh_lds(B + (size_t)s * bl * br, fr, fi, br, bl, kr, acc);
                if (have) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) { tot.re[t] += acc.re[t]; tot.im[t] += acc.im[t]; }
                } else {
                    tot = acc;
                }
                have = true;
                __syncthreads();   // the F planes have been read
            }
            if (!have) acc_zero(tot);
            if (q + 1 < a.n) acc_to_mem(tot, e_next + (size_t)b * nsize, kr, br, kr);
        }
        cplx* swap = e_cur; e_cur = e_next; e_next = swap;
        __syncthreads();   // E_{q+1} is in place
    }
    if (tid == 0) a.out[job.out] = make_double2(tot.re[0][0], tot.im[0][0]);   // E_n[0][0][0]: register 0 of tile 0 of wave 0, lane 0
}

// grid (blocks over max(x v, u v) elements, slots = 2 D_{q+1}, jobs)
__global__ void mps_melem_combine_kernel(const MpsMelemOp* op_ptr, int q, const cplx* f, cplx* g, cplx* e_next, size_t stride, int x, int u, int v) {
    const MpsMelemOp op = *op_ptr;
    const int slot = blockIdx.y, b = slot >> 1, s = slot & 1;
    const size_t job = blockIdx.z, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int m = op.mask[op.mask_off[q] + b];
    if (m == 0) {
        if (s == 0 && i < (size_t)u * v) e_next[job * stride + (size_t)b * u * v + i] = make_double2(0.0, 0.0);
        return;
    }
    const size_t fsize = (size_t)x * v;
    if (!((m >> s) & 1) || i >= fsize) return;
    const int* so = op.slot_off + 2 * op.mask_off[q] + q;
    const cplx* fj = f + job * stride;
    cplx val = make_double2(0.0, 0.0);
    for (int e = so[slot]; e < so[slot + 1]; ++e) {
        const MpsMelemEntry t = op.ent_by_slot[e];
        const cplx fv = fj[(size_t)(2 * t.a + t.sp) * fsize + i];
        const double re = t.wr * fv.x - t.wi * fv.y, im = t.wr * fv.y + t.wi * fv.x;
        val = t.first ? make_double2(re, im) : make_double2(val.x + re, val.y + im);
    }
    g[job * stride + (size_t)slot * fsize + i] = val;
}

hipError_t launch_mps_melem_fused(const MpsMelemFusedArgs& a, int njobs, hipStream_t s) {
    const hipError_t e = grant_dynamic_lds<kFusedLds, mps_melem_fused_kernel>();
    if (e != hipSuccess) return e;
    if (njobs <= 0) return hipSuccess;
    mps_melem_fused_kernel<<<njobs, 256, kFusedLds, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mps_melem_combine(const MpsMelemOp* op, int q, const double2* f, double2* g, double2* e_next, size_t stride, int x, int u, int v,
                                    int slots, int njobs, hipStream_t s) {
    if (slots <= 0 || njobs <= 0) return hipSuccess;
    const size_t most = std::max((size_t)x * v, (size_t)u * v);
    mps_melem_combine_kernel<<<dim3((unsigned)((most + 255) / 256), slots, njobs), 256, 0, s>>>(op, q, f, g, e_next, stride, x, u, v);
    return hipGetLastError();
}

}  // namespace aqc
