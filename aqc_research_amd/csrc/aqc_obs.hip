// Reduced density matrices of 4-qubit sets on the fp64 matrix cores (rules: aqc_obs_rule.h), [lanes][2^n] complex128 state vectors.
//   obs_pass_kernel   one launch per pass of the plan, grid (min(tile groups, kObsGridCap), lanes), 256 threads.  A tile is the 2^T
//                     amplitudes that share the index bits outside the pass's bit set B, T = min(n, 11); it is gathered with 16-byte
//                     loads (B holds the low 5 bits: runs of 512 bytes) into LDS as a re and an im plane (32 KiB; slots by
//                     obs_lds_slot), zero-filled beyond 2^n.  The next tile's loads are in flight while the matrix cores work.
//                     Wave w owns the subsets w, w + 4, ...: for a subset S and each of the 32 blocks of 4 columns a lane reads
//                     the one element A[lane % 16][4 kb + lane / 16] -- the operand layout of aqc_mps.hip, where A and B^T = A of a
//                     Gram product are the same register -- and issues v_mfma_f64_16x16x4_f64 three times:
//                       T1 += Ar Ar^T,  T2 += Ai Ai^T,  M += Ai Ar^T        Re rho = T1 + T2,  Im rho = M - M^T
//                     Which of the 128 columns a (kb, lane / 16) is, is a fixed bijection onto the 7 tile bits outside S; the sum
//                     over columns does not care.  A pass of one or two subsets splits the 32 column blocks of each over 4 or 2
//                     waves (ksplit), so that no matrix core idles: a wave's unit u = w + 4 j is part u % ksplit of subset
//                     u / ksplit.  The accumulators stay in registers over all tile groups g = blockIdx.x, blockIdx.x + gridDim.x,
//                     ... of the block; at the end it writes one partial [3][16][16] per subset (the parts of a split subset
//                     are added in LDS, in the order of the parts).
//   obs_final_kernel  grid (subsets, lanes): entry (a, b) adds the partials of the blocks in index order, reading T1 and T2 at
//                     (min, max) and M at both places, for (a, b) and (b, a) alike: the diagonal's imaginary part is 0 and the
//                     lower triangle the conjugate of the upper, bit for bit.
// No atomics: the summation order is fixed by the grid, which does not depend on the number of lanes.
#include <hip/hip_runtime.h>

#include "aqc_launch.h"
#include "aqc_obs_rule.h"

namespace aqc {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
static_assert(kObsSubsetCap == kObsMaxSubsets && kObsThreads == 64 * kObsWaves, "the launch description and the rule");
constexpr int kObsTile = 1 << kObsTileBits;
constexpr int kObsPer = kObsTile / kObsThreads;                 // amplitudes of a tile per thread
constexpr int kObsKBlocks = (kObsTile / 16) / 4;                // 4-column blocks of the 16 x 128 operand
constexpr size_t kObsPartial = 3 * 256;                         // doubles per (block, subset)
static_assert(kObsWaves * kObsPartial <= 2 * (size_t)kObsTile, "the parts of split subsets meet in the tile's LDS");

__global__ __launch_bounds__(kObsThreads) void obs_pass_kernel(ObsArgs a) {
    __shared__ double lds[2 * kObsTile];
    double* const sre = lds;
    double* const sim = lds + kObsTile;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = a.n, tb = a.tile_bits;
    const uint64_t all = ((uint64_t)1 << n) - 1, bmask = a.bits & all, rest = all & ~bmask;
    const uint64_t dim = (uint64_t)1 << n, ngroups = (uint64_t)1 << (n - tb);
    const unsigned tsize = 1u << tb;
    // the gather: thread tid owns the tile-local indices tid + 256 j
    const uint64_t dep_tid = obs_deposit((uint64_t)tid, bmask);
    const unsigned slot_tid = obs_lds_slot((unsigned)tid);
    uint64_t dep_j[kObsPer];
#pragma unroll
    for (int j = 0; j < kObsPer; ++j) dep_j[j] = obs_deposit((uint64_t)(kObsThreads * j), bmask);
    // the operand reads: per owned unit the lane's row / first-columns address, the mask the column blocks walk and the first block
    const int ksplit = a.ksplit, nunits = a.nsub * ksplit, kblocks = kObsKBlocks / ksplit;
    unsigned radr[kObsPerWave], cmhi[kObsPerWave], xfirst[kObsPerWave];
#pragma unroll
    for (int j = 0; j < kObsPerWave; ++j) {
        const int u = wave + kObsWaves * j;
        radr[j] = cmhi[j] = xfirst[j] = 0;
        if (u < nunits) {
            const unsigned S = a.subsets[u / ksplit], cm = (unsigned)(kObsTile - 1) & ~S;
            const unsigned lo1 = cm & (~cm + 1), cm1 = cm & (cm - 1), lo2 = lo1 | (cm1 & (~cm1 + 1));
            radr[j] = obs_lds_slot((unsigned)obs_deposit((uint64_t)(lane & 15), S) | (unsigned)obs_deposit((uint64_t)(lane >> 4), lo2));
            cmhi[j] = cm & ~lo2;
            xfirst[j] = (unsigned)obs_deposit((uint64_t)((u % ksplit) * kblocks), cmhi[j]);   // the kb-th submask of the walk
        }
    }
    for (int sl = blockIdx.y; sl < a.lanes; sl += gridDim.y) {
        const double2* __restrict__ src = a.src + (size_t)sl * dim;
        double4_t t1[kObsPerWave], t2[kObsPerWave], mm[kObsPerWave];
#pragma unroll
        for (int j = 0; j < kObsPerWave; ++j) t1[j] = t2[j] = mm[j] = double4_t{0, 0, 0, 0};
        double2 v[kObsPer];
        uint64_t g = blockIdx.x;
        {
            const uint64_t gbase = obs_deposit(g, rest);
#pragma unroll
            for (int j = 0; j < kObsPer; ++j) {
                const unsigned l = (unsigned)tid + kObsThreads * j;
                v[j] = l < tsize ? src[gbase | dep_tid | dep_j[j]] : make_double2(0.0, 0.0);
            }
        }
        for (;;) {
            __syncthreads();   // the reads of the tile before
#pragma unroll
            for (int j = 0; j < kObsPer; ++j) {
                const unsigned slot = slot_tid ^ obs_lds_slot((unsigned)(kObsThreads * j));
                sre[slot] = v[j].x;
                sim[slot] = v[j].y;
            }
            __syncthreads();
            const uint64_t gn = g + gridDim.x;
            if (gn < ngroups) {   // (ngroups > 1: a full tile, every l is valid)
                const uint64_t gbase = obs_deposit(gn, rest);
#pragma unroll
                for (int j = 0; j < kObsPer; ++j) v[j] = src[gbase | dep_tid | dep_j[j]];
            }
#pragma unroll
            for (int j = 0; j < kObsPerWave; ++j) {
                if (wave + kObsWaves * j >= nunits) continue;
                const unsigned walk = (unsigned)__builtin_amdgcn_readfirstlane((int)cmhi[j]);
                unsigned x = (unsigned)__builtin_amdgcn_readfirstlane((int)xfirst[j]);
                for (int kb0 = 0; kb0 < kblocks; kb0 += 8) {   // 32, 16 or 8 blocks, eight at a time
#pragma unroll
                    for (int kb = 0; kb < 8; ++kb) {
                        const unsigned at = radr[j] ^ obs_lds_slot(x);
                        const double ar = sre[at], ai = sim[at];
                        t1[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, ar, t1[j], 0, 0, 0);
                        t2[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, ai, t2[j], 0, 0, 0);
                        mm[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, ar, mm[j], 0, 0, 0);
                        x = (x - walk) & walk;   // the next submask of the walk
                    }
                }
            }
            if (gn >= ngroups) break;
            g = gn;
        }
        // D[4 r + lane / 16][lane % 16] in register r: row-major [16][16] at r * 64 + lane
        double* __restrict__ const pblock = a.partial + ((size_t)sl * gridDim.x + blockIdx.x) * (size_t)a.nsub * kObsPartial;
        if (ksplit > 1) {   // one or two subsets over four waves (nunits <= 4: unit = wave): the parts meet in LDS and are added in their order
            __syncthreads();   // the last tile's reads
            if (wave < nunits) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    lds[(size_t)wave * kObsPartial + r * 64 + lane] = t1[0][r];
                    lds[(size_t)wave * kObsPartial + 256 + r * 64 + lane] = t2[0][r];
                    lds[(size_t)wave * kObsPartial + 512 + r * 64 + lane] = mm[0][r];
                }
            }
            __syncthreads();
            for (int e = tid; e < a.nsub * (int)kObsPartial; e += kObsThreads) {
                const int s = e / (int)kObsPartial, at = e % (int)kObsPartial;
                double sum = lds[(size_t)(s * ksplit) * kObsPartial + at];
                for (int part = 1; part < ksplit; ++part) sum += lds[(size_t)(s * ksplit + part) * kObsPartial + at];
                pblock[e] = sum;
            }
            continue;   // (the next lane's first barrier stands before its writes of the tile)
        }
#pragma unroll
        for (int j = 0; j < kObsPerWave; ++j) {
            const int s = wave + kObsWaves * j;
            if (s >= a.nsub) continue;
            double* __restrict__ p = pblock + (size_t)s * kObsPartial;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r * 64 + lane] = t1[j][r];
                p[256 + r * 64 + lane] = t2[j][r];
                p[512 + r * 64 + lane] = mm[j][r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void obs_final_kernel(const double* __restrict__ partial, unsigned nblocks, int nsub, int lanes,
                                                        double2* __restrict__ rho, size_t lane_stride) {
    const int s = blockIdx.x, e = threadIdx.x, ra = e >> 4, rb = e & 15;
    const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra, iu = lo * 16 + hi, il = hi * 16 + lo;
    for (int sl = blockIdx.y; sl < lanes; sl += gridDim.y) {
        double s1 = 0.0, s2 = 0.0, mu = 0.0, ml = 0.0;
        const double* __restrict__ base = partial + ((size_t)sl * nblocks * (size_t)nsub + (size_t)s) * kObsPartial;
        // sixteen blocks' loads are issued before their additions, which keep the order of the blocks
        const unsigned count = nblocks;
        auto at = [&](unsigned i) { return base + (size_t)i * (size_t)nsub * kObsPartial; };
        unsigned i = 0;
        for (; i + 16 <= count; i += 16) {
            double v1[16], v2[16], vu[16], vl[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const double* __restrict__ p = at(i + k);
                v1[k] = p[iu]; v2[k] = p[256 + iu]; vu[k] = p[512 + iu]; vl[k] = p[512 + il];
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) { s1 += v1[k]; s2 += v2[k]; mu += vu[k]; ml += vl[k]; }
        }
        for (; i < count; ++i) {
            const double* __restrict__ p = at(i);
            s1 += p[iu]; s2 += p[256 + iu]; mu += p[512 + iu]; ml += p[512 + il];
        }
        const double up = mu - ml;   // Im rho[lo][hi]
        rho[(size_t)sl * lane_stride + (size_t)s * 256 + e] = make_double2(s1 + s2, ra == rb ? 0.0 : (ra < rb ? up : -up));
    }
}

}  // namespace

unsigned obs_grid_x(int n, int tile_bits) {
    const uint64_t ngroups = (uint64_t)1 << (n - tile_bits);
    return (unsigned)(ngroups < (uint64_t)kObsGridCap ? ngroups : (uint64_t)kObsGridCap);
}

hipError_t launch_obs_pass(const ObsArgs& a, hipStream_t s) {
    const dim3 grid(obs_grid_x(a.n, a.tile_bits), (unsigned)(a.lanes < 65535 ? a.lanes : 65535), 1);
    if (a.ksplit != obs_ksplit(a.nsub)) return hipErrorInvalidValue;
    obs_pass_kernel<<<grid, kObsThreads, 0, s>>>(a);
    return hipGetLastError();
}

int obs_ksplit(int nsub) { return nsub == 1 ? 4 : nsub == 2 ? 2 : 1; }

hipError_t launch_obs_final(const double* partial, unsigned nblocks, int nsub, int lanes, double2* rho, size_t lane_stride, hipStream_t s) {
    const dim3 grid((unsigned)nsub, (unsigned)(lanes < 65535 ? lanes : 65535), 1);
    obs_final_kernel<<<grid, 256, 0, s>>>(partial, nblocks, nsub, lanes, rho, lane_stride);
    return hipGetLastError();
}

}  // namespace aqc
