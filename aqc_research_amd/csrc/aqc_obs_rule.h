// The rules of the reduced density matrices (aqc_obs.hip), HIP-free: the same text is compiled for the device and by a plain C++
// compiler (tests/native/obs_rule_selftest.cpp); tests/obs_ref.py states the result in NumPy.
//   convention  state index bit q is qubit q.  For listed qubits (q_0 .. q_{k-1}) the matrix's row index has bit m = the value of q_m:
//               rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b)
//   primitive   a set S of 4 qubits; the state as a 16 x 2^(n-4) matrix A with the rows indexed by the bits of S (row bit m = the m-th
//               lowest qubit of S); rho_S = A A^H.  Every matrix of k <= 4 qubits inside S is a partial trace of it (obs_partial_trace).
//   plan        requests (sets of 2 .. 4 qubits, pairs for the ABI) -> passes.  A pass is a set B of min(n, T) tile bits, T = 11; with
//               n > T it holds the low c = 5 bits (runs of 32 contiguous amplitudes) and T - c free positions.  A pass carries at most
//               kObsMaxSubsets 4-subsets of B in tile-local bit positions (position j = the j-th lowest bit of B; with n < 4 the
//               positions n .. 3 are virtual qubits, always 0); more of them repeat the same B in a further pass.  Greedy cover: the
//               free bit that completes most uncovered requests (ties: obs_detail::pick_bit) joins B
//               until it is full, then the requests inside B are covered by 4-subsets chosen the same way.  A request is served by the
//               first (pass, subset) in plan order that holds it.  The plan depends on n and the request list only.
//   addressing  tile-local index l of tile group g <-> global index obs_deposit(l, B) | obs_deposit(g, all bits but B)
// All index arithmetic is 64-bit: n goes up to 30 and lanes << n up to 2^kMaxBits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define AQC_OBS_FN __host__ __device__ inline
#else
#define AQC_OBS_FN inline
#endif

namespace aqc {

enum { kObsMinQubits = 2, kObsMaxQubits = 30, kObsTileBits = 11, kObsLowBits = 5, kObsSetBits = 4, kObsWaves = 4, kObsPerWave = 4,
       kObsMaxSubsets = kObsWaves * kObsPerWave };

// the bits of v, lowest first, at the positions of the set bits of mask, lowest first (pdep)
AQC_OBS_FN uint64_t obs_deposit(uint64_t v, uint64_t mask) {
    uint64_t out = 0;
    while (mask) {
        const uint64_t low = mask & (~mask + 1);
        if (v & 1) out |= low;
        v >>= 1;
        mask &= mask - 1;
    }
    return out;
}

// global index of the tile-local index l in tile group g of a pass with bit set `bits` (a mask of n-bit positions)
AQC_OBS_FN uint64_t obs_global_index(uint64_t l, uint64_t g, uint64_t bits, int n) {
    const uint64_t all = ((uint64_t)1 << n) - 1;
    return obs_deposit(l, bits & all) | obs_deposit(g, all & ~bits);
}

// the tile's image in LDS: tile-local index l lives at plane offset obs_lds_slot(l).  The low five bits are folded with an odd-weight
// word per higher bit, so the eleven address bits have eleven different odd-weight images in the five bank bits.  The 32 lanes of a
// half wave differ in five address bits (the 4 of a subset and one column bit).  A relation among different odd-weight words has an
// even number of terms; two different relations of 4 terms among 5 words would add up to one of 2 terms, two equal words.  So the five
// images have rank >= 4: lanes meet on a bank at most in pairs, whichever positions the subset holds (the self-test walks all 330).
AQC_OBS_FN unsigned obs_lds_slot(unsigned l) {
    unsigned f = 0;
    f ^= (l >> 5) & 1u ? 0x07u : 0u;
    f ^= (l >> 6) & 1u ? 0x0Bu : 0u;
    f ^= (l >> 7) & 1u ? 0x0Du : 0u;
    f ^= (l >> 8) & 1u ? 0x0Eu : 0u;
    f ^= (l >> 9) & 1u ? 0x13u : 0u;
    f ^= (l >> 10) & 1u ? 0x15u : 0u;
    return l ^ f;
}

// rho16: the 16 x 16 matrix of a subset, row-major (re, im) pairs.  pos[m] (0 .. 3, distinct) is the bit of the subset's row index that
// listed qubit m is.  out: 2^k x 2^k, row-major (re, im) pairs, by the convention above; the other 4 - k bits are traced out.
inline void obs_partial_trace(const double* rho16, int k, const int* pos, double* out) {
    unsigned keep = 0;
    for (int m = 0; m < k; ++m) keep |= 1u << pos[m];
    const unsigned rest = 0xFu & ~keep;
    const int dim = 1 << k, nrest = 1 << (kObsSetBits - k);
    for (int a = 0; a < dim; ++a)
        for (int b = 0; b < dim; ++b) {
            unsigned ra = 0, rb = 0;
            for (int m = 0; m < k; ++m) {
                ra |= ((unsigned)(a >> m) & 1u) << pos[m];
                rb |= ((unsigned)(b >> m) & 1u) << pos[m];
            }
            double re = 0.0, im = 0.0;
            for (int r = 0; r < nrest; ++r) {
                const unsigned d = (unsigned)obs_deposit((uint64_t)r, rest);
                const double* e = rho16 + 2 * ((size_t)(ra | d) * 16 + (rb | d));
                re += e[0];
                im += e[1];
            }
            out[2 * ((size_t)a * dim + b)] = re;
            out[2 * ((size_t)a * dim + b) + 1] = im;
        }
}

struct ObsPass {
    uint32_t bits = 0;                       // B as a mask of qubits
    int nbits = 0;                           // |B| = min(n, kObsTileBits)
    std::vector<uint16_t> subsets;           // masks of 4 tile-local positions each, at most kObsMaxSubsets
};
struct ObsPlan {
    std::vector<ObsPass> passes;
    std::vector<int> serve_pass, serve_subset;   // per request
};

namespace obs_detail {

inline int popcount32(uint32_t v) { return __builtin_popcount(v); }

// The bit of `candidates` to add to `have` (masks over the same positions) for the requests still open: the one that completes most
// requests that fit `limit` bits together with have, then the one that leaves a request it touches the fewest bits short, then the one
// most such requests touch, then the lowest.  -1: no request gains.
inline int pick_bit(const std::vector<uint32_t>& req, const std::vector<char>& open, uint32_t have, uint32_t candidates, int limit) {
    int best = -1, best_done = -1, best_short = 99, best_touch = -1;
    for (int p = 0; p < 32; ++p) {
        if (!((candidates >> p) & 1u)) continue;
        const uint32_t with = have | (1u << p);
        int done = 0, touch = 0, shortest = 99;
        for (size_t r = 0; r < req.size(); ++r) {
            if (!open[r] || !((req[r] >> p) & 1u) || (req[r] & ~(have | candidates))) continue;
            if (popcount32(req[r] | with) > limit) continue;
            ++touch;
            const int missing = popcount32(req[r] & ~with);
            if (missing == 0) ++done;
            if (missing < shortest) shortest = missing;
        }
        if (touch == 0) continue;
        if (done > best_done || (done == best_done && (shortest < best_short || (shortest == best_short && touch > best_touch)))) {
            best = p; best_done = done; best_short = shortest; best_touch = touch;
        }
    }
    return best;
}

}  // namespace obs_detail

// The plan of requests req[r] (masks of 2 .. 4 qubits below n).  Host only.
inline ObsPlan obs_plan(int n, const std::vector<uint32_t>& req) {
    using namespace obs_detail;
    ObsPlan plan;
    plan.serve_pass.assign(req.size(), -1);
    plan.serve_subset.assign(req.size(), -1);
    const uint32_t all = (uint32_t)(((uint64_t)1 << n) - 1);
    const int T = n < kObsTileBits ? n : kObsTileBits;
    std::vector<char> open(req.size(), 1);
    size_t left = req.size();
    while (left) {
        // the pass's bit set
        uint32_t B = n > kObsTileBits ? (1u << kObsLowBits) - 1 : all;
        while (popcount32(B) < T) {
            int p = pick_bit(req, open, B, all & ~B, T);
            if (p < 0)
                for (p = 0; (B >> p) & 1u; ++p) {}   // nothing to gain: the lowest unused position keeps the tile full
            B |= 1u << p;
        }
        // tile-local requests inside B (with n < 4 the tile has the virtual positions n .. 3)
        const int positions = T < kObsSetBits ? kObsSetBits : T;
        const uint32_t local_all = (1u << positions) - 1;
        std::vector<uint32_t> loc(req.size(), 0);
        std::vector<char> in(req.size(), 0);
        size_t inside = 0;
        for (size_t r = 0; r < req.size(); ++r) {
            if (!open[r] || (req[r] & ~B)) continue;
            for (int q = 0; q < n; ++q)
                if ((req[r] >> q) & 1u) loc[r] |= 1u << popcount32(B & ((1u << q) - 1));
            in[r] = 1;
            ++inside;
        }
        if (!inside) return plan;   // (cannot happen for requests of at most 4 qubits below n; their serve entries stay -1)
        while (inside) {   // one pass per kObsMaxSubsets subsets, the same B
            ObsPass pass;
            pass.bits = B;
            pass.nbits = T;
            while (inside && (int)pass.subsets.size() < kObsMaxSubsets) {
                uint32_t S = 0;
                while (popcount32(S) < kObsSetBits) {
                    int p = pick_bit(loc, in, S, local_all & ~S, kObsSetBits);
                    if (p < 0)
                        for (p = 0; (S >> p) & 1u; ++p) {}
                    S |= 1u << p;
                }
                for (size_t r = 0; r < req.size(); ++r)
                    if (in[r] && !(loc[r] & ~S)) {
                        in[r] = 0; open[r] = 0; --inside; --left;
                        plan.serve_pass[r] = (int)plan.passes.size();
                        plan.serve_subset[r] = (int)pass.subsets.size();
                    }
                pass.subsets.push_back((uint16_t)S);
            }
            plan.passes.push_back(pass);
        }
    }
    return plan;
}

}  // namespace aqc
