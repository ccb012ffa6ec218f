// The rules of the conversion of MPS states into dense vectors and into blocks of amplitudes (aqc_mps_tovec.hip, aqc_mps_tovec_api.cpp),
// HIP-free: the same text is compiled into the library and by a plain C++ compiler (tests/native/mps_tovec_rule_selftest.cpp);
// tests/mps_obs_ref.dense states the result in NumPy.  psi(b) = T_0[b_0] T_1[b_1] ... T_{n-1}[b_{n-1}], index = sum_q b_q 2^q, site
// tensors T_q [2][chi_q][chi_{q+1}] in any gauge and of any norm.
//   split   k low sites: L[l][j] = (T_0[l_0] ... T_{k-1}[l_{k-1}])[0][j], H[r][j] = (T_k[r_0] ... T_{n-1}[r_{n-k-1}])[j][0],
//           out[r 2^k + l] = sum_j H[r][j] L[l][j], j in order.  Whole vectors: k = n / 2, a function of n alone; blocks: the caller's
//           low_qubits, and r runs over the listed rows (the bits of the sites k .. n - 1) only
//   halves  L_0 = H_0 = [1]; L_{j+1}[b 2^j + l] = L_j[l] T_j[b] (the new site is the highest bit of l), H_{j+1}[2 r + b] =
//           H_j[r] T_{n-1-j}[b]^T (the new site is the lowest bit of r: r ends in the register's bit order).  The first
//           kMpsToVecHeadSteps steps of a half (factors of at most kMpsToVecTile rows) run in one launch, every later one in a launch of
//           its own, a workgroup per kMpsToVecTile rows of the factor it reads; the two stores of a half take turns
//   outer   a workgroup owns kMpsToVecTile rows of H and kMpsToVecChunksPerBlock column chunks of kMpsToVecTile rows of L
//   route   per state: fused when every bond is at most kMpsObsFusedCap (the planes of aqc_mps_planes.h), else gemm (the chain of
//           products of the workspace's mps_to_vec, whole vectors only)
//   chunks  the lanes (distinct states) of a call go in chunks whose output lanes and halves stay within a budget of device bytes
#pragma once
#include <stddef.h>

#include "aqc_mps_obs_rule.h"
#include "aqc_mps_states_rule.h"

namespace aqc {

enum { kMpsToVecByRule = 0, kMpsToVecFused = 1, kMpsToVecGemm = 2 };
enum { kMpsToVecMaxQubits = 30, kMpsToVecMaxLow = 24 };       // whole vectors; the low qubits of a block
enum { kMpsToVecTile = 64, kMpsToVecHeadSteps = 6, kMpsToVecChunksPerBlock = 8, kMpsToVecMaxChunkLanes = 65535 };
constexpr size_t kMpsToVecBudget = (size_t)8 << 30;            // device bytes of a chunk's output lanes and halves
static_assert((1 << kMpsToVecHeadSteps) == kMpsToVecTile && kMpsToVecTile == kMpsObsFusedCap, "the head of a half fills one tile of the planes");

inline bool mps_tovec_method_ok(int method) { return method == kMpsToVecByRule || method == kMpsToVecFused || method == kMpsToVecGemm; }
inline int mps_tovec_route(int n, const int* dims) { return mps_max_bond(n, dims) <= kMpsObsFusedCap ? kMpsToVecFused : kMpsToVecGemm; }

// the split of a whole vector and the row counts of the two halves
inline int mps_tovec_split(int n) { return n / 2; }
inline size_t mps_tovec_low_rows(int k) { return (size_t)1 << k; }
inline size_t mps_tovec_high_rows(int n, int k) { return (size_t)1 << (n - k); }
inline size_t mps_tovec_tiles(size_t rows) { return (rows + kMpsToVecTile - 1) / kMpsToVecTile; }
// the outer product's grid: row tiles of H x groups of column chunks of L
inline size_t mps_tovec_row_tiles(size_t high_rows) { return mps_tovec_tiles(high_rows); }
inline size_t mps_tovec_col_chunks(int k) { return mps_tovec_tiles(mps_tovec_low_rows(k)); }
inline size_t mps_tovec_col_groups(int k) { return (mps_tovec_col_chunks(k) + kMpsToVecChunksPerBlock - 1) / kMpsToVecChunksPerBlock; }

// a half of `len` sites: its launches (the head, then a step per further site), and which of its two stores holds the result
inline int mps_tovec_half_launches(int len) { return 1 + (len > kMpsToVecHeadSteps ? len - kMpsToVecHeadSteps : 0); }
inline int mps_tovec_half_store(int len) { return len > kMpsToVecHeadSteps ? (len - kMpsToVecHeadSteps) & 1 : 0; }
// launches of the fused route of a chunk: the halves side by side in the grid (blocks: the low half, the walk of the rows), the outer product
inline int mps_tovec_launches(int n, int k, bool blocks) {
    const int longer = blocks || k > n - k ? k : n - k;
    return mps_tovec_half_launches(longer) + (blocks ? 1 : 0) + 1;
}

// elements of one store of a half of `rows` rows at bonds up to max_bond (the stores of all lanes of a call are at the same stride:
// its largest bond on the fused route)
inline size_t mps_tovec_half_elems(size_t rows, int max_bond = kMpsObsFusedCap) { return rows * (size_t)max_bond; }
// device bytes of one lane, a function of the shape alone (the bonds at the cap): the output and the two stores of each half.  Whole
// vectors: high_rows = 2^(n-k); blocks: the listed rows
inline size_t mps_tovec_lane_bytes(int k, size_t high_rows) {
    return 16 * ((high_rows << k) + 2 * mps_tovec_half_elems(mps_tovec_low_rows(k)) + 2 * mps_tovec_half_elems(high_rows));
}
// lanes per chunk (0: not even one fits), and the chunks of `lanes` lanes: chunk c takes the lanes [c chunk, min(lanes, (c + 1) chunk))
inline int mps_tovec_chunk(size_t lane_bytes, size_t lanes, size_t budget_bytes) {
    size_t g = budget_bytes / lane_bytes;
    if (g > lanes) g = lanes;
    if (g > kMpsToVecMaxChunkLanes) g = kMpsToVecMaxChunkLanes;
    return (int)g;
}
inline size_t mps_tovec_chunks(size_t lanes, int chunk) { return chunk > 0 ? (lanes + (size_t)chunk - 1) / (size_t)chunk : 0; }

// blocks: what the call refuses about its shape; null: fine
inline const char* mps_tovec_check_blocks(int n, int low_qubits, long long rows) {
    if (n < 2) return "blocks of amplitudes need at least 2 qubits";
    if (low_qubits < 1 || low_qubits > n - 1 || low_qubits > kMpsToVecMaxLow) return "low_qubits must be in 1 .. min(n - 1, 24)";
    if (rows < 1) return "at least one row is needed";
    if (rows > (long long)kMpsToVecTile * 65535) return "too many rows in one call";
    return nullptr;
}
// the first entry of high_bits that is not 0 or 1, or -1
inline long long mps_tovec_bad_bit(const unsigned char* bits, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (bits[i] > 1) return (long long)i;
    return -1;
}

}  // namespace aqc
