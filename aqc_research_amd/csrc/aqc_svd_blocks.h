// The host-visible decisions of the batched block-Jacobi SVD (aqc_svd_batch.hip), HIP-free: the same text is compiled for the device
// and by a plain C++ compiler (tests/native/svd_blocks_selftest.cpp); tests/svd_block_ref.py states the same rules in NumPy.
//   blocks      the columns of the work matrix in blocks of 16, the last one ragged
//   tournament  which block pairs meet in which round of a sweep (circle method; a bye when the block count is odd)
//   transpose   a wide matrix (cols > rows) is factorised through its conjugate transpose, as aqc_svd does
//   LDS bytes   what one workgroup keeps in LDS, against the 160 KiB of a CU
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define AQC_SVDB_FN __host__ __device__ inline
#else
#define AQC_SVDB_FN inline
#endif

namespace aqc {

enum { kSvdbBlock = 16, kSvdbPanel = 2 * kSvdbBlock, kSvdbMaxDim = 256, kSvdbThreads = 256, kSvdbMaxSweeps = 60, kSvdbInnerSweeps = 2 };
enum { kSvdbConverged = 0, kSvdbSweepLimit = 1, kSvdbNonFinite = 2 };   // status[i] of aqc_svd_batch
enum { kSvdbLdsPerCu = 160 * 1024 };

AQC_SVDB_FN int svdb_blocks(int cols) { return cols < 1 ? 0 : (cols + kSvdbBlock - 1) / kSvdbBlock; }
// columns of block b (0 for a block that does not exist, the bye included)
AQC_SVDB_FN int svdb_block_width(int b, int cols) {
    if (b < 0 || b >= svdb_blocks(cols)) return 0;
    const int left = cols - b * kSvdbBlock;
    return left < kSvdbBlock ? left : kSvdbBlock;
}
// A sweep over nb blocks: n2 = nb rounded up to even seats, n2 - 1 rounds of n2 / 2 slots (one block: one round, one slot).
AQC_SVDB_FN int svdb_rounds(int nb) { const int n2 = nb + (nb & 1); return n2 < 2 ? (nb > 0 ? 1 : 0) : n2 - 1; }
AQC_SVDB_FN int svdb_slots(int nb) { const int n2 = nb + (nb & 1); return n2 < 2 ? (nb > 0 ? 1 : 0) : n2 / 2; }
// The pair of (round, slot): seat n2 - 1 stays, the others move one seat per round.  x < y, or y = -1: block x has the bye and
// plays alone (its own columns against each other).  With an even count the columns inside a block meet in every pair the block is in.
AQC_SVDB_FN void svdb_pair(int nb, int round, int slot, int* x, int* y) {
    const int n2 = nb + (nb & 1), ring = n2 - 1;
    int a, b;
    if (slot == 0) { a = round % ring; b = ring; }
    else { a = (round + slot) % ring; b = (round + ring - slot) % ring; }
    if (a > b) { const int t = a; a = b; b = t; }
    *x = a;
    *y = b < nb ? b : -1;
}
// mode 0: the work matrix is A (rows x cols, rows >= cols); mode 1: A^H (cols x rows).  Either way work rows >= work columns.
AQC_SVDB_FN int svdb_mode(int rows, int cols) { return cols > rows ? 1 : 0; }
AQC_SVDB_FN int svdb_work_rows(int rows, int cols) { return cols > rows ? cols : rows; }
AQC_SVDB_FN int svdb_work_cols(int rows, int cols) { return cols > rows ? rows : cols; }
// LDS of one workgroup, array by array as the kernel declares them (a static_assert there compares the sum): the Gram matrix G and
// the accumulated unitary J of a panel (32 x 32 complex each), the rotations of one inner round (16 x 4 doubles), the pairs of that
// round (2 x 16 ints), the panel's column indices (32 ints), the singular values and their ranks (kSvdbMaxDim each) and the reduction
// scratch (a double per wave).  The same at every size: the panel's columns themselves stream from L2 straight into the matrix
// cores' operands -- at 256 rows a panel is 128 KiB, which with G and J would leave no room for a second workgroup on the CU.
AQC_SVDB_FN constexpr size_t svdb_lds_bytes(int work_rows, int work_cols) {
    (void)work_rows;
    (void)work_cols;
    return (size_t)2 * kSvdbPanel * kSvdbPanel * 16 + (size_t)kSvdbBlock * 4 * 8 + (size_t)2 * kSvdbBlock * 4 + (size_t)kSvdbPanel * 4 +
           (size_t)kSvdbMaxDim * (8 + 4) + (size_t)(kSvdbThreads / 64) * 8;
}
AQC_SVDB_FN int svdb_workgroups_per_cu(int work_rows, int work_cols) { return (int)((size_t)kSvdbLdsPerCu / svdb_lds_bytes(work_rows, work_cols)); }

}  // namespace aqc
