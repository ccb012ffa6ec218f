// Stand-alone check of csrc/aqc_svd_blocks.h (the host-visible decisions of the batched block-Jacobi SVD), built by a plain C++
// compiler under ASan + UBSan (tests/test_svd_block_host.py).  Exit status 0 and the line "ok" mean every check held; with the
// argument "schedule N" it prints the tournament of N blocks instead, one round per line, for the comparison with the NumPy statement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_svd_blocks.h"

using namespace aqc;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "schedule") == 0) {
        const int nb = std::atoi(argv[2]);
        for (int r = 0; r < svdb_rounds(nb); ++r) {
            for (int s = 0; s < svdb_slots(nb); ++s) {
                int x, y;
                svdb_pair(nb, r, s, &x, &y);
                std::printf("%d,%d ", x, y);
            }
            std::printf("\n");
        }
        return 0;
    }
    for (int nb = 1; nb <= 17; ++nb) {
        const int rounds = svdb_rounds(nb), slots = svdb_slots(nb);
        std::vector<int> met((size_t)nb * nb, 0), byes(nb, 0);
        for (int r = 0; r < rounds; ++r) {
            std::vector<int> seen(nb, 0);   // a block plays at most once per round: the pairs of a round are disjoint
            for (int s = 0; s < slots; ++s) {
                int x = -7, y = -7;
                svdb_pair(nb, r, s, &x, &y);
                CHECK(x >= 0 && x < nb, "nb %d round %d slot %d: x = %d", nb, r, s, x);
                CHECK(y == -1 || (y > x && y < nb), "nb %d round %d slot %d: (x, y) = (%d, %d)", nb, r, s, x, y);
                if (x < 0 || x >= nb || y >= nb) continue;
                ++seen[x];
                if (y >= 0) { ++seen[y]; ++met[(size_t)x * nb + y]; } else { ++byes[x]; }
            }
            int nbye = 0;
            for (int b = 0; b < nb; ++b) CHECK(seen[b] == 1, "nb %d round %d: block %d plays %d times", nb, r, b, seen[b]);
            for (int s = 0; s < slots; ++s) { int x, y; svdb_pair(nb, r, s, &x, &y); nbye += y < 0; }
            CHECK(nbye == (nb & 1), "nb %d round %d: %d byes", nb, r, nbye);   // odd count: exactly one bye in every round
        }
        for (int x = 0; x < nb; ++x)
            for (int y = x + 1; y < nb; ++y) CHECK(met[(size_t)x * nb + y] == 1, "nb %d: pair (%d, %d) met %d times in a sweep", nb, x, y, met[(size_t)x * nb + y]);
        for (int b = 0; b < nb; ++b) CHECK(byes[b] == (nb & 1), "nb %d: block %d has %d byes in a sweep", nb, b, byes[b]);
        CHECK(rounds * slots * 2 >= nb, "nb %d: %d rounds of %d slots", nb, rounds, slots);
    }
    for (int cols = 1; cols <= kSvdbMaxDim; ++cols) {   // ragged last block: the widths add up, only the last one is short
        const int nb = svdb_blocks(cols);
        int total = 0;
        for (int b = 0; b < nb; ++b) {
            const int w = svdb_block_width(b, cols);
            CHECK(w >= 1 && w <= kSvdbBlock && (w == kSvdbBlock || b == nb - 1), "cols %d block %d: width %d", cols, b, w);
            total += w;
        }
        CHECK(total == cols, "cols %d: widths add up to %d", cols, total);
        CHECK(svdb_block_width(nb, cols) == 0 && svdb_block_width(-1, cols) == 0, "cols %d: a block that does not exist has columns", cols);
        CHECK(nb == (cols + 15) / 16 && nb <= 16, "cols %d: %d blocks", cols, nb);
    }
    CHECK(svdb_blocks(0) == 0 && svdb_rounds(0) == 0 && svdb_slots(0) == 0, "no columns");
    for (int rows = 1; rows <= kSvdbMaxDim; rows += 5)   // transposition: the work matrix is never wide; LDS within a CU
        for (int cols = 1; cols <= kSvdbMaxDim; cols += 3) {
            const int wr = svdb_work_rows(rows, cols), wc = svdb_work_cols(rows, cols);
            CHECK(svdb_mode(rows, cols) == (cols > rows ? 1 : 0), "%d x %d: mode", rows, cols);
            CHECK(wr >= wc && wr == (rows > cols ? rows : cols) && wc == (rows < cols ? rows : cols), "%d x %d: work %d x %d", rows, cols, wr, wc);
            CHECK(svdb_lds_bytes(wr, wc) <= (size_t)kSvdbLdsPerCu && svdb_workgroups_per_cu(wr, wc) >= 1, "%d x %d: %zu bytes of LDS", rows, cols, svdb_lds_bytes(wr, wc));
        }
    CHECK(svdb_lds_bytes(256, 256) >= (size_t)2 * 32 * 32 * 16, "G and J alone take 32 KiB");
    if (failures == 0) std::printf("ok\n");
    return failures == 0 ? 0 : 1;
}
