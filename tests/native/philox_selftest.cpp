// Host build of csrc/aqc_philox.h (tests/test_sketch_host.py, under ASan + UBSan).
//   philox_selftest raw  key0 key1 c0 c1 c2 c3 nblocks : the blocks NumPy's generator hands out after Philox(key, counter) -- the
//       counter is advanced BEFORE every block, carries included -- as "word(hex) double(hex of its bits)" lines
//   philox_selftest plane seed stream it lane plane count : elements 0..count-1 of a plane by the draw rule, as hex of the doubles
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../aqc_research_amd/csrc/aqc_philox.h"

static uint64_t bits_of(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char** argv) {
    if (argc == 9 && !strcmp(argv[1], "raw")) {
        uint64_t key[2], ctr[4];
        for (int i = 0; i < 2; ++i) key[i] = strtoull(argv[2 + i], nullptr, 0);
        for (int i = 0; i < 4; ++i) ctr[i] = strtoull(argv[4 + i], nullptr, 0);
        const long nblocks = strtol(argv[8], nullptr, 0);
        for (long b = 0; b < nblocks; ++b) {
            uint64_t out[4];
            aqc::philox_advance(ctr, 1);
            aqc::philox4x64_10(ctr, key, out);
            for (int w = 0; w < 4; ++w) printf("%016" PRIx64 " %016" PRIx64 "\n", out[w], bits_of(aqc::philox_uniform(out[w])));
        }
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "plane")) {
        uint64_t a[5];
        for (int i = 0; i < 5; ++i) a[i] = strtoull(argv[2 + i], nullptr, 0);
        const uint64_t count = strtoull(argv[7], nullptr, 0);
        for (uint64_t e = 0; e < count; ++e) printf("%016" PRIx64 "\n", bits_of(aqc::philox_plane_uniform(a[0], a[1], a[2], a[3], a[4], e)));
        return 0;
    }
    fprintf(stderr, "usage: philox_selftest raw key0 key1 c0 c1 c2 c3 nblocks | plane seed stream it lane plane count\n");
    return 2;
}
