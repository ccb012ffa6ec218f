// Self-test of csrc/aqc_mps_sample_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_sample_rule.py): the draw
// rule against words that NumPy's Philox produced, the decision at its edges, the weight check, the route rule at the fused cap, the
// chunk sizes of the gemm route and the validity checks.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_sample_rule.h"

using namespace aqc;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// np.random.Philox(key=[seed, 16], counter=[0, shot, lane, 0]).random_raw(8), key and counter as uint64 arrays
struct Draws { uint64_t seed, lane, shot, words[8]; };
static const Draws kDraws[] = {
    {2024, 0, 0,
     {0xeb34924288a5ea28ull, 0x305eb1dfaf380c0eull, 0xbe27932c5cfffbe5ull, 0xa823b97bf4d683bcull, 0x65cb473864420e2cull, 0x873cb3d9f3adf188ull,
      0x07f825e9b11962c6ull, 0x87370e028dd8efbaull}},
    {2024, 2, 777,
     {0xdae926611d74ce3full, 0xbcb53d51e18cfc19ull, 0x26edf60702a35e04ull, 0x1fee7193fd7bf1a0ull, 0xd93d508008875ddbull, 0xcf8ca0be791334a9ull,
      0xff6796a6eef8b48eull, 0x309fddb5a6149422ull}},
    {0xFFFFFFFFFFFFFFFFull, 1, (1ull << 40) + 5,
     {0x8f79cfbe51195a6dull, 0xac3f3b0688171c35ull, 0xb138f05eae407359ull, 0x7b9ed5ed9d03aae5ull, 0x1a1cb0445ecd5967ull, 0x8709930c5c3d6705ull,
      0xd942d62576fd66b2ull, 0x4a90e6dad39fa6dbull}},
};

int main() {
    CHECK(kMpsSampleStream == 16);
    for (const Draws& d : kDraws)
        for (uint64_t q = 0; q < 8; ++q) {
            uint64_t blk[4];
            mps_sample_block(d.seed, d.lane, d.shot, q >> 2, blk);
            CHECK(blk[q & 3] == d.words[q]);
            CHECK(mps_sample_uniform(d.seed, d.lane, d.shot, q) == philox_uniform(d.words[q]));
        }
    // .random(8) of the first generator: the first and the sixth double
    CHECK(mps_sample_uniform(2024, 0, 0, 0) == 0.9187709248004904);
    CHECK(mps_sample_uniform(2024, 0, 0, 5) == 0.5282699973210396);

    // the decision u (m0 + m1) < m0 at its edges
    const double umax = philox_uniform(~0ull);   // 1 - 2^-53
    CHECK(umax < 1.0 && umax == 1.0 - std::ldexp(1.0, -53) && philox_uniform(0) == 0.0);
    for (double m : {1.0, 3e-300, 7e300, 0.3}) {
        for (double u : {0.0, 0.5, umax}) {
            CHECK(mps_sample_decide(u, 0.0, m) == 1);   // a branch of zero weight is never taken
            CHECK(mps_sample_decide(u, m, 0.0) == 0);
        }
        CHECK(mps_sample_decide(0.0, m, m) == 0 && mps_sample_decide(umax, m, m) == 1);
        CHECK(mps_sample_decide(0.5, m, m) == 1 && mps_sample_decide(std::nextafter(0.5, 0.0), m, m) == 0);   // the threshold itself goes to 1
    }
    CHECK(mps_sample_decide(0.25, 1.0, 3.0) == 1 && mps_sample_decide(0.2499, 1.0, 3.0) == 0);

    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(mps_sample_weights_ok(1.0, 0.0) && mps_sample_weights_ok(0.0, 5e-324) && mps_sample_weights_ok(1e308, 1e307));
    CHECK(!mps_sample_weights_ok(0.0, 0.0) && !mps_sample_weights_ok(-1.0, 0.5) && !mps_sample_weights_ok(1.0, -1.0));
    CHECK(!mps_sample_weights_ok(inf, 1.0) && !mps_sample_weights_ok(nan, 1.0) && !mps_sample_weights_ok(1.0, nan) && !mps_sample_weights_ok(1e308, 1e308));

    // route: fused up to the cap, on every bond
    {
        const int a[] = {1, 2, 64, 64, 2, 1}, b[] = {1, 2, 65, 2, 1}, c[] = {1, 1}, d[] = {1, 64, 1, 100, 1};
        CHECK(mps_sample_route(5, a) == kMpsSampleFused && mps_max_bond(5, a) == 64);
        CHECK(mps_sample_route(4, b) == kMpsSampleGemm && mps_max_bond(4, b) == 65);
        CHECK(mps_sample_route(1, c) == kMpsSampleFused);
        CHECK(mps_sample_route(4, d) == kMpsSampleGemm);
    }

    // chunks: as many shots as keep five [chunk][bond] complex matrices within 256 MiB, at least 64, at most 2^20 and the call's own
    CHECK(mps_sample_chunk(65, 1 << 24) == (int64_t)((size_t)(256 << 20) / (80 * 65)));
    CHECK(mps_sample_chunk(512, 1 << 24) == 6553 && mps_sample_chunk(512, 1000) == 1000 && mps_sample_chunk(512, 1) == 1);
    CHECK(mps_sample_chunk(1, 1 << 24) == kMpsSampleMaxChunk && mps_sample_chunk(1, 100) == 100);
    CHECK(mps_sample_chunk(1 << 20, 1 << 24) == 64 && mps_sample_chunk(1 << 20, 10) == 10);   // never below 64 while the call has them
    for (int bond : {1, 3, 64, 65, 100, 512, 4096, 100000})
        for (int64_t shots : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)1000, (int64_t)1 << 24}) {
            const int64_t c = mps_sample_chunk(bond, shots);
            CHECK(c >= 1 && c <= shots && c <= kMpsSampleMaxChunk);
            CHECK(c == shots || c >= 64);
            CHECK(c <= 64 || (size_t)c * bond * 80 <= kMpsSampleScratch);
        }

    // validity
    CHECK(mps_sample_check_counts(1, 1) == nullptr && mps_sample_check_counts(3, kMpsSampleMaxShots) == nullptr);
    CHECK(mps_sample_check_counts(0, 1) != nullptr && mps_sample_check_counts(1, 0) != nullptr && mps_sample_check_counts(1, -5) != nullptr);
    CHECK(mps_sample_check_counts(1, kMpsSampleMaxShots + 1) != nullptr);
    CHECK(mps_sample_method_ok(0) && mps_sample_method_ok(1) && mps_sample_method_ok(2) && !mps_sample_method_ok(3) && !mps_sample_method_ok(-1));
    {
        std::vector<uint8_t> bits(40, 0);
        bits[7] = 1;
        CHECK(mps_sample_bad_bit(bits.data(), bits.size()) == -1 && mps_sample_bad_bit(bits.data(), 0) == -1);
        bits[33] = 2;
        bits[35] = 255;
        CHECK(mps_sample_bad_bit(bits.data(), bits.size()) == 33 && mps_sample_bad_bit(bits.data(), 33) == -1);
    }
    std::printf("mps_sample_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
