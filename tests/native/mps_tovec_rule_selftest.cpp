// Self-test of csrc/aqc_mps_tovec_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_tovec_rule.py): the split,
// the row, tile and chunk counts and the store sizes for n = 1 .. 30, the launches of a half and the store that holds its result by a
// host walk of the ping-pong, the route at bonds 64 / 65, the chunking under small budgets, the checks of a block call, and the split
// statement itself against the one-sided product on a small state.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_tovec_rule.h"

using namespace aqc;
typedef std::complex<double> cd;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { ++failures; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, in (-1, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 4503599627370496.0 - 1.0;
}

static void sizes() {
    for (int n = 1; n <= kMpsToVecMaxQubits; ++n) {
        const int k = mps_tovec_split(n);
        CHECK(k == n / 2 && k >= 0 && n - k >= 1 && n - k - k <= 1);
        const size_t low = mps_tovec_low_rows(k), high = mps_tovec_high_rows(n, k);
        CHECK(low * high == (size_t)1 << n);
        CHECK(mps_tovec_row_tiles(high) == (high + 63) / 64 && mps_tovec_row_tiles(high) >= 1 && mps_tovec_row_tiles(high) <= 65535);
        CHECK(mps_tovec_col_chunks(k) == (low + 63) / 64 && mps_tovec_col_chunks(k) >= 1);
        const size_t groups = mps_tovec_col_groups(k);
        CHECK(groups >= 1 && groups * kMpsToVecChunksPerBlock >= mps_tovec_col_chunks(k) && (groups - 1) * kMpsToVecChunksPerBlock < mps_tovec_col_chunks(k));
        CHECK(mps_tovec_half_elems(low) == low * 64 && mps_tovec_half_elems(high) == high * 64);
        CHECK(mps_tovec_half_elems(high, 1) == high && mps_tovec_half_elems(high, 37) == high * 37 && mps_tovec_half_elems(low, 64) == mps_tovec_half_elems(low));
        // every factor of a half fits its store: 2^j rows of at most 64 columns
        for (int j = 0; j <= n - k; ++j) CHECK(((size_t)1 << j) * kMpsObsFusedCap <= mps_tovec_half_elems(high));
        for (int j = 0; j <= k; ++j) CHECK(((size_t)1 << j) * kMpsObsFusedCap <= mps_tovec_half_elems(low));
        CHECK(mps_tovec_lane_bytes(k, high) == 16 * (((size_t)1 << n) + 128 * low + 128 * high));
        CHECK(mps_tovec_launches(n, k, false) == mps_tovec_half_launches(n - k) + 1);
    }
    CHECK(mps_tovec_row_tiles(256) == 4 && mps_tovec_col_chunks(8) == 4);     // 16 qubits: 4 row tiles x 4 column chunks
    CHECK(mps_tovec_row_tiles(128) == 2);                                       // 13 qubits: k = 6, 128 rows of H
    CHECK(mps_tovec_tiles(1) == 1 && mps_tovec_tiles(64) == 1 && mps_tovec_tiles(65) == 2 && mps_tovec_tiles(200) == 4);
}

static void halves() {
    for (int len = 0; len <= 30; ++len) {
        // the walk of the ping-pong: the head leaves its factor in store 0, every later step reads one store and writes the other
        int store = 0, launches = 1;
        for (int j = kMpsToVecHeadSteps; j < len; ++j) {
            const int from = (j - kMpsToVecHeadSteps) & 1;
            CHECK(from == store);
            store = from ^ 1;
            ++launches;
        }
        CHECK(mps_tovec_half_store(len) == store && mps_tovec_half_launches(len) == launches);
    }
    CHECK(mps_tovec_half_launches(0) == 1 && mps_tovec_half_launches(6) == 1 && mps_tovec_half_launches(7) == 2 && mps_tovec_half_launches(15) == 10);
    CHECK(mps_tovec_launches(16, 8, false) == 4 && mps_tovec_launches(3, 1, false) == 2 && mps_tovec_launches(30, 15, false) == 11);
    CHECK(mps_tovec_launches(40, 6, true) == 3 && mps_tovec_launches(32, 10, true) == 7);
}

static void routes() {
    std::vector<int> d = {1, 2, 4, 64, 4, 2, 1};
    CHECK(mps_tovec_route(6, d.data()) == kMpsToVecFused);
    d[3] = 65;
    CHECK(mps_tovec_route(6, d.data()) == kMpsToVecGemm);
    d[3] = 64; d[6] = 65;   // (the last entry counts as every other)
    CHECK(mps_tovec_route(6, d.data()) == kMpsToVecGemm);
    const int one[2] = {1, 1};
    CHECK(mps_tovec_route(1, one) == kMpsToVecFused);
    CHECK(mps_tovec_method_ok(0) && mps_tovec_method_ok(1) && mps_tovec_method_ok(2) && !mps_tovec_method_ok(3) && !mps_tovec_method_ok(-1));
}

static void chunks() {
    for (int n = 1; n <= 12; ++n) {
        const int k = mps_tovec_split(n);
        const size_t per = mps_tovec_lane_bytes(k, mps_tovec_high_rows(n, k));
        CHECK(mps_tovec_chunk(per, 5, per - 1) == 0 && mps_tovec_chunks(5, 0) == 0);    // not even one lane
        for (size_t lanes = 1; lanes <= 9; ++lanes)
            for (size_t fit = 1; fit <= 10; ++fit) {
                const int chunk = mps_tovec_chunk(per, lanes, fit * per + per / 2);
                CHECK(chunk == (int)(fit < lanes ? fit : lanes));
                const size_t count = mps_tovec_chunks(lanes, chunk);
                std::vector<int> seen(lanes, 0);
                for (size_t c = 0; c < count; ++c) {
                    const size_t first = c * (size_t)chunk, last = first + (size_t)chunk < lanes ? first + (size_t)chunk : lanes;
                    CHECK(first < last);                                                  // no empty chunk
                    for (size_t l = first; l < last; ++l) ++seen[l];
                }
                for (size_t l = 0; l < lanes; ++l) CHECK(seen[l] == 1);                   // every lane in exactly one chunk
            }
    }
    CHECK(mps_tovec_chunk(16, 100000, (size_t)1 << 40) == kMpsToVecMaxChunkLanes);
    CHECK(mps_tovec_chunk(mps_tovec_lane_bytes(4, 16), 5, 2 * mps_tovec_lane_bytes(4, 16)) == 2 && mps_tovec_chunks(5, 2) == 3);
}

static void blocks() {
    CHECK(mps_tovec_check_blocks(1, 1, 1) != nullptr && mps_tovec_check_blocks(2, 1, 1) == nullptr);
    CHECK(mps_tovec_check_blocks(13, 0, 1) != nullptr && mps_tovec_check_blocks(13, 13, 1) != nullptr && mps_tovec_check_blocks(13, 12, 1) == nullptr);
    CHECK(mps_tovec_check_blocks(40, 24, 1) == nullptr && mps_tovec_check_blocks(40, 25, 1) != nullptr);
    CHECK(mps_tovec_check_blocks(40, 6, 0) != nullptr && mps_tovec_check_blocks(40, 6, 64ll * 65535) == nullptr && mps_tovec_check_blocks(40, 6, 64ll * 65535 + 1) != nullptr);
    const unsigned char bits[6] = {0, 1, 1, 0, 2, 1};
    CHECK(mps_tovec_bad_bit(bits, 4) == -1 && mps_tovec_bad_bit(bits, 6) == 4 && mps_tovec_bad_bit(bits, 0) == -1);
    // the lane bytes of a block call: rows x 2^k amplitudes, the low stores, the rows' store
    CHECK(mps_tovec_lane_bytes(6, 70) == 16 * ((size_t)70 * 64 + 128 * 64 + 128 * 70));
}

// the statement: out[r 2^k + l] = sum_j H[r][j] L[l][j] with the halves grown as the rule says, against the one-sided product
static void statement() {
    const int n = 5, dims[6] = {1, 2, 3, 4, 2, 1};
    std::vector<std::vector<cd>> t(n);
    for (int q = 0; q < n; ++q) {
        t[q].resize((size_t)2 * dims[q] * dims[q + 1]);
        for (cd& x : t[q]) x = cd(uniform(), uniform());
    }
    auto T = [&](int q, int b, int x, int u) { return t[q][((size_t)b * dims[q] + x) * dims[q + 1] + u]; };
    std::vector<cd> want((size_t)1 << n);
    for (size_t idx = 0; idx < want.size(); ++idx) {
        std::vector<cd> v(1, cd(1.0, 0.0));
        for (int q = 0; q < n; ++q) {
            std::vector<cd> w(dims[q + 1], cd(0.0, 0.0));
            for (int x = 0; x < dims[q]; ++x)
                for (int u = 0; u < dims[q + 1]; ++u) w[u] += v[x] * T(q, (int)(idx >> q) & 1, x, u);
            v.swap(w);
        }
        want[idx] = v[0];
    }
    double norm = 0.0;
    for (const cd& x : want) norm += std::norm(x);
    for (int k = 0; k <= n; ++k) {   // every split, the rule's own (n / 2) among them
        std::vector<cd> L(1, cd(1.0, 0.0)), H(1, cd(1.0, 0.0));
        for (int j = 0; j < k; ++j) {           // L_{j+1}[b 2^j + l] = L_j[l] T_j[b]
            const size_t rows = (size_t)1 << j;
            std::vector<cd> next(2 * rows * dims[j + 1], cd(0.0, 0.0));
            for (int b = 0; b < 2; ++b)
                for (size_t l = 0; l < rows; ++l)
                    for (int x = 0; x < dims[j]; ++x)
                        for (int u = 0; u < dims[j + 1]; ++u) next[(b * rows + l) * dims[j + 1] + u] += L[l * dims[j] + x] * T(j, b, x, u);
            L.swap(next);
        }
        for (int j = 0; j < n - k; ++j) {       // H_{j+1}[2 r + b] = H_j[r] T_q[b]^T, q = n - 1 - j
            const int q = n - 1 - j;
            const size_t rows = (size_t)1 << j;
            std::vector<cd> next(2 * rows * dims[q], cd(0.0, 0.0));
            for (int b = 0; b < 2; ++b)
                for (size_t r = 0; r < rows; ++r)
                    for (int x = 0; x < dims[q]; ++x)
                        for (int u = 0; u < dims[q + 1]; ++u) next[(2 * r + b) * dims[q] + x] += H[r * dims[q + 1] + u] * T(q, b, x, u);
            H.swap(next);
        }
        double worst = 0.0;
        for (size_t r = 0; r < mps_tovec_high_rows(n, k); ++r)
            for (size_t l = 0; l < mps_tovec_low_rows(k); ++l) {
                cd s(0.0, 0.0);
                for (int j = 0; j < dims[k]; ++j) s += H[r * dims[k] + j] * L[l * dims[k] + j];
                worst = std::max(worst, std::abs(s - want[(r << k) + l]));
            }
        CHECK(worst <= 1e-14 * std::sqrt(norm));
    }
}

int main() {
    sizes();
    halves();
    routes();
    chunks();
    blocks();
    statement();
    std::printf("mps_tovec_rule_selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
