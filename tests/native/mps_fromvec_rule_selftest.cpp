// Self-test of csrc/aqc_mps_fromvec_rule.h under a plain C++ compiler (run under ASan + UBSan by tests/test_mps_fromvec_rule.py): the
// route table, the partial factors, the chunk rule, the R of the block recursion against the Gram matrix, and one full conversion at
// n = 5 against a brute-force SVD (one-sided Jacobi) of every cut of the dense vector.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_fromvec_rule.h"

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

// brute force: one-sided Jacobi on the columns of a (rows x cols, rows >= cols or not), u [rows][count], s [count] descending
static void jacobi_svd(int rows, int cols, const cd* a, cd* u, double* s) {
    std::vector<cd> w(a, a + (size_t)rows * cols);
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < cols; ++p)
            for (int q = p + 1; q < cols; ++q) {
                double app = 0.0, aqq = 0.0;
                cd apq = 0.0;
                for (int i = 0; i < rows; ++i) {
                    app += std::norm(w[(size_t)i * cols + p]);
                    aqq += std::norm(w[(size_t)i * cols + q]);
                    apq += std::conj(w[(size_t)i * cols + p]) * w[(size_t)i * cols + q];
                }
                const double g = std::abs(apq);
                if (g == 0.0 || g <= 1e-17 * std::sqrt(app * aqq)) continue;
                off = std::max(off, g / std::sqrt(app * aqq));
                const cd phase = apq / g;
                const double zeta = (aqq - app) / (2.0 * g), t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < rows; ++i) {
                    const cd x = w[(size_t)i * cols + p], y = w[(size_t)i * cols + q];
                    w[(size_t)i * cols + p] = cs * x - sn * std::conj(phase) * y;
                    w[(size_t)i * cols + q] = sn * phase * x + cs * y;
                }
            }
        if (off <= 1e-15) break;
    }
    const int count = std::min(rows, cols);
    std::vector<double> norms(cols);
    std::vector<int> order(cols);
    for (int j = 0; j < cols; ++j) {
        double nn = 0.0;
        for (int i = 0; i < rows; ++i) nn += std::norm(w[(size_t)i * cols + j]);
        norms[j] = std::sqrt(nn);
        order[j] = j;
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return norms[x] > norms[y]; });
    for (int j = 0; j < count; ++j) {
        s[j] = norms[order[j]];
        for (int i = 0; i < rows; ++i) u[(size_t)i * count + j] = s[j] > 0.0 ? w[(size_t)i * cols + order[j]] / s[j] : cd(0.0, 0.0);
    }
}

static std::vector<cd> dense_of(int n, const MpsFromVec& m) {   // index bit q is site q
    std::vector<cd> acc(1, cd(1.0, 0.0));   // [index so far][bond]
    int chi = 1;
    for (int q = 0; q < n; ++q) {
        const int cl = m.bonds[q], cr = m.bonds[q + 1];
        const size_t have = acc.size() / chi;
        std::vector<cd> next(2 * have * cr, cd(0.0, 0.0));
        for (int s = 0; s < 2; ++s)
            for (size_t i = 0; i < have; ++i)
                for (int l = 0; l < cl; ++l)
                    for (int j = 0; j < cr; ++j) next[(s * have + i) * cr + j] += acc[i * cl + l] * m.site[q][((size_t)s * cl + l) * cr + j];
        acc.swap(next);
        chi = cr;
    }
    return acc;
}

int main() {
    {   // the route table
        CHECK(mps_fromvec_route(11, 0) == kMpsFromVecFused && mps_fromvec_route(12, 0) == kMpsFromVecHost);
        CHECK(mps_fromvec_route(12, 32) == kMpsFromVecFused && mps_fromvec_route(12, 33) == kMpsFromVecHost);
        CHECK(mps_fromvec_route(30, 32) == kMpsFromVecFused && mps_fromvec_route(30, 1) == kMpsFromVecFused && mps_fromvec_route(31, 32) == kMpsFromVecHost);
        CHECK(mps_fromvec_route(2, 0) == kMpsFromVecFused && mps_fromvec_route(1, 0) == kMpsFromVecHost && mps_fromvec_route(10, 64) == kMpsFromVecFused);
        CHECK(mps_fromvec_route(30, 0) == kMpsFromVecHost && mps_fromvec_route(13, 0) == kMpsFromVecHost);
        CHECK(mps_fromvec_method_ok(0) && mps_fromvec_method_ok(1) && mps_fromvec_method_ok(2) && !mps_fromvec_method_ok(3) && !mps_fromvec_method_ok(-1));
        const std::vector<int> b = mps_fromvec_bounds(12, 5);
        const int want[13] = {1, 2, 4, 5, 5, 5, 5, 5, 5, 5, 4, 2, 1};
        CHECK(b.size() == 13 && std::equal(b.begin(), b.end(), want));
        CHECK(mps_fromvec_bound(30, 15, 0) == 32768 && mps_fromvec_bound(64, 32, 0) == (1 << 30));
    }
    {   // parts: a function of the rows alone; no part is empty; the tree ends at one factor
        const size_t rows[] = {1, 64, 256, 257, 512, 1024, (size_t)1 << 16, (size_t)1 << 17, (size_t)1 << 29};
        const int want[] = {1, 1, 1, 2, 2, 4, 256, 256, 256};
        for (int i = 0; i < 9; ++i) CHECK(mps_fromvec_parts(rows[i]) == want[i]);
        CHECK(mps_fromvec_blocks_per_part((size_t)1 << 17) == 8 && mps_fromvec_blocks_per_part(512) == 4 && mps_fromvec_blocks_per_part(1) == 1);
        for (size_t r : {(size_t)1, (size_t)63, (size_t)65, (size_t)1000, ((size_t)1 << 16) + 1, (size_t)3 * 16384 + 5}) {
            const size_t blocks = mps_fromvec_blocks(r), per = mps_fromvec_blocks_per_part(r), p = (size_t)mps_fromvec_parts(r);
            CHECK((p - 1) * per < blocks && blocks <= p * per && p <= kMpsFromVecMaxParts);
        }
        int p = 256, levels = 0;
        while (p > 1) { p = mps_fromvec_fold(p); ++levels; }
        CHECK(levels == 4 && mps_fromvec_fold(5) == 2 && mps_fromvec_fold(1) == 1);
    }
    {   // chunks
        CHECK(mps_fromvec_lane_bytes(10) == 32768);
        CHECK(mps_fromvec_chunk(10, 5, 2 * 32768) == 2 && mps_fromvec_chunk(10, 5, kMpsFromVecBudget) == 5 && mps_fromvec_chunk(10, 5, 32767) == 0);
        CHECK(mps_fromvec_chunk(28, 3, kMpsFromVecBudget) == 1 && mps_fromvec_chunk(29, 3, kMpsFromVecBudget) == 0 && mps_fromvec_chunk(2, 100000, kMpsFromVecBudget) == 65535);
    }
    {   // R of the block recursion: R^H R = A^H A, upper triangular, for tall, ragged, several-part and wide matrices
        const int shapes[][2] = {{1, 2}, {2, 2}, {65, 6}, {300, 64}, {1100, 10}, {2, 8}, {40, 64}};
        for (const auto& sh : shapes) {
            const int rows = sh[0], cols = sh[1];
            std::vector<cd> a((size_t)rows * cols);
            for (cd& x : a) x = cd(uniform(), uniform());
            if (rows > 2)
                for (int i = 0; i < rows; ++i) a[(size_t)i * cols + cols / 2] = a[(size_t)i * cols];   // exactly rank-deficient
            const std::vector<cd> r = mps_fromvec_r(rows, cols, a.data());
            double worst = 0.0, scale = 0.0, below = 0.0;
            for (int i = 0; i < cols; ++i)
                for (int j = 0; j < cols; ++j) {
                    cd g = 0.0, h = 0.0;
                    for (int k = 0; k < rows; ++k) g += std::conj(a[(size_t)k * cols + i]) * a[(size_t)k * cols + j];
                    for (int k = 0; k < cols; ++k) h += std::conj(r[(size_t)k * cols + i]) * r[(size_t)k * cols + j];
                    worst = std::max(worst, std::abs(g - h));
                    scale = std::max(scale, std::abs(g));
                    if (i > j || i >= rows) below = std::max(below, std::abs(r[(size_t)i * cols + j]));
                }
            std::printf("R of %d x %d (%d parts): max |R^H R - A^H A| = %.3g of %.3g\n", rows, cols, mps_fromvec_parts(rows), worst, scale);
            CHECK(worst <= 1e-12 * scale && below == 0.0);
        }
    }
    {   // one full conversion at n = 5 against brute-force SVDs of the cuts of the dense vector: exact, capped, and a basis state
        const int n = 5;
        std::vector<cd> psi(32);
        double norm2 = 0.0;
        for (cd& x : psi) { x = cd(uniform(), uniform()); norm2 += std::norm(x); }
        const double norm = std::sqrt(norm2);
        const MpsFromVec m = mps_fromvec_convert(n, psi.data(), 0.0, 0, jacobi_svd);
        const int natural[6] = {1, 2, 4, 4, 2, 1};
        CHECK(m.status == kMpsCompressOk && m.failed_at == -1 && std::equal(m.bonds.begin(), m.bonds.end(), natural));
        const std::vector<cd> back = dense_of(n, m);
        double err = 0.0;
        for (int i = 0; i < 32; ++i) err += std::norm(back[i] - psi[i]);
        std::printf("n = 5: |dense(converted) - psi| = %.3g (|psi| = %.3g), discarded %.3g\n", std::sqrt(err), norm, m.discarded);
        CHECK(std::sqrt(err) <= 1e-12 * norm && std::fabs(m.discarded) <= 1e-12 * norm2);
        for (int q = 1; q < n; ++q) {   // bond q: the singular values of psi as [2^(n-q)][2^q]
            const int rows = 1 << (n - q), cols = 1 << q, count = std::min(rows, cols);
            std::vector<cd> u((size_t)rows * count);
            std::vector<double> s(count);
            jacobi_svd(rows, cols, psi.data(), u.data(), s.data());
            CHECK((int)m.lam[q - 1].size() == count);
            for (int j = 0; j < count && j < (int)m.lam[q - 1].size(); ++j) CHECK(std::fabs(m.lam[q - 1][j] - s[j]) <= 1e-12 * norm);
        }
        const MpsFromVec capped = mps_fromvec_convert(n, psi.data(), 0.0, 2, jacobi_svd);
        const int two[6] = {1, 2, 2, 2, 2, 1};
        CHECK(capped.status == kMpsCompressOk && std::equal(capped.bonds.begin(), capped.bonds.end(), two) && capped.discarded > 0.0);
        const std::vector<cd> cut = dense_of(n, capped);
        double kept = 0.0;
        for (int i = 0; i < 32; ++i) kept += std::norm(cut[i]);
        CHECK(std::fabs(std::sqrt(kept) - norm) <= 1e-12 * norm);   // the rescaling keeps the norm
        std::vector<cd> e(32, cd(0.0, 0.0));
        e[22] = cd(0.0, 2.0);
        const MpsFromVec b = mps_fromvec_convert(n, e.data(), 0.0, 0, jacobi_svd);
        const int ones[6] = {1, 1, 1, 1, 1, 1};
        CHECK(b.status == kMpsCompressOk && std::equal(b.bonds.begin(), b.bonds.end(), ones));
        const std::vector<cd> eb = dense_of(n, b);
        for (int i = 0; i < 32; ++i) CHECK(std::abs(eb[i] - e[i]) <= 1e-15);
        const std::vector<cd> zero(32, cd(0.0, 0.0));
        const MpsFromVec z = mps_fromvec_convert(n, zero.data(), 0.0, 0, jacobi_svd);
        CHECK(z.status == kMpsCompressNonFinite && z.failed_at == 0 && z.bonds[1] == 0);
    }
    std::printf("mps_fromvec_rule selftest: %d failures\n", failures);
    return failures ? 1 : 0;
}
