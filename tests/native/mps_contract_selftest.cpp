// Stand-alone self-test of csrc/aqc_mps_contract.h (host only): the site steps and the overlap chain, run by an executor whose products
// are plain loops with the semantics aqc_launch.h declares for launch_zgemm / launch_zgemm_bh, against the dense vectors of the two
// states.  The operands have DIFFERENT bond dimensions, so that every leading dimension of a step is distinguishable, and every
// buffer is a heap block of exactly the size the header asks for: a wrong size is an AddressSanitizer report.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_contract.h"
#include "../../aqc_research_amd/csrc/aqc_mps_walk.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const double kTol = 1e-12;   // states of norm 1: every output sums fewer than 10^3 fp64 products of numbers of magnitude <= 1

// C (M x N, ldc) (+)= op(A) . op(B): op(A) = A^H with A stored K x M when conj_t; gemm_bh: B^H with B stored N x K
struct CpuOps {
    int product(bool conj_t, bool b_h, bool accum, int M, int N, int K, const cd* A, int lda, const cd* B, int ldb, cd* C, int ldc) {
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) {
                cd s = accum ? C[(size_t)m * ldc + n] : cd(0.0, 0.0);
                for (int k = 0; k < K; ++k) {
                    const cd a = conj_t ? std::conj(A[(size_t)k * lda + m]) : A[(size_t)m * lda + k];
                    const cd b = b_h ? std::conj(B[(size_t)n * ldb + k]) : B[(size_t)k * ldb + n];
                    s += a * b;
                }
                C[(size_t)m * ldc + n] = s;
            }
        return 0;
    }
    int gemm(bool conj_t, bool accum, int M, int N, int K, const cd* A, int lda, const cd* B, int ldb, cd* C, int ldc) {
        return product(conj_t, false, accum, M, N, K, A, lda, B, ldb, C, ldc);
    }
    int gemm_bh(bool conj_t, bool accum, int M, int N, int K, const cd* A, int lda, const cd* B, int ldb, cd* C, int ldc) {
        return product(conj_t, true, accum, M, N, K, A, lda, B, ldb, C, ldc);
    }
};

struct Mps {
    int n;
    std::vector<int> dims;                 // n + 1 bond dimensions
    std::vector<std::vector<cd>> t;        // site q: [2][dims[q]][dims[q + 1]]
};

static std::mt19937_64 rng(20240611);
static cd rand_cd() {
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    const double re = u(rng), im = u(rng);
    return cd(re, im);
}

// amplitude of every basis state (index bit q = the value of site q), by nested loops over the sites
static std::vector<cd> dense(const Mps& m) {
    std::vector<cd> psi((size_t)1 << m.n);
    for (size_t idx = 0; idx < psi.size(); ++idx) {
        std::vector<cd> row(1, cd(1.0, 0.0));
        for (int q = 0; q < m.n; ++q) {
            const int bit = (int)((idx >> q) & 1), x = m.dims[q], u = m.dims[q + 1];
            std::vector<cd> next(u, cd(0.0, 0.0));
            for (int i = 0; i < x; ++i)
                for (int j = 0; j < u; ++j) next[j] += row[i] * m.t[q][((size_t)bit * x + i) * u + j];
            row = next;
        }
        psi[idx] = row[0];
    }
    return psi;
}

static Mps random_mps(const std::vector<int>& dims) {
    Mps m{(int)dims.size() - 1, dims, {}};
    for (int q = 0; q < m.n; ++q) {
        m.t.emplace_back((size_t)2 * dims[q] * dims[q + 1]);
        for (cd& v : m.t.back()) v = rand_cd();
    }
    double norm2 = 0.0;
    for (const cd& v : dense(m)) norm2 += std::norm(v);
    const double s = std::pow(norm2, -0.5 / m.n);   // the same factor on every site: the state has norm 1, no site grows
    for (auto& site : m.t)
        for (cd& v : site) v *= s;
    return m;
}

static cd vdot(const std::vector<cd>& a, const std::vector<cd>& b) {
    cd s(0.0, 0.0);
    for (size_t i = 0; i < a.size(); ++i) s += std::conj(a[i]) * b[i];
    return s;
}

// G on qubit q of a dense vector: out[.., i, ..] = sum_j G[i][j] psi[.., j, ..]
static std::vector<cd> apply_dense(const M2& g, int q, const std::vector<cd>& psi) {
    std::vector<cd> out(psi.size());
    for (size_t idx = 0; idx < psi.size(); ++idx) {
        const int i = (int)((idx >> q) & 1);
        const size_t i0 = idx & ~((size_t)1 << q), i1 = i0 | ((size_t)1 << q);
        out[idx] = g.m[2 * i] * psi[i0] + g.m[2 * i + 1] * psi[i1];
    }
    return out;
}

// a random complex 2 x 2 that is neither Hermitian nor unitary (nor real, nor symmetric: a transpose or a conjugate is not its adjoint)
static M2 random_op() {
    for (;;) {
        const M2 g = {{rand_cd(), rand_cd(), rand_cd(), rand_cd()}};
        const M2 gg = adjoint(g) * g;
        const bool hermitian = std::abs(g.m[1] - std::conj(g.m[2])) < 0.1 || std::abs(g.m[0].imag()) < 0.1;
        const bool unitary = std::abs(gg.m[0] - 1.0) < 0.1 && std::abs(gg.m[3] - 1.0) < 0.1 && std::abs(gg.m[1]) < 0.1;
        const bool symmetric = std::abs(g.m[1] - g.m[2]) < 0.1, real = std::abs(g.m[1].imag()) < 0.1 || std::abs(g.m[2].imag()) < 0.1;
        if (!hermitian && !unitary && !symmetric && !real) return g;
    }
}

// <(prod G_i on q_i) a|b> by the overlap chain: site q_i of b is read through adjoint(G_i), as the 1-qubit gate kernel applies it to a
// site ([2][ne]: out[i][c] = sum_j G^H[i][j] site[j][c])
static cd chain_overlap(const Mps& a, const Mps& b, const std::vector<int>& qs, const std::vector<M2>& gs) {
    const size_t need = overlap_scratch_elems(a.n, a.dims.data(), b.dims.data());
    std::vector<cd> e(need), en(need), t(need), bsite;
    CpuOps ops;
    auto site_a = [&](int q) { return a.t[q].data(); };
    auto site_b = [&](int q) -> const cd* {
        for (size_t i = 0; i < qs.size(); ++i)
            if (qs[i] == q) {
                double g8[8];
                pack(adjoint(gs[i]), g8);
                const size_t ne = (size_t)b.dims[q] * b.dims[q + 1];
                bsite.assign(2 * ne, cd(0.0, 0.0));
                for (int r = 0; r < 2; ++r)
                    for (int j = 0; j < 2; ++j)
                        for (size_t c = 0; c < ne; ++c) bsite[r * ne + c] += cd(g8[2 * (2 * r + j)], g8[2 * (2 * r + j) + 1]) * b.t[q][j * ne + c];
                return bsite.data();
            }
        return b.t[q].data();
    };
    const cd* res = overlap_chain(ops, a.n, a.dims.data(), b.dims.data(), site_a, site_b, e.data(), en.data(), t.data());
    CHECK(res == e.data() || res == en.data());
    return res ? *res : cd(NAN, NAN);
}

// <a|b> at the cut behind site c: the left environment through site c against the conjugated right environment of the sites > c, closed
// by the rule of launch_mps_env_dot: sum_i E[i] conj(Rc[i])
static void check_cuts(const Mps& a, const Mps& b, cd want) {
    const int n = a.n;
    CpuOps ops;
    std::vector<std::vector<cd>> L(n + 1), R(n);
    L[0].assign(1, cd(1.0, 0.0));
    R[n - 1].assign(1, cd(1.0, 0.0));
    for (int p = 0; p < n; ++p) {
        const SiteDims d = site_dims(a.dims.data(), b.dims.data(), p);
        std::vector<cd> tmp((size_t)d.xa * d.vb);
        L[p + 1].resize((size_t)d.ua * d.vb);
        CHECK(contract_left(ops, (const cd*)L[p].data(), a.t[p].data(), b.t[p].data(), d, tmp.data(), L[p + 1].data()) == 0);
    }
    for (int p = n - 1; p >= 1; --p) {
        const SiteDims d = site_dims(a.dims.data(), b.dims.data(), p);
        std::vector<cd> tmp((size_t)d.ua * d.yb);
        R[p - 1].resize((size_t)d.xa * d.yb);
        CHECK(contract_right(ops, (const cd*)R[p].data(), a.t[p].data(), b.t[p].data(), d, tmp.data(), R[p - 1].data()) == 0);
    }
    for (int c = 0; c < n; ++c) {
        CHECK(L[c + 1].size() == R[c].size());
        cd s(0.0, 0.0);
        for (size_t i = 0; i < R[c].size(); ++i) s += L[c + 1][i] * std::conj(R[c][i]);
        CHECK(std::abs(s - want) < kTol);
    }
}

static void check_pair(const std::vector<int>& dims_a, const std::vector<int>& dims_b) {
    const Mps a = random_mps(dims_a), b = random_mps(dims_b);
    const int n = a.n;
    const std::vector<cd> va = dense(a), vb = dense(b);
    CHECK(std::abs(vdot(va, va) - 1.0) < kTol && std::abs(vdot(vb, vb) - 1.0) < kTol);
    const cd want = vdot(va, vb);
    CHECK(std::abs(want) > 1e-6);                                     // (a comparison of two zeros would show nothing)
    CHECK(std::abs(chain_overlap(a, b, {}, {}) - want) < kTol);      // (a) <a|b>
    for (int q : {0, n / 2, n - 1}) {                                // (b) <G a|b>, G on the first, a middle and the last site
        const M2 g = random_op();
        CHECK(std::abs(chain_overlap(a, b, {q}, {g}) - vdot(apply_dense(g, q, va), vb)) < kTol);
    }
    for (int q1 = 0; q1 < n; ++q1)                                    // ... and two operators, every pair of sites
        for (int q2 = q1 + 1; q2 < n; ++q2) {
            const M2 g1 = random_op(), g2 = random_op();
            CHECK(std::abs(chain_overlap(a, b, {q1, q2}, {g1, g2}) - vdot(apply_dense(g2, q2, apply_dense(g1, q1, va)), vb)) < kTol);
        }
    check_cuts(a, b, want);                                           // (c) environments from both ends, every cut
}

int main() {
    check_pair({1, 2, 1}, {1, 1, 1});
    check_pair({1, 2, 2, 1}, {1, 1, 2, 1});
    check_pair({1, 2, 3, 4, 2, 1}, {1, 2, 4, 3, 2, 1});
    check_pair({1, 2, 4, 2, 1}, {1, 2, 1, 2, 1});   // the step's T (xa * vb = 8) is larger than every environment (4): it sets the scratch size
    if (fails) return 1;
    std::puts("ok");
    return 0;
}
