// Stand-alone check of csrc/aqc_obs_rule.h for tests/test_obs_host.py (g++ -std=c++17 under ASan + UBSan; no HIP).  Exit status 0 and
// "ok" on stdout when every check holds; the first failing check is named on stderr.
//   plan      every set inside its recorded subset, every subset inside its pass, |B| = min(n, T), the low c bits when n > T, one pass
//             for pairs when n <= T, at most kObsMaxSubsets subsets a pass, the caps on the number of passes
//   deposit   obs_deposit / obs_global_index at n = 30 (bit 29, indices above 2^31 of the doubles), a bijection per pass
//   slots     obs_lds_slot is a bijection of the tile and XOR-linear (the kernel adds the slots of disjoint index parts); for every
//             subset the 32 lanes of a half wave meet on a bank at most in pairs
//   trace     the whole route on the host -- tiles by obs_global_index, the 16 x 128 operand of a subset, A A^H, obs_partial_trace --
//             against a brute-force rho of random 6- and 13-qubit states, for pairs in both orders and sets of 1, 3 and 4 qubits
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_obs_rule.h"

using namespace aqc;
typedef std::complex<double> cd;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static int popc(uint32_t v) { return __builtin_popcount(v); }

static void check_plan(int n, const std::vector<uint32_t>& req, const ObsPlan& plan) {
    const int T = n < kObsTileBits ? n : kObsTileBits;
    CHECK(plan.serve_pass.size() == req.size() && plan.serve_subset.size() == req.size());
    CHECK(!plan.passes.empty());
    bool pairs = true;   // lists of pairs fit one pass of a tile; larger sets may fill several, all with the same bits
    for (uint32_t m : req) pairs = pairs && popc(m) == 2;
    if (n <= kObsTileBits && pairs) CHECK(plan.passes.size() == 1);
    for (const ObsPass& p : plan.passes) {
        CHECK(p.nbits == T && popc(p.bits) == T && !(p.bits >> n));
        if (n > kObsTileBits) CHECK((p.bits & 31u) == 31u);
        CHECK(!p.subsets.empty() && (int)p.subsets.size() <= kObsMaxSubsets);
        for (uint16_t S : p.subsets) CHECK(popc(S) == 4 && !(S >> (T < 4 ? 4 : T)));
    }
    for (size_t r = 0; r < req.size(); ++r) {
        CHECK(plan.serve_pass[r] >= 0 && plan.serve_pass[r] < (int)plan.passes.size());
        const ObsPass& p = plan.passes[(size_t)plan.serve_pass[r]];
        CHECK(plan.serve_subset[r] >= 0 && plan.serve_subset[r] < (int)p.subsets.size());
        CHECK(!(req[r] & ~p.bits));
        const uint32_t S = p.subsets[(size_t)plan.serve_subset[r]];
        for (int q = 0; q < n; ++q)
            if ((req[r] >> q) & 1u) CHECK((S >> popc(p.bits & ((1u << q) - 1))) & 1u);
        // the first in plan order
        for (int pi = 0; pi <= plan.serve_pass[r]; ++pi) {
            const ObsPass& e = plan.passes[(size_t)pi];
            if (req[r] & ~e.bits) continue;
            uint32_t loc = 0;
            for (int q = 0; q < n; ++q)
                if ((req[r] >> q) & 1u) loc |= 1u << popc(e.bits & ((1u << q) - 1));
            const int upto = pi == plan.serve_pass[r] ? plan.serve_subset[r] : (int)e.subsets.size();
            for (int si = 0; si < upto; ++si) CHECK(loc & ~(uint32_t)e.subsets[(size_t)si]);
        }
    }
}

// rho of the listed qubits by the convention of the header, brute force
static std::vector<cd> brute(const std::vector<cd>& psi, int n, const std::vector<int>& qs) {
    const int k = (int)qs.size(), dim = 1 << k;
    std::vector<cd> rho((size_t)dim * dim, cd(0, 0));
    uint64_t keep = 0;
    for (int q : qs) keep |= (uint64_t)1 << q;
    const uint64_t N = (uint64_t)1 << n;
    for (uint64_t rest = 0; rest < N; ++rest) {
        if (rest & keep) continue;
        for (int a = 0; a < dim; ++a)
            for (int b = 0; b < dim; ++b) {
                uint64_t ia = rest, ib = rest;
                for (int m = 0; m < k; ++m) {
                    if ((a >> m) & 1) ia |= (uint64_t)1 << qs[(size_t)m];
                    if ((b >> m) & 1) ib |= (uint64_t)1 << qs[(size_t)m];
                }
                rho[(size_t)a * dim + b] += psi[ia] * std::conj(psi[ib]);
            }
    }
    return rho;
}

// the 16 x 16 matrices of every (pass, subset) by the route of the kernel, on the host
static std::vector<std::vector<std::vector<cd>>> route(const std::vector<cd>& psi, int n, const ObsPlan& plan) {
    std::vector<std::vector<std::vector<cd>>> all;
    const int T = n < kObsTileBits ? n : kObsTileBits, tile = 1 << kObsTileBits;
    for (const ObsPass& p : plan.passes) {
        std::vector<std::vector<cd>> rhos(p.subsets.size(), std::vector<cd>(256, cd(0, 0)));
        for (uint64_t g = 0; g < ((uint64_t)1 << (n - T)); ++g) {
            std::vector<cd> lds((size_t)tile, cd(0, 0));
            for (unsigned l = 0; l < (unsigned)tile; ++l) {
                const unsigned slot = obs_lds_slot(l);
                CHECK(slot < (unsigned)tile);
                if (l < (1u << T)) {
                    const uint64_t at = obs_global_index(l, g, p.bits, n);
                    CHECK(at < psi.size());
                    lds[slot] = psi[at];
                }
            }
            for (size_t s = 0; s < p.subsets.size(); ++s) {
                const unsigned S = p.subsets[s], cm = (unsigned)(tile - 1) & ~S;
                for (int col = 0; col < tile / 16; ++col)
                    for (int a = 0; a < 16; ++a)
                        for (int b = 0; b < 16; ++b) {
                            const unsigned la = (unsigned)obs_deposit((uint64_t)a, S) | (unsigned)obs_deposit((uint64_t)col, cm);
                            const unsigned lb = (unsigned)obs_deposit((uint64_t)b, S) | (unsigned)obs_deposit((uint64_t)col, cm);
                            rhos[s][(size_t)a * 16 + b] += lds[obs_lds_slot(la)] * std::conj(lds[obs_lds_slot(lb)]);
                        }
            }
        }
        all.push_back(rhos);
    }
    return all;
}

static void check_route(int n, int k, const std::vector<std::vector<int>>& sets, unsigned seed) {
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> gauss;
    std::vector<cd> psi((size_t)1 << n);
    double norm = 0;
    for (cd& v : psi) { v = cd(gauss(rng), gauss(rng)); norm += std::norm(v); }
    for (cd& v : psi) v /= std::sqrt(norm);
    std::vector<uint32_t> req;
    for (const std::vector<int>& qs : sets) {
        uint32_t m = 0;
        for (int q : qs) m |= 1u << q;
        if (k == 1) m |= (m & 1u) ? 2u : 1u;
        req.push_back(m);
    }
    const ObsPlan plan = obs_plan(n, req);
    check_plan(n, req, plan);
    const auto rhos = route(psi, n, plan);
    for (size_t r = 0; r < sets.size(); ++r) {
        const ObsPass& p = plan.passes[(size_t)plan.serve_pass[r]];
        const uint32_t S = p.subsets[(size_t)plan.serve_subset[r]];
        int pos[4];
        for (int m = 0; m < k; ++m) pos[m] = popc(S & ((1u << popc(p.bits & ((1u << sets[r][(size_t)m]) - 1))) - 1));
        const std::vector<cd>& rho16 = rhos[(size_t)plan.serve_pass[r]][(size_t)plan.serve_subset[r]];
        std::vector<double> out((size_t)2 << (2 * k));
        obs_partial_trace(reinterpret_cast<const double*>(rho16.data()), k, pos, out.data());
        const std::vector<cd> ref = brute(psi, n, sets[r]);
        for (size_t e = 0; e < ref.size(); ++e) CHECK(std::abs(cd(out[2 * e], out[2 * e + 1]) - ref[e]) <= 1e-13);
    }
}

int main() {
    // ---- plan ----
    for (int n = kObsMinQubits; n <= kObsMaxQubits; ++n) {
        std::vector<uint32_t> all, nn;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) all.push_back((1u << i) | (1u << j));
        for (int i = 0; i + 1 < n; ++i) nn.push_back(3u << i);
        const ObsPlan pa = obs_plan(n, all), pn = obs_plan(n, nn);
        check_plan(n, all, pa);
        check_plan(n, nn, pn);
        CHECK((int)pa.passes.size() <= n && (int)pn.passes.size() <= 6);
    }
    std::mt19937 rng(11);
    for (int t = 0; t < 40; ++t) {
        const int n = 2 + (int)(rng() % 29), k = 2 + (int)(rng() % 3);
        if (k > n) continue;
        std::vector<uint32_t> req;
        for (int c = 1 + (int)(rng() % 60); c > 0; --c) {
            uint32_t m = 0;
            while (popc(m) < k) m |= 1u << (rng() % (unsigned)n);
            req.push_back(m);
        }
        check_plan(n, req, obs_plan(n, req));
    }
    // ---- deposit ----
    CHECK(obs_deposit(0x5, 0x30) == 0x10 && obs_deposit(0x3, 0x30) == 0x30 && obs_deposit(0xFF, 0) == 0);
    {
        const int n = 30;
        const uint64_t bits = 31u | ((uint64_t)1 << 29) | ((uint64_t)1 << 17) | (0xFu << 9);   // 11 bits, bit 29 among them
        CHECK(popc((uint32_t)bits) == 11);
        const uint64_t top = obs_global_index(2047, 0, bits, n);
        CHECK(top == bits && top > ((uint64_t)1 << 29) && 2 * top + 1 > ((uint64_t)1 << 30));
        const uint64_t last = obs_global_index(2047, ((uint64_t)1 << 19) - 1, bits, n);
        CHECK(last == ((uint64_t)1 << 30) - 1 && 16 * last > ((uint64_t)1 << 31));   // the byte offset of the amplitude
        CHECK(obs_global_index(1024, 0, bits, n) == ((uint64_t)1 << 29));
        CHECK(obs_global_index(0, (uint64_t)1 << 18, bits, n) == ((uint64_t)1 << 28));
        std::mt19937_64 r64(3);
        for (int t = 0; t < 2000; ++t) {   // tile and group parts never meet, and both come back
            const uint64_t l = r64() & 2047, g = r64() & (((uint64_t)1 << 19) - 1), at = obs_global_index(l, g, bits, n);
            CHECK(at < ((uint64_t)1 << n) && (at & bits) == obs_deposit(l, bits) && (at & ~bits) == obs_deposit(g, ~bits & (((uint64_t)1 << n) - 1)));
        }
    }
    {   // a bijection at a small size: every index exactly once
        const int n = 13;
        const uint32_t bits = 31u | (1u << 12) | (0x1Fu << 6);
        std::vector<int> seen((size_t)1 << n, 0);
        for (uint64_t g = 0; g < 4; ++g)
            for (uint64_t l = 0; l < 2048; ++l) ++seen[obs_global_index(l, g, bits, n)];
        for (int v : seen) CHECK(v == 1);
    }
    // ---- slots ----
    {
        std::vector<int> seen(2048, 0);
        for (unsigned l = 0; l < 2048; ++l) {
            CHECK(obs_lds_slot(l) < 2048);
            ++seen[obs_lds_slot(l)];
            CHECK((obs_lds_slot(l & 0x0FF) ^ obs_lds_slot(l & 0x700)) == obs_lds_slot(l));
        }
        for (int v : seen) CHECK(v == 1);
        // the operand read of a half wave: rows 0 .. 15 at the positions of S and one column bit at the lowest position outside S (the
        // other half has the next column bit set, a constant XOR); a b64 read has 32 banks of 8 bytes: at most two lanes a bank, for every S
        int worst = 0;
        for (unsigned S = 0; S < 2048; ++S) {
            if (popc(S) != 4) continue;
            const unsigned cm = 2047u & ~S, lo1 = cm & (~cm + 1);
            int bank[32] = {0};
            for (unsigned lane = 0; lane < 32; ++lane) {
                const unsigned l = (unsigned)obs_deposit(lane & 15, S) | (unsigned)obs_deposit(lane >> 4, lo1);
                const int m = ++bank[obs_lds_slot(l) & 31u];
                if (m > worst) worst = m;
            }
        }
        CHECK(worst == 2);
        // the gather's writes: 32 consecutive tile-local indices fill 32 different banks
        for (unsigned base = 0; base < 2048; base += 32) {
            unsigned hit = 0;
            for (unsigned l = base; l < base + 32; ++l) hit |= 1u << (obs_lds_slot(l) & 31u);
            CHECK(hit == 0xFFFFFFFFu);
        }
    }
    // ---- the route against brute force ----
    for (int n : {2, 3, 6}) {
        std::vector<std::vector<int>> pairs, singles;
        for (int i = 0; i < n; ++i) {
            singles.push_back({i});
            for (int j = 0; j < n; ++j)
                if (i != j) pairs.push_back({i, j});
        }
        check_route(n, 2, pairs, 100u + (unsigned)n);
        check_route(n, 1, singles, 200u + (unsigned)n);
    }
    check_route(6, 3, {{0, 1, 2}, {5, 0, 3}, {4, 2, 1}}, 7);
    check_route(6, 4, {{0, 1, 2, 3}, {5, 0, 3, 1}}, 8);
    check_route(13, 2, {{0, 12}, {12, 11}, {5, 6}, {7, 3}, {11, 12}, {9, 10}}, 9);
    check_route(13, 4, {{0, 6, 11, 12}, {12, 5, 7, 9}}, 10);
    check_route(13, 3, {{12, 0, 8}}, 12);
    printf("ok\n");
    return 0;
}
