// Dense state-vector executor of the MPS side's gate walk (aqc_mps_walk.h, aqc_mps_gradwalk.h; built with -fsanitize=address,undefined
// by tests/test_native_sanitizers.py): the third executor next to the single-lane engine and the lockstep lanes.  It evaluates circuit_ops
// with 2 x 2 and 4 x 4 matrices on a std::vector<std::complex<double>> (qubit q = bit q, n <= 6) and runs the SAME gradient_walk / env_dot
// as the two engines.  The value of an inner product is computed densely; an "environment" L[p] / Rc[p] holds only the version stamps
// of the sites it contracted when it was built, every gate bumps the version of the sites it touches, and every use of an environment
// asserts that its stamps are current: a missing or too narrow `touched`, which the engines would answer with a plausible wrong
// gradient, ends the program with "stale environment".  Each gradient is walked twice, with the recorded rotations taken step by step
// (the single-lane engine's calling pattern) and fused (the lanes': advance once, read L[q] and Rc[q], up to three parameters).
// argv[1]: the name of the case (for messages)
// stdin:  n entangler num_blocks trotter second_order, blocks[2][num_blocks], T thetas, x (2^n x re im), y, lo_blk hi_blk
// stdout: V x, V^H y, the full gradient of <V x|y>, the gradient of the blocks [lo_blk, hi_blk) with front_layer off: one "re im" a line
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_gradwalk.h"

typedef std::vector<cd> Vec;
static const char* g_case = "?";

static void apply1(Vec& v, int q, const M2& g) {
    const size_t h = (size_t)1 << q;
    for (size_t i = 0; i < v.size(); ++i)
        if (!(i & h)) {
            const cd a0 = v[i], a1 = v[i | h];
            v[i] = g.m[0] * a0 + g.m[1] * a1;
            v[i | h] = g.m[2] * a0 + g.m[3] * a1;
        }
}
// 4 x 4 on the sites (q, q + 1), index 2 * bit_q + bit_{q+1}
static void apply2(Vec& v, int q, const double* g32) {
    const size_t ha = (size_t)1 << q, hb = (size_t)1 << (q + 1);
    for (size_t i = 0; i < v.size(); ++i)
        if (!(i & ha) && !(i & hb)) {
            const size_t at[4] = {i, i | hb, i | ha, i | ha | hb};
            cd in[4], out[4];
            for (int k = 0; k < 4; ++k) in[k] = v[at[k]];
            for (int r = 0; r < 4; ++r) {
                out[r] = 0.0;
                for (int k = 0; k < 4; ++k) out[r] += cd(g32[2 * (4 * r + k)], g32[2 * (4 * r + k) + 1]) * in[k];
            }
            for (int k = 0; k < 4; ++k) v[at[k]] = out[k];
        }
}
static void run_circuit(Vec& v, const aqc_circuit& c, const double* th, bool inverse) {
    for (const CircuitOp& op : circuit_ops(&c, c.num_qubits, inverse)) {
        if (!op.two) { apply1(v, op.op1.q, gate1_matrix(op.op1.g, th)); continue; }
        double g32[32];
        gate2_matrix(op.op2.g, th, g32);
        apply2(v, op.op2.q, g32);
    }
}

// the executor of aqc_mps_gradwalk.h on dense vectors
struct DenseExec {
    // what an environment was built from: stamp[s] = the version of site s when it was contracted, -1 = not contained
    struct Env {
        std::vector<int> stamp;
        bool built = false;
    };
    int n;
    const double* th;
    bool fused;                 // recorded rotations the lanes' way
    Vec w, z;
    std::vector<int> version;   // per site: the gates it has taken
    std::vector<Env> L, R;      // L[p] holds the sites < p, R[p] the sites > p
    Env e[2];
    std::vector<std::pair<int, const M2*>> ops;   // the operators of the chain under way
    std::vector<cd> vals;

    DenseExec(int n_, const double* th_, bool fused_, const Vec& w_, const Vec& z_, int nvals)
        : n(n_), th(th_), fused(fused_), w(w_), z(z_), version(n_, 0), L(n_ + 1), R(n_), vals(nvals) {
        L[0].stamp.assign(n, -1); L[0].built = true;
        R[n - 1].stamp.assign(n, -1); R[n - 1].built = true;
    }
    // a use of `env`, which must hold exactly the sites [from, to) at their current versions
    void use(const Env& env, const char* name, int p, int from, int to, const char* where) const {
        const char* mode = fused ? "fused" : "step-by-step";
        if (!env.built) {
            fprintf(stderr, "%s: stale environment: %s[%d] read by %s was never built (%s rotations)\n", g_case, name, p, where, mode);
            exit(3);
        }
        for (int s = 0; s < n; ++s) {
            const bool in = from <= s && s < to;
            if (in ? env.stamp[s] == version[s] : env.stamp[s] == -1) continue;
            fprintf(stderr, "%s: stale environment: %s[%d] read by %s holds site %d at version %d, the site is at version %d (%s rotations)\n", g_case, name, p,
                    where, s, env.stamp[s], version[s], mode);
            exit(3);
        }
    }
    static void extend(const Env& in, int p, int ver, Env& out) {
        Env next = in;   // (out may be in)
        next.stamp[p] = ver;
        out = next;
    }
    cd dense_dot() const {   // <(ops) w|z>
        Vec v = w;
        for (const auto& o : ops) apply1(v, o.first, *o.second);
        cd s = 0.0;
        for (size_t i = 0; i < v.size(); ++i) s += std::conj(v[i]) * z[i];
        return s;
    }

    int left(int p) { use(L[p], "L", p, 0, p, "left"); extend(L[p], p, version[p], L[p + 1]); return 0; }
    int right(int p) { use(R[p], "R", p, p + 1, n, "right"); extend(R[p], p, version[p], R[p - 1]); return 0; }
    int chain(int p, bool first, int k, const M2* op) {
        if (first) { use(L[p], "L", p, 0, p, "the start of a chain"); ops.clear(); }
        extend(first ? L[p] : e[k ^ 1], p, version[p], e[k]);
        if (op) ops.emplace_back(p, op);
        return 0;
    }
    int close(int hi, int k, int slot) {
        use(e[k], "chain", hi, 0, hi + 1, "the close");
        use(R[hi], "R", hi, hi + 1, n, "the close");
        vals.at(slot) = dense_dot();
        return 0;
    }
    int entangle(const GradStep& s) {   // z takes it before w
        for (const RouteStep& r : route_pair(s.q, s.q2)) {
            double g32[32];
            gate2_matrix(routed_gate(r, s.ent), th, g32);
            apply2(z, r.q, g32);
            apply2(w, r.q, g32);
            ++version[r.q]; ++version[r.q + 1];
        }
        return 0;
    }
    int rotate(int q, const LaneGate1& g1) {
        const M2 g = gate1_matrix(g1, th);
        apply1(w, q, g);
        apply1(z, q, g);
        ++version[q];
        return 0;
    }
    int rotate_recorded(PairEnvs& env, const GradStep& s, int slot) {
        if (!fused) return rotate_recorded_stepwise(*this, env, s, slot);
        // the lanes' launch_lanes_grad_step: the environments next to the site once, then every parameter's rotation and inner product
        if (env_advance(*this, env, s.q, s.q)) return 1;
        use(L[s.q], "L", s.q, 0, s.q, "a fused rotation");
        use(R[s.q], "R", s.q, s.q + 1, n, "a fused rotation");
        for (int k = 0; k < s.count; ++k) {
            rotate(s.q, s.r[k].g);
            ops.assign(1, std::make_pair(s.q, &pauli_of(s.r[k].pauli)));
            vals.at(slot + k) = dense_dot();
        }
        env.touched(s.q, s.q);
        return 0;
    }
};

static Vec gradient(const Vec& w, const Vec& z, const aqc_circuit& c, const double* th, int lo, int hi, bool front_layer) {
    const int n = c.num_qubits;
    const WalkSizes sz = walk_sizes(&c, n);
    const std::vector<GradStep> steps = gradient_steps(&c, n, lo, hi, front_layer);
    Vec grad[2];
    for (int fused = 0; fused < 2; ++fused) {
        DenseExec ex(n, th, fused != 0, w, z, sz.max_records);
        PairEnvs env;
        env.reset(n);
        GradRecords rec;
        if (gradient_walk(ex, env, steps, 0, rec) || (int)rec.size() > sz.max_records) exit(4);
        grad[fused].resize(sz.T);
        assemble_gradient(rec, ex.vals.data(), sz.T, grad[fused].data());
    }
    if (grad[0] != grad[1]) {   // (the same dense arithmetic on the same operands)
        fprintf(stderr, "%s: the step-by-step and the fused walk differ\n", g_case);
        exit(5);
    }
    return grad[0];
}

static bool read_vec(Vec& v) {
    for (cd& a : v) {
        double re, im;
        if (scanf("%lf %lf", &re, &im) != 2) return false;
        a = cd(re, im);
    }
    return true;
}
static void print_vec(const Vec& v) { for (const cd& a : v) printf("%.17g %.17g\n", a.real(), a.imag()); }

int main(int argc, char** argv) {
    if (argc > 1) g_case = argv[1];
    int n, ent, L, trotter, second, T, lo, hi;
    if (scanf("%d %d %d %d %d", &n, &ent, &L, &trotter, &second) != 5 || n < 1 || n > 6 || L < 0 || L > 4096 || ent < AQC_CX || ent > AQC_CP) return 2;
    std::vector<int32_t> blocks(2 * (size_t)L + 1);
    for (int i = 0; i < 2 * L; ++i)
        if (scanf("%d", &blocks[i]) != 1 || blocks[i] < 0 || blocks[i] >= n) return 2;
    for (int i = 0; i < L; ++i)
        if (blocks[i] == blocks[L + i]) return 2;
    const aqc_circuit c = {n, ent, L, trotter, second, blocks.data()};
    if (scanf("%d", &T) != 1 || T != walk_sizes(&c, n).T) return 2;
    std::vector<double> th((size_t)T + 1);
    for (int i = 0; i < T; ++i)
        if (scanf("%lf", &th[i]) != 1) return 2;
    Vec x((size_t)1 << n), y((size_t)1 << n);
    if (!read_vec(x) || !read_vec(y) || scanf("%d %d", &lo, &hi) != 2) return 2;
    Vec vx = x, vhy = y;
    run_circuit(vx, c, th.data(), false);
    run_circuit(vhy, c, th.data(), true);
    print_vec(vx);
    print_vec(vhy);
    print_vec(gradient(x, vhy, c, th.data(), 0, L, true));
    print_vec(gradient(x, vhy, c, th.data(), lo, hi, false));
    return 0;
}
