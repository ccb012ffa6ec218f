// Dense state-vector executor of the MPS side's gate walk (aqc_mps_walk.h; built with -fsanitize=address,undefined by
// tests/test_native_sanitizers.py): the third, trivial executor next to the single-lane engine and the lockstep lanes.  It evaluates
// circuit_ops and gradient_steps with 2 x 2 and 4 x 4 matrices on a std::vector<std::complex<double>> (qubit q = bit q, n <= 6).
// stdin:  n entangler num_blocks trotter second_order, blocks[2][num_blocks], T thetas, x (2^n x re im), y, lo_blk hi_blk
// stdout: V x, V^H y, the full gradient of <V x|y>, the gradient of the blocks [lo_blk, hi_blk) with front_layer off: one "re im" a line
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../aqc_research_amd/csrc/aqc_mps_walk.h"

typedef std::vector<cd> Vec;

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
// <(G on q)(G2 on q2) w|z>
static cd dot_ops(Vec w, const Vec& z, int q, const M2& g, int q2 = -1, const M2* g2 = nullptr) {
    apply1(w, q, g);
    if (g2) apply1(w, q2, *g2);
    cd s = 0.0;
    for (size_t i = 0; i < w.size(); ++i) s += std::conj(w[i]) * z[i];
    return s;
}
static std::vector<cd> gradient(Vec w, Vec z, const aqc_circuit& c, const double* th, int T, int lo, int hi, bool front_layer) {
    std::vector<cd> grad(T, cd(0.0, 0.0));
    for (const GradStep& s : gradient_steps(&c, c.num_qubits, lo, hi, front_layer)) {
        if (s.kind == GradStep::RecordP11) {
            grad[s.tindex] += s.factor * dot_ops(w, z, s.q, kProj1, s.q2, &kProj1);
        } else if (s.kind == GradStep::Entangle) {
            for (const RouteStep& r : route_pair(s.q, s.q2)) {
                double g32[32];
                gate2_matrix(routed_gate(r, s.ent), th, g32);
                apply2(z, r.q, g32);
                apply2(w, r.q, g32);
            }
        } else {
            for (int k = 0; k < s.count; ++k) {
                const M2 g = gate1_matrix(s.r[k].g, th);
                apply1(w, s.q, g);
                apply1(z, s.q, g);
                if (s.recorded) grad[s.r[k].tindex] += s.factor * dot_ops(w, z, s.q, pauli_of(s.r[k].pauli));
            }
        }
    }
    return grad;
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

int main() {
    int n, ent, L, trotter, second, T, lo, hi;
    if (scanf("%d %d %d %d %d", &n, &ent, &L, &trotter, &second) != 5 || n < 1 || n > 6 || L < 0 || L > 4096 || ent < AQC_CX || ent > AQC_CP) return 2;
    std::vector<int32_t> blocks(2 * (size_t)L + 1);
    for (int i = 0; i < 2 * L; ++i)
        if (scanf("%d", &blocks[i]) != 1 || blocks[i] < 0 || blocks[i] >= n) return 2;
    for (int i = 0; i < L; ++i)
        if (blocks[i] == blocks[L + i]) return 2;
    const aqc_circuit c = {n, ent, L, trotter, second, blocks.data()};
    if (scanf("%d", &T) != 1 || T != 3 * n + thetas_per_block(&c) * L) return 2;
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
    print_vec(gradient(x, vhy, c, th.data(), T, 0, L, true));
    print_vec(gradient(x, vhy, c, th.data(), T, lo, hi, false));
    return 0;
}
