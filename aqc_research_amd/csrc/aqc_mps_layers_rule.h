// The rules of gate layers on single-lane MPS states (aqc_mps_layers.hip, aqc_mps_layers_api.cpp), HIP-free: the same text is compiled
// into the library and by a plain C++ compiler (tests/native/mps_layers_rule_selftest.cpp); tests/mps_layers_ref.py states the result in
// NumPy.  A program is an ordered list of ops on n qubits: a 2 x 2 matrix on one qubit, or a 4 x 4 matrix (index 2 bit_a + bit_b) on any
// pair (a, b).  The engine's gauge: T_q = Gamma_q lambda_q; a gate on the sites (q, q + 1) reads lambda_{q-1} and writes T_q, T_{q+1}
// and lambda_q (gate_adjacent of aqc_mps_engine.cpp, the statement of tests/mps_trunc_ref.py).
//   routing   a pair that is not adjacent goes through route_pair of aqc_mps_walk.h: swaps down, the gate (flipped when a is the upper
//             qubit), swaps back -- what gate2_pair does.  After routing every 2-qubit op acts on sites (q, q + 1).
//   folding   exact: a 1-qubit unitary on a physical index changes no singular value.  Every 1-qubit op is multiplied into the NEXT
//             2-qubit op that acts on its qubit; where no later one does, into the LAST earlier one, from the left; a qubit that no 2-qubit
//             op touches keeps the product of its 1-qubit ops (one site launch at the end).  What is left: 4 x 4 matrices on adjacent
//             sites, and at most one 2 x 2 per untouched qubit.  The structure is that of the program; the numbers may differ per state.
//   layering  as soon as possible: a gate on (q, q + 1) goes into layer max(ready[q], ready[q+1]), and both become that + 1.  The gates
//             of a layer act on disjoint sites and bonds: run "at once" they give the numbers of any order.  The layer of a gate depends
//             on the structure only.
//   bounds    bond b can never exceed natural_b = min(2^b, 2^(n-b), max_bond if > 0).  Storage is sized by
//             bound_b = max(min(natural_b, kMpsLayersCap), the input's own bond b): the input's is larger only without max_bond or on
//             hand-made states.  A rank above bound_b (numerical noise above the rank floor on a hand-made state) fails that state
//             with kMpsLayersOverflow; it is never cut silently.
//   route     per call: fused when every natural_b and every input bond is <= kMpsLayersCap (max_bond in 1 .. 64, or n <= 13), else
//             gatewise (gate_adjacent in layer order on a clone, the same folded matrices).
//   chunk     the matrices of a layer (gates x states) share the stores of one batched SVD of 2K x 2K matrices, K the largest bound.
//   decision  of a split: mps_compress_decide of aqc_mps_compress_rule.h (the engine's mps_rank_rule, then total, kept, rescale).
#pragma once
#include <assert.h>

#include <complex>
#include <vector>

#include "aqc_mps_compress_rule.h"
#include "aqc_mps_walk.h"

namespace aqc {

enum { kMpsLayersCap = 64 };
enum { kMpsLayersByRule = 0, kMpsLayersFused = 1, kMpsLayersGatewise = 2 };
enum { kMpsLayersOk = 0, kMpsLayersSweepLimit = 1, kMpsLayersNonFinite = 2, kMpsLayersOverflow = 3 };   // status of a state (0 .. 2: kMpsCompress*)

inline bool mps_layers_method_ok(int method) { return method == kMpsLayersByRule || method == kMpsLayersFused || method == kMpsLayersGatewise; }

struct MpsLayersOp { int two, a, b; };                    // an op of the program: two = 0: on qubit a; two = 1: on the pair (a, b)
struct MpsLayersRouted { int two, q, src, swap, flip; };  // after routing: on site q or on the sites (q, q + 1); src: the op it came from
struct MpsLayersGate { int q, layer; };                   // a folded gate on the sites (q, q + 1)

inline std::vector<MpsLayersRouted> mps_layers_route_ops(const std::vector<MpsLayersOp>& ops) {
    std::vector<MpsLayersRouted> out;
    for (size_t i = 0; i < ops.size(); ++i) {
        if (!ops[i].two) { out.push_back({0, ops[i].a, (int)i, 0, 0}); continue; }
        for (const RouteStep& r : route_pair(ops[i].a, ops[i].b)) out.push_back({1, r.q, (int)i, r.swap ? 1 : 0, r.flip});
    }
    return out;
}

// the structure of a routed program: its folded gates in program order with their layers, the gates of every layer (ascending program
// order, which within a layer is no order of the arithmetic), and the qubits that no 2-qubit op touches
struct MpsLayersPlan {
    int n = 0;
    std::vector<MpsLayersGate> gates;
    std::vector<std::vector<int>> layers;
    std::vector<int> touched;      // [n]
    std::vector<int> has_single;   // [n]: an untouched qubit with at least one 1-qubit op
    size_t widest() const {
        size_t w = 0;
        for (const std::vector<int>& l : layers) w = l.size() > w ? l.size() : w;
        return w;
    }
};
inline MpsLayersPlan mps_layers_plan(int n, const std::vector<MpsLayersRouted>& ops) {
    MpsLayersPlan p;
    p.n = n;
    p.touched.assign(n, 0);
    p.has_single.assign(n, 0);
    std::vector<int> ready(n, 0);
    for (const MpsLayersRouted& op : ops) {
        if (!op.two) continue;
        const int layer = ready[op.q] > ready[op.q + 1] ? ready[op.q] : ready[op.q + 1];
        ready[op.q] = ready[op.q + 1] = layer + 1;
        p.touched[op.q] = p.touched[op.q + 1] = 1;
        if ((int)p.layers.size() <= layer) p.layers.resize(layer + 1);
        p.layers[layer].push_back((int)p.gates.size());
        p.gates.push_back({op.q, layer});
    }
    for (const MpsLayersRouted& op : ops)
        if (!op.two && !p.touched[op.q]) p.has_single[op.q] = 1;
    return p;
}

// ---- folding: mats holds 16 complex numbers per routed op (a 1-qubit op uses the first 4, row-major; a 2-qubit op is the 4 x 4 on the
// index 2 bit_q + bit_{q+1}, swaps and flips already applied).  gates: 16 per folded gate of the plan; singles: 4 per qubit (the
// identity where has_single is 0)
namespace layers_detail {
typedef std::complex<double> cd;
inline void kron_right(cd* g, const cd* pa, const cd* pb) {   // g <- g (pa x pb)
    cd k[16], r[16];
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) for (int c = 0; c < 2; ++c) for (int d = 0; d < 2; ++d)
        k[4 * (2 * a + b) + 2 * c + d] = pa[2 * a + c] * pb[2 * b + d];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
        cd acc = 0.0;
        for (int m = 0; m < 4; ++m) acc += g[4 * i + m] * k[4 * m + j];
        r[4 * i + j] = acc;
    }
    for (int i = 0; i < 16; ++i) g[i] = r[i];
}
inline void kron_left(cd* g, const cd* pa, const cd* pb) {    // g <- (pa x pb) g
    cd k[16], r[16];
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) for (int c = 0; c < 2; ++c) for (int d = 0; d < 2; ++d)
        k[4 * (2 * a + b) + 2 * c + d] = pa[2 * a + c] * pb[2 * b + d];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
        cd acc = 0.0;
        for (int m = 0; m < 4; ++m) acc += k[4 * i + m] * g[4 * m + j];
        r[4 * i + j] = acc;
    }
    for (int i = 0; i < 16; ++i) g[i] = r[i];
}
inline void mul2(cd* p, const cd* u) {   // p <- u p
    const cd r[4] = {u[0] * p[0] + u[1] * p[2], u[0] * p[1] + u[1] * p[3], u[2] * p[0] + u[3] * p[2], u[2] * p[1] + u[3] * p[3]};
    for (int i = 0; i < 4; ++i) p[i] = r[i];
}
}  // namespace layers_detail

inline void mps_layers_fold(const MpsLayersPlan& plan, const std::vector<MpsLayersRouted>& ops, const std::complex<double>* mats,
                            std::complex<double>* gates, std::complex<double>* singles) {
    using namespace layers_detail;
    const int n = plan.n;
    const cd eye[4] = {1.0, 0.0, 0.0, 1.0};
    std::vector<cd> pending((size_t)4 * n);
    for (int q = 0; q < n; ++q) for (int i = 0; i < 4; ++i) pending[4 * q + i] = eye[i];
    std::vector<int> last(n, -1);
    int g = 0;
    for (size_t i = 0; i < ops.size(); ++i) {
        const cd* m = mats + 16 * i;
        const int q = ops[i].q;
        if (!ops[i].two) { mul2(&pending[4 * q], m); continue; }
        cd* out = gates + (size_t)16 * g;
        for (int e = 0; e < 16; ++e) out[e] = m[e];
        kron_right(out, &pending[4 * q], &pending[4 * (q + 1)]);
        for (int e = 0; e < 4; ++e) pending[4 * q + e] = pending[4 * (q + 1) + e] = eye[e];
        last[q] = last[q + 1] = g++;
    }
    assert(g == (int)plan.gates.size());
    for (int q = 0; q < n; ++q) {
        for (int e = 0; e < 4; ++e) singles[4 * q + e] = eye[e];
        if (last[q] < 0) { for (int e = 0; e < 4; ++e) singles[4 * q + e] = pending[4 * q + e]; continue; }
        cd* out = gates + (size_t)16 * last[q];
        if (plan.gates[last[q]].q == q) kron_left(out, &pending[4 * q], eye);
        else kron_left(out, eye, &pending[4 * q]);
    }
}

// ---- bounds and route
inline int mps_layers_natural(int n, int b, int max_bond) {   // min(2^b, 2^(n-b), max_bond if > 0), saturating far above any cap
    const int lo = b < n - b ? b : n - b;
    int v = lo >= 20 ? 1 << 20 : 1 << lo;
    if (max_bond > 0 && max_bond < v) v = max_bond;
    return v;
}
// dims: the input's n + 1 bonds, or null
inline std::vector<int> mps_layers_bounds(int n, int max_bond, const int* dims) {
    std::vector<int> out(n + 1, 1);
    for (int b = 0; b <= n; ++b) {
        const int nat = mps_layers_natural(n, b, max_bond);
        out[b] = nat < kMpsLayersCap ? nat : (int)kMpsLayersCap;
        if (dims && dims[b] > out[b]) out[b] = dims[b];
    }
    return out;
}
inline int mps_layers_route(int n, const int* dims, int max_bond) {
    for (int b = 0; b <= n; ++b)
        if (mps_layers_natural(n, b, max_bond) > kMpsLayersCap || (dims && dims[b] > kMpsLayersCap)) return kMpsLayersGatewise;
    return kMpsLayersFused;
}
// on the fused route a rank above its bound cannot leave the device (the split fails the state instead)
inline bool mps_layers_ranks_fit(int n, const int* bounds, const int* dims) {
    for (int b = 0; b <= n; ++b)
        if (dims[b] > bounds[b]) return false;
    return true;
}

// matrices (gates x states) per chunk of a layer: the five stores of the batched SVD of 2k x 2k matrices within budget_bytes
inline int mps_layers_chunk(int k, size_t total, size_t budget_bytes) { return mps_svd_chunk(2 * k, 2 * k, total, budget_bytes, (size_t)1 << 16); }

}  // namespace aqc
