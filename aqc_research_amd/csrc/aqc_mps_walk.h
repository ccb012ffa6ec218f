// The ansatz as the native MPS side walks it, stated ONCE: the program of V / V^H (core_operations.py:671-708, :787-818) and the
// gate-by-gate gradient walk (mps_dot_objective.py:41-242, core_operations.py:921-935, core_op_matrix.py:430-477) as plain lists
// that the single-lane engine (aqc_mps_engine.cpp) and the lockstep lanes (aqc_mps_batch.cpp) execute, each with its own launches.
// Gate order, signs, theta indices, the Trotter pre / post rotations, the Rx / Rz choice, the CPhase rule, the swap routing of
// long-range entanglers and the block-range rule live here and nowhere else on the MPS side.  HOW a gradient walk is executed
// (environments, slots, the final sum) is stated once as well, in aqc_mps_gradwalk.h.
// HIP-free (a plain C++ compiler builds it: tests/native/walk_selftest.cpp evaluates both lists on a dense state vector against
// the reference's golden outputs).  Private to csrc/; the functions have internal linkage.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <initializer_list>
#include <vector>

#include "../../include/aqc_hip.h"

namespace aqc {
// ---- gate notation (read by the kernels of aqc_mps_lanes.hip: layouts are part of the launch interface)
struct LaneRot { int kind /* 0 none, 1 rz, 2 ry, 3 rx */, idx; double scale; };        // angle = scale * thetas[lane][idx], or = scale when idx < 0
struct LaneGate1 { LaneRot r[3]; };                                                    // the product r[0] r[1] r[2]
struct LaneGate2 { int kind /* 0 swap, 1 cx, 2 cz, 3 cp */, idx, flip, pad; double scale; };   // cp angle = scale * thetas[lane][idx]; flip: control on site q + 1
struct LaneOp1 { int q, pad; LaneGate1 g; };   // a 1-qubit gate on site q
struct LaneOp2 { int q, pad; LaneGate2 g; };   // a 2-qubit gate on the sites (q, q + 1)
}  // namespace aqc

namespace {
using namespace aqc;

// ---- 2 x 2 / 4 x 4 gate algebra on the host
typedef std::complex<double> cd;
struct M2 { cd m[4]; };   // row-major 2x2
[[maybe_unused]] M2 operator*(const M2& x, const M2& y) {
    return {{x.m[0] * y.m[0] + x.m[1] * y.m[2], x.m[0] * y.m[1] + x.m[1] * y.m[3], x.m[2] * y.m[0] + x.m[3] * y.m[2], x.m[2] * y.m[1] + x.m[3] * y.m[3]}};
}
[[maybe_unused]] M2 adjoint(const M2& g) { return {{std::conj(g.m[0]), std::conj(g.m[2]), std::conj(g.m[1]), std::conj(g.m[3])}}; }
[[maybe_unused]] M2 rz_m(double t) { return {{std::polar(1.0, -0.5 * t), 0.0, 0.0, std::polar(1.0, 0.5 * t)}}; }
[[maybe_unused]] M2 ry_m(double t) { const double c = std::cos(0.5 * t), s = std::sin(0.5 * t); return {{c, -s, s, c}}; }
[[maybe_unused]] M2 rx_m(double t) { const double c = std::cos(0.5 * t), s = std::sin(0.5 * t); return {{c, cd(0, -s), cd(0, -s), c}}; }
[[maybe_unused]] const M2 kPauliX = {{0.0, 1.0, 1.0, 0.0}}, kPauliY = {{0.0, cd(0, -1), cd(0, 1), 0.0}}, kPauliZ = {{1.0, 0.0, 0.0, -1.0}}, kProj1 = {{0.0, 0.0, 0.0, 1.0}};
[[maybe_unused]] void pack(const M2& g, double* out8) { for (int i = 0; i < 4; ++i) { out8[2 * i] = g.m[i].real(); out8[2 * i + 1] = g.m[i].imag(); } }
[[maybe_unused]] M2 unpack(const double* g8) { return {{cd(g8[0], g8[1]), cd(g8[2], g8[3]), cd(g8[4], g8[5]), cd(g8[6], g8[7])}}; }

constexpr int RZ = 1, RY = 2, RX = 3;   // LaneRot::kind; also names the Pauli generator of a recorded rotation
[[maybe_unused]] const M2& pauli_of(int kind) { return kind == RZ ? kPauliZ : (kind == RY ? kPauliY : kPauliX); }
// a LaneGate1 for one set of parameters, multiplied left to right starting from the first rotation (as the kernels do)
[[maybe_unused]] M2 gate1_matrix(const LaneGate1& g, const double* th) {
    auto one = [&](const LaneRot& r) {
        const double t = r.idx >= 0 ? r.scale * th[r.idx] : r.scale;
        return r.kind == RZ ? rz_m(t) : (r.kind == RY ? ry_m(t) : rx_m(t));
    };
    M2 u = one(g.r[0]);
    for (int k = 1; k < 3 && g.r[k].kind; ++k) u = u * one(g.r[k]);
    return u;
}

[[maybe_unused]] void entangler_matrix(int ent, double angle, double* out32) {   // |0><0| x I + |1><1| x {X, Z, diag(1, e^{i angle})}, index 2 c + t
    std::fill(out32, out32 + 32, 0.0);
    out32[0] = 1.0; out32[2 * 5] = 1.0;
    if (ent == AQC_CX) { out32[2 * 11] = 1.0; out32[2 * 14] = 1.0; }
    else if (ent == AQC_CZ) { out32[2 * 10] = 1.0; out32[2 * 15] = -1.0; }
    else { out32[2 * 10] = 1.0; out32[2 * 15] = std::cos(angle); out32[2 * 15 + 1] = std::sin(angle); }
}
[[maybe_unused]] void permute_gate(const double* g, bool flip, double* out) {   // flip: swap the roles of the two qubits (index 2a+b -> 2b+a)
    static const int p[4] = {0, 2, 1, 3};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const int si = flip ? p[i] : i, sj = flip ? p[j] : j;
            out[2 * (4 * i + j)] = g[2 * (4 * si + sj)];
            out[2 * (4 * i + j) + 1] = g[2 * (4 * si + sj) + 1];
        }
}
// the 4 x 4 (c128, row-major, index 2 * bit_q + bit_{q+1}) of a routed 2-qubit op for one set of parameters
[[maybe_unused]] void gate2_matrix(const LaneGate2& g, const double* th, double* out32) {
    static const double swap_gate[32] = {1, 0, 0, 0, 0, 0, 0, 0,  0, 0, 0, 0, 1, 0, 0, 0,  0, 0, 1, 0, 0, 0, 0, 0,  0, 0, 0, 0, 0, 0, 1, 0};
    if (g.kind == 0) { std::copy(swap_gate, swap_gate + 32, out32); return; }
    double ent[32];
    entangler_matrix(g.kind - 1, g.idx >= 0 ? g.scale * th[g.idx] : 0.0, ent);   // (LaneGate2::kind = 1 + AQC_CX / AQC_CZ / AQC_CP)
    permute_gate(ent, g.flip != 0, out32);
}

// ---- the blocks of an ansatz
struct BlockRef { int i, j, c, t; };   // running index, parameter block, control, target
// incl. the virtual trailing half-layer of a 2nd-order Trotter ansatz (parametric_circuit.py:328-333)
[[maybe_unused]] std::vector<BlockRef> blocks_of(const aqc_circuit* c) {
    const int L = c->num_blocks, tail = (c->trotter && c->second_order) ? 3 * (c->num_qubits / 2) : 0;
    std::vector<BlockRef> out;
    for (int i = 0; i < L + tail && L > 0; ++i) out.push_back({i, i % L, c->blocks[i % L], c->blocks[L + i % L]});
    return out;
}

// ---- a 2-qubit gate (index 2 * bit_ctrl + bit_targ) on any pair of qubits: swaps bring the upper qubit down next to the lower one, the
// gate acts on the sites (lo, lo + 1) -- site lo carries the lower qubit: flip when ctrl is the upper one --, the swaps go back (the route
// Aer takes as well)
struct RouteStep { int q; bool swap; int flip; };   // on the sites (q, q + 1): a swap, or the gate itself
[[maybe_unused]] std::vector<RouteStep> route_pair(int ctrl, int targ) {
    const int lo = std::min(ctrl, targ), hi = std::max(ctrl, targ);
    std::vector<RouteStep> out;
    for (int p = hi - 1; p > lo; --p) out.push_back({p, true, 0});
    out.push_back({lo, false, ctrl > targ ? 1 : 0});
    for (int p = lo + 1; p < hi; ++p) out.push_back({p, true, 0});
    return out;
}
[[maybe_unused]] LaneGate2 routed_gate(const RouteStep& r, const LaneGate2& g) { return r.swap ? LaneGate2{0, -1, 0, 0, 0.0} : LaneGate2{g.kind, g.idx, r.flip, 0, g.scale}; }

// ---- the rules of a block, shared by the two programs below
struct BlockGates {
    bool pre, post;     // Trotter: Rz(-pi/2) on the control in front of blocks 0, 3, 6, ..., Rz(+pi/2) on the target behind blocks 2, 5, 8, ...
    int base, rt;       // theta index of the block's first parameter (Ry, Rz on the control; Ry, Rx | Rz on the target; CPhase angle); kind of the 4th
    LaneGate2 ent;      // the entangler, before routing (scale 1)
};
[[maybe_unused]] LaneRot rot(int kind, int idx, double scale) { return LaneRot{kind, idx, scale}; }
[[maybe_unused]] LaneGate1 g1(LaneRot a, LaneRot b = LaneRot{0, -1, 0.0}, LaneRot c = LaneRot{0, -1, 0.0}) { return LaneGate1{{a, b, c}}; }
constexpr double kHalfPi = 1.5707963267948966;
[[maybe_unused]] int thetas_per_block(const aqc_circuit* c) { return c->entangler == AQC_CP ? 5 : 4; }
[[maybe_unused]] BlockGates block_gates(const aqc_circuit* c, int n, const BlockRef& b) {
    const int base = 3 * n + thetas_per_block(c) * b.j;
    return {c->trotter && b.i % 3 == 0, c->trotter && b.i % 3 == 2, base, c->entangler == AQC_CX ? RX : RZ,
            LaneGate2{1 + c->entangler, c->entangler == AQC_CP ? base + 4 : -1, 0, 0, 1.0}};
}

// ---- V or V^H in program order, long-range entanglers already routed
struct CircuitOp { bool two; LaneOp1 op1; LaneOp2 op2; };   // a 1-qubit gate on site op1.q, or a 2-qubit gate on the sites (op2.q, op2.q + 1)
[[maybe_unused]] std::vector<CircuitOp> circuit_ops(const aqc_circuit* c, int n, bool inverse) {
    const std::vector<BlockRef> blocks = blocks_of(c);
    const double s = inverse ? -1.0 : 1.0;
    std::vector<CircuitOp> out;
    auto one = [&](int q, const LaneGate1& g) { out.push_back({false, LaneOp1{q, 0, g}, LaneOp2{}}); };
    auto two = [&](const BlockRef& b, LaneGate2 g) {
        g.scale = s;
        for (const RouteStep& r : route_pair(b.c, b.t)) out.push_back({true, LaneOp1{}, LaneOp2{r.q, 0, routed_gate(r, g)}});
    };
    if (!inverse) {
        for (int q = 0; q < n; ++q) one(q, g1(rot(RZ, 3 * q, s), rot(RY, 3 * q + 1, s), rot(RZ, 3 * q + 2, s)));
        for (const BlockRef& b : blocks) {
            const BlockGates k = block_gates(c, n, b);
            if (k.pre) one(b.c, g1(rot(RZ, -1, -kHalfPi)));
            two(b, k.ent);
            one(b.c, g1(rot(RZ, k.base + 1, s), rot(RY, k.base, s)));
            one(b.t, g1(rot(k.rt, k.base + 3, s), rot(RY, k.base + 2, s)));
            if (k.post) one(b.t, g1(rot(RZ, -1, kHalfPi)));
        }
    } else {   // the same backwards, every angle negated
        for (auto it = blocks.rbegin(); it != blocks.rend(); ++it) {
            const BlockRef& b = *it;
            const BlockGates k = block_gates(c, n, b);
            if (k.post) one(b.t, g1(rot(RZ, -1, -kHalfPi)));
            one(b.t, g1(rot(RY, k.base + 2, s), rot(k.rt, k.base + 3, s)));
            one(b.c, g1(rot(RY, k.base, s), rot(RZ, k.base + 1, s)));
            two(b, k.ent);
            if (k.pre) one(b.c, g1(rot(RZ, -1, kHalfPi)));
        }
        for (int q = 0; q < n; ++q) one(q, g1(rot(RZ, 3 * q + 2, s), rot(RY, 3 * q + 1, s), rot(RZ, 3 * q, s)));
    }
    return out;
}

// ---- the gradient walk: w = lhs and z = V^H|target> take the gates of V one after the other; behind the rotation of parameter k the
// derivative is 0.5j <P_k w|z> (P_k the rotation's Pauli), for a CPhase angle it is -1j <P11 w|z> taken BEFORE the entangler.  A block
// outside [lo_blk, hi_blk) is applied but not recorded, the front layer likewise when front_layer is off.  Every recorded inner product
// takes the next slot, in the order of this list; several may add into one theta (Trotter tail).
struct GradRot { int tindex; LaneGate1 g; int pauli /* RZ / RY / RX */; };
struct GradStep {
    enum Kind { Rotate, RecordP11, Entangle } kind;
    int q, q2;            // Rotate: site q.  RecordP11: the sites q < q2.  Entangle: control q, target q2 (z takes it before w)
    int count;            // Rotate: 1-3 consecutive parameters on site q, each applied to both operands and then, if `recorded`, recorded
    GradRot r[3];
    bool recorded;
    int tindex;           // RecordP11: the theta it adds into
    LaneGate2 ent;        // Entangle: the gate before routing (ent.idx: theta index of the CPhase angle, or -1)
    cd factor;            // of a recorded inner product
};
[[maybe_unused]] std::vector<GradStep> gradient_steps(const aqc_circuit* c, int n, int lo_blk, int hi_blk, bool front_layer) {
    std::vector<GradStep> out;
    auto rotate = [&](int q, bool recorded, std::initializer_list<LaneRot> rs) {
        GradStep s{};
        s.kind = GradStep::Rotate; s.q = q; s.recorded = recorded; s.factor = cd(0, 0.5);
        for (const LaneRot& r : rs) s.r[s.count++] = GradRot{r.idx, g1(r), r.kind};
        out.push_back(s);
    };
    for (int q = 0; q < n; ++q)   // front layer Rz(t0) Ry(t1) Rz(t2): rightmost first
        rotate(q, front_layer, {rot(RZ, 3 * q + 2, 1.0), rot(RY, 3 * q + 1, 1.0), rot(RZ, 3 * q, 1.0)});
    for (const BlockRef& b : blocks_of(c)) {
        const BlockGates k = block_gates(c, n, b);
        const bool live = lo_blk <= b.j && b.j < hi_blk;
        if (k.pre) rotate(b.c, false, {rot(RZ, -1, -kHalfPi)});
        GradStep s{};
        s.tindex = k.ent.idx; s.factor = cd(0, -1.0);
        if (live && c->entangler == AQC_CP) { s.kind = GradStep::RecordP11; s.q = std::min(b.c, b.t); s.q2 = std::max(b.c, b.t); out.push_back(s); }
        s.kind = GradStep::Entangle; s.q = b.c; s.q2 = b.t; s.ent = k.ent;
        out.push_back(s);
        rotate(b.c, live, {rot(RY, k.base, 1.0), rot(RZ, k.base + 1, 1.0)});
        rotate(b.t, live, {rot(RY, k.base + 2, 1.0), rot(k.rt, k.base + 3, 1.0)});
        if (k.post) rotate(b.t, false, {rot(RZ, -1, kHalfPi)});
    }
    return out;
}

}  // namespace
