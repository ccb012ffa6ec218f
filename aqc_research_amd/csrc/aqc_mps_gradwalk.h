// How the native MPS side executes a gradient walk (gradient_steps of aqc_mps_walk.h), stated ONCE: which environments of the pair
// (w, z) a gate leaves valid, how an inner product <(ops) w|z> is taken from them, when `touched` is called and with what range,
// which slot a record takes, and the final sum.  Three executors run this skeleton, each with its own site steps: the single-lane
// engine (struct Environments of aqc_mps_engine.cpp), the lockstep lanes (struct LanesExec of aqc_mps_batch.cpp) and the dense
// executor of tests/native/walk_selftest.cpp, whose "environments" are version stamps that make a stale read an error.
// HIP-free like aqc_mps_walk.h; private to csrc/, internal linkage.
//
// An executor `ex` provides (every function returns 0, or 1 after reporting a failure):
//   ex.left(p)              L[p + 1] from L[p] and the sites p of w and z
//   ex.right(p)             Rc[p - 1] from Rc[p] and the sites p
//   ex.chain(p, first, k, op)   scratch k (0 / 1) from L[p] (first) or from scratch 1 - k, through site p with `op` (may be null) on w's side
//   ex.close(hi, k, slot)   vals[slot] = scratch k against Rc[hi]
//   ex.entangle(step)       the routed entangler of an Entangle step on both operands
//   ex.rotate(q, g)         the 1-qubit gate g on site q of both operands
//   ex.rotate_recorded(env, step, slot)   a recorded Rotate step: slots slot, slot + 1, ... (rotate_recorded_stepwise below, or fused)
// The site steps behind left / right / chain of the single-lane executors are stated in aqc_mps_contract.h.
#pragma once
#include <utility>
#include <vector>

#include "aqc_mps_walk.h"

namespace {

// thetas of a circuit, and the most inner products one gradient walk records (the virtual Trotter tail records as well)
struct WalkSizes { int T, max_records; };
[[maybe_unused]] WalkSizes walk_sizes(const aqc_circuit* c, int n) {
    const int tpb = thetas_per_block(c);
    return {3 * n + tpb * c->num_blocks, 3 * n + tpb * (int)blocks_of(c).size()};
}

// Validity of the environments of the pair (w, z): L[q] = contraction of the sites < q, Rc[q] = that of the sites > q.  L[0 .. valid_l]
// and Rc[valid_r .. n - 1] are current.  A gate on the sites [lo, hi] leaves L[<= lo] and Rc[>= hi] valid, so the ~T inner products of
// one gradient cost a few site steps each instead of a full chain of n.
struct PairEnvs {
    int n = 0, valid_l = 0, valid_r = 0;
    void reset(int n_) { n = n_; valid_l = 0; valid_r = n - 1; }
    void touched(int lo, int hi) { valid_l = std::min(valid_l, lo); valid_r = std::max(valid_r, hi); }
};

// left environments up to site lo, right environments down to site hi
template <class Exec>
int env_advance(Exec& ex, PairEnvs& env, int lo, int hi) {
    for (; env.valid_l < lo; ++env.valid_l)
        if (ex.left(env.valid_l)) return 1;
    for (; env.valid_r > hi; --env.valid_r)
        if (ex.right(env.valid_r)) return 1;
    return 0;
}

// vals[slot] = <(G_1 on q_1)(G_2 on q_2) w | z>, q_1 < q_2 (nops = 1: only q_1)
template <class Exec>
int env_dot(Exec& ex, PairEnvs& env, int slot, int nops, const int* q, const M2* const* g) {
    const int lo = q[0], hi = q[nops - 1];
    if (env_advance(ex, env, lo, hi)) return 1;
    for (int p = lo; p <= hi; ++p) {
        const M2* op = p == q[0] ? g[0] : (nops > 1 && p == q[1] ? g[1] : nullptr);
        if (ex.chain(p, p == lo, (p - lo) & 1, op)) return 1;
    }
    return ex.close(hi, (hi - lo) & 1, slot);
}

// a recorded Rotate step, parameter by parameter: the rotation on both operands, then its inner product <P w|z>
template <class Exec>
int rotate_recorded_stepwise(Exec& ex, PairEnvs& env, const GradStep& s, int slot) {
    for (int k = 0; k < s.count; ++k) {
        if (ex.rotate(s.q, s.r[k].g)) return 1;
        env.touched(s.q, s.q);
        const M2* op = &pauli_of(s.r[k].pauli);
        if (env_dot(ex, env, slot + k, 1, &s.q, &op)) return 1;
    }
    return 0;
}

// every recorded inner product: (theta index, factor); several may add into one theta (Trotter tail)
typedef std::vector<std::pair<int, cd>> GradRecords;

// the walk: w and z take the steps one after the other; the inner products go to the slots slot0, slot0 + 1, ... in the order of the list
template <class Exec>
int gradient_walk(Exec& ex, PairEnvs& env, const std::vector<GradStep>& steps, int slot0, GradRecords& rec) {
    rec.clear();
    for (const GradStep& s : steps) {
        const int slot = slot0 + (int)rec.size();
        if (s.kind == GradStep::RecordP11) {
            const int qq[2] = {s.q, s.q2};
            const M2* gg[2] = {&kProj1, &kProj1};
            if (env_dot(ex, env, slot, 2, qq, gg)) return 1;
            rec.emplace_back(s.tindex, s.factor);
        } else if (s.kind == GradStep::Entangle) {
            if (ex.entangle(s)) return 1;
            env.touched(std::min(s.q, s.q2), std::max(s.q, s.q2));   // (the swaps of the routing pass through every site in between)
        } else if (!s.recorded) {
            for (int k = 0; k < s.count; ++k) {
                if (ex.rotate(s.q, s.r[k].g)) return 1;
                env.touched(s.q, s.q);
            }
        } else {
            if (ex.rotate_recorded(env, s, slot)) return 1;
            for (int k = 0; k < s.count; ++k) rec.emplace_back(s.r[k].tindex, s.factor);
        }
    }
    return 0;
}

// out[T] from one lane's recorded inner products (vals[i] belongs to rec[i])
[[maybe_unused]] void assemble_gradient(const GradRecords& rec, const cd* vals, int T, cd* out) {
    std::fill(out, out + T, cd(0.0, 0.0));
    for (size_t i = 0; i < rec.size(); ++i) out[rec[i].first] += rec[i].second * vals[i];
}

}  // namespace
