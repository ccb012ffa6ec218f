// Device-resident matrix-product states with truncated 2-qubit gates (C ABI: aqc_mps_*, aqc_svd).
//
// This is the arithmetic the reference delegates to qiskit-aer's matrix_product_state simulator
// (mps_operations.py:252-257, reached from mps_dot_objective.py:245-468): 1-qubit gates act on the physical index
// of one site tensor; a 2-qubit gate contracts two neighbouring sites, applies the 4x4 matrix, and splits the
// result with an SVD whose smallest singular values are discarded while the sum of their squares stays below
// `trunc_thr`; non-neighbouring qubits are brought together by swaps.  Aer itself is third party and absent from
// this image, so its truncation arithmetic is PARITY UNPINNED; with trunc_thr -> 0 every operation is exact and
// is tested against the dense state-vector oracle (the level the reference's own tests pin).
//
// Representation: site q holds T_q = Gamma_q . diag(lambda_q) as a [2][chi_l][chi_r] row-major complex128 tensor
// (the form _preprocess_mps builds, mps_operations.py:126-156) plus the Schmidt vector lambda_q of the bond to
// its right; |psi> = prod_q T_q.  A gate on (q, q+1) forms theta = diag(lambda_{q-1}) T_q T_{q+1}, so only one
// division by lambda (on the left bond) is needed when the new T_q is extracted.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/aqc_hip.h"
#include "aqc_devbuf.h"
#include "aqc_launch.h"
#include "aqc_mps_ent_rule.h"
#include "aqc_mps_host.h"

using namespace aqc;

namespace {

// Round-robin tournament: rounds x (n2/2) pairs over n2 = even(cols) players; index >= cols is a bye (-1).
void tournament(int cols, std::vector<int>& pairs, int& rounds, int& per_round) {
    const int n2 = cols + (cols & 1);
    rounds = n2 - 1;
    per_round = n2 / 2;
    pairs.assign((size_t)std::max(rounds, 0) * per_round * 2, -1);
    std::vector<int> ring(n2);
    std::iota(ring.begin(), ring.end(), 0);
    for (int r = 0; r < rounds; ++r) {
        for (int i = 0; i < per_round; ++i) {
            int a = ring[i], b = ring[n2 - 1 - i];
            if (a > b) std::swap(a, b);
            if (b >= cols) { a = -1; b = -1; }
            pairs[((size_t)r * per_round + i) * 2] = a;
            pairs[((size_t)r * per_round + i) * 2 + 1] = b;
        }
        std::rotate(ring.begin() + 1, ring.end() - 1, ring.end());   // player 0 stays, the others move one seat
    }
}

struct SvdWork {
    DevBuf<int> pairs, flag;
    DevBuf<double> sigma;
    std::vector<int> h_pairs;
    int cached_cols = -1, cached_blocked = -1, rounds = 0, per_round = 0;
};

// Tournament over column blocks: a block without a partner (odd number of blocks) still plays, alone (.y = -1).
void block_tournament(int nblocks, std::vector<int>& pairs, int& rounds, int& per_round) {
    const int n2 = nblocks + (nblocks & 1);
    rounds = std::max(n2 - 1, 1);
    per_round = std::max(n2 / 2, 1);
    pairs.assign((size_t)rounds * per_round * 2, -1);
    if (nblocks == 1) { pairs[0] = 0; return; }
    std::vector<int> ring(n2);
    std::iota(ring.begin(), ring.end(), 0);
    for (int r = 0; r < rounds; ++r) {
        for (int i = 0; i < per_round; ++i) {
            int a = ring[i], b = ring[n2 - 1 - i];
            if (a > b) std::swap(a, b);
            pairs[((size_t)r * per_round + i) * 2] = a;
            pairs[((size_t)r * per_round + i) * 2 + 1] = b < nblocks ? b : -1;
        }
        std::rotate(ring.begin() + 1, ring.end() - 1, ring.end());
    }
}

// Orthogonalises the columns of the column-major W (rows x cols) in place, accumulating V (cols x cols);
// returns the column norms in h_sigma.  `sweeps_out` reports the number of sweeps used.
int jacobi_svd(SvdWork& sw, void* W, int rows, void* V, int cols, hipStream_t st, std::vector<double>& h_sigma, int* sweeps_out) {
    const bool blocked_ok = switch_now("AQC_SVD_BLOCKED") != 0;   // (0: round-per-launch cross-check)
    const bool small = svd_fits_small(rows, cols);
    const bool blocked = !small && blocked_ok && svd_fits_block(rows, cols);
    if (!small && (sw.cached_cols != cols || sw.cached_blocked != (int)blocked)) {   // (the one-workgroup kernel works its pairing out itself)
        if (blocked) block_tournament((cols + svd_block_size() - 1) / svd_block_size(), sw.h_pairs, sw.rounds, sw.per_round);
        else tournament(cols, sw.h_pairs, sw.rounds, sw.per_round);
        if (sw.pairs.reserve(std::max<size_t>(sw.h_pairs.size(), 2))) return 1;
        if (!sw.h_pairs.empty()) HIP_OK(hipMemcpyAsync(sw.pairs, sw.h_pairs.data(), sw.h_pairs.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        sw.cached_cols = cols;
        sw.cached_blocked = (int)blocked;
    }
    constexpr int kFlagInts = 64 + 4;   // [0..63] rotations per sweep | [64] barrier | [65] sweeps used | [66] barrier timeout
    if (sw.flag.reserve(kFlagInts) || sw.sigma.reserve((size_t)std::max(cols, 1) + 2)) return 1;   // sigma | fro2 | sweeps
    double* fro2 = sw.sigma + std::max(cols, 1);   // scale of the negligible-column rule (aqc_mps_dev.h: kNegligible2)
    int* flag = sw.flag;
    const double tol = 1e-15;
    int sweeps = 0;
    int status[2] = {0, 0};
    if (small) {   // one launch: matrix and V live in the LDS of one workgroup
        HIP_OK(launch_jacobi_small(W, rows, V, cols, tol, 60, flag, sw.sigma, st));
    } else if (blocked) {   // one cooperative launch: persistent workgroups, 16 columns at a time in LDS
        HIP_OK(launch_svd_identity(V, cols, st));
        HIP_OK(launch_svd_fro2(W, (size_t)rows * cols, fro2, st));
        HIP_OK(hipMemsetAsync(flag, 0, sizeof(int) * kFlagInts, st));
        int debug = 0;
#ifdef AQC_TUNING
        debug = (int)switch_now("AQC_SVD_DEBUG");
#endif
        HIP_OK(launch_jacobi_block(W, rows, V, cols, sw.pairs, sw.rounds, sw.per_round, tol, 60, fro2, flag, reinterpret_cast<unsigned*>(flag + 64), flag + 65, st, debug));
        HIP_OK(hipMemcpyAsync(status, flag + 65, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    } else {
        HIP_OK(launch_svd_identity(V, cols, st));
        HIP_OK(launch_svd_fro2(W, (size_t)rows * cols, fro2, st));
    }
    for (; !small && !blocked && sweeps < 60 && cols > 1; ++sweeps) {
        HIP_OK(hipMemsetAsync(flag, 0, sizeof(int), st));
        for (int r = 0; r < sw.rounds; ++r)
            HIP_OK(launch_jacobi_round(W, rows, V, cols, sw.pairs + (size_t)r * sw.per_round * 2, sw.per_round, tol, fro2, flag, st));
        int rotations = 0;
        HIP_OK(hipMemcpyAsync(&rotations, flag, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (rotations == 0) { ++sweeps; break; }
    }
    h_sigma.resize(cols + 2);
    if (!small) HIP_OK(launch_svd_norms(W, rows, cols, sw.sigma, st));   // (the one-launch kernel delivers them itself)
    HIP_OK(hipMemcpyAsync(h_sigma.data(), sw.sigma, sizeof(double) * (small ? cols + 2 : cols), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (small) sweeps = (int)h_sigma[cols + 1];   // the sweep count came with the singular values
    h_sigma.resize(cols);
    if (blocked) {
        if (status[1] != 0) return failf("Jacobi SVD: a grid barrier of the persistent kernel timed out (%d x %d)", rows, cols);
        sweeps = status[0];
    }
    if (sweeps_out) *sweeps_out = sweeps;   // the single-launch paths deliver their count with this synchronisation
    // every path stops at 60 sweeps; matrices of this engine converge in 6-14, so the cap means "did not converge"
    if (cols > 1 && sweeps >= 60) return failf("Jacobi SVD: no convergence within 60 sweeps (%d x %d)", rows, cols);
    return 0;
}

}  // namespace

struct aqc_mps {
    int device = 0, n = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;
    std::vector<int> dims;                    // n + 1 bond dimensions, dims[0] = dims[n] = 1
    std::vector<DevBuf<double2>> t;           // per site: [2][dims[q]][dims[q+1]] (the buffers only grow)
    std::vector<std::vector<double>> lam;     // n - 1 Schmidt vectors (host copy)
    std::vector<DevBuf<double>> d_lam;        // the same on the device (grow-only)
    DevBuf<double2> theta, work, vmat, tmp;
    DevBuf<char> ord;                         // column order (ints) | new Schmidt values (doubles, 16-byte aligned)
    // Pinned staging of what the host decides per 2-qubit gate (column order, new Schmidt values): two buffers used in turn.
    // A gate's uploads are asynchronous; the NEXT gate synchronises the stream to read its singular values, so by the time a
    // buffer is written again (two gates later) the copy out of it has completed -- no synchronisation of its own.
    PinBuf<char> stage[2];
    unsigned stage_turn = 0;
    SvdWork svd;
    double discarded = 0.0;                   // accumulated discarded weight (sum of squared singular values)
    int last_sweeps = 0;
};

namespace {

size_t site_elems(const aqc_mps* m, int q) { return (size_t)2 * m->dims[q] * m->dims[q + 1]; }

int reserve_lambda(aqc_mps* m, int bond, size_t count) {
    if (count <= m->d_lam[bond].capacity()) return 0;
    HIP_OK(hipStreamSynchronize(m->stream));
    return m->d_lam[bond].reserve(count);
}

int set_lambda(aqc_mps* m, int bond, const std::vector<double>& v) {
    m->lam[bond] = v;
    if (reserve_lambda(m, bond, v.size())) return 1;
    HIP_OK(hipMemcpyAsync(m->d_lam[bond], m->lam[bond].data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, m->stream));
    HIP_OK(hipStreamSynchronize(m->stream));   // the host vector may be replaced by the next gate
    return 0;
}

// pinned staging buffer of this gate (see aqc_mps::stage)
int stage_buffer(aqc_mps* m, size_t bytes, void** out) {
    const unsigned i = m->stage_turn++ & 1u;
    if (bytes > m->stage[i].capacity()) {
        HIP_OK(hipStreamSynchronize(m->stream));
        if (m->stage[i].reserve(std::max<size_t>(bytes * 2, 4096))) return 1;
    }
    *out = (char*)m->stage[i];
    return 0;
}

int reserve_site(aqc_mps* m, int q, size_t elems) {   // contents are NOT preserved
    if (elems <= m->t[q].capacity()) return 0;
    HIP_OK(hipStreamSynchronize(m->stream));
    return m->t[q].reserve(elems);
}

void destroy(aqc_mps* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    hipStream_t own = m->owns_stream ? m->stream : nullptr;
    delete m;   // (the buffers go before the stream, as they always have)
    if (own) (void)hipStreamDestroy(own);
}

int new_mps(int device, int n, aqc_mps** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return failf("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return failf("device out of range");
    if (n < 1 || n > 4096) return failf("number of qubits out of range");
    HIP_OK(hipSetDevice(device));
    aqc_mps* m = new aqc_mps();
    m->device = device; m->n = n;
    m->dims.assign(n + 1, 1);
    m->t.resize(n);
    m->lam.assign(std::max(n - 1, 0), {});
    m->d_lam.resize(std::max(n - 1, 0));
    if (hipStreamCreate(&m->stream) != hipSuccess) { delete m; return failf("hipStreamCreate failed"); }
    *out = m;
    return 0;
}

// One 4x4 gate on the neighbouring sites (q, q+1); matrix index = 2 * bit_q + bit_{q+1}.
int gate_adjacent(aqc_mps* m, int q, const double* g16, double trunc_thr, int max_bond) {
    const int chil = m->dims[q], chim = m->dims[q + 1], chir = m->dims[q + 2];
    const int rows = 2 * chil, cols = 2 * chir;
    hipStream_t st = m->stream;
    // Jacobi runs on the side with fewer columns
    const int mode = cols <= rows ? 0 : 1;
    const int wrows = mode == 0 ? rows : cols, wcols = mode == 0 ? cols : rows;
    if (m->work.reserve((size_t)wrows * wcols) || m->vmat.reserve((size_t)wcols * wcols)) return 1;
    const double* lam_left = q > 0 ? (double*)m->d_lam[q - 1] : nullptr;
    if (chim <= 64 && (size_t)chil * chir <= 4096) {   // small bonds: product, scaling and gate in one launch
        HIP_OK(launch_mps_theta_fused(m->t[q], m->t[q + 1], lam_left, chil, chim, chir, g16, mode, m->work, st));
    } else {
        if (m->theta.reserve((size_t)rows * cols)) return 1;
        // theta0[(a,l), (b,r)] = sum_m T_q[(a,l), m] T_{q+1}[b][m][r]
        for (int b = 0; b < 2; ++b)
            HIP_OK(launch_zgemm(false, false, rows, chir, chim, m->t[q], chim, m->t[q + 1] + (size_t)b * chim * chir, chir,
                                m->theta + (size_t)b * chir, cols, st));
        HIP_OK(launch_mps_theta(m->theta, lam_left, chil, chir, g16, mode, m->work, st));
    }
    std::vector<double> sigma;
    if (jacobi_svd(m->svd, m->work, wrows, m->vmat, wcols, st, sigma, &m->last_sweeps)) return 1;
    // order, rank and truncation (host: wcols numbers)
    std::vector<int> ord(wcols);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return sigma[a] > sigma[b]; });
    std::vector<double> sorted(wcols);
    for (int j = 0; j < wcols; ++j) sorted[j] = sigma[ord[j]];
    int k = 0;
    double dropped = 0.0;   // floor, max_bond, tail: the rule of aqc_mps_ent_rule.h
    if (!mps_rank_rule(wcols, sorted.data(), trunc_thr, max_bond, &k, &dropped)) return failf("2-qubit gate produced a zero or non-finite state");
    double total = 0.0;
    for (int j = 0; j < wcols; ++j) total += sorted[j] * sorted[j];
    double kept = 0.0;
    for (int j = 0; j < k; ++j) kept += sigma[ord[j]] * sigma[ord[j]];
    const double rescale = kept > 0.0 ? std::sqrt(total / kept) : 1.0;   // keep the norm of the state
    m->discarded += total - kept;
    // new tensors
    // theta has consumed the old site tensors: the new ones go into the same (grow-only) buffers
    if (reserve_site(m, q, (size_t)rows * k) || reserve_site(m, q + 1, (size_t)k * cols)) return 1;
    const size_t lam_off = (sizeof(int) * (size_t)wcols + 15) & ~(size_t)15;
    if (m->ord.reserve(lam_off + sizeof(double) * (size_t)wcols) || reserve_lambda(m, q, (size_t)k)) return 1;
    // column order and new Schmidt values go up through the pinned staging buffer of this gate: asynchronous, no wait (the
    // one synchronisation of a gate is the read-back of its singular values in jacobi_svd)
    void* stage = nullptr;
    if (stage_buffer(m, lam_off + sizeof(double) * (size_t)k, &stage)) return 1;
    memcpy(stage, ord.data(), sizeof(int) * wcols);
    double* h_lam = reinterpret_cast<double*>(static_cast<char*>(stage) + lam_off);
    std::vector<double>& lam = m->lam[q];
    lam.resize(k);
    for (int j = 0; j < k; ++j) h_lam[j] = lam[j] = sigma[ord[j]] * rescale;
    // ONE upload (column order | new Schmidt values); the split kernel copies the latter into the bond's vector
    HIP_OK(hipMemcpyAsync(m->ord, stage, lam_off + sizeof(double) * (size_t)k, hipMemcpyHostToDevice, st));
    HIP_OK(launch_mps_split(m->work, m->vmat, reinterpret_cast<int*>((char*)m->ord), m->svd.sigma, lam_left, chil, chir, k,
                            mode, rescale, m->t[q], m->t[q + 1], reinterpret_cast<const double*>(m->ord + lam_off),
                            m->d_lam[q], st));
    m->dims[q + 1] = k;
    return 0;
}

int gate1_site(aqc_mps* m, int q, const double* g8) {
    HIP_OK(launch_gate1q(m->t[q], m->t[q], 1, (size_t)m->dims[q] * m->dims[q + 1], 0, g8, m->stream));
    return 0;
}

// one routed 2-qubit op on the sites (q, q + 1)
int gate2_site(aqc_mps* m, int q, const LaneGate2& g, const double* th, double trunc_thr, int max_bond) {
    double g32[32];
    gate2_matrix(g, th, g32);
    return gate_adjacent(m, q, g32, trunc_thr, max_bond);
}

// 4x4 gate (index 2 * bit_ctrl + bit_targ) on any pair of qubits, routed by route_pair (aqc_mps_walk.h)
int gate2_pair(aqc_mps* m, int ctrl, int targ, const double* gate, double trunc_thr, int max_bond) {
    static const double swap_gate[32] = {1, 0, 0, 0, 0, 0, 0, 0,  0, 0, 0, 0, 1, 0, 0, 0,  0, 0, 1, 0, 0, 0, 0, 0,  0, 0, 0, 0, 0, 0, 1, 0};
    for (const RouteStep& r : route_pair(ctrl, targ)) {
        double g[32];
        if (!r.swap) permute_gate(gate, r.flip != 0, g);
        if (gate_adjacent(m, r.q, r.swap ? swap_gate : g, trunc_thr, max_bond)) return 1;
    }
    return 0;
}

// ---- the ansatz, gate by gate (host side of aqc_mps_apply_circuit / aqc_mps_fast_dot_gradient): executors of the lists of aqc_mps_walk.h
int gate1(aqc_mps* m, int q, const M2& g) { double g8[8]; pack(g, g8); return gate1_site(m, q, g8); }

int apply_circuit(aqc_mps* m, const aqc_circuit* c, const double* th, bool inverse, double trunc_thr, int max_bond) {
    for (const CircuitOp& op : circuit_ops(c, m->n, inverse))
        if (op.two ? gate2_site(m, op.op2.q, op.op2.g, th, trunc_thr, max_bond) : gate1(m, op.op1.q, gate1_matrix(op.op1.g, th))) return 1;
    return 0;
}

// The single-lane executor of the gradient walk (aqc_mps_gradwalk.h: validity of the environments, the chain of an inner product and
// the step driver are stated there): the buffers of L[q] ([chi_w][chi_z]) and Rc[q] (the CONJUGATE of the contraction of the sites > q),
// the two site steps and the gates of a step.
struct Environments {
    aqc_mps* w; aqc_mps* z;
    const aqc_circuit* c; const double* th; double trunc_thr; int max_bond;   // what the gates of a walk run with
    int n, nvals;
    std::vector<DevBuf<double2>> L, R;
    DevBuf<double2> t, e[2], bsite, vals;
    hipStream_t st;
    int init(aqc_mps* w_, aqc_mps* z_, int nvals_) {
        w = w_; z = z_; n = w->n; st = w->stream; nvals = std::max(nvals_, 1);
        L.resize(n + 1); R.resize(n);
        const double one[2] = {1.0, 0.0};
        if (L[0].reserve(1) || R[n - 1].reserve(1) || vals.reserve(nvals)) return 1;
        HIP_OK(hipMemcpyAsync(L[0], one, sizeof one, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(R[n - 1], one, sizeof one, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        return 0;
    }
    // the two site steps (env_left / env_right of aqc_mps_host.h), `op` an operator on w's side; the gemm form alone takes t and bsite
    int step_left(int p, const double2* in, const M2* op, DevBuf<double2>& out) {
        const SiteDims d = site_dims(w->dims.data(), z->dims.data(), p);
        const bool gemm = !mps_env_fits_small(d.xa, d.ua, d.yb, d.vb);
        if (gemm && ((op && bsite.reserve((size_t)2 * d.yb * d.vb)) || t.reserve((size_t)d.xa * d.vb))) return 1;
        if (out.reserve((size_t)d.ua * d.vb)) return 1;
        double g8[8];
        return env_left(st, in, w->t[p], z->t[p], d, adjoint8(op, g8), bsite, t, out);
    }
    int left(int p) { return step_left(p, L[p], nullptr, L[p + 1]); }
    int right(int p) {
        const SiteDims d = site_dims(w->dims.data(), z->dims.data(), p);
        if (!mps_env_fits_small(d.xa, d.ua, d.yb, d.vb) && t.reserve((size_t)d.ua * d.yb)) return 1;
        if (R[p - 1].reserve((size_t)d.xa * d.yb)) return 1;
        return env_right(st, R[p], w->t[p], z->t[p], d, t, R[p - 1]);
    }
    int chain(int p, bool first, int k, const M2* op) { return step_left(p, first ? L[p] : e[k ^ 1], op, e[k]); }
    int close(int hi, int k, int slot) {
        if (slot >= nvals) return failf("inner-product slot out of range");
        HIP_OK(launch_mps_env_dot(e[k], R[hi], (size_t)w->dims[hi + 1] * z->dims[hi + 1], vals + slot, st));
        return 0;
    }
    int entangle(const GradStep& s) {   // z takes it before w
        double ent[32];
        entangler_matrix(c->entangler, s.ent.idx >= 0 ? s.ent.scale * th[s.ent.idx] : 0.0, ent);
        return gate2_pair(z, s.q, s.q2, ent, trunc_thr, max_bond) || gate2_pair(w, s.q, s.q2, ent, trunc_thr, max_bond);
    }
    int rotate(int q, const LaneGate1& g1) {
        const M2 g = gate1_matrix(g1, th);
        return gate1(w, q, g) || gate1(z, q, g);
    }
    int rotate_recorded(PairEnvs& env, const GradStep& s, int slot) { return rotate_recorded_stepwise(*this, env, s, slot); }
};

int fast_dot_gradient(const aqc_circuit* c, aqc_mps* w, aqc_mps* z, const double* th, double trunc_thr, int max_bond, int lo_blk, int hi_blk,
                      bool front_layer, double* grad) {
    const int n = w->n;
    const WalkSizes sz = walk_sizes(c, n);
    GradRecords rec;
    rec.reserve(sz.max_records);
    Environments ex;
    ex.c = c; ex.th = th; ex.trunc_thr = trunc_thr; ex.max_bond = max_bond;
    if (ex.init(w, z, sz.max_records)) return 1;
    PairEnvs env;
    env.reset(n);
    if (gradient_walk(ex, env, gradient_steps(c, n, lo_blk, hi_blk, front_layer), 0, rec)) return 1;
    std::vector<cd> vals(rec.size());
    if (!rec.empty() && hipMemcpyAsync(vals.data(), ex.vals, sizeof(cd) * rec.size(), hipMemcpyDeviceToHost, ex.st) != hipSuccess) return failf("gradient download failed");
    if (hipStreamSynchronize(ex.st) != hipSuccess) return failf("stream synchronisation failed");
    assemble_gradient(rec, vals.data(), sz.T, reinterpret_cast<cd*>(grad));
    return 0;
}

}  // namespace

int aqc::mps_peek(const aqc_mps* m, int q, const void** site, const double** lam) {
    if (!m || q < 0 || q >= m->n) return failf("mps_peek: invalid argument");
    HIP_OK(hipStreamSynchronize(m->stream));
    *site = m->t[q];
    *lam = q < m->n - 1 ? (double*)m->d_lam[q] : nullptr;
    return 0;
}

int aqc::mps_view(const aqc_mps* m, int* dims, const double2** sites) {
    if (!m || !dims || !sites) return failf("mps_view: invalid argument");
    HIP_OK(hipStreamSynchronize(m->stream));
    for (int q = 0; q <= m->n; ++q) dims[q] = m->dims[q];
    for (int q = 0; q < m->n; ++q) sites[q] = m->t[q];
    return 0;
}

hipStream_t aqc::mps_stream(const aqc_mps* m) { return m->stream; }

int aqc::mps_adopt(int device, int n, const int* dims, const void* const* sites, const double* const* lams, double discarded, aqc_mps** out) {
    aqc_mps* m = nullptr;
    if (new_mps(device, n, &m)) return 1;
    m->dims.assign(dims, dims + n + 1);
    m->discarded = discarded;
    for (int q = 0; q < n; ++q) {
        const size_t ne = site_elems(m, q);
        if (reserve_site(m, q, ne) || hipMemcpyAsync(m->t[q], sites[q], sizeof(double2) * ne, hipMemcpyDeviceToDevice, m->stream) != hipSuccess) {
            destroy(m);
            return failf("MPS copy failed");
        }
        if (q < n - 1) {
            std::vector<double> lam(dims[q + 1]);
            if (hipMemcpy(lam.data(), lams[q], sizeof(double) * lam.size(), hipMemcpyDeviceToHost) != hipSuccess || set_lambda(m, q, lam)) {
                destroy(m);
                return failf("MPS copy failed");
            }
        }
    }
    if (hipStreamSynchronize(m->stream) != hipSuccess) { destroy(m); return failf("MPS copy failed"); }
    *out = m;
    return 0;
}

extern "C" {

int aqc_mps_create(int device, int n, const int32_t* dims, const double* gammas, const double* lambdas, aqc_mps** out) {
    if (!dims || !gammas || !out || (n > 1 && !lambdas)) return failf("null MPS argument");
    if (n < 1) return failf("number of qubits out of range");
    if (dims[0] != 1 || dims[n] != 1) return failf("MPS boundary bond dimensions must be 1");
    for (int q = 0; q <= n; ++q) if (dims[q] < 1) return failf("MPS bond dimensions must be positive");
    aqc_mps* m = nullptr;
    if (new_mps(device, n, &m)) return 1;
    m->dims.assign(dims, dims + n + 1);
    size_t off = 0, loff = 0;
    for (int q = 0; q < n; ++q) {
        const size_t ne = site_elems(m, q);
        if (reserve_site(m, q, ne) ||
            hipMemcpyAsync(m->t[q], gammas + 2 * off, sizeof(double2) * ne, hipMemcpyHostToDevice, m->stream) != hipSuccess) {
            destroy(m);
            return failf("MPS upload failed");
        }
        off += ne;
        if (q < n - 1) {
            std::vector<double> lam(lambdas + loff, lambdas + loff + dims[q + 1]);
            loff += dims[q + 1];
            for (double v : lam) if (!(v > 0.0)) { destroy(m); return failf("MPS Schmidt coefficients must be positive"); }
            if (set_lambda(m, q, lam)) { destroy(m); return 1; }
            if (launch_mps_colscale(m->t[q], m->d_lam[q], (size_t)2 * dims[q], dims[q + 1], 1, m->stream) != hipSuccess) { destroy(m); return failf("MPS scale failed"); }
        }
    }
    if (hipStreamSynchronize(m->stream) != hipSuccess) { destroy(m); return failf("MPS upload failed"); }
    *out = m;
    return 0;
}

int aqc_mps_destroy(aqc_mps* m) {
    destroy(m);
    return 0;
}

int aqc_mps_clone(const aqc_mps* src, aqc_mps** out) {
    if (!src || !out) return failf("null argument");
    aqc_mps* m = nullptr;
    if (new_mps(src->device, src->n, &m)) return 1;
    m->dims = src->dims;
    m->discarded = src->discarded;
    for (int q = 0; q < src->n; ++q) {
        const size_t bytes = sizeof(double2) * site_elems(src, q);
        if (reserve_site(m, q, site_elems(src, q)) || hipMemcpy(m->t[q], src->t[q], bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
            destroy(m);
            return failf("MPS clone failed");
        }
        if (q < src->n - 1 && set_lambda(m, q, src->lam[q])) { destroy(m); return 1; }
    }
    *out = m;
    return 0;
}

int aqc_mps_num_qubits(const aqc_mps* m) { return m ? m->n : -1; }
int aqc_mps_device(const aqc_mps* m) { return m ? m->device : -1; }

int aqc_mps_dims(const aqc_mps* m, int32_t* dims) {
    if (!m || !dims) return failf("null argument");
    for (int q = 0; q <= m->n; ++q) dims[q] = m->dims[q];
    return 0;
}

double aqc_mps_discarded_weight(const aqc_mps* m) { return m ? m->discarded : -1.0; }

/* Gamma_q = T_q / lambda_q and the lambdas, packed like the inputs of aqc_mps_create */
int aqc_mps_export(aqc_mps* m, double* gammas, double* lambdas) {
    if (!m || !gammas || (m->n > 1 && !lambdas)) return failf("null argument");
    HIP_OK(hipSetDevice(m->device));
    size_t off = 0, loff = 0;
    for (int q = 0; q < m->n; ++q) {
        const size_t ne = site_elems(m, q);
        if (m->tmp.reserve(ne)) return 1;
        HIP_OK(hipMemcpyAsync(m->tmp, m->t[q], sizeof(double2) * ne, hipMemcpyDeviceToDevice, m->stream));
        if (q < m->n - 1) {
            HIP_OK(launch_mps_colscale(m->tmp, m->d_lam[q], (size_t)2 * m->dims[q], m->dims[q + 1], 0, m->stream));
            std::memcpy(lambdas + loff, m->lam[q].data(), sizeof(double) * m->lam[q].size());
            loff += m->lam[q].size();
        }
        HIP_OK(hipMemcpyAsync(gammas + 2 * off, m->tmp, sizeof(double2) * ne, hipMemcpyDeviceToHost, m->stream));
        HIP_OK(hipStreamSynchronize(m->stream));
        off += ne;
    }
    return 0;
}

int aqc_mps_gate1(aqc_mps* m, int qubit, const double* gate) {
    if (!m || !gate) return failf("null argument");
    if (qubit < 0 || qubit >= m->n) return failf("qubit out of range");
    HIP_OK(hipSetDevice(m->device));
    return gate1_site(m, qubit, gate);
}

/* 4x4 gate (index 2 * bit_ctrl + bit_targ) on any pair of qubits */
int aqc_mps_gate2(aqc_mps* m, int ctrl, int targ, const double* gate, double trunc_thr, int max_bond) {
    if (!m || !gate) return failf("null argument");
    if (ctrl < 0 || ctrl >= m->n || targ < 0 || targ >= m->n || ctrl == targ) return failf("invalid qubit pair");
    if (!(trunc_thr >= 0.0)) return failf("trunc_thr must be non-negative");
    HIP_OK(hipSetDevice(m->device));
    return gate2_pair(m, ctrl, targ, gate, trunc_thr, max_bond);
}

/* V(thetas)|mps> (inverse = 0) or V(thetas)^H|mps> (inverse = 1) in place, the whole ansatz in one call
 * (mps_operations.py:326-371: v_mul_mps / v_dagger_mul_mps) */
int aqc_mps_apply_circuit(aqc_mps* m, const aqc_circuit* circ, const double* thetas, int inverse, double trunc_thr, int max_bond) {
    if (!m || !thetas) return failf("null argument");
    if (check_circuit(circ, m->n)) return 1;
    if (!(trunc_thr >= 0.0)) return failf("trunc_thr must be non-negative");
    HIP_OK(hipSetDevice(m->device));
    return apply_circuit(m, circ, thetas, inverse != 0, trunc_thr, max_bond);
}

/* complex gradient of <V lvec|phi> given vh_phi = V^H|phi>, the whole gate-by-gate walk in one call
 * (mps_dot_objective.py:41-242 fast_dot_gradient); block_from < 0: all blocks.  The operands are left intact. */
int aqc_mps_fast_dot_gradient(const aqc_circuit* circ, const aqc_mps* lvec, const aqc_mps* vh_phi, const double* thetas, double trunc_thr,
                              int max_bond, int block_from, int block_to, int front_layer, double* grad) {
    if (!lvec || !vh_phi || !thetas || !grad) return failf("null argument");
    if (lvec->n != vh_phi->n || lvec->device != vh_phi->device) return failf("MPS operands differ in size or device");
    if (check_circuit(circ, lvec->n)) return 1;
    if (!(trunc_thr >= 0.0)) return failf("trunc_thr must be non-negative");
    if (check_block_range(circ, block_from, block_to)) return 1;
    HIP_OK(hipSetDevice(lvec->device));
    aqc_mps *w = nullptr, *z = nullptr;
    if (aqc_mps_clone(lvec, &w)) return 1;
    if (aqc_mps_clone(vh_phi, &z)) { destroy(w); return 1; }
    (void)hipStreamDestroy(z->stream);   // one stream orders the gates on both operands and the environments
    z->stream = w->stream;
    z->owns_stream = false;
    const int rc = fast_dot_gradient(circ, w, z, thetas, trunc_thr, max_bond, block_from, block_to, front_layer != 0, grad);
    destroy(z);
    destroy(w);
    return rc;
}

/* <(prod_i G_i on qubit_i) a | b> by transfer matrices (mps_dot, mps_operations.py:192-213; with one Pauli this is
 * the 0.5j<P w|z> of mps_dot_objective.py:471-516 without building P.w).  G_i acts on a's side, so site qubit_i of b
 * is read through G_i^H: <G a|b> = <a|G^H b>.  nops = 0: plain <a|b>. */
int aqc_mps_dot_ops(aqc_mps* a, aqc_mps* b, int nops, const int32_t* qubits, const double* gates, double* out) {
    if (!a || !b || !out || nops < 0 || (nops > 0 && (!qubits || !gates))) return failf("invalid argument");
    if (a->n != b->n || a->device != b->device) return failf("MPS operands differ in size or device");
    HIP_OK(hipSetDevice(a->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    hipStream_t st = a->stream;
    const int n = a->n;
    std::vector<int> op_of(n, -1);
    for (int i = 0; i < nops; ++i) {
        if (qubits[i] < 0 || qubits[i] >= n || op_of[qubits[i]] >= 0) return failf("operator qubits must be distinct and in range");
        op_of[qubits[i]] = i;
    }
    const size_t need = overlap_scratch_elems(n, a->dims.data(), b->dims.data());
    size_t site_max = 1;
    for (int q = 0; q < n; ++q)
        if (op_of[q] >= 0) site_max = std::max(site_max, site_elems(b, q));
    if (a->tmp.reserve((3 * need + site_max))) return 1;
    double2* e = a->tmp;
    double2* bsite = e + 3 * need;
    StreamOps ops{st};
    auto a_site = [&](int q) { return (const double2*)a->t[q]; };
    auto b_site = [&](int q) {   // site q of b, seen through G^H when an operator sits there
        const M2 g = op_of[q] >= 0 ? unpack(gates + 8 * (size_t)op_of[q]) : M2{};
        double gh8[8];
        return site_through(st, b->t[q], (size_t)b->dims[q] * b->dims[q + 1], adjoint8(op_of[q] >= 0 ? &g : nullptr, gh8), bsite);
    };
    const double2* res = overlap_chain(ops, n, a->dims.data(), b->dims.data(), a_site, b_site, e, e + need, e + 2 * need);
    if (!res) return 1;
    HIP_OK(hipMemcpyAsync(out, res, sizeof(double2), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}

int aqc_mps_dot(aqc_mps* a, aqc_mps* b, double* out) { return aqc_mps_dot_ops(a, b, 0, nullptr, nullptr, out); }

/* A (m x n, row-major, host) = U diag(S) Vh with k = min(m, n), S descending; U (m x k), Vh (k x n) row-major.
 * The SVD kernel of the MPS engine, exposed for testing and for callers that need a device SVD. */
int aqc_svd(int device, int m, int n, const double* a_in, double* u_out, double* s_out, double* vh_out, int* sweeps) {
    if (!a_in || !u_out || !s_out || !vh_out || m < 1 || n < 1) return failf("invalid SVD arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return failf("no HIP device available: the aqc_hip path has no CPU fallback");
    if (device < 0 || device >= ndev) return failf("device out of range");
    HIP_OK(hipSetDevice(device));
    const int mode = n <= m ? 0 : 1, k = std::min(m, n);
    const int wrows = mode == 0 ? m : n, wcols = k;
    const size_t na = (size_t)m * n;
    DevBuf<double2> da, dw, dv, du, dvh;
    DevBuf<int> dord;
    DevBuf<double> dss;
    SvdWork sw;
    std::vector<double> sigma;
    int rc = 1;
    hipStream_t st = nullptr;
    HIP_OK(hipStreamCreate(&st));   // the rounds are many short dependent launches: keep them off the legacy default stream
    do {
        if (da.reserve(na) || dw.reserve(na) || dv.reserve((size_t)wcols * wcols) ||
            du.reserve((size_t)m * k) || dvh.reserve((size_t)k * n) || dord.reserve(k) ||
            dss.reserve(k)) break;
        if (hipMemcpy(da, a_in, sizeof(double2) * na, hipMemcpyHostToDevice) != hipSuccess) { failf("SVD upload failed"); break; }
        if (launch_svd_load(da, m, n, mode, dw, st) != hipSuccess) { failf("SVD load kernel failed"); break; }
        if (jacobi_svd(sw, dw, wrows, dv, wcols, st, sigma, sweeps)) break;
        std::vector<int> ord(wcols);
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return sigma[x] > sigma[y]; });
        if (hipMemcpy(dord, ord.data(), sizeof(int) * k, hipMemcpyHostToDevice) != hipSuccess) { failf("SVD upload failed"); break; }
        if (launch_svd_assemble(dw, dv, dord, sw.sigma, m, n, k, mode, du, dvh,
                                dss, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { failf("SVD assemble kernel failed"); break; }
        if (hipMemcpy(u_out, du, sizeof(double2) * (size_t)m * k, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(vh_out, dvh, sizeof(double2) * (size_t)k * n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(s_out, dss, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess) { failf("SVD download failed"); break; }
        rc = 0;
    } while (false);
    (void)hipStreamDestroy(st);
    return rc;
}

}  // extern "C"
