/*
 * aqc_hip.h -- C ABI of the MI355X-native fidelity/gradient path of aqc-research.
 *
 * The reference (qiskit-community/aqc-research v0.1.0) has no FFI: the boundary
 * of this path is a set of Python functions and duck-typed objective objects.
 * Each entry point below names the reference interface it replaces (file:line
 * relative to the reference tree); INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - complex128 arrays travel as interleaved (re, im) doubles;
 *   - qubit q is bit q of the amplitude index (Qiskit order,
 *     core_operations.py:34-43); a (d, k) matrix is row-major
 *     (core_op_matrix.py:56);
 *   - blocks is int32[2][L] row-major: row 0 = control, row 1 = target
 *     (parametric_circuit.py:24-70);
 *   - every function returns 0 on success; on failure a non-zero code is
 *     returned and aqc_last_error() gives the message (the ABI never throws
 *     and never calls back into the host language).  One code has a name:
 *     AQC_LANES_REFUSED, from the aqc_mpsb_* functions only (see below);
 *   - a context is immutable after creation and may be shared; a workspace
 *     owns one HIP device + one stream and is NOT thread-safe (one workspace
 *     per thread / process, exactly like the reference's one-objective-per-
 *     process model, job_executor.py:141).
 */
#ifndef AQC_HIP_H
#define AQC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aqc_ctx aqc_ctx; /* ansatz description + gate program (host only) */
typedef struct aqc_ws aqc_ws;   /* device-resident batch workspace            */

enum { AQC_CX = 0, AQC_CZ = 1, AQC_CP = 2 };
/* Status of an aqc_mpsb_* call that the lockstep lanes cannot do (a bond beyond their 32, in what was loaded or on the way; a lane's
 * SVD or state gone bad; no memory for the lanes): nothing was returned, and the single-lane engine (aqc_mps_*) may still do the
 * work -- the code a caller falls back on.  Every other failure is some other non-zero code and is final. */
enum { AQC_LANES_REFUSED = 3 };
/* device buffers of a workspace, each [batch][2^n][ncols] complex128: Y target, Z = V^H Y, X / X2 lhs states of the sweep,
 * W / ZW scratch of the sweep: what a sweep leaves there is unspecified (the register-blocked sweep, for one, walks w and z without
 * the lane sign that the cos >= 0 normalisation of the half angles drops -- it cancels in every inner product -- so its final w is
 * +-V x).  ZW doubles as the checkpoint of V^H: aqc_ws_apply(inverse, Y -> Z) leaves there the state before
 * its last stage, which is what the sweep's second stage takes as z when the lhs state is sparse (aqc_ws_set_basis /
 * aqc_ws_set_combo; grad_of_dot_product, core_operations.py:892-935, copies x into w: a one-hot x leaves w zero outside one tile
 * during the first stage).  One-call evaluations (aqc_ws_eval, aqc_ws_objective_launch, aqc_ws_surrogate_eval, aqc_ws_lbfgs) may
 * leave Z computed only on the tiles they read; any reader of AQC_BUF_Z through this interface completes it first, or fails
 * ("BUF_Z holds ...") once the thetas have changed since.  A writer of ZW completes such a Z before it overwrites the checkpoint.
 * A writer of some lanes of Z (aqc_ws_upload_lane, aqc_ws_copy_lane, aqc_ws_mps_to_vec[_batch]) completes the other lanes the
 * same way, or refuses with the readers' message; with batch 1 it writes the whole buffer and takes it over. */
enum { AQC_BUF_Y = 0, AQC_BUF_Z = 1, AQC_BUF_X = 2, AQC_BUF_W = 3, AQC_BUF_ZW = 4, AQC_BUF_X2 = 5, AQC_NUM_BUFS = 6 };
/* kernel families for aqc_ws_profile_get */
enum { AQC_K_APPLY = 0, AQC_K_SWEEP = 1, AQC_K_COEF = 2, AQC_K_FINALIZE = 3, AQC_K_MISC = 4,
       AQC_K_SWEEP_LIST = 5, AQC_K_APPLY_LIST = 6,   /* stage launches over a subset of the tiles (sparse lhs state / objective V^H) */
       AQC_K_PROJECT = 7, AQC_K_SWEEP_VIRTUAL = 8,   /* projected route: a pass over z / the target, the sweep's later stages on the virtual register, */
       AQC_K_APPLY_VIRTUAL = 9,                      /* their gates (or the inverses) applied to one virtual state (objective by projection) */
       AQC_NUM_KINDS = 10 };

const char* aqc_version(void);
const char* aqc_last_error(void);
/* number of visible HIP devices (0 when HIP is unusable); the reference's counterpart is
 * joblib's worker count, job_executor.py:136-143 */
int aqc_device_count(void);
/* live allocations behind this library's handles (workspaces, contexts' one-shot workspaces, MPS engines, lockstep lanes and the
 * calls' own temporaries): device blocks and pinned host blocks; either pointer may be null.  Every handle owns its memory, so
 * both counts return to their earlier values when a handle is destroyed -- the check of a leak test.  Process-wide, all devices;
 * the communicator's buffers are not counted. */
int aqc_live_buffers(int64_t* device, int64_t* pinned);

/* ---- ansatz description: ParametricCircuit / TrotterAnsatz
 *      (parametric_circuit.py:24-70,267-320; validity rules :234-254,391-423) */
int aqc_create(int num_qubits, int entangler, const int32_t* blocks, int num_blocks,
               int trotter, int second_order, aqc_ctx** out);
int aqc_destroy(aqc_ctx* ctx);
int aqc_num_thetas(const aqc_ctx* ctx);          /* parametric_circuit.py:108-112 */
int aqc_num_gate_groups(const aqc_ctx* ctx);     /* G = n + L_eff     */

/* ---- one-shot, host-pointer entry points (function-level drop-ins).
 * vec/out/x/vh_y: complex128[2^n]; grad: complex128[num_thetas]. */
/* core_operations.py:606  v_mul_vec(circ, thetas, vec, out, workspace) */
int aqc_v_mul_vec(aqc_ctx* ctx, const double* thetas, const double* vec, double* out);
/* core_operations.py:713  v_dagger_mul_vec(circ, thetas, vec, out, workspace) */
int aqc_vdag_mul_vec(aqc_ctx* ctx, const double* thetas, const double* vec, double* out);
/* core_operations.py:823  grad_of_dot_product(circ, thetas, x_vec, vh_y_vec, workspace,
 *                          block_range, front_layer); block_from<0 => full range */
int aqc_grad_dot_vec(aqc_ctx* ctx, const double* thetas, const double* x, const double* vh_y,
                     int block_from, int block_to, int front_layer, double* grad);
/* core_op_matrix.py:480 / :562  v_mul_mat / v_dagger_mul_mat(circ, thetas, mat, workspace);
 * mat: complex128[2^n][ncols], updated in place */
int aqc_v_mul_mat(aqc_ctx* ctx, const double* thetas, double* mat, int ncols);
int aqc_vdag_mul_mat(aqc_ctx* ctx, const double* thetas, double* mat, int ncols);
/* core_op_matrix.py:645  grad_of_matrix_dot_product(circ, thetas, x_mat, vh_y_mat, workspace);
 * unlike the reference the inputs are left intact (the Python shim reproduces the clobbering
 * contract where callers rely on it) */
int aqc_grad_dot_mat(aqc_ctx* ctx, const double* thetas, const double* x_mat, const double* vh_y_mat,
                     int ncols, double* grad);

/* ---- device-resident batch workspace: `batch` independent evaluations
 * (own thetas, own target) advance together in every launch.  This is what the
 * objective objects (objective_lhs_sur_max.py:82-191, sk_core.py:167-222) and
 * the job executor (job_executor.py:96) sit on.
 * ncols = 1 for state vectors, k for (2^n x k) matrices.
 * tile_bits_* = 0 selects the default LDS tile size. */
int aqc_ws_create(aqc_ctx* ctx, int device, int batch, int ncols, int tile_bits_apply,
                  int tile_bits_sweep, aqc_ws** out);
int aqc_ws_destroy(aqc_ws* ws);
int aqc_ws_set_thetas(aqc_ws* ws, const double* thetas /* [batch][T] */);
int aqc_ws_upload(aqc_ws* ws, int buf, const double* src /* [batch][2^n][ncols] c128 */);
int aqc_ws_upload_lane(aqc_ws* ws, int buf, int lane, const double* src);
int aqc_ws_broadcast(aqc_ws* ws, int buf, const double* src /* [2^n][ncols] c128, same for all lanes */);
int aqc_ws_download(aqc_ws* ws, int buf, double* dst);
int aqc_ws_download_lane(aqc_ws* ws, int buf, int lane, double* dst);
/* X_lane <- one-hot basis state |index[lane]>  (ThinStateHandler.init_state, objective_base.py:99-116) */
/* dst_ws.buf[dst_lane] <- src_ws.buf[src_lane] on the device (same device, same lane size; asynchronous on dst's stream) */
int aqc_ws_copy_lane(aqc_ws* dst_ws, int dst_buf, int dst_lane, aqc_ws* src_ws, int src_buf, int src_lane);
int aqc_ws_set_basis(aqc_ws* ws, int buf, const int64_t* index /* [batch] */);
/* buffer[lane] = coef[lane][0] |index[lane][0]> + coef[lane][1] |index[lane][1]> (index[lane][1] < 0: one term).  The
 * gradient of <V x|y> is conjugate-linear in x, so the two sweeps of the surrogate objective (|state_0> and the leading
 * flip state, objective_lhs_sur_max.py:147-155,167-175) combined as c_0 g_0 + c_max g_max are ONE sweep from
 * x = conj(c_0) |state_0> + conj(c_max) |state_max>. */
int aqc_ws_set_combo(aqc_ws* ws, int buf, const int64_t* index /* [batch][2] */, const double* coef /* [batch][2] c128 */);
/* X <- identity matrix (FullRangeSketchingVectors.generate, sk_core.py:317-326); needs ncols == 2^n (any other workspace is
 * refused: the buffer and the record of what it holds stay as they were) */
int aqc_ws_set_identity(aqc_ws* ws, int buf);
/* dst <- V src (inverse=0) or V^H src (inverse=1), per lane, with the lane's thetas */
int aqc_ws_apply(aqc_ws* ws, int inverse, int src_buf, int dst_buf);
/* grads <- complex gradient of <V X|Y> from X and Z = V^H Y (kept intact); W/ZW are scratch */
int aqc_ws_grad(aqc_ws* ws, int block_from, int block_to, int front_layer);
int aqc_ws_get_grads(aqc_ws* ws, double* grads /* [batch][T] c128 */);
/* out[lane][i] = buf[lane][index[i]], index[i] a flat element index of the lane's row-major [2^n][ncols] matrix, 0 <= index[i] <
 * 2^n ncols (ncols = 1: the amplitude index; ThinStateHandler.state_dot_vector, objective_base.py:166-177).  The registered set of
 * aqc_ws_gather_setup names rows: amplitudes of a state vector, column 0 of a matrix. */
int aqc_ws_gather(aqc_ws* ws, int buf, const int64_t* index, int count, double* out);
/* out[lane] = <a_lane|b_lane> (np.vdot; GenericStateHandler.state_dot_vector, sk_core.py:192) */
int aqc_ws_vdot(aqc_ws* ws, int buf_a, int buf_b, double* out /* [batch] c128 */);
int aqc_ws_sync(aqc_ws* ws);

/* ---- one-call evaluation: what objective(thetas) + gradient(thetas) of the objective objects need
 * (objective_lhs_sur_max.py:82-191), with a single host synchronisation:
 *   thetas -> device, coefficients, [Z = V^H Y], [gather of the amplitudes selected by
 *   aqc_ws_gather_setup from Z], [sweep with lhs buffer x_buf -> grads], results -> host.
 * Any of gathered / grads may be NULL to skip that part.  Host buffers are staged through pinned
 * memory owned by the workspace. */
int aqc_ws_eval(aqc_ws* ws, const double* thetas /* [batch][T] or NULL = keep */, int do_vdag,
                double* gathered /* [batch][count] c128 */, int x_buf, int block_from, int block_to,
                int front_layer, double* grads /* [batch][T] c128 */);
/* sweep with an explicit lhs buffer (aqc_ws_grad uses AQC_BUF_X) */
int aqc_ws_grad_from(aqc_ws* ws, int x_buf, int block_from, int block_to, int front_layer);

/* ---- fully asynchronous variants: inputs stay resident in HBM, nothing below synchronises.
 * A theta bank holds `nsets` parameter sets [nsets][batch][T]; selecting one only launches the
 * coefficient kernel.  Gathered amplitudes stay on the device until fetched. */
int aqc_ws_theta_bank(aqc_ws* ws, const double* thetas, int nsets);
int aqc_ws_use_theta_set(aqc_ws* ws, int set_index);
int aqc_ws_gather_setup(aqc_ws* ws, const int64_t* index, int count);
int aqc_ws_gather_launch(aqc_ws* ws, int buf);
int aqc_ws_gather_fetch(aqc_ws* ws, double* out /* [batch][count] c128 */);
int aqc_ws_vdot_launch(aqc_ws* ws, int buf_a, int buf_b);
int aqc_ws_vdot_fetch(aqc_ws* ws, double* out /* [batch] c128 */);
/* what the optimizer on the host reads after every evaluation (optimizer.py:579-590 consumes objective(theta) and
 * gradient(theta)): aqc_ws_results_async enqueues the copies of the gradients and of the gathered amplitudes (or of <A|B>
 * after aqc_ws_vdot_launch) into pinned host memory behind the kernels already on the stream, without synchronising;
 * aqc_ws_results_fetch waits for the stream and hands them out (either pointer may be NULL). */
int aqc_ws_results_async(aqc_ws* ws);
/* one evaluation of an objective with the thetas in use, enqueued and not waited for: Z = V^H Y (where the evaluation reads it),
 * the amplitudes registered with aqc_ws_gather_setup (if any; objective_lhs_sur_max.py:99-106), the sweep from x_buf
 * (:147-175).  Same results as aqc_ws_apply(1, Y, Z); aqc_ws_gather_launch(Z); aqc_ws_grad_from(x_buf, ...). */
int aqc_ws_objective_launch(aqc_ws* ws, int x_buf, int block_from, int block_to, int front_layer);
int aqc_ws_results_fetch(aqc_ws* ws, double* small_out /* [batch][count] c128 */, double* grads_out /* [batch][T] c128 */);

/* ---- MPS helpers (state-vector workspaces only).  An MPS arrives in the reference's QiskitMPS
 * layout (mps_operations.py:33,87-123): site q has Gamma^0, Gamma^1 of shape (dims[q], dims[q+1]),
 * dims[0] = dims[n] = 1, and lambda_q (float64[dims[q+1]]) for q < n-1.
 *   gammas : per site [2][dims[q]][dims[q+1]] complex128, sites concatenated
 *   lambdas: per site [dims[q+1]] float64, sites 0..n-2 concatenated
 * Upload folds lambda into the right bond of Gamma on the device (_preprocess_mps, :126-156). */
enum { AQC_MPS_SLOTS = 64 };   /* 0..3: explicit calls; the rest: resident copies managed by the host side (engine.py slot cache) */
int aqc_ws_mps_upload(aqc_ws* ws, int slot, const int32_t* dims /* [n+1] */, const double* gammas,
                      const double* lambdas);
/* buf[lane] <- dense state of the MPS; index bit q <-> site q   (mps_to_vector, :159-189) */
int aqc_ws_mps_to_vec(aqc_ws* ws, int slot, int buf, int lane);
/* the same for `count` (slot, lane) pairs; slots of equal bond dimensions (the lanes of a batched objective,
 * mps_dot_objective.py:41 called once per lane in the reference) share every launch of the contraction chain */
int aqc_ws_mps_to_vec_batch(aqc_ws* ws, int count, const int32_t* slots, int buf, const int32_t* lanes);
/* out <- <mps_a|mps_b> by transfer matrices                      (mps_dot, :192-213) */
int aqc_ws_mps_dot(aqc_ws* ws, int slot_a, int slot_b, double* out /* 1 c128 */);

/* ---- dense complex GEMM on the device: C (M x N) = op(A) B with op(A) = A (M x K) or A^H (A stored K x M),
 * row-major, host pointers.  Used by the sketching-vector generators (Y = U X, sk_core.py:357,463) and by
 * the MPS contractions internally. */
int aqc_zgemm(int device, int conj_trans_a, int M, int N, int K, const double* A, int lda, const double* B, int ldb,
              double* C, int ldc);

/* ---- gate-level building blocks, one pass per call over a (2^n x ncols) row-major c128 array in HOST memory
 * (ncols = 1: state vector).  Qubit numbers are bit indices of the row (Qiskit order); the Python shim converts
 * the big-endian `pos` of the state-vector functions (core_operations.py:34-43).  dst may equal src.
 * aqc_gate_1q: dst = (I x g x I) src, g = row-major 2x2 (4 c128)
 *   replaces gate2x2_mul_vec :46, proj00/11_mul_vec :122,:143, rx/ry/rz_mul_vec :164,:200,:236 of core_operations.py
 *   and rx/ry/rz_mul_mat :32,:66,:100, gate2x2_mul_mat :392 of core_op_matrix.py.
 * aqc_gate_2q: dst = (4x4 on the pair, index 2*bit_ctrl + bit_targ; 16 c128 row-major) src
 *   replaces cx/cz/cp_mul_vec :422,:468,:514, derv_cphase_mul_vec :561, block_mul_vec :354 (core_operations.py)
 *   and cx/cz/cp_mul_mat :130,:181,:232 (core_op_matrix.py).
 * aqc_gate_dot: kind 0 / 1 / 2 = 0.5j<Xw|z>, 0.5j<Yw|z>, 0.5j<Zw|z> on qubit q0 (dot_x/y/z :267,:296,:325;
 *   x/y/z_dot_mat :284,:320,:356); kind 3 = -1j<P11(q0,q1) w|z> (derv_cphase, core_op_matrix.py:430). */
int aqc_gate_1q(int device, int n, int64_t ncols, int qubit, const double* gate, const double* src, double* dst);
int aqc_gate_2q(int device, int n, int64_t ncols, int ctrl, int targ, const double* gate, const double* src, double* dst);
int aqc_gate_dot(int device, int n, int64_t ncols, int kind, int q0, int q1, const double* w, const double* z,
                 double* out /* 1 c128 */);

/* ---- XXZ chain Hamiltonian, matrix-free, and exact time evolution by a Chebyshev series: one-shot calls over [lanes][2^n] c128
 * state vectors in HOST memory (qubit q = index bit q), 2 <= n <= 30; dst may equal src.
 *   H = -1/4 sum_i (X_i X_i+1 + Y_i Y_i+1 + delta Z_i Z_i+1), open chain  (make_hamiltonian, trotter.py:183-230, without the matrix)
 *   exp(-i H t) psi = sum_k c_k T_k(H / R) psi,  R = (n - 1)(1/2 + |delta| / 4),  c_0 = J_0(R t),  c_k = 2 (-i)^k J_k(R t);
 *   the series ends at the smallest K >= ceil(|R t|) + 20 with |J_K| <= 1e-17: exact to rounding where the reference's
 *   exact_evolution (trotter.py:233-266, a dense expm) ends near 12 qubits.  The Bessel values are computed by the library
 *   (csrc/aqc_xxz_rule.h); one kernel launch per term; lanes with different times share the launches.
 * aqc_xxz_energy: energy[l] = Re <src_l| H |src_l>, summed in a fixed order.
 * aqc_xxz_evolve: dst[l] = exp(-i H times[l]) src[shared_src ? 0 : l]; terms_out (may be NULL) receives K per lane. */
int aqc_xxz_mul_vec(int device, int n, int lanes, double delta, const double* src, double* dst);
int aqc_xxz_energy(int device, int n, int lanes, double delta, const double* src, double* energy /* [lanes] f64 */);
int aqc_xxz_evolve(int device, int n, int lanes, int shared_src, double delta, const double* times /* [lanes] */, const double* src,
                   double* dst, int32_t* terms_out);

/* ---- reduced density matrices of up to 4 qubits of [lanes][2^n] c128 state vectors in HOST memory, 2 <= n <= 30 (inputs are only
 * read).  Convention: index bit q is qubit q; for listed qubits (q_0 .. q_k-1) the matrix's row index has bit m = the value of q_m,
 * rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b).  Every matrix is a partial trace of the 16 x 16 matrix of a set of 4 qubits,
 * a Gram product on the fp64 matrix cores; the plan (csrc/aqc_obs_rule.h) groups the sets into passes over the state: a pass is a
 * set of min(n, AQC_OBS_TILE_BITS) tile bits (the low AQC_OBS_LOW_BITS among them when n is larger) and carries at most
 * AQC_OBS_MAX_SUBSETS 4-subsets of it.  Sums run in a fixed order: two calls give the same bits, whatever the number of lanes.
 * aqc_obs_plan: host only, needs no device.  pairs [npairs][2] (two different qubits each, either order).  Outputs: *npasses and
 *   *nsubsets always; with max_passes >= *npasses and max_subsets >= *nsubsets (else an error) also pass_bits
 *   [max_passes][AQC_OBS_TILE_BITS] (the qubits of the pass ascending, -1 beyond), pass_nsub [max_passes], subsets [max_subsets][4]
 *   (tile-local positions ascending -- position j is the j-th lowest qubit of the pass; with n < 4 the positions n .. 3 are virtual
 *   qubits that are always 0 -- the subsets of pass 0 first) and serves [npairs][2] = the (pass, subset within the pass) a pair is
 *   read from, the first in plan order that holds it.
 * aqc_obs_rdm: out [lanes][nsets][2^k][2^k] c128 for the nsets >= 1 sets qubits [nsets][k] of 1 <= k <= min(4, n) different qubits. */
#define AQC_OBS_TILE_BITS 11
#define AQC_OBS_LOW_BITS 5
#define AQC_OBS_MAX_SUBSETS 16
int aqc_obs_plan(int n, int npairs, const int32_t* pairs, int max_passes, int max_subsets, int32_t* npasses, int32_t* nsubsets,
                 int32_t* pass_bits, int32_t* pass_nsub, int32_t* subsets, int32_t* serves);
int aqc_obs_rdm(int device, int n, int lanes, const double* src, int k, int nsets, const int32_t* qubits, double* out);

/* ---- device-resident MPS with truncated 2-qubit gates: the arithmetic the reference hands to qiskit-aer's
 * matrix_product_state simulator (mps_operations.py:216-298 mps_from_circuit / qcircuit_mul_mps; gate level:
 * mps_dot_objective.py:245-468).  Qiskit MPS format in and out (mps_operations.py:33): `dims` = n+1 bond
 * dimensions (dims[0] = dims[n] = 1), `gammas` = per site [2][dims[q]][dims[q+1]] c128 packed back to back,
 * `lambdas` = the n-1 Schmidt vectors packed back to back.  trunc_thr: the smallest singular values are dropped
 * while the sum of their squares stays below it (Aer's matrix_product_state_truncation_threshold); max_bond <= 0
 * means unlimited.  Aer's own arithmetic is third party: truncated results are parity unpinned. */
typedef struct aqc_mps aqc_mps;
int aqc_mps_create(int device, int n, const int32_t* dims, const double* gammas, const double* lambdas, aqc_mps** out);
int aqc_mps_destroy(aqc_mps* mps);
int aqc_mps_clone(const aqc_mps* src, aqc_mps** out);
int aqc_mps_num_qubits(const aqc_mps* mps);
int aqc_mps_device(const aqc_mps* mps);   /* the HIP device the state lives on */
int aqc_mps_dims(const aqc_mps* mps, int32_t* dims /* n+1 */);
double aqc_mps_discarded_weight(const aqc_mps* mps);
int aqc_mps_export(aqc_mps* mps, double* gammas, double* lambdas);
/* {x,y,z,rx,ry,rz}_mul_mps (mps_dot_objective.py:245-377): 2x2 gate, row-major 4 c128 */
int aqc_mps_gate1(aqc_mps* mps, int qubit, const double* gate);
/* {cx,cp,cz}_mul_mps (:380-468) and any other 4x4 (index 2*bit_ctrl + bit_targ, 16 c128) on any qubit pair */
int aqc_mps_gate2(aqc_mps* mps, int ctrl, int targ, const double* gate, double trunc_thr, int max_bond);
/* <a|b>  (mps_dot, mps_operations.py:192-213) */
int aqc_mps_dot(aqc_mps* a, aqc_mps* b, double* out /* 1 c128 */);
/* <(prod_i G_i on qubits[i]) a|b> without forming G.a: dot_{x,y,z} (mps_dot_objective.py:471-516) up to the factor
 * 0.5j with one Pauli; two projectors |1><1| give the CPhase derivative term.  gates: nops 2x2 matrices (4 c128 each) */
int aqc_mps_dot_ops(aqc_mps* a, aqc_mps* b, int nops, const int32_t* qubits, const double* gates, double* out);
/* Two-qubit reduced density matrices of one or several MPS states in one call (rules: csrc/aqc_mps_obs_rule.h, kernels:
 * csrc/aqc_mps_obs.hip).  Convention of aqc_obs_rdm: for the pair (i, j) the row index is value(i) + 2 value(j),
 * rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b); no normalisation (tr rho = <psi|psi>); states are taken in whatever gauge they
 * are in and are not modified.  All pairs with the same lower qubit i share one chain that walks from site i to the farthest
 * requested partner and emits a matrix at every requested j; a pair given as (j, i), j > i, is the matrix of (i, j) with its two
 * index bits transposed.  Every matrix is exactly Hermitian with an exactly real diagonal, sums run in a fixed order, and a pair's
 * matrix does not depend on which other pairs or states are in the call.
 * aqc_mps_obs_plan: host only, needs no device.  pairs [npairs][2].  Outputs: chain_last [n] = the last site the chain that starts
 *   at a site walks to (-1: none starts there), *nemits = the number of different (chain, site) emissions, serves [npairs][3] =
 *   (chain, emitting site, 1 if the pair was given as (higher, lower)).
 * aqc_mps_obs_route: the route the rule picks for bond dimensions dims [n + 1]: AQC_MPS_OBS_FUSED when every one is at most
 *   AQC_MPS_OBS_FUSED_CAP, else AQC_MPS_OBS_GEMM (-1: invalid argument).
 * aqc_mps_obs_pairs: out [nstates][npairs][4][4] c128.  method: AQC_MPS_OBS_BY_RULE (per state), AQC_MPS_OBS_FUSED (an error when a
 *   bond exceeds the cap) or AQC_MPS_OBS_GEMM.  The states share n >= 2 and the device; the work is ordered on the first state's
 *   stream after the others' have drained. */
#define AQC_MPS_OBS_BY_RULE 0
#define AQC_MPS_OBS_FUSED 1
#define AQC_MPS_OBS_GEMM 2
#define AQC_MPS_OBS_FUSED_CAP 64
int aqc_mps_obs_plan(int n, int npairs, const int32_t* pairs, int32_t* chain_last, int32_t* nemits, int32_t* serves);
int aqc_mps_obs_route(int n, const int32_t* dims);
int aqc_mps_obs_pairs(aqc_mps* const* states, int nstates, int npairs, const int32_t* pairs, int method, double* out);
/* Measurement of one or several MPS states in the computational basis (rules: csrc/aqc_mps_sample_rule.h, kernels:
 * csrc/aqc_mps_sample.hip): shots drawn from |psi(b)|^2 by perfect sampling along the chain, and the amplitudes psi(b) of given bit
 * strings.  bits[s][q] is the value of qubit q (= site q = index bit q of the dense vector).  Nothing is rescaled: an amplitude is that
 * of the state as it is, and p(b) = |psi(b)|^2 / norm2 with norm2 = <psi|psi>.  The uniform of shot s, qubit q of lane l (the position
 * of the state in the call) is word q % 4 of philox4x64_10(counter = {1 + q / 4, first_shot + s, l, 0}, key = {seed,
 * AQC_SAMPLE_STREAM}) as a double of [0, 1): a shot depends on (state, seed, lane, shot number) alone.  A branch of zero weight is
 * never taken; weights that do not add up to a finite positive number fail the call with the lane and the shot named.  States are taken
 * in whatever gauge they are in and are not modified; they share n >= 1 and the device; the work is ordered on the first state's stream
 * after the others' have drained.
 * sample_route: the route the rule picks for bond dimensions dims [n + 1]: AQC_MPS_SAMPLE_FUSED (64 shots per workgroup walk the whole
 *   chain inside one launch) when every one is at most AQC_MPS_SAMPLE_FUSED_CAP, else AQC_MPS_SAMPLE_GEMM (-1: invalid argument).
 * sample: 1 <= shots <= 2^24.  bits [nstates][shots][n]; amps [nstates][shots] c128 (psi of the sampled strings) and norm2 [nstates] may
 *   be NULL.  method: AQC_MPS_SAMPLE_BY_RULE (per state), _FUSED (an error when a bond exceeds the cap) or _GEMM.
 * amplitudes: bits [count][n] of 0 / 1, shared by the states; amps [nstates][count] c128. */
#define AQC_MPS_SAMPLE_BY_RULE 0
#define AQC_MPS_SAMPLE_FUSED 1
#define AQC_MPS_SAMPLE_GEMM 2
#define AQC_MPS_SAMPLE_FUSED_CAP 64
#define AQC_SAMPLE_STREAM 16 /* Philox key word of the measurement draws; the sketching generators use AQC_SKETCH_* = 0, 1, 2 */
int aqc_mps_sample_route(int n, const int32_t* dims);
int aqc_mps_sample(aqc_mps* const* states, int nstates, int64_t shots, uint64_t first_shot, uint64_t seed, int method,
                   uint8_t* bits /* [nstates][shots][n] */, double* amps /* [nstates][shots] c128, may be null */,
                   double* norm2 /* [nstates], may be null */);
int aqc_mps_amplitudes(aqc_mps* const* states, int nstates, int64_t count, const uint8_t* bits /* [count][n], shared by the states */,
                       int method, double* amps /* [nstates][count] c128 */);
/* Pauli strings between MPS states, many strings and pairs of states per call (rules: csrc/aqc_mps_pauli_rule.h, kernels:
 * csrc/aqc_mps_pauli.hip): out[p][s] = <bras[p]| P_s |kets[p]> with no normalisation.  strings [nstrings][n] of 0, 1, 2, 3 = I, X, Y, Z;
 * entry q acts on qubit q (= site q = index bit q of the dense vector).  bras NULL is expectation mode, <kets[p]| P_s |kets[p]>: a
 * string is walked over its support only, between the environments of the ket (one sweep per distinct ket).  States are taken in
 * whatever gauge they are in and are not modified; a state may be listed many times; they share n >= 1 and the device; the work is
 * ordered on the first ket's stream after the others' have drained.  A value does not depend on which other strings or pairs are in the
 * call.
 * pauli_route: the route the rule picks for a pair with bond dimensions bra_dims, ket_dims [n + 1] (bra_dims NULL: the ket's):
 *   AQC_MPS_PAULI_FUSED (one workgroup walks a whole string inside one launch) when every bond of both is at most
 *   AQC_MPS_PAULI_FUSED_CAP, else AQC_MPS_PAULI_GEMM (-1: invalid argument).
 * pauli_support: host only, needs no device.  first / last [nstrings]: the first and last non-identity site of each string (all
 *   identity: 0, 0).
 * pauli: method AQC_MPS_PAULI_BY_RULE (per pair), _FUSED (an error when a bond exceeds the cap) or _GEMM. */
#define AQC_MPS_PAULI_BY_RULE 0
#define AQC_MPS_PAULI_FUSED 1
#define AQC_MPS_PAULI_GEMM 2
#define AQC_MPS_PAULI_FUSED_CAP 64
int aqc_mps_pauli_route(int n, const int32_t* bra_dims /* null: the ket's */, const int32_t* ket_dims);
int aqc_mps_pauli_support(int n, int nstrings, const uint8_t* strings, int32_t* first, int32_t* last);
int aqc_mps_pauli(aqc_mps* const* bras /* null: expectation mode */, aqc_mps* const* kets, int npairs, int nstrings,
                  const uint8_t* strings /* [nstrings][n] */, int method, double* out /* [npairs][nstrings] c128 */);
/* Schmidt spectra of MPS states: the singular values of every cut q = 1 .. n - 1 (qubits 0 .. q-1 | q .. n-1) of one or many states per
 * call (rules: csrc/aqc_mps_ent_rule.h, kernels: csrc/aqc_mps_ent.hip).  States are taken in whatever gauge they are in and are not
 * modified; nothing is normalised: the squares of a cut's values add up to <psi|psi>.  A state may be listed many times; the states
 * share n >= 1 and the device; the fused work is ordered on the first state's stream after the others' have drained.  A state's values
 * do not depend on which other states are in the call.
 * ent_route: the route the rule picks for bond dimensions dims [n + 1]: AQC_MPS_ENT_FUSED (QR chains of the left and right factors
 *   inside one launch, then all cuts' SVDs in one batch) when every bond is at most AQC_MPS_ENT_FUSED_CAP, else AQC_MPS_ENT_CANONICAL (the
 *   engine's identity sweeps on a clone; the bond vectors, zero-padded) (-1: invalid argument).
 * ent_schmidt: method AQC_MPS_ENT_BY_RULE (per state), _FUSED (an error when a bond exceeds the cap) or _CANONICAL.  kmax: at least the
 *   largest bond dimension of the states.  s: descending, zero beyond chi_q; the whole row NaN where the state is not finite (status 2).
 *   status: 0 converged, 1 the SVD of the cut reached its sweep limit (without status that is an error), 2 not finite.  factors: per state
 *   in call order the block C_1 .. C_{n-1} then the block D_1 .. D_{n-1} (chi_q x chi_q c128 each, back to back), states of the fused
 *   route only: C_q^H C_q is the left environment of bond q, D_q^H D_q the conjugate of the right one.
 * rank_rule: host only, needs no device.  The engine's rank decision on a descending spectrum: the floor 1e-14 s[0], then max_bond
 *   (> 0), then the tail dropped while its weight stays below trunc_thr; dropped: the weight of that tail. */
#define AQC_MPS_ENT_BY_RULE 0
#define AQC_MPS_ENT_FUSED 1
#define AQC_MPS_ENT_CANONICAL 2
#define AQC_MPS_ENT_FUSED_CAP 64
int aqc_mps_ent_route(int n, const int32_t* dims);
int aqc_mps_ent_schmidt(aqc_mps* const* states, int nstates, int method, int kmax,
                        double* s /* [nstates][max(n-1,1)][kmax], zero beyond chi_q */,
                        int32_t* sweeps, int32_t* status /* [nstates][max(n-1,1)], may be null */,
                        double* factors /* may be null: C_q then D_q per state, fused route only */);
int aqc_mps_rank_rule(int count, const double* s /* descending */, double trunc_thr, int max_bond, int32_t* rank, double* dropped);
/* Compression of MPS states: canonical form and truncation of every bond, one or many states per call (rules:
 * csrc/aqc_mps_compress_rule.h, kernels: csrc/aqc_mps_compress.hip).  The states may be in any gauge, share n >= 1 and the device, and are
 * left as they are; out[i] is a NEW state (the caller destroys it) in the engine's gauge, its bond vectors the Schmidt values, every
 * bond cut left to right by the engine's rank rule at trunc_thr / max_bond (aqc_mps_rank_rule) with the rescaling of a truncating gate:
 * the sequence of decisions of canonicalisation followed by a sweep of truncating identity gates.  Its discarded weight is the
 * input's plus the weights the cuts dropped.  A state listed many times is compressed once; a state's result does not depend on
 * which other states are in the call.  n = 1 gives copies.
 * compress_route: AQC_MPS_ENT_FUSED (every state of the call advances through the sweep together, a workgroup per state, the rank
 *   decisions on the device, one synchronisation per call) when every bond is at most AQC_MPS_ENT_FUSED_CAP, else AQC_MPS_ENT_CANONICAL
 *   (the engine's identity sweeps and its truncating sweep on a clone) (-1: invalid argument).
 * compress: method AQC_MPS_ENT_BY_RULE (per state), _FUSED (an error when a bond exceeds the cap) or _CANONICAL.  ranks: the new bond
 *   dimension of every cut, 0 from the cut on at which a state failed; dropped: the weight each cut dropped (what the floor and max_bond
 *   took included); sweeps: of the cut's SVD (fused route; 0 on the canonical one); status per state: 0 compressed, 1 an SVD reached
 *   its sweep limit (fused route; on the canonical route the engine's gate reports that as an error and the call returns 1), 2 a zero
 *   or non-finite state -- such a state gets a null handle in out and the call still returns 0.  out is nulled before anything else
 *   can fail, so after an error it holds nothing to destroy.  ranks,
 *   dropped, sweeps and status may be null.  Argument errors (a negative or non-finite trunc_thr, a negative max_bond, states that differ
 *   in size or device, the fused route beyond its cap) are reported before any device work. */
int aqc_mps_compress_route(int n, const int32_t* dims);
/* bytes the stores of a step's batched SVD may take (default 256 MiB): the states of a call are swept in chunks that fit.  Sets it
 * (bytes <= 0: the default) and returns the earlier value; results do not depend on it.  For tests of the chunked sweep. */
int64_t aqc_mps_compress_svd_budget(int64_t bytes);
int aqc_mps_compress(aqc_mps* const* states, int nstates, double trunc_thr, int max_bond, int method, aqc_mps** out /* [nstates] */,
                     int32_t* ranks /* [nstates][n-1] */, double* dropped /* [nstates][n-1] */, int32_t* sweeps /* [nstates][n-1] */,
                     int32_t* status /* [nstates] */);
/* Linear combinations of MPS states: output j = sum over its terms of c_t psi_{term_state[t]}, t = term_off[j] .. term_off[j+1] - 1,
 * compressed; one or many outputs per call (rules: csrc/aqc_mps_combine_rule.h, kernel: csrc/aqc_mps_combine.hip, the sweep of
 * aqc_mps_compress).  The states may be in any gauge, share n >= 1 and the device, and are left bit for bit as they are; a state may
 * appear in several terms and several outputs.  The direct sum S of an output's terms (summed bonds Sigma_q = sum_k chi^k_q, the
 * coefficients on site 0, block-diagonal middle sites) is assembled on the device, and out[j] is compress(S, trunc_thr, max_bond) as
 * aqc_mps_compress states it: a NEW state (the caller destroys it) in the engine's gauge, every bond cut left to right by the engine's
 * rank rule, the same statuses.  Its discarded weight is what the cuts of THIS call dropped: the weights the terms carry are not taken
 * over.  Errors are of the size of rounding relative to scale = sum_k |c_k| |psi_k|, not to the norm of the result: an exact
 * cancellation is not detected (what is left of psi - psi is rounding of that size, normalised by the cuts' spectra as any state).
 * n = 1: the 2-vector sum_k c_k T^k_0.  An output's result does not depend on which other outputs are in the call.
 * combine_route: host only, needs no device.  dims: the bonds of one output's terms.  AQC_MPS_ENT_FUSED when every summed bond is at most
 *   AQC_MPS_ENT_FUSED_CAP (all outputs advance through one sweep together, one synchronisation per call), else AQC_MPS_ENT_CANONICAL
 *   (the assembled sum becomes an engine state with unit bond vectors and takes the canonical route of aqc_mps_compress)
 *   (-1: invalid argument).
 * combine_svd_budget: as aqc_mps_compress_svd_budget, for this call.
 * combine: method as for aqc_mps_compress, per output.  coeffs: (re, im) per term; they need not be finite: an output with a NaN
 *   coefficient or tensor fails alone with status 2 and a null out[j], as does a zero sum of one qubit; status 1 as for compression.
 *   ranks, dropped, sweeps, status as there, per output; they may be null.  out is nulled before anything else can fail.  Argument
 *   errors (null pointers, states that differ in size or device, a term table that does not start at 0, has an output without terms
 *   or names a state outside the call, a negative or non-finite trunc_thr, a negative max_bond, the fused route beyond its cap) are
 *   reported before any device work. */
int aqc_mps_combine_route(int n, int nterms, const int32_t* dims /* [nterms][n+1] */);
int64_t aqc_mps_combine_svd_budget(int64_t bytes);
int aqc_mps_combine(aqc_mps* const* states, int nstates, int nout, const int32_t* term_off /* [nout+1] */, const int32_t* term_state /* [terms] */,
                    const double* coeffs /* [terms][2] */, double trunc_thr, int max_bond, int method, aqc_mps** out /* [nout] */,
                    int32_t* ranks /* [nout][n-1] */, double* dropped /* [nout][n-1] */, int32_t* sweeps /* [nout][n-1] */, int32_t* status /* [nout] */);
/* Operator sums on MPS states: output j = sum over its terms of c_t O_t psi_t, t = term_off[j] .. term_off[j+1] - 1, compressed; O_t is
 * operator term_op[t] of the call, or absent (term_op[t] = -1: the identity), psi_t is state term_state[t]; one or many outputs per call
 * (rules: csrc/aqc_mps_opsum_rule.h, kernel: csrc/aqc_mps_opsum.hip, the sweep of aqc_mps_compress).  A strict generalisation of
 * aqc_mps_combine: H psi, (H - E) psi and a Lanczos residual H v - alpha v - beta w are one call with one truncating sweep each.
 * An operator (MPO) on n qubits has sites W_q [D_q][D_{q+1}][2][2], complex, indexed [a][b][s_out][s_in], D_0 = D_n = 1:
 * O(b_out, b_in) = W_0[., ., b_out0, b_in0] ... W_{n-1}[...] as a product of D x D matrices, qubit q index bit q of the dense vector; no
 * gauge or Hermiticity is assumed.  The operators of a call come packed: op_dims[o] are D_0 .. D_n of operator o, its site q lies at
 * complex element op_site_off[o][q] of op_data and is 4 D_q D_{q+1} elements long, op_site_off[o][n] is the operator's end.  The
 * product O psi has sites P_q[s][(a, i), (b, j)] = sum_{s'} W_q[a][b][s][s'] T_q[s'][i][j] with bonds D_q chi_q (the operator index is the
 * major one); the direct sum of an output's terms (the coefficients on site 0) is assembled on the device, and out[j] is
 * compress(S, trunc_thr, max_bond) as aqc_mps_compress states it: a NEW state (the caller destroys it), its discarded weight what the cuts
 * of THIS call dropped.  The states are left bit for bit as they are.  Errors are of the size of rounding relative to
 * scale = sum_t |c_t| |O_t|_2 |psi_t|, not to the norm of the result.  n = 1: the 2-vector sum_t c_t W^t_0[0][0] T^t_0.  An output's
 * result does not depend on which other outputs are in the call.
 * opsum_route: host only.  state_dims, op_dims: the bonds of one output's terms and of their operators (a row of ones for a term without
 *   operator).  AQC_MPS_ENT_FUSED when every summed product bond sum_t D^t_q chi^t_q is at most AQC_MPS_ENT_FUSED_CAP, else
 *   AQC_MPS_ENT_CANONICAL, as for aqc_mps_combine (-1: invalid argument).  An XXZ Hamiltonian (D = 5) alone stays fused for state bonds
 *   up to 12, Pauli strings (D = 1) up to 64.
 * opsum_svd_budget: as aqc_mps_compress_svd_budget, for this call.
 * opsum: method as for aqc_mps_compress, per output.  coeffs: (re, im) per term.  Coefficients and operator entries need not be
 *   finite: an output with a NaN in them or in a tensor fails alone with status 2 and a null out[j], as does an output that is exactly
 *   zero (a projector that annihilates the state); status 1 as for compression.  nops may be 0 (then the op_* arrays may be null).
 *   ranks, dropped, sweeps, status as for aqc_mps_combine; they may be null.  out is nulled before anything else can fail.  Argument errors
 *   (null pointers, states that differ in size or device, a term table that does not start at 0, has an output without terms or names
 *   a state or an operator outside the call, operator dims that are not those of an operator on n qubits or offsets that are not their
 *   packed layout, a negative or non-finite trunc_thr, a negative max_bond, the fused route beyond its cap, a summed product bond
 *   beyond 2^20) are reported before any device work. */
int aqc_mps_opsum_route(int n, int nterms, const int32_t* state_dims /* [nterms][n+1] */, const int32_t* op_dims /* [nterms][n+1] */);
int64_t aqc_mps_opsum_svd_budget(int64_t bytes);
int aqc_mps_opsum(aqc_mps* const* states, int nstates, int nops, const int32_t* op_dims /* [nops][n+1] */, const int64_t* op_site_off /* [nops][n+1] */,
                  const double* op_data /* complex elements (re, im) */, int nout, const int32_t* term_off /* [nout+1] */,
                  const int32_t* term_state /* [terms] */, const int32_t* term_op /* [terms], -1: none */, const double* coeffs /* [terms][2] */,
                  double trunc_thr, int max_bond, int method, aqc_mps** out /* [nout] */, int32_t* ranks /* [nout][n-1] */,
                  double* dropped /* [nout][n-1] */, int32_t* sweeps /* [nout][n-1] */, int32_t* status /* [nout] */);
/* Matrix elements of operators between MPS states: out[j] = <phi|O|psi> for job j = (state job_bra[j], operator job_op[j] or -1: the
 * identity, state job_ket[j]) of the call's tables, many jobs per call, without forming O psi: no SVD, no truncation, no new state
 * (rules: csrc/aqc_mps_melem_rule.h, kernels: csrc/aqc_mps_melem.hip).  Operators are packed as aqc_mps_opsum takes them.  The walk
 * E_0 = [1], E_{q+1}[b] = sum_a sum_{s,s'} W_q[a][b][s][s'] B_q[s]^H E_q[a] T_q[s'] carries the operator's bond: D_q matrices of
 * beta_q x chi_q; out[j] = E_n[0][0][0], not normalised.  Entries of W_q that are exactly zero are skipped, and with them the products
 * that only they would read: a site of an XXZ Hamiltonian costs 20 matrix products, not 100.  States and operators are left bit for bit
 * as they are; a state or an operator listed in many jobs is read once.  Errors are of the size of rounding relative to
 * scale = |phi| |O|_2 |psi|.  A job's value does not depend on which other jobs are in the call, and non-finite inputs are data: their
 * jobs return what the arithmetic gives.
 * melem_route: host only.  AQC_MPS_MELEM_FUSED (one workgroup walks a whole chain inside one launch) when every bond of bra and ket is at
 *   most AQC_MPS_MELEM_FUSED_CAP and every operator bond at most AQC_MPS_MELEM_OP_CAP, else AQC_MPS_MELEM_GEMM (-1: invalid argument).
 * melem_entries: host only.  The entries of one operator site that the walk does not skip, in the order of the rule (a, s', b, s), with
 *   the mark of the first entry of every G_{b,s}, and per b the mask of the G_{b,s} that exist; returns their number (-1: invalid argument).
 * melem_budget: the bytes of scratch that the jobs of one group may take together; bytes > 0 sets it, else the default comes back; returns
 *   the value before.  Results do not depend on it.
 * melem: method AQC_MPS_MELEM_BY_RULE (per job), _FUSED (an error that names the job when a bond exceeds a cap) or _GEMM.  nops may be 0
 *   (then the op_* arrays may be null).  Argument errors (null pointers, states that differ in size or device, a job that names a state
 *   or an operator outside the call, operator dims that are not those of an operator on n qubits or offsets that are not their packed
 *   layout, an unknown method, the fused route beyond a cap) are reported before any device work. */
#define AQC_MPS_MELEM_BY_RULE 0
#define AQC_MPS_MELEM_FUSED 1
#define AQC_MPS_MELEM_GEMM 2
#define AQC_MPS_MELEM_FUSED_CAP 64
#define AQC_MPS_MELEM_OP_CAP 32
int aqc_mps_melem_route(int n, const int32_t* bra_dims /* [n+1], null: the ket's */, const int32_t* ket_dims /* [n+1] */,
                        const int32_t* op_dims /* [n+1], null: the identity */);
int aqc_mps_melem_entries(int dl, int dr, const double* w /* [dl][dr][2][2] c128, null: the identity site */,
                          int32_t* out /* [4 dl dr][5]: a, s', b, s, first */, int32_t* mask /* [dr] */);
int64_t aqc_mps_melem_budget(int64_t bytes);
int aqc_mps_melem(aqc_mps* const* states, int nstates, int nops, const int32_t* op_dims /* [nops][n+1] */, const int64_t* op_site_off /* [nops][n+1] */,
                  const double* op_data /* complex elements (re, im) */, int njobs, const int32_t* job_bra /* [njobs] */,
                  const int32_t* job_op /* [njobs], -1: the identity */, const int32_t* job_ket /* [njobs] */, int method, double* out /* [njobs] c128 */);
/* Dense vectors into MPS states: one or many vectors of 2^n c128 amplitudes (index bit q is site q, any norm, left as they are) per call
 * (rules: csrc/aqc_mps_fromvec_rule.h, kernels: csrc/aqc_mps_fromvec.hip).  out[i] is a NEW state (the caller destroys it) in the engine's
 * gauge, as aqc_mps_compress returns it: every bond cut left to right by the engine's rank rule at trunc_thr / max_bond
 * (aqc_mps_rank_rule) with the rescaling of a truncating gate; its discarded weight is what the cuts dropped.  A lane's result does not
 * depend on which other vectors are in the call.
 * from_vec_route: host only, needs no device.  AQC_MPS_FROM_VEC_FUSED when 2 <= n <= 30 and every bond bound min(2^b, 2^(n-b), max_bond
 *   if > 0) is at most AQC_MPS_FROM_VEC_CAP (max_bond in 1 .. 32, or n <= 11): the remainder stays on the device, R-only Householder
 *   factors of its tall-skinny matrix, the SVD of R^T, the rank decision and the projection per site, one synchronisation per call.
 *   Else AQC_MPS_FROM_VEC_HOST: the caller's loop of LAPACK SVDs (mps_operations.vector_to_canonical_mps) (-1: invalid argument).
 * from_vec_budget: bytes the two ping-pong work buffers (2 x lanes x 2^n x 16) may take (default 8 GiB): the lanes of a call go in chunks
 *   that fit; one lane that does not fit is an error that names the size.  Sets it (bytes <= 0: the default) and returns the earlier
 *   value; results do not depend on it.
 * from_vec: method AQC_MPS_FROM_VEC_BY_RULE or _FUSED (an error where the rule answers _HOST: that route is the caller's).  bonds: the
 *   n + 1 bond dimensions of every new state, 0 from the site on at which a lane failed; dropped: the weight each cut dropped; sweeps: of
 *   the site's SVD; status per lane: 0 converted, 1 an SVD reached its sweep limit, 2 a zero or non-finite spectrum -- such a lane gets
 *   a null handle in out, failed_at names its site (else -1), and the call still returns 0.  parts: the partial R factors of every
 *   site, a function of n alone.  out is nulled before anything else can fail.  bonds, dropped, sweeps, status, failed_at and parts may
 *   be null.  Argument errors are reported before any device work and before anything is allocated. */
#define AQC_MPS_FROM_VEC_BY_RULE 0
#define AQC_MPS_FROM_VEC_FUSED 1
#define AQC_MPS_FROM_VEC_HOST 2
#define AQC_MPS_FROM_VEC_CAP 32
int aqc_mps_from_vec_route(int n, int max_bond);
int64_t aqc_mps_from_vec_budget(int64_t bytes);
int aqc_mps_from_vec(int device, int n, int lanes, const double* vecs /* [lanes][2^n] c128 */, double trunc_thr, int max_bond, int method,
                     aqc_mps** out /* [lanes] */, int32_t* bonds /* [lanes][n+1] */, double* dropped /* [lanes][n-1] */,
                     int32_t* sweeps /* [lanes][n-1] */, int32_t* status /* [lanes] */, int32_t* failed_at /* [lanes] */, int32_t* parts /* [n-1] */);
/* MPS states into dense vectors, and into blocks of amplitudes, one or many states per call (rules: csrc/aqc_mps_tovec_rule.h, kernels:
 * csrc/aqc_mps_tovec.hip): the inverse of aqc_mps_from_vec.  psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}] at index sum_q b_q 2^q, the site
 * tensors as the engine keeps them (any gauge, any norm).  With k low sites, L[l] = the row vector of the sites 0 .. k - 1 and H[r] the
 * column vector of the sites k .. n - 1, out[r 2^k + l] = sum_j H[r][j] L[l][j].  The states share n and the device and are left as
 * they are; a state listed several times is contracted once and delivered to each of its lanes; a lane's result does not depend on
 * which other states are in the call.  A state that holds NaN gives NaN in its own lanes, and the call returns 0.
 * to_vec_route: host only, needs no device.  AQC_MPS_TO_VEC_FUSED when every one of the n + 1 bond dimensions is at most 64: the two
 *   halves grow site by site on the matrix cores, all states of a chunk in every launch, and one pass writes the 2^n amplitudes
 *   straight into the output lane.  Else AQC_MPS_TO_VEC_GEMM: the chain of batched products of aqc_ws_mps_to_vec_batch on the states'
 *   own tensors, states of equal bonds together (-1: invalid argument).
 * to_vec_budget: device bytes the output lanes and halves of a chunk may take (default 8 GiB): the distinct states of a call go in
 *   chunks that fit, one synchronisation and one download per chunk; one state that does not fit is an error that names the size.  Sets
 *   it (bytes <= 0: the default) and returns the earlier value; results do not depend on it.
 * to_vec: 1 <= n <= 30, k = n / 2.  method AQC_MPS_TO_VEC_BY_RULE (per state), _FUSED (an error for a state with a bond above 64) or
 *   _GEMM.  info (may be null): [nstates] the route of every state | k | chunks | launches.
 * amp_blocks: any n >= 2, k = low_qubits in 1 .. min(n - 1, 24).  high_bits [rows][n - k]: the bits (0 / 1) of the sites k .. n - 1 of
 *   every row, shared by the states; out [nstates][rows][2^k]: the amplitudes that share those high bits.  Fused route only: a bond
 *   above 64 is an error that names it. */
#define AQC_MPS_TO_VEC_BY_RULE 0
#define AQC_MPS_TO_VEC_FUSED 1
#define AQC_MPS_TO_VEC_GEMM 2
int aqc_mps_to_vec_route(int n, const int32_t* dims /* [n+1] */);
int64_t aqc_mps_to_vec_budget(int64_t bytes);
/* device milliseconds (HIP events) of the outer-product launches of the calling thread's last to_vec / amp_blocks, summed over its
 * chunks; -1 when that call had no state on the fused route.  For tools/mps_tovec_probe.py. */
double aqc_mps_to_vec_outer_ms(void);
int aqc_mps_to_vec(aqc_mps* const* states, int nstates, int method, double* out /* host [nstates][2^n] c128 */, int32_t* info /* [nstates+3] */);
int aqc_mps_amp_blocks(aqc_mps* const* states, int nstates, int low_qubits, int64_t rows, const uint8_t* high_bits /* [rows][n-low_qubits] */,
                       int method, double* out /* host [nstates][rows][2^low_qubits] c128 */);
/* Whole programs of gates on MPS states, layer by layer, one or many states per call (rules: csrc/aqc_mps_layers_rule.h, kernels:
 * csrc/aqc_mps_layers.hip).  A program is nops ops in order: kinds[i] = 1, a 2 x 2 matrix on qubit qubits[i][0], or kinds[i] = 2, a 4 x 4
 * matrix (index 2 bit_a + bit_b) on the pair (qubits[i][0], qubits[i][1]), adjacent or not (routed as aqc_mps_gate2 routes it).  mats:
 * the matrices back to back in the order of the ops (4 or 16 c128 each), once for all states (per_state = 0) or one such set per listed
 * state (per_state = 1: the same structure, different numbers).  1-qubit ops are folded into neighbouring 2-qubit ops (exact), the
 * 2-qubit ops are scheduled into layers of gates on disjoint sites as soon as possible, and every layer runs for all states at once.
 * The states share n >= 1 and the device and are left as they are; out[i] is a NEW state (the caller destroys it) in the engine's gauge,
 * every split decided by the engine's rank rule at trunc_thr / max_bond (aqc_mps_rank_rule) with the rescaling of a truncating gate.  Its
 * discarded weight is the input's plus what the splits dropped.  With per_state = 0 a state listed many times is evolved once; with
 * per_state = 1 every listing is its own lane.  A lane's result does not depend on which other lanes are in the call.
 * apply_route: AQC_MPS_ENT_FUSED when no bond can pass AQC_MPS_ENT_FUSED_CAP (max_bond in 1 .. 64, or n <= 13, and no input bond above
 *   the cap; dims may be null): the working copies stay on the device, the rank decisions are made there, the host waits once per call.
 *   Else AQC_MPS_APPLY_GATEWISE: the engine's 2-qubit gate, folded matrix by folded matrix in layer order, on a clone (-1: invalid argument).
 * apply_plan: counts[0] = layers, counts[1] = folded 2-qubit gates of the program; gate_sites / gate_layers (may be null): site q and
 *   layer of every folded gate, in program order.  apply_circuit_plan: the counts of an ansatz.
 * apply_gates: method AQC_MPS_ENT_BY_RULE (the route of the call by the rule), AQC_MPS_ENT_FUSED (an error where the rule does not allow
 *   it) or AQC_MPS_APPLY_GATEWISE.  ranks: the n + 1 bond dimensions of every new state (0 for a failed lane); dropped: the weight the
 *   call dropped per lane; sweeps: of every folded gate's SVD (0 on the gatewise route); status per lane: {code, layer, site} with code
 *   0 done, 1 an SVD reached its sweep limit, 2 a zero or non-finite state, 3 a rank passed the static bound of its bond (hand-made
 *   states; never a silent cut) -- such a lane gets a null handle in out and the call still returns 0.  out is nulled before anything
 *   else can fail.  ranks, dropped, sweeps and status may be null.  Argument errors (a negative or non-finite trunc_thr, a negative
 *   max_bond, states that differ in size or device, a qubit out of range, a matrix that is not finite, the fused route where the rule
 *   refuses it) are reported before any device work.
 * apply_circuit_many: V(thetas) (inverse = 1: its conjugate transpose) of an ansatz on every state; thetas: num_thetas numbers for all
 *   states (per_state = 0) or [nstates][num_thetas]. */
#define AQC_MPS_APPLY_GATEWISE 2
int aqc_mps_apply_route(int n, const int32_t* dims, int max_bond);
int64_t aqc_mps_apply_svd_budget(int64_t bytes);   /* as aqc_mps_compress_svd_budget, for the stores of a layer's batched SVD */
int aqc_mps_apply_plan(int n, int nops, const int32_t* qubits /* [nops][2] */, const int32_t* kinds /* [nops] */, int32_t* counts /* [2] */,
                       int32_t* gate_sites, int32_t* gate_layers);
int aqc_mps_apply_gates(aqc_mps* const* states, int nstates, int nops, const int32_t* qubits /* [nops][2] */, const int32_t* kinds /* [nops] */,
                        const double* mats, int per_state, double trunc_thr, int max_bond, int method, aqc_mps** out /* [nstates] */,
                        int32_t* ranks /* [nstates][n+1] */, double* dropped /* [nstates] */, int32_t* sweeps /* [nstates][gates] */,
                        int32_t* status /* [nstates][3] */);
/* ansatz description for the MPS entry points (ParametricCircuit / TrotterAnsatz, parametric_circuit.py:24-70,267-333);
 * unlike aqc_ctx it is not limited to dense-reachable registers.  blocks: int32[2][num_blocks], row 0 = control */
typedef struct aqc_circuit {
    int32_t num_qubits, entangler /* AQC_CX / AQC_CZ / AQC_CP */, num_blocks, trotter, second_order;
    const int32_t* blocks;
} aqc_circuit;
/* v_mul_mps / v_dagger_mul_mps(circ, thetas, mps, trunc_thr) (mps_operations.py:326-371): the whole ansatz (inverse = 1:
 * its conjugate transpose) applied in place, one call instead of one per gate */
int aqc_mps_apply_circuit(aqc_mps* mps, const aqc_circuit* circ, const double* thetas, int inverse, double trunc_thr, int max_bond);
int aqc_mps_apply_circuit_plan(const aqc_circuit* circ, int inverse, int32_t* counts /* [2] */);
int aqc_mps_apply_circuit_many(const aqc_circuit* circ, const double* thetas, int num_thetas, int per_state, aqc_mps* const* states, int nstates,
                               int inverse, double trunc_thr, int max_bond, int method, aqc_mps** out, int32_t* ranks, double* dropped,
                               int32_t* sweeps, int32_t* status);
/* fast_dot_gradient(circ, thetas, lvec, vh_phi, trunc_thr, block_range, front_layer) (mps_dot_objective.py:41-242):
 * complex gradient (c128[num_thetas]) of <V lvec|phi> from vh_phi = V^H|phi>.  One call walks all gates on device copies
 * of both operands; the ~num_thetas inner products 0.5j<P w|z> reuse cached left / right environments of the pair and
 * come back in a single transfer.  block_from < 0: all blocks.  lvec and vh_phi are left intact. */
int aqc_mps_fast_dot_gradient(const aqc_circuit* circ, const aqc_mps* lvec, const aqc_mps* vh_phi, const double* thetas,
                              double trunc_thr, int max_bond, int block_from, int block_to, int front_layer, double* grad);
/* ---- lockstep lanes of the MPS objective: `lanes` independent problems that share one ansatz (the seeds / restarts / targets
 * the reference evaluates one per job, job_executor.py:141 around mps_dot_objective.py:41) evaluated TOGETHER and device-resident:
 * every step of the gate walk is one launch for all lanes (grid dimension = lane); a truncated 2-qubit gate is one workgroup per
 * lane (two-site tensor, Jacobi SVD, rank / truncation decision, new tensors -- the lane's bond dimensions never leave the device);
 * gate matrices are formed by the kernels from thetas[lane][index].  The host enqueues the whole evaluation without waiting and
 * reads all results in one transfer.  Bonds up to 32 per lane; a lane whose bond would grow beyond that makes the call fail with
 * AQC_LANES_REFUSED (never a silent truncation) and the caller falls back to aqc_mps_fast_dot_gradient lane by lane.  Truncation rule and outputs per lane
 * are those of aqc_mps_apply_circuit + aqc_mps_dot + aqc_mps_fast_dot_gradient (sums of the rule are taken in a different order:
 * last-bit differences). */
typedef struct aqc_mpsb aqc_mpsb;
int aqc_mpsb_create(int device, int num_qubits, int lanes, aqc_mpsb** out);
int aqc_mpsb_destroy(aqc_mpsb* b);
/* work and time of the truncated 2-qubit gates of the lanes (the SVDs that qiskit-aer runs per gate, mps_operations.py:252-257):
 * enable 1 / 0 / -1 (leave); out[6] = fp64 flops of the Jacobi rotations that ran, SVDs, sweeps, rotations, launches timed, their ms */
int aqc_mpsb_gate2_stats(aqc_mpsb* b, int enable, double* out, int reset);
/* |phi_l> of every lane (the objective's target, objective_base.py:112 set_target) and <lhs_l| (its left-hand state |0> or the
 * surrogate's low-entangled state, objective_lhs_sur_fast_mps_trotter.py:99); shared != 0: handles[0] serves every lane */
int aqc_mpsb_set_targets(aqc_mpsb* b, aqc_mps* const* handles, int shared);
int aqc_mpsb_set_lhs(aqc_mpsb* b, aqc_mps* const* handles, int shared);
/* lhs states of all lanes = computational-basis states built on the device: bits[lane][n] (0 / 1), bit q = qubit q (the |state_i> of
 * objective_base.py:42-255: |0>, X_q|0> on top of a basis preparation such as the Neel pattern) */
int aqc_mpsb_set_lhs_basis(aqc_mpsb* b, const uint8_t* bits);
/* per lane l with thetas[l][T]: vh = V(theta_l)^H|phi_l> (v_dagger_mul_mps, mps_operations.py:350), h[l] = <lhs_l|vh> (c128) and
 * grad[l][T] (c128) = fast_dot_gradient(circ, theta_l, lhs_l, vh, trunc_thr, block_range, front_layer) (mps_dot_objective.py:41).
 * discarded[l] (optional) = weight truncated while forming vh, max_bond_out[l] (optional) = its largest bond. */
int aqc_mpsb_eval(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int block_from,
                  int block_to, int front_layer, double* h /* [lanes] c128 */, double* grad /* [lanes][T] c128 */,
                  double* discarded /* [lanes] or NULL */, int32_t* max_bond_out /* [lanes] or NULL */);
/* v_mul_mps / v_dagger_mul_mps(circ, thetas, mps, trunc_thr) (mps_operations.py:326-371) for every lane: the batch's working state <-
 * V(theta_l)|phi_l> (inverse = 0) or V(theta_l)^H|phi_l> (inverse = 1), the gates of a circuit layer in one launch; aqc_mpsb_export hands
 * lane `lane` of it out as a single-lane MPS of its own (caller destroys it). */
int aqc_mpsb_apply_circuit(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, int inverse, double trunc_thr, int max_bond,
                           double* discarded /* [lanes] or NULL */, int32_t* max_bond_out /* [lanes] or NULL */);
int aqc_mpsb_export(aqc_mpsb* b, int lane, aqc_mps** out);
/* The same in two phases, for objectives that choose the lhs state after seeing amplitudes (objective_lhs_sur_max.py:82-191: the
 * leading flip state).  Phase 1: vh of every lane, kept in the batch, and amps[lane][0] = <lhs_l|vh_l>, amps[lane][1 + q] =
 * <X_q lhs_l|vh_l> (num_amps = 1 or 1 + n; with a basis state as lhs: the amplitudes of its single-flip states, :99-111).
 * half != 0: lanes [lanes/2, lanes) repeat targets and thetas of the first half (the same problems seen from a second lhs state):
 * V^H runs on the first half only and is copied.  Phase 2: the gradient walk from the CURRENT lhs states (they may have been
 * replaced since phase 1) and the vh, thetas, trunc_thr, max_bond of phase 1 (same circuit). */
int aqc_mpsb_vh(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int half, int num_amps,
                double* amps /* [lanes][num_amps] c128 */, double* discarded /* [lanes] or NULL */, int32_t* max_bond_out /* or NULL */);
int aqc_mpsb_grad(aqc_mpsb* b, const aqc_circuit* circ, int block_from, int block_to, int front_layer, double* grad /* [lanes][T] c128 */);
/* Phase 1 against a bank of K general lhs states shared by all lanes -- the states S|0>, S X_i|0> of a general state-preparation circuit
 * S (the reference's MpsStateHandler, objective_base.py:345-435, whose state_dot_vector it replaces): aqc_mpsb_set_bank copies the K
 * states (bonds <= 32, count = K) into the batch; aqc_mpsb_vh_bank takes the arguments of aqc_mpsb_vh with num_amps = K and returns
 * amps[lane][k] = <bank_k|vh_l>, one launch for all (k, lane) pairs, read back with V^H's results in one transfer.  Phase 2
 * (aqc_mpsb_grad) follows from whatever lhs states are set then. */
int aqc_mpsb_set_bank(aqc_mpsb* b, aqc_mps* const* states, int count);
int aqc_mpsb_vh_bank(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int half, int num_amps,
                     double* amps /* [lanes][num_amps] c128 */, double* discarded /* [lanes] or NULL */, int32_t* max_bond_out /* or NULL */);
/* fast_dot_gradient with vh_phi formed by the caller, as the reference's function takes it (mps_dot_objective.py:41): the states given to
 * aqc_mpsb_set_targets ARE vh_phi_l = V^H|phi_l>, those given to aqc_mpsb_set_lhs the lvec_l */
int aqc_mpsb_gradient_of(aqc_mpsb* b, const aqc_circuit* circ, const double* thetas, double trunc_thr, int max_bond, int block_from,
                         int block_to, int front_layer, double* grad /* [lanes][T] c128 */);
/* one-sided Jacobi SVD on the device (the kernel behind aqc_mps_gate2): A (m x n row-major) = U diag(S) Vh,
 * k = min(m, n), S descending, U (m x k), Vh (k x n); *sweeps (optional) = Jacobi sweeps used.  The input is not rescaled: the
 * rotations work with squared column norms and |<x, y>|^2, which leave the double range when |A|_F is beyond about 2^+-250 (every
 * rotation is skipped then); scalings by 2^+-100 are tested. */
int aqc_svd(int device, int m, int n, const double* a, double* u, double* s, double* vh, int* sweeps);
/* the same factorisation for MANY matrices in one call, by block one-sided Jacobi on the fp64 matrix cores (csrc/aqc_svd_batch.hip), a
 * workgroup per matrix: the SVD of the truncated two-qubit gate (mps_operations.py:252-257) for a batch of two-site tensors whose bonds
 * differ.  The store has fixed strides, matrix i is active in its leading rows[i] x cols[i] corner (NULL: all m / all n; m, n <= 256);
 * k = min(m, n), k_i = min(rows[i], cols[i]).  Only the leading rows[i] x k_i of u, k_i of s and k_i x cols[i] of vh are meaningful, the
 * rest is written as zero.  status[i]: 0 converged, 1 sweep limit reached (results still written), 2 non-finite input (outputs zero, the
 * other matrices unaffected).  The return value is non-zero only for argument errors (count < 1, sizes out of range, null pointers).
 * A matrix's result does not depend on its position in the batch or on its neighbours.  Scaling as for aqc_svd. */
int aqc_svd_batch(int device, int count, int m, int n, const int32_t* rows, const int32_t* cols /* NULL: all m / n */,
                  const double* a /* [count][m][n] c128 row-major, host */, double* u /* [count][m][k] */, double* s /* [count][k] */,
                  double* vh /* [count][k][n] */, int32_t* sweeps /* [count] or NULL */, int32_t* status /* [count] */);
/* milliseconds the device core of this thread's last aqc_svd_batch call took (HIP events around the zeroing of the outputs and the
 * kernel; uploads, downloads and allocations are outside), -1 if that call failed.  For tools/svd_batch_probe.py. */
double aqc_svd_batch_core_ms(void);

/* ---- coordinate descent (core_op_matrix.py:765  coord_descent_single_sweep(circ, thetas, target,
 * workspace)).  Square workspace (ncols == 2^n) with the target unitary in AQC_BUF_Y.  One
 * Gauss-Seidel sweep over all parameters of 1 - |<V,U>|^2/d^2; thetas are updated in place and
 * the objective at the end of the sweep is returned.  cx / cz entanglers only (:818-827).
 * A single-lane workspace (batch == 1).  Where aqc_ws_cd_fits_one_launch this is aqc_ws_cd_sweeps(ws, thetas_io, fobj, 1, -1);
 * larger problems, and every problem where the switch AQC_CD_CHAIN is on (cross-checks, timing), take one sweep of the
 * wide walk of aqc_ws_cd_minimize.
 * Side effects, the same on either route: AQC_BUF_X, Z, W and ZW are unspecified afterwards (the wide walk rewrites X and Z in place
 * and leaves a checkpoint in ZW; the persistent launch touches none of them), Y and X2 are kept, and the thetas in use when it returns
 * are thetas_io as returned, with the coefficients derived from them valid. */
int aqc_ws_cd_sweep(aqc_ws* ws, double* thetas_io /* [T] */, double* fobj);
/* The same walk for EVERY lane of the workspace (lane = an independent problem: a random restart of the ansatz and / or its
 * own target in AQC_BUF_Y) and for `nsweeps` consecutive sweeps, as ONE persistent launch: a workgroup per lane keeps the two
 * d x d operands in LDS, re-derives z = V(theta)^H U at the start of every sweep (:806-810) and walks all parameters (:852-912)
 * without leaving the kernel.  Needs 2 d^2 16 B + 24 T B <= 160 KiB (up to 6 qubits; aqc_ws_cd_fits_one_launch); larger
 * problems are refused here: lanes beyond LDS are served by aqc_ws_cd_minimize.  fobj[lane][s] = the objective at the end of sweep s (:917).
 * max_steps >= 0 stops every sweep's walk after that many parameters (tests pin single steps with it); -1 = all.
 * Side effects: AQC_BUF_X, Z, W and ZW are unspecified afterwards (as for aqc_ws_cd_sweep), Y and X2 are kept, and the thetas in use
 * when it returns are thetas_io as returned, with the coefficients derived from them valid. */
int aqc_ws_cd_sweeps(aqc_ws* ws, double* thetas_io /* [batch][T] */, double* fobj /* [batch][nsweeps] */, int nsweeps, int max_steps);
int aqc_ws_cd_fits_one_launch(const aqc_ws* ws);
/* The whole coordinate-descent driver (aqc_coord_descent.py:70-121, _single_simulation) for every lane, without a host visit per
 * sweep: sweeps from thetas0 until a lane's rule ends it, the best objective value and its thetas kept on the device.  At the end of a
 * sweep, in the reference's order: profile[lane][nit] = fobj, nit += 1, a value below best_f is recorded with the sweep's thetas, then
 *   fobj < fobj_thr                 -> AQC_CD_EARLY    (SmallObjectiveStopper)
 *   max |theta - theta_prev| < dtheta_thr, or nit == maxiter -> AQC_CD_NORMAL
 * (csrc/aqc_cd_rule.h).  The host enqueues `chunk` sweeps at a time, reads ONE word (lanes still running) and looks at its clock:
 * once time_limit_s (> 0; <= 0: none) has passed, the lanes still running end as AQC_CD_TIMEOUT -- the time limit acts between
 * chunks, never inside one.  A finished lane is skipped by every later launch: its thetas and counters do not move.
 * route: AQC_CD_ROUTE_AUTO (the persistent launch where aqc_ws_cd_fits_one_launch, else the wide walk), _PERSISTENT (an error where
 * it does not fit), _WIDE: operands in HBM, T + (n + L) walk launches per sweep on a grid of (workgroups per lane, lanes), any
 * number of qubits and lanes.  max_steps as in aqc_ws_cd_sweeps.  Square workspace, targets in AQC_BUF_Y, cx / cz, no Trotter.
 * Outputs: best_thetas[batch][T], best_f[batch], nit[batch], status[batch], profile[batch][maxiter] (entries from nit on are 0).
 * Side effects, the same on every route: AQC_BUF_X, Z, W and ZW are unspecified afterwards (the wide route rewrites X and Z and leaves
 * a checkpoint in ZW, the persistent route touches none of them: a caller may rely on neither), Y and X2 are kept, and the thetas in
 * use when it returns are best_thetas -- not the last sweep's -- with the coefficients derived from them valid. */
enum { AQC_CD_RUNNING = 0, AQC_CD_NORMAL = 1, AQC_CD_EARLY = 2, AQC_CD_TIMEOUT = 3 };
enum { AQC_CD_ROUTE_AUTO = 0, AQC_CD_ROUTE_PERSISTENT = 1, AQC_CD_ROUTE_WIDE = 2 };
int aqc_ws_cd_minimize(aqc_ws* ws, const double* thetas0 /* [batch][T] */, int maxiter, int chunk, double dtheta_thr, double fobj_thr,
                       double time_limit_s, int route, int max_steps, double* best_thetas, double* best_f, int64_t* nit, int32_t* status,
                       double* profile);

/* ---- measurement hooks (bench.py): HIP events on the workspace's own stream */
int aqc_ws_timer_start(aqc_ws* ws);
int aqc_ws_timer_stop(aqc_ws* ws, float* elapsed_ms); /* synchronises */
/* per-kernel-family timing: when enabled every launch is bracketed by events */
int aqc_ws_profile_enable(aqc_ws* ws, int on);
int aqc_ws_profile_get(aqc_ws* ws, int kind, int64_t* launches, double* total_ms);
int aqc_ws_profile_reset(aqc_ws* ws);
/* the launches profiled since the last reset, in order: kinds[i], ms[i] for i < min(*count, cap); *count = their number */
int aqc_ws_profile_log(aqc_ws* ws, int32_t* kinds, double* ms, int cap, int* count);
/* stage `stage` of plan `which` as this workspace runs it: sub-stages, gate groups, local address bits (bits_out: [tile_bits]) */
int aqc_ws_plan_stage(aqc_ws* ws, int which, int stage, int* num_subs, int* num_groups, int* bits_out);
/* per sub-stage of that stage, what a sweep from ONE basis state per lane leaves out (out[sub][2]): log2 of the share of 16-chunk
 * groups whose W and R products are issued, log2 of the share of K-steps of the W product (both <= 0); zeros when nothing is skipped */
int aqc_ws_plan_skips(aqc_ws* ws, int which, int stage, int* out, int max_subs);
/* index (over all stages) of the sweep's sub-stage that is taken from its inputs alone -- the last one of the last stage,
 * R = U (Z W^H) U^H: a third of a sub-stage's matrix work -- or -1 when the sweep runs it like the others */
int aqc_ws_sweep_r_only_sub(aqc_ws* ws);
/* 1 when an objective by projection walks its virtual stage BACK from (M_end, Y_end) inside the launch that leaves Y_0 -- one walk over
 * the virtual tiles instead of two, every R of the virtual plan from its sub-stage's inputs --, 0 when that stage is swept forwards */
int aqc_ws_virtual_backwalk(aqc_ws* ws);
/* item lists of the last sparse evaluation (synchronises): counts[0] first-stage items of the sweep, [1] tiles it cleared in W,
 * [2] last-stage items of V^H; -1 where that list has never been built */
int aqc_ws_sparse_counts(aqc_ws* ws, int64_t* counts);
/* projected route of the sparse-lhs sweep (the stages after the first on a virtual register, csrc/aqc_ws_project.cpp): info[0] 1 if
 * the workspace has it, [1] virtual qubits, [2] qubits the later stages touch, [3] of them local to the first stage, [4] stages and
 * [5] sub-stages of the virtual plan, [6] its tile bits, [7] sub-stages left on the real register, [8] bits of the first stage the
 * pass over z sums over, [9] virtual qubits after padding (>= 8), [10..15] sub-stages of the virtual stages; info holds 16 entries */
int aqc_ws_projected_info(aqc_ws* ws, int32_t* info);
/* host-only (no GPU needed): the same for the state-vector workspace a context would get at this tiling */
int aqc_plan_projected(aqc_ctx* ctx, int tile_bits, int low_bits, int32_t* info);
/* ---- run-time switches: the AQC_* environment variables.  aqc_switches.def, next to this file, is the one table of them: name,
 * default, when each is read (import / create / call), who reads it, what it selects.  Both calls are host-only (no GPU needed).
 * Line `index` of the table; returns 1 past the end.  Any output pointer may be NULL. */
int aqc_switch_info(int index, const char** name, const char** dflt, const char** when, const char** reader, const char** doc);
/* the value the workspace was created with (a workspace reads its switches once, in aqc_ws_create); an error for a name that is not
 * a `create` switch read by the library */
int aqc_ws_switch(const aqc_ws* ws, const char* name, int64_t* value);
/* plan introspection: number of fused stages (kernel launches) of V^H and of the sweep */
int aqc_ws_plan_info(aqc_ws* ws, int which /*0 apply-inverse, 1 sweep, 2 apply-forward*/,
                     int* num_stages, int* tile_bits, int* num_tiles);
/* number of sub-stages (16 x 16 unitaries per lane on the matrix-core path) of plan `which`; 0 for the per-group kernels */
int aqc_ws_plan_substages(aqc_ws* ws, int which);
/* kernel family that runs plan `which`: 1 per-gate-group (VALU), 2 register-blocked (VALU), 3 matrix-core (MFMA) */
int aqc_ws_kernel_family(aqc_ws* ws, int which);
/* host-only planner introspection (no GPU needed): stage s of plan `which` for the given tiling (which: 0 V^H planned on its
 * own, 1 sweep, 2 V, 3 V^H as the sweep's plan walked backwards -- what matrix-core workspaces run, see AQC_BUF_ZW above);
 * ops_out receives gate-group indices (forward program order), bits_out the local address bits */
int aqc_plan_query(aqc_ctx* ctx, int ncols, int which, int tile_bits, int low_bits, int stage,
                   int* num_stages, int* bits_out, int* num_bits, int* ops_out, int* num_ops);

/* host-only: the sub-stages of stage `stage` as the matrix-core kernels run it: subs_out[i] = {4 register bits as local
 * positions inside the stage's tile (-1: unused), number of gate groups}; at most max_subs entries are written */
int aqc_plan_substages(aqc_ctx* ctx, int ncols, int which, int tile_bits, int low_bits, int stage, int* num_subs,
                       int* subs_out /* [max_subs][5] */, int max_subs);

/* ---- device-resident multi-start L-BFGS on the lane-batched surrogate objective: one optimisation per lane, thetas /
 * gradients / history stay in HBM (stand-in for the scipy L-BFGS-B behind AqcOptimizer.optimize, optimizer.py:579-590,
 * on objective_lhs_sur_max.py:82-191).  Preconditions: targets in buffer Y, flip-state indices registered with
 * aqc_ws_gather_setup (state 0 first); buffer X2 is used for the lhs states.  An evaluation is V^H, the amplitudes and ONE
 * sweep from conj(c_0)|state_0> + conj(c_max)|state_max> (see aqc_ws_set_combo).  block_from / block_to / front_layer as in
 * aqc_ws_grad (block_from < 0: all blocks).  x0 / x_out: [batch][T]; f / fidelity / nit / weight / max_no: [batch]; the
 * last two are the objective's state at exit (smoothed weight, index of the leading state), either may be NULL. */
/* One evaluation of that objective as a call of its own (the evaluate step of aqc_ws_lbfgs; stand-in for one
 * objective(theta) + gradient(theta) pair of objective_lhs_sur_max.py:82-191 on every lane, one host synchronisation):
 * thetas [batch][T]; weight_io / max_no_io [batch]: the objective state of every lane (smoothed weight, index of the leading
 * state), updated in place when update_state != 0 -- 1: hysteresis :113-117 and smoothing :186 FIRST, then value and gradient
 * under the new state (one accepted optimizer step); 2: hysteresis only, the weight stays (what objective(theta) does before
 * gradient(theta) moves the weight) -- and left alone when it is 0 (line-search trials); f_out [batch]; fidelity_out [batch] (|h_0|^2, written on an
 * update; may be NULL); hs_out [batch][states] complex amplitudes (may be NULL); grads_out [batch][T] COMPLEX gradient of the
 * lane's one sweep from conj(c_0)|state_0> + conj(c_max)|state_max> (may be NULL); grad_real_out [batch][T] its real part,
 * which is the surrogate's gradient (may be NULL; with grads_out NULL only the real parts cross the bus). */
int aqc_ws_surrogate_eval(aqc_ws* ws, const double* thetas, int update_state, double* weight_io, int64_t* max_no_io,
                          int block_from, int block_to, int front_layer, double* f_out, double* fidelity_out, double* hs_out,
                          double* grads_out, double* grad_real_out);
int aqc_ws_lbfgs(aqc_ws* ws, const double* x0, int maxiter, int memory, double gtol, double ftol, double fid_thr,
                 int max_backtracks, int block_from, int block_to, int front_layer, double* x_out, double* f_out,
                 double* fidelity_out, int64_t* nit_out, int64_t* nfev_out, double* weight_out, int64_t* max_no_out);
/* The same L-BFGS on the matrix objective of full / fixed-sketch AQC, f = 1 - Re tr(X^H V^H Y) / ncols per lane (stand-in for the
 * L-BFGS-B run of _full_aqc, aqc_sketching.py:35-50, on SketchingObjectiveEx, sk_core.py:167-212).  Preconditions: buffer Y holds
 * U X, buffer X the sketching matrix X (aqc_ws_set_identity for full AQC); any ncols the workspace supports (1: a state vector is
 * a one-column matrix).  The objective has no state: an accepted trial's value and gradient are final, and the host reads one
 * flag word per line-search trial.  A lane stops at max|g| <= gtol, at a relative decrease <= ftol, at f <= fobj_thr (the role
 * of SmallObjectiveStopper; 0: off) or at |tr|^2 / ncols^2 >= fidelity_thr (the Hilbert-Schmidt fidelity when X = I; 0: off).
 * memory in [1, 32].  x0 / x_out: [batch][T]; f / fidelity / nit / status: [batch]; *nfev_out: evaluations of the whole batch.
 * status (may be NULL): 0, or 1 for a lane whose value or gradient was not finite -- it stops where it is (at x0 when the start
 * point is the bad one) and the other lanes finish as if it were not there.
 * Side effects: rewrites AQC_BUF_Z, W and ZW, which are unspecified afterwards (they belong to the last line-search trial, accepted
 * or not); X, Y and X2 are kept; the thetas in use when it returns are x_out -- not that trial -- with the coefficients derived from
 * them valid.  Refuses a Trotter ansatz, like every matrix path, and changes nothing then.  Sums run in a fixed order: a call repeated gives the same bits, and a lane of a batch gives the
 * bits of the same problem run alone on a workspace with the same plan.  The plan does not depend on the batch below 2^8 elements
 * per lane; above, the tile size may (aqc_ws_plan_info shows it), and the tile-size switches or the tile
 * arguments of aqc_ws_create pin it. */
int aqc_ws_lbfgs_mat(aqc_ws* ws, const double* x0, int maxiter, int memory, double gtol, double ftol, double fobj_thr,
                     double fidelity_thr, int max_backtracks, double* x_out, double* f_out, double* fidelity_out,
                     int64_t* nit_out, int64_t* nfev_out, int32_t* status_out);

/* ---- sketched AQC on the device: the stochastic optimisation of aqc_sketching.py:53-104 (ADAM on SketchingObjectiveEx with a fresh
 * set of `rand` / `alt` / `eigen` sketching vectors on every objective call, sk_core.py:329-464) with every iteration resident in HBM.
 * Matrix workspaces with ncols = k sketching vectors, k a power of two, 1 < k <= 64, k < 2^n; no Trotter ansatz.  Draws come from
 * Philox4x64-10 by the rule at the head of csrc/aqc_philox.h (NumPy's Philox reproduces them bit for bit); the host path
 * (model_sketching/sk_core.py with np.random) is untouched. */
enum { AQC_SKETCH_RAND = 0, AQC_SKETCH_ALT = 1, AQC_SKETCH_EIGEN = 2 };
enum { AQC_QR_OK = 0, AQC_QR_RANK_DEFICIENT = 1 };   /* per-matrix status word of the device QR */
/* np.linalg.qr(a)[0] of sk_core.py:353,459 up to the choice of basis: q_out (m x k, row-major) has orthonormal columns spanning the
 * columns of a (m x k, k a power of two <= 64, m >= k), by CholeskyQR2 on the matrix cores; host pointers, one matrix, like the SVD entry.
 * Status 0 means an orthonormal q_out.  *status = AQC_QR_RANK_DEFICIENT and q_out = a, bit for bit (status NULL: the call fails
 * instead), when a is rank deficient -- a Cholesky pivot of either pass not finite or not above 1e-10 of its column's squared norm --
 * or so ill-conditioned that the first pass's Q is not orthonormal to 1e-4 entrywise, which happens from a condition number
 * (columns scaled to norm 1) of about 1e6 on: double precision determines no range to better than 1e-6 there. */
int aqc_qr(int device, int m, int k, const double* a, double* q_out, int32_t* status);
/* the target unitary of every lane (shared != 0: one for all), [batch or 1][2^n][2^n] c128, kept resident: what
 * SketchingVectorsBase holds as target_matrix (sk_core.py:34-91).  The buffer is allocated on first use. */
int aqc_ws_sketch_target(aqc_ws* ws, const double* U, int shared);
/* SketchingVectorsBase.generate (sk_core.py:350-357 rand, :385-399 alt, :447-463 eigen) for every lane, on the device: AQC_BUF_X <- X,
 * AQC_BUF_Y <- U X, with the thetas in use (eigen).  `iteration` numbers the sketch (part of the Philox counter); omega, when not
 * NULL, is a host draw [batch][2^n][k] c128 used instead of the device's; alt_idx [batch][k] are the columns of `alt` (required
 * there).  status (optional, [batch]; synchronises): the QR's word per lane (see aqc_qr) -- a flagged lane keeps its
 * un-orthonormalised matrix in X bit for bit, and the other lanes are complete.
 * Side effects: rewrites AQC_BUF_X and Y (the result); Z and X2 are kept, W and ZW are unspecified afterwards; the thetas in use are
 * read (eigen) and not changed. */
int aqc_ws_sketch_generate(aqc_ws* ws, int kind, uint64_t seed, int64_t iteration, const int32_t* alt_idx, const double* omega,
                           int32_t* status);
/* the draw alone: buf <- Omega of every lane for (kind = rand or eigen, seed, iteration), as the generate entry would draw it
 * (np.random.rand / randn of sk_core.py:352,449-451; asynchronous) */
int aqc_ws_sketch_draw(aqc_ws* ws, int kind, uint64_t seed, int64_t iteration, int buf);
/* optimizer.py:178-189 (ADAM) driving sk_core.py:175-212 on every lane: niter iterations are enqueued without a host synchronisation
 * in between (generate, V^H Y, trace, sweep, ADAM step per iteration), then one fetch.  Iteration t = 1..niter evaluates at x_{t-1}
 * under sketch number iter0 + t; one more evaluation under sketch iter0 + niter + 1 follows without a step.  A lane whose step norm
 * falls below tol stops moving; its nit counts the steps it took in this call, and fobj_profile[lane][nit] is the cost at its final
 * point, as ADAM's result reports fun(x).  fobj_profile: [batch][niter + 1].  best_f / best_x: the smallest value seen since the
 * lane's last restart and its thetas (sk_core.py:198-200).  lr: [batch].  reset (NULL: restart all on the first call, continue
 * after): per lane 0 = continue with the m / v / t state and from the point this lane's run reached in the last aqc_ws_sketch_adam
 * call -- kept with that state, so whatever put other thetas in use in between (aqc_ws_set_thetas, an evaluation, a theta set,
 * another driver) does not move it; x0 ignored -- 1 = restart from x0[lane], 2 = parked (no further steps, at that same point).
 * alt_idx: [niter + 1][batch][k].  status: [batch] QR words, OR over the call.
 * Side effects: rewrites AQC_BUF_X and Y (the last sketch) and Z, W, ZW, all of which are unspecified afterwards; X2 is kept; the
 * thetas in use when it returns are x_out, with the coefficients derived from them valid. */
int aqc_ws_sketch_adam(aqc_ws* ws, int kind, const double* x0, int niter, const double* lr, double beta1, double beta2, double eps,
                       double tol, uint64_t seed, int64_t iter0, const int32_t* reset, const int32_t* alt_idx, double* x_out,
                       double* fobj_profile, double* best_f, double* best_x, int64_t* nit, int32_t* status);

/* ---- multi-GPU: the one collective layer of the path, bound straight to librccl (RCCL over xGMI; loaded lazily).
 * One process per GPU; jobs are sharded over the ranks (job_executor.py:136-143: joblib processes in the reference) and
 * only fixed-size result records cross GPUs.  All buffers are HOST pointers (the records are a few KB).
 * Bootstrap: rank 0 calls aqc_comm_unique_id and passes the 128 bytes to the other ranks (file / environment),
 * every rank calls aqc_comm_create. */
typedef struct aqc_comm aqc_comm;
int aqc_comm_unique_id(char* out128);
int aqc_comm_create(const char* id128, int nranks, int rank, int device, aqc_comm** out);
int aqc_comm_destroy(aqc_comm* comm);
int aqc_comm_rank(const aqc_comm* comm);
int aqc_comm_size(const aqc_comm* comm);
/* recv[r * count + i] = send[i] of rank r (the final gather of run_jobs: job_executor.py:141-161) */
int aqc_comm_allgather(aqc_comm* comm, const double* send, double* recv, size_t count);
/* in place, op 0 = sum (column-sharded AQC objective: (trace, gradient) record), 2 = max (timing) */
int aqc_comm_allreduce(aqc_comm* comm, double* data, size_t count, int op);
int aqc_comm_barrier(aqc_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* AQC_HIP_H */
