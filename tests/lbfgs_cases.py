"""Problems with more than 256 parameters per lane for the optimiser tests (tests/test_lbfgs_ref.py on the CPU,
tests/test_hip_optimisers_wide.py on the GPU): planted unitaries / states, the CPU oracle as ``fun`` of tests/lbfgs_ref.py, the
conditions an input has to meet, and the measured spread of the reference that bounds the device's deviation.  Everything is
built once per process and made read-only."""
import functools

import numpy as np

from oracle import aqc_oracle as orc
from tests.lbfgs_ref import lbfgs_ref

# name: (qubits, entangler, layout, blocks, T).  T = 3 n + (5 if cp else 4) blocks; one workgroup of 256 threads walks them.
CASES = {
    "A": (3, "cx", "spin", 62, 257),          # first index of the second pass, one thread only
    "B": (3, "cx", "spin", 130, 529),         # three passes, ragged last one
    "C": (4, "cp", "spin", 65, 337),          # five thetas per block
    "D": (5, "cx", "cyclic_spin", 180, 735),  # the notebook's full-AQC ansatz
}
SURROGATE = (6, "cx", "spin", 70, 298)        # aqc_ws_lbfgs, |state_0> leading
LANES = 3
# (jitter, seed) of the starts truth + jitter N(0, 1), searched on the CPU so that the conditions of check_inputs hold
STARTS = {"A": (0.3, 11), "B": (0.3, 11), "C": (0.3, 11), "D": (0.3, 11), "S": (0.15, 11)}
NOISE, NOISE_SEEDS = 1e-10, 5                 # the project's TOL on f and g, as N(0, 1) noise on the oracle's results
F_CAP, X_CAP = 1e-6, 1e-5                     # the bounds of the existing device-against-host comparisons: never looser
# (case, maxiter, memory) of every device run: the per-iteration trajectories, the end points at the memory edges, full_aqc on D and
# the surrogate.  tests/test_lbfgs_ref.py holds the reference to the host loop on all of them (and on A, which only takes one step
# on the device).
TRAJECTORIES = [("B", 8, 3), ("B", 12, 10), ("C", 8, 3), ("C", 12, 10)]
MEMORY_EDGES = [("B", 8, 1), ("B", 8, 32)]
SETTINGS = [("A", 8, 3)] + TRAJECTORIES + MEMORY_EDGES + [("D", 8, 10), ("S", 8, 3)]
# Case B is at f ~ 1e-8 after twelve iterations from every start tried (jitter 0.3, 0.4, 0.5, 1.0, 2.0), so from iteration 9 on its
# Armijo margins are 1e-7, below the 1e-6 max(1, |f|) asked of every other run.  Its (12, 10) run keeps a floor of 1e-8 instead: a
# hundred times the 1e-10 a kernel may be off in f, on either side of the test.
MARGIN_FLOOR = {("B", 12, 10): 1e-8}


def blocks_of(n, layout, depth):
    return orc.spin_blocks(n, depth) if layout == "spin" else orc.cyclic_spin_blocks(n, depth)


def ansatz(n, ent, layout, depth):
    return orc.Ansatz(n, ent, blocks_of(n, layout, depth))


def _frozen(*arrays):
    for arr in arrays:
        arr.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def planted(name):
    """(ansatz, truth[B][T], targets[B][d][d], starts[B][T]) of a matrix case: lane b's target is V(truth_b)."""
    n, ent, layout, depth, T = CASES[name]
    jitter, seed = STARTS[name]
    a = ansatz(n, ent, layout, depth)
    assert a.num_thetas == T
    rng = np.random.default_rng(seed)
    eye = np.eye(1 << n, dtype=complex)
    truth = np.stack([orc.rand_thetas(T, rng) for _ in range(LANES)])
    targets = np.stack([orc.v_mul_mat(a, t, eye) for t in truth])
    starts = truth + jitter * rng.standard_normal(truth.shape)
    return (a,) + _frozen(truth, targets, starts)


@functools.lru_cache(maxsize=None)
def planted_states():
    """(ansatz, truth, targets[B][d], starts) of the surrogate case: lane b's target is V(truth_b)|0>."""
    n, ent, layout, depth, T = SURROGATE
    jitter, seed = STARTS["S"]
    a = ansatz(n, ent, layout, depth)
    assert a.num_thetas == T
    rng = np.random.default_rng(seed)
    zero = np.zeros(1 << n, dtype=complex)
    zero[0] = 1.0
    truth = np.stack([orc.rand_thetas(T, rng) for _ in range(LANES)])
    targets = np.stack([orc.v_mul_vec(a, t, zero) for t in truth])
    starts = truth + jitter * rng.standard_normal(truth.shape)
    return (a,) + _frozen(truth, targets, starts)


def matrix_fun(a, targets):
    """The matrix objective 1 - Re tr(V^H U_b) / d of every lane and its gradient, from the oracle."""
    eye = np.eye(a.dim, dtype=complex)

    def fun(x):
        out = [orc.sketching_objective_and_gradient(a, x[b], eye, targets[b]) for b in range(len(targets))]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out])

    return fun


def surrogate_fun(a, targets):
    """The surrogate while |state_0> leads, which has no state: f = 1 - |h_0|^2, g = Re(-2 conj(h_0) g_0) with h_0 = <0|V^H|target>
    and g_0 the complex gradient of the sweep from |0> (what lb_prepare_kernel and lb_commit0_kernel state for that case)."""
    zero = np.zeros(a.dim, dtype=complex)
    zero[0] = 1.0

    def fun(x):
        fs, gs = [], []
        for b in range(len(targets)):
            vh = orc.v_dagger_mul_vec(a, x[b], targets[b])
            h0 = vh[0]
            g0 = orc.grad_of_dot_product(a, x[b], zero, vh)
            fs.append(1.0 - abs(h0) ** 2)
            gs.append((-2.0 * np.conj(h0) * g0).real)
        return np.array(fs), np.stack(gs)

    return fun


def problem(name):
    """(ansatz, fun, truth, targets, starts) of a case; "S" is the surrogate case."""
    if name == "S":
        a, truth, targets, starts = planted_states()
        return a, surrogate_fun(a, targets), truth, targets, starts
    a, truth, targets, starts = planted(name)
    return a, matrix_fun(a, targets), truth, targets, starts


GTOL, FTOL = 1e-7, 1e-12                      # the drivers' defaults


@functools.lru_cache(maxsize=None)
def reference(name, maxiter, memory):
    """The reference run of a case from its committed start, computed once and shared (nobody writes into it)."""
    _, fun, _, _, starts = problem(name)
    return lbfgs_ref(fun, starts, maxiter=maxiter, memory=memory, gtol=GTOL, ftol=FTOL)


@functools.lru_cache(maxsize=None)
def measured(name, maxiter, memory):
    """(spread of x_k, spread of f_k, bound on x_k, bound on f_k), k = 1 .. maxiter, of that run."""
    _, fun, _, _, starts = problem(name)
    sx, sf = spread(fun, starts, reference(name, maxiter, memory), maxiter=maxiter, memory=memory, gtol=GTOL, ftol=FTOL)
    return (sx, sf) + bounds(sx, sf)


def noisy(fun, seed):
    """``fun`` with NOISE N(0, 1) on every value and gradient entry: results as far from the oracle's as the project lets a kernel be."""
    rng = np.random.default_rng(1000 + seed)

    def wrapped(x):
        f, g = fun(x)
        return f + NOISE * rng.standard_normal(f.shape), g + NOISE * rng.standard_normal(g.shape)

    return wrapped


def points(ref, x0):
    """x_k[K+1][B][T] (and f_k[K][B] for k >= 1) of a reference run: the start and the point after every iteration."""
    return np.stack([np.asarray(x0)] + [t["x"] for t in ref["trace"]]), np.stack([t["f"] for t in ref["trace"]])


def check_inputs(ref, maxiter, memory, gtol, *, wrap=True, disagreement=True, all_active=True, margin_floor=1e-6):
    """The conditions on an input, taken from the reference's trace alone.  A failure here says the inputs (jitter, seed) are
    wrong for the test, not the kernel.  ``margin_floor``: see MARGIN_FLOOR."""
    trace = ref["trace"]
    assert len(trace) == maxiter, f"the reference stopped after {len(trace)} of {maxiter} iterations"
    if wrap:
        assert maxiter > memory, "the history ring never wraps"
    if disagreement:   # some lane halves its step while another has accepted its first trial: was_done, the deferred history kernel
        assert any(t["trials"].max() >= 2 and (t["trials"] == 1).any() for t in trace), [t["trials"].tolist() for t in trace]
    for k, t in enumerate(trace):
        scale = margin_floor * np.maximum(1.0, np.abs(t["f_in"]))
        for m in t["margins"]:
            ok = np.isnan(m) | (np.abs(m) >= scale)
            assert ok.all(), f"iteration {k}: Armijo margin {m} is a knife edge"
        far = (t["gmax"] >= 10.0 * gtol) | (t["gmax"] <= 0.1 * gtol)
        assert (far | ~t["tested"]).all(), f"iteration {k}: max|g| {t['gmax']} within a decade of gtol {gtol}"
        if all_active:
            assert t["active_in"].all() and t["active"].all(), f"iteration {k}: a lane stopped"
    far = (ref["gmax"] >= 10.0 * gtol) | (ref["gmax"] <= 0.1 * gtol) | ~ref["active"]
    assert far.all(), f"final max|g| {ref['gmax']} within a decade of gtol {gtol}"
    if all_active:     # still running after the last iteration too
        assert ref["active"].all() and (ref["gmax"] >= 10.0 * gtol).all(), f"a lane is finished at the last point: max|g| {ref['gmax']}"


def spread(fun, x0, ref, **kw):
    """Largest deviation of x_k and f_k (k = 1 .. K) over NOISE_SEEDS reference runs on noisy(fun) from the run on fun: what a
    difference of NOISE in f and g does to this trajectory.  The noisy runs must take the decisions of the clean one."""
    xs, fs = points(ref, x0)
    sx, sf = np.zeros(len(fs)), np.zeros(len(fs))
    for seed in range(NOISE_SEEDS):
        run = lbfgs_ref(noisy(fun, seed), x0, **kw)
        assert [t["trials"].tolist() for t in run["trace"]] == [t["trials"].tolist() for t in ref["trace"]], "a decision flipped under noise"
        xn, fn = points(run, x0)
        sx = np.maximum(sx, np.abs(xn[1:] - xs[1:]).reshape(len(fs), -1).max(axis=1))
        sf = np.maximum(sf, np.abs(fn - fs).max(axis=1))
    return sx, sf


def bounds(sx, sf):
    """The device may deviate by ten times the measured spread (one decade for reductions in another order over up to 735 terms),
    and never by more than the existing comparisons allow."""
    return np.minimum(10.0 * sx, X_CAP), np.minimum(10.0 * sf, F_CAP)


def nfev_of(trace):
    """Evaluations of the batch: the start point and, per iteration, as many trials as the slowest lane took."""
    return 1 + sum(int(t["trials"].max()) for t in trace)
