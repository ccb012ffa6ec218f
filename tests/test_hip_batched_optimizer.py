"""GPU: vectorised multi-start L-BFGS on the lane-batched surrogate objective (batched_optimizer.py) reaches what
scipy's L-BFGS-B reaches lane by lane on SpSurrogateObjectiveMax, and its first evaluation equals that objective's."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff

pytestmark = pytest.mark.gpu


def _problem(n=8, layers=2, lanes=6, seed=5):
    from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index, trotter_ansatz, trotter_state

    circ = trotter_ansatz(n, layers, True)
    neel = neel_state_index(n)
    rng = np.random.default_rng(seed)
    targets, starts = [], []
    for j in range(lanes):
        t = 0.5 + 0.25 * j
        targets.append(trotter_state(n, evol_time=t, num_steps=6, delta=1.0, second_order=True))
        starts.append(init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=t, delta=1.0) + 0.05 * rng.standard_normal(circ.num_thetas))
    return circ, neel, np.stack(targets), np.stack(starts)


def test_first_evaluation_equals_single_lane_objective():
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_max import SpSurrogateObjectiveMax

    circ, neel, targets, starts = _problem(lanes=4)
    bo = BatchedSurrogateObjective(circ, targets, base_index=neel)
    f, g = bo.value_and_grad(starts, update_state=False)      # weight = 1, leading state = |state_0>: 1 - |h_0|^2
    for b in range(4):
        user = dict(num_qubits=circ.num_qubits, max_flips=1, state_prep_func=lambda _n: neel, enable_optim_stats=False, verbose=0, maxiter=5)
        o = SpSurrogateObjectiveMax(user_parameters=user, circ=circ, front_layer=True)
        o.set_target(targets[b])
        assert abs(o.objective(starts[b]) - f[b]) < TOL
        assert maxdiff(o.gradient(starts[b]), g[b]) < TOL
    bo.close()


def test_batched_lbfgs_reaches_scipy_fidelities():
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective, batched_lbfgs
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_max import SpSurrogateObjectiveMax
    from aqc_research_amd.optimizer import AqcOptimizer

    circ, neel, targets, starts = _problem()
    ref = []
    for b in range(len(targets)):
        user = dict(num_qubits=circ.num_qubits, max_flips=1, state_prep_func=lambda _n: neel, enable_optim_stats=False, verbose=0, maxiter=40)
        o = SpSurrogateObjectiveMax(user_parameters=user, circ=circ, front_layer=True)
        o.set_target(targets[b])
        ref.append(AqcOptimizer(optimizer_name="lbfgs", maxiter=40).optimize(o, circ, starts[b])["fidelity"])
    bo = BatchedSurrogateObjective(circ, targets, base_index=neel)
    res = batched_lbfgs(bo.value_and_grad, starts, maxiter=40)
    fid = bo.fidelity
    bo.close()
    assert res["x"].shape == starts.shape and np.isfinite(res["fun"]).all()
    for b in range(len(targets)):
        assert fid[b] > 0.99 and fid[b] > ref[b] - 5e-3, (b, fid[b], ref[b])
    # the final point really has that fidelity (independent check through the oracle on one lane)
    a = orc.as_ansatz(circ)
    x = np.zeros(1 << circ.num_qubits, complex)
    x[neel] = 1
    assert abs(abs(np.vdot(orc.v_mul_vec(a, res["x"][2], x), targets[2])) ** 2 - fid[2]) < 1e-9


def test_batched_lbfgs_on_plain_quadratics():
    """The optimizer alone, on B independent convex quadratics with known minimisers (no GPU state involved)."""
    from aqc_research_amd.batched_optimizer import batched_lbfgs

    rng = np.random.default_rng(2)
    B, T = 5, 12
    A = np.stack([(lambda m: m @ m.T + 0.5 * np.eye(T))(rng.standard_normal((T, T))) for _ in range(B)])
    xs = rng.standard_normal((B, T))

    def fun(x, _update):
        r = x - xs
        return 0.5 * np.einsum("bt,btu,bu->b", r, A, r), np.einsum("btu,bu->bt", A, r)

    res = batched_lbfgs(fun, np.zeros((B, T)), maxiter=300, gtol=1e-10, ftol=0.0)
    assert maxdiff(res["x"], xs) < 1e-7


def test_asp_driver_with_vectorised_restarts():
    from aqc_research_amd.model_sp_lhs.time_evol import UserOptions, run_simulation

    base = dict(num_qubits=8, num_horizons=2, num_layers_inc=1, trotter_steps_per_horizon=6, maxiter=25)
    single = run_simulation(UserOptions(**base))
    multi = run_simulation(UserOptions(num_seeds=6, theta_jitter=0.02, vectorised_lbfgs=True, **base))
    assert [r["status"] for r in multi] == ["ok", "ok"]
    for s, m in zip(single, multi):
        assert len(m["fidelities"]) == 6 and m["thetas"].shape == (m["num_thetas"],)
        assert m["fidelity"] > s["fidelity"] - 5e-3 and m["fidelity"] > 0.9


def test_batched_aqc_restarts_recover_planted_unitaries():
    """Full-range AQC objective over lanes: first evaluation == the oracle's objective and gradient per lane; the
    vectorised L-BFGS then compiles every planted unitary from a perturbed start."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.batched_optimizer import BatchedSketchingObjective, batched_lbfgs
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    n, lanes = 3, 5
    rng = np.random.default_rng(9)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", 14))
    a = orc.as_ansatz(circ)
    eye = np.eye(1 << n, dtype=complex)
    truth = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    targets = np.stack([orc.v_mul_mat(a, t, eye) for t in truth])
    starts = truth + 0.1 * rng.standard_normal(truth.shape)
    bo = BatchedSketchingObjective(circ, targets)
    f, g = bo.value_and_grad(starts)
    for b in range(lanes):
        fr, gr = orc.sketching_objective_and_gradient(a, starts[b], eye, targets[b])
        assert abs(f[b] - fr) < TOL and maxdiff(g[b], gr) < TOL
    res = batched_lbfgs(bo.value_and_grad, starts, maxiter=300, gtol=1e-9)
    bo.close()
    assert np.all(res["fun"] < 1e-6)
    for b in range(lanes):
        v = orc.v_mul_mat(a, res["x"][b], eye)
        assert abs(np.vdot(v, targets[b])) / (1 << n) > 1 - 1e-6


def test_device_resident_lbfgs_matches_the_host_version():
    """aqc_ws_lbfgs: the same multi-start L-BFGS with thetas / gradients / history resident in HBM.  Same algorithm as
    batched_lbfgs on the same objective => the same trajectories up to rounding: every lane ends at the fidelity the
    host version (and scipy, see the test above) reaches, and the reported point really has that fidelity."""
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective, batched_lbfgs

    circ, neel, targets, starts = _problem()
    bo = BatchedSurrogateObjective(circ, targets, base_index=neel)
    host = batched_lbfgs(bo.value_and_grad, starts, maxiter=40)
    fid_host = bo.fidelity.copy()
    bo.close()
    bo = BatchedSurrogateObjective(circ, targets, base_index=neel)
    dev = bo.minimize_on_device(starts, maxiter=40)
    fid_dev = bo.fidelity.copy()
    bo.close()
    assert dev["x"].shape == starts.shape and np.isfinite(dev["fun"]).all() and dev["nfev"] > 0
    for b in range(len(targets)):
        assert fid_dev[b] > 0.99 and fid_dev[b] > fid_host[b] - 5e-3, (b, fid_dev[b], fid_host[b])
        assert abs(dev["fun"][b] - (1.0 - fid_dev[b])) < 1e-9      # leading state is |state_0> here: f = 1 - fidelity
    a = orc.as_ansatz(circ)
    x = np.zeros(1 << circ.num_qubits, complex)
    x[neel] = 1
    for b in (0, len(targets) - 1):
        assert abs(abs(np.vdot(orc.v_mul_vec(a, dev["x"][b], x), targets[b])) ** 2 - fid_dev[b]) < 1e-9


def _leading_flip_state_case(depth):
    """Targets close to a flipped basis state: the surrogate's second sweep (leading state != |state_0>) runs inside the
    device loop; the device result must agree with the host version lane by lane.  The CPU oracle has no evaluation under a
    frozen state (its SurMaxOracle updates the state with every call, where a line-search trial must not), so for this branch
    the host loop on the device's value_and_grad is the comparison; tests/test_hip_optimisers_wide.py compares the same
    kernels with the oracle while |state_0> leads."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective, batched_lbfgs
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    n, B = 8, 3
    rng = np.random.default_rng(808)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", depth))
    targets = []
    for b in range(B):   # mostly the state with qubit b flipped, a little of everything else
        t = 0.05 * (rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n))
        t[1 << b] += 1.0
        targets.append(t / np.linalg.norm(t))
    targets = np.stack(targets)
    starts = 0.02 * rng.standard_normal((B, circ.num_thetas))
    bo = BatchedSurrogateObjective(circ, targets)
    host = batched_lbfgs(bo.value_and_grad, starts, maxiter=15)
    f_host, lead_host = host["fun"].copy(), bo.max_no.copy()
    bo.close()
    bo = BatchedSurrogateObjective(circ, targets)
    dev = bo.minimize_on_device(starts, maxiter=15)
    lead_dev = bo.max_no.copy()
    bo.close()
    df, dx = np.max(np.abs(dev["fun"] - f_host)), np.max(np.abs(dev["x"] - host["x"]))
    print(f"T = {circ.num_thetas}: leading states {lead_host}, |f_dev - f_host| = {df:.2e}, |x_dev - x_host| = {dx:.2e}, nit {dev['nit']} / {host['nit']}")
    assert (lead_host != 0).any()                      # the case this test is about really occurs
    assert df < 1e-6 and dx < 1e-5
    return circ, host, dev, lead_host, lead_dev


def test_device_resident_lbfgs_with_leading_flip_state():
    _leading_flip_state_case(10)


def test_device_resident_lbfgs_with_leading_flip_state_past_256_parameters():
    """Depth 60 at 8 qubits, T = 264: the kMat = false step kernels, lb_copy_raw and the second evaluation of accepted points
    with more than one parameter per thread.  The same bounds, and the same leading states and iteration counts besides."""
    circ, host, dev, lead_host, lead_dev = _leading_flip_state_case(60)
    assert circ.num_thetas == 264
    assert (lead_dev == lead_host).all() and (dev["nit"] == host["nit"]).all()
