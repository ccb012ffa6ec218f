"""GPU: device-resident L-BFGS on the matrix objective of full / fixed-sketch AQC (aqc_ws_lbfgs_mat,
BatchedSketchingObjective.minimize_on_device, model_sketching.aqc_sketching.full_aqc) against the host loop
(batched_lbfgs on value_and_grad) and the CPU oracle."""
import functools

import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff

pytestmark = pytest.mark.gpu


def _circ(n, ent, depth):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, ent, create_ansatz_structure(n, "spin", "full", depth))


@functools.lru_cache(maxsize=None)
def _planted(n=3, ent="cx", depth=14, lanes=5, seed=9):
    """The problem of test_batched_aqc_restarts_recover_planted_unitaries: planted unitaries, starts truth + 0.1 N(0, 1).
    Built once and shared; nobody writes into the arrays (they are made read-only)."""
    rng = np.random.default_rng(seed)
    circ = _circ(n, ent, depth)
    a = orc.as_ansatz(circ)
    eye = np.eye(1 << n, dtype=complex)
    truth = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    targets = np.stack([orc.v_mul_mat(a, t, eye) for t in truth])
    starts = truth + 0.1 * rng.standard_normal(truth.shape)
    for arr in (truth, targets, starts):
        arr.setflags(write=False)
    return circ, a, truth, targets, starts


def _device(circ, targets, starts, x_mat=None, **kw):
    from aqc_research_amd.batched_optimizer import BatchedSketchingObjective

    bo = BatchedSketchingObjective(circ, targets, x_mat=x_mat)
    try:
        return bo.minimize_on_device(np.array(starts), **kw)
    finally:
        bo.close()


def _host(circ, targets, starts, x_mat=None, **kw):
    from aqc_research_amd.batched_optimizer import BatchedSketchingObjective, batched_lbfgs

    bo = BatchedSketchingObjective(circ, targets, x_mat=x_mat)
    try:
        return batched_lbfgs(bo.value_and_grad, np.array(starts), **kw)
    finally:
        bo.close()


@functools.lru_cache(maxsize=None)
def _converged():
    circ, _, _, targets, starts = _planted()
    return _device(circ, targets, starts, maxiter=300, gtol=1e-9)


def test_trajectory_matches_the_host_loop():
    """15 iterations of the device loop and of batched_lbfgs on value_and_grad, same memory / gtol / ftol: same algorithm on
    the same kernels' results, so the same trajectory up to the rounding of the host's NumPy sums against the device's."""
    circ, _, _, targets, starts = _planted()
    kw = dict(maxiter=15, memory=10, gtol=1e-7, ftol=1e-12)
    host = _host(circ, targets, starts, **kw)
    dev = _device(circ, targets, starts, **kw)
    df, dx = maxdiff(dev["fun"], host["fun"]), maxdiff(dev["x"], host["x"])
    print(f"trajectory: max|f_dev - f_host| = {df:.3e}, max|x_dev - x_host| = {dx:.3e}, nit dev {dev['nit']} host {host['nit']}")
    assert set(dev) == {"x", "fun", "nit", "nfev", "fidelity", "status"}
    assert (dev["status"] == 0).all()
    assert df < 1e-6 and dx < 1e-5
    assert (dev["nit"] == host["nit"]).all()


def test_end_point_is_what_the_oracle_says():
    """maxiter=300, gtol=1e-9: every lane compiles its planted unitary, and the oracle -- not the code under test -- confirms the
    reported value and the overlap at the returned point."""
    circ, a, _, targets, _ = _planted()
    res = _converged()
    d = circ.dimension
    eye = np.eye(d, dtype=complex)
    print("end point: fun", res["fun"], "nit", res["nit"], "nfev", res["nfev"])
    assert (res["status"] == 0).all()
    for b in range(len(targets)):
        fr, _ = orc.sketching_objective_and_gradient(a, res["x"][b], eye, targets[b])
        ov = abs(np.vdot(orc.v_mul_mat(a, res["x"][b], eye), targets[b])) / d
        print(f"  lane {b}: |fun - oracle| = {abs(res['fun'][b] - fr):.3e}, overlap = 1 - {1 - ov:.3e}")
        assert abs(res["fun"][b] - fr) < TOL
        assert res["fun"][b] < 1e-6
        assert ov > 1 - 1e-6
        assert abs(res["fidelity"][b] - ov * ov) < 1e-9          # |tr|^2 / d^2 with X = I


@pytest.mark.parametrize("n,ent,depth", [(4, "cp", 8), (3, "cz", 6)])
def test_other_entanglers_and_a_fixed_sketch(n, ent, depth):
    """cp (5 thetas per block) and cz, with X = the first 4 columns of a fixed unitary (k < d): 10 iterations against the host
    loop, bounds of the trajectory test."""
    circ, _, _, targets, starts = _planted(n, ent, depth, 3, 21)
    d = circ.dimension
    rng = np.random.default_rng(4)
    x_mat = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0][:, :4])
    kw = dict(maxiter=10, memory=10, gtol=1e-7, ftol=1e-12)
    host = _host(circ, targets, starts, x_mat=x_mat, **kw)
    dev = _device(circ, targets, starts, x_mat=x_mat, **kw)
    df, dx = maxdiff(dev["fun"], host["fun"]), maxdiff(dev["x"], host["x"])
    print(f"{ent}: max|f_dev - f_host| = {df:.3e}, max|x_dev - x_host| = {dx:.3e}, fun {dev['fun']}")
    assert (dev["status"] == 0).all() and (dev["nit"] > 0).all()
    assert df < 1e-6 and dx < 1e-5
    a = orc.as_ansatz(circ)
    for b in range(3):   # the value reported is the sketched objective at the returned point
        fr, _ = orc.sketching_objective_and_gradient(a, dev["x"][b], x_mat, targets[b] @ x_mat)
        assert abs(dev["fun"][b] - fr) < TOL


def test_lane_isolation_and_repeatability():
    circ, _, _, targets, starts = _planted()
    kw = dict(maxiter=12)
    one = _device(circ, targets[:4], starts[:4], **kw)
    two = _device(circ, targets[:4], starts[:4], **kw)
    assert one["x"].tobytes() == two["x"].tobytes() and one["fun"].tobytes() == two["fun"].tobytes()
    alone = _device(circ, targets[2:3], starts[2:3], **kw)
    assert alone["x"][0].tobytes() == one["x"][2].tobytes() and alone["fun"][0].tobytes() == one["fun"][2].tobytes()
    assert alone["nit"][0] == one["nit"][2] > 0


def test_stops():
    circ, _, truth, targets, starts = _planted()
    free = _converged()
    thr = _device(circ, targets, starts, maxiter=300, gtol=1e-9, fobj_thr=1e-3)
    print("stops: fun", thr["fun"], "nit", thr["nit"], "unconstrained nit", free["nit"])
    assert (thr["fun"] <= 1e-3).all() and (thr["nit"] < free["nit"]).all() and (thr["status"] == 0).all()
    fid = _device(circ, targets, starts, maxiter=300, gtol=1e-9, fidelity_thr=0.99)
    assert (fid["fidelity"] >= 0.99).all() and (fid["nit"] < free["nit"]).all()
    # a lane that starts at its planted thetas has nothing to do
    mixed = np.array(starts)
    mixed[1] = truth[1]
    res = _device(circ, targets, mixed, maxiter=20)
    assert res["nit"][1] == 0 and res["x"][1].tobytes() == truth[1].tobytes() and (res["nit"][[0, 2, 3, 4]] > 0).all()
    # maxiter = 1: exactly one accepted step
    step = _device(circ, targets, starts, maxiter=1)
    f0 = _device(circ, targets, starts, maxiter=1, fobj_thr=10.0)      # stopped before the first step: the start point's values
    assert (f0["nit"] == 0).all() and f0["x"].tobytes() == starts.tobytes() and f0["nfev"] == 1
    assert (step["nit"] == 1).all() and (step["fun"] < f0["fun"]).all()
    assert (np.abs(step["x"] - starts).max(axis=1) > 0).all()
    assert 2 <= step["nfev"] <= 13                                     # the start point and at most max_backtracks trials


def test_a_bad_lane_does_not_poison_the_batch():
    circ, _, _, targets, starts = _planted()
    good = _device(circ, targets, starts, maxiter=12)
    bad = np.array(starts)
    bad[3, 7] = np.nan
    res = _device(circ, targets, bad, maxiter=12)
    assert res["status"][3] != 0 and res["x"][3].tobytes() == bad[3].tobytes() and res["nit"][3] == 0
    keep = [0, 1, 2, 4]
    assert (res["status"][keep] == 0).all()
    assert res["x"][keep].tobytes() == good["x"][keep].tobytes() and res["fun"][keep].tobytes() == good["fun"][keep].tobytes()
    assert (res["nit"][keep] == good["nit"][keep]).all()


def test_argument_checks_and_a_one_column_workspace():
    from aqc_research_amd import _lib
    from aqc_research_amd.batched_optimizer import BatchedSketchingObjective

    circ, a, _, targets, starts = _planted()
    d = circ.dimension
    rng = np.random.default_rng(2)
    x = rng.standard_normal((d, 1)) + 1j * rng.standard_normal((d, 1))
    x /= np.linalg.norm(x)
    bo = BatchedSketchingObjective(circ, targets[:2], x_mat=x)           # ncols = 1: a state vector is a one-column matrix
    assert bo.ws.ncols == 1
    L, h = bo.ws._L, bo.ws.handle
    th = np.array(starts[:2])
    xo, f = np.empty_like(th), np.empty(2)

    def call(x0=th, maxiter=5, memory=5, out=xo, fo=f, ws=h):
        return L.aqc_ws_lbfgs_mat(ws, None if x0 is None else _lib.dptr(x0), maxiter, memory, 1e-7, 1e-12, 0.0, 0.0, 12,
                                  None if out is None else _lib.dptr(out), None if fo is None else _lib.dptr(fo), None, None, None, None)

    for bad in (dict(memory=0), dict(memory=33), dict(maxiter=0), dict(x0=None), dict(out=None), dict(fo=None), dict(ws=None)):
        with pytest.raises(RuntimeError, match="aqc_hip: .*(null|memory|maxiter)"):
            _lib.check(call(**bad))
    assert call() == 0                                                   # optional outputs may all be NULL
    res = bo.minimize_on_device(th, maxiter=8)
    bo.close()
    assert (res["status"] == 0).all() and (res["nit"] > 0).all()
    for b in range(2):
        f0, _ = orc.sketching_objective_and_gradient(a, starts[b], x, targets[b] @ x)
        fr, _ = orc.sketching_objective_and_gradient(a, res["x"][b], x, targets[b] @ x)
        assert abs(res["fun"][b] - fr) < TOL and res["fun"][b] < f0


def test_full_aqc():
    from aqc_research_amd.model_sketching.aqc_sketching import full_aqc, stochastic_aqc

    circ, _, _, targets, starts = _planted()
    ref = _device(circ, targets, starts, maxiter=12)
    many = full_aqc(circ, targets, starts, maxiter=12)
    assert isinstance(many, list) and len(many) == 5
    for b, r in enumerate(many):
        assert set(r) >= {"cost", "num_fun_ev", "num_grad_ev", "num_iters", "thetas", "entangler", "blocks", "exit_status"}
        assert r["thetas"].tobytes() == ref["x"][b].tobytes() and r["cost"] == ref["fun"][b]
        assert r["exit_status"] == "normal" and r["num_iters"] == ref["nit"][b] and r["entangler"] == "cx"
    single = full_aqc(circ, targets[2], starts[2], maxiter=12)
    assert isinstance(single, dict) and single["thetas"].shape == (circ.num_thetas,)
    alone = _device(circ, targets[2:3], starts[2:3], maxiter=12)
    assert single["thetas"].tobytes() == alone["x"][0].tobytes() and single["cost"] == alone["fun"][0]
    early = full_aqc(circ, targets, starts, maxiter=300, fobj_thr=1e-3)
    assert all(r["exit_status"] == "early" and r["cost"] <= 1e-3 for r in early)
    with pytest.raises(ValueError, match="full_aqc"):
        stochastic_aqc(circ, targets[0], "full", 8, starts[0], maxiter=5, learn_rate=0.1)
