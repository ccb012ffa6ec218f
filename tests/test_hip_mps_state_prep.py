"""GPU: general state-preparation circuits on the native MPS route -- MpsStateHandler (the reference's objective_base.py:345-435),
the lanes' bank of lhs states with its overlap kernel (lanes_bank_dot_kernel, aqc_mpsb_vh_bank), and the surrogate objective on
both engine paths, checked against the dense route within its reach and against the NumPy transfer-matrix walk (tests/mps_trunc_ref.py)
beyond it."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import maxdiff
from tests.mps_trunc_ref import RefMPS, apply_circuit, dot as ref_dot, fast_dot_gradient
from tests.test_mps_state_prep import _Circ, ref_prep_states

pytestmark = pytest.mark.gpu


def _random_unitary(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _bank_state(n, layers, rng, cap=32):
    """A normalised device MPS: random brickwork of `layers` layers on |0..0>, bonds capped at `cap` (0 layers: a basis state)."""
    from aqc_research_amd.mps_engine import DeviceMPS

    m = DeviceMPS.basis_state(n, int(rng.integers(0, 2 ** min(n, 62))))
    for lay in range(layers):
        for q in range(lay % 2, n - 1, 2):
            m.gate2(_random_unitary(rng, 4), q, q + 1, 1e-16, cap)
    return m


def _trotter(n, layers=1, second_order=False):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit

    return TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=second_order)


def _ref(m):
    return RefMPS.from_qiskit(m.to_qiskit())


_BANKS = {}


def _bank(n, kind):
    """(states, their RefMPS): K = 1 with the largest bond, or K = n + 1 with bonds 1, mixed and (where the register allows) 32."""
    key = (n, kind)
    if key not in _BANKS:
        rng = np.random.default_rng(100 + n)
        if kind == "one":
            states = [_bank_state(n, 12, rng)]
        else:
            states = [_bank_state(n, k % 13, rng) for k in range(n + 1)]
        _BANKS[key] = (states, [_ref(m) for m in states])
    return _BANKS[key]


@pytest.mark.parametrize("n", [2, 3, 16, 32])
@pytest.mark.parametrize("kind", ["one", "all"])
@pytest.mark.parametrize("lanes,half", [(1, False), (2, False), (2, True), (64, False), (64, True)])
def test_bank_overlaps_match_single_dots_and_reference(n, kind, lanes, half):
    from aqc_research_amd.mps_engine import LockstepLanes

    states, refs = _bank(n, kind)
    bonds = [int(m.bond_dims.max()) for m in states]
    if n >= 16:   # bonds 1, mixed and exactly 32 are all in the bank
        assert max(bonds) == 32 and (kind == "one" or min(bonds) == 1)
    rng = np.random.default_rng(7 * n + lanes)
    circ = _trotter(n)
    distinct = lanes // 2 if half else lanes
    targets = [_bank_state(n, 2, rng, cap=4) for _ in range(min(distinct, 4))]
    tg = [targets[l % len(targets)] for l in range(distinct)]
    th = 0.4 * np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(distinct)])
    if half:
        tg, th = tg + tg, np.concatenate([th, th])
    lk = LockstepLanes(n, lanes).set_targets(tg).set_bank(states)
    amps = lk.apply_vh_bank(circ, th, trunc_thr=1e-16, max_bond=32, half=half)
    assert amps.shape == (lanes, len(states))
    again = lk.apply_vh_bank(circ, th, trunc_thr=1e-16, max_bond=32, half=half)
    assert np.array_equal(amps.view(np.float64), again.view(np.float64))   # bit-reproducible
    check = sorted({0, lanes // 2 - 1 if lanes > 1 else 0, lanes // 2, lanes - 1} & set(range(lanes)))
    for l in check:
        vh = lk.export(l)
        rv = _ref(vh)
        for k, (m, r) in enumerate(zip(states, refs)):
            scale = np.sqrt(abs(ref_dot(r, r)) * abs(ref_dot(rv, rv)))
            assert abs(amps[l, k] - m.dot(vh)) <= 1e-12 * scale, (l, k)
            assert abs(amps[l, k] - ref_dot(r, rv)) <= 1e-12 * scale, (l, k)
        vh.close()
    lk.close()


def test_bank_refuses_bonds_beyond_the_lanes():
    from aqc_research_amd.mps_engine import LockstepLanes

    n = 14
    rng = np.random.default_rng(33)
    big = _bank_state(n, 12, rng, cap=33)
    assert int(big.bond_dims.max()) == 33
    lk = LockstepLanes(n, 2)
    with pytest.raises(RuntimeError, match="lockstep lanes"):
        lk.set_bank([_bank_state(n, 0, rng), big])
    lk.close()


def _prep_circuit(n, rng):
    """Non-adjacent cx / cp / swap both ways, u, rotations and a global phase."""
    qc = _Circ(n, phase=-0.7)
    for q in range(n):
        qc.add("ry", [q], [float(rng.uniform(-1, 1))])
    qc.add("h", [0]).add("cx", [0, n - 1]).add("cp", [n - 2, 1], [0.9]).add("swap", [2, n - 3]).add("u", [3], [0.3, 1.2, -0.5])
    qc.add("cx", [4, 5]).add("cz", [n - 1, 2]).add("sx", [1]).add("cy", [5, 0]).add("rz", [n - 1], [0.4])
    return qc


def test_handler_states_match_generic_state_handler_columns():
    from aqc_research_amd.model_sp_lhs.objective_base import GenericStateHandler, MpsStateHandler

    n = 8
    qc = _prep_circuit(n, np.random.default_rng(8))
    mh = MpsStateHandler(n, 1, lambda _n: qc)
    gh = GenericStateHandler(n, 1, lambda _n: qc)
    assert mh.num_states == gh.num_states == n + 1
    for i in range(n + 1):
        assert maxdiff(orc.mps_to_vector(mh.init_state(i)), gh.init_state(i)) < 1e-13
    assert maxdiff(orc.mps_to_vector(mh.state0), gh.state0) < 1e-13
    vec = mh.device_state(3)
    assert abs(mh.state_dot_vector(2, vec) - np.vdot(gh.init_state(2), gh.init_state(3))) < 1e-13
    assert abs(mh.state_dot_vector(2, mh.init_state(3)) - np.vdot(gh.init_state(2), gh.init_state(3))) < 1e-13
    with pytest.raises(NotImplementedError):
        mh.init_composite_state(np.zeros(2))
    mh.close()


def _target(circ, th, start):
    from aqc_research_amd.mps_engine import v_mul_mps

    return v_mul_mps(circ, th, start, trunc_thr=1e-16, method="single").to_qiskit()


def _run(objv, th, iters, step, rng):
    out = []
    for _ in range(iters):
        f = objv.objective(th)
        g = objv.gradient(th)
        out.append((f, g, objv._max_no, objv._weight))
        th = th - step * g + 0.01 * rng.standard_normal(th.size)
    return out


def _assert_same(a, b, tol):
    for (f1, g1, m1, w1), (f2, g2, m2, w2) in zip(a, b):
        assert m1 == m2 and abs(f1 - f2) < tol and abs(w1 - w2) < tol and maxdiff(g1, g2) < tol


@pytest.mark.parametrize("n", [8, 10])
def test_objective_mps_route_matches_dense_route(monkeypatch, n):
    from aqc_research_amd import mps_engine
    from aqc_research_amd.model_sp_lhs.objective_base import GenericStateHandler, MpsStateHandler
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter

    rng = np.random.default_rng(n)
    qc = _prep_circuit(n, rng)
    circ = _trotter(n, 1, second_order=True)
    th = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    start = MpsStateHandler(n, 1, qc).device_state(n // 2)   # the target leans towards a flip state: the leading state changes
    target = _target(circ, th + 0.05 * rng.standard_normal(th.size), start)
    runs = {}
    for route in ("dense", "lanes", "single"):
        monkeypatch.setenv("AQC_MPS_METHOD", "dense" if route == "dense" else "mps")
        monkeypatch.setattr(mps_engine, "LOCKSTEP_MAX_BOND", 0 if route == "single" else 32)
        user = dict(num_qubits=n, max_flips=1, state_prep_func=lambda _n: qc, enable_optim_stats=False, verbose=0, maxiter=5, trunc_thr=1e-16)
        o = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
        o.set_target(target)
        assert isinstance(o._state_handler, GenericStateHandler if route == "dense" else MpsStateHandler)
        runs[route] = _run(o, th.copy(), 4, 0.05, np.random.default_rng(1))
        if route != "dense":
            assert o._native_mps and o._lk_live == (route == "lanes")
    assert any(m != 0 for _, _, m, _ in runs["dense"])   # the combined sweep was taken
    _assert_same(runs["dense"], runs["lanes"], 1e-11)
    _assert_same(runs["dense"], runs["single"], 1e-11)


def _surrogate_reference(circ, target_q, states, th, iters, step, rng, thr=1e-16):
    """The surrogate objective's state machine (objective_lhs_sur_max.py) on RefMPS: amplitudes and sweeps by transfer matrices."""
    tgt = RefMPS.from_qiskit(target_q)
    w, max_no, out = 1.0, 0, []
    for _ in range(iters):
        vh = apply_circuit(circ, th, tgt.copy(), inverse=True, thr=thr)
        hs = np.array([ref_dot(x, vh) for x in states])
        hs2 = np.abs(hs) ** 2
        best = hs2[max_no]
        for i in range(len(hs)):
            if 1.1 * best < hs2[i]:
                best, max_no = hs2[i], i
        f = float(1.0 - (1.0 - w) * hs2[0] - w * hs2[max_no])
        if max_no == 0:
            g = (fast_dot_gradient(circ, th, states[0], vh, thr)[0] * (-2 * np.conj(hs[0]))).real
        else:
            c0, cm = -2 * (1 - w) * np.conj(hs[0]), -2 * w * np.conj(hs[max_no])
            g = (c0 * fast_dot_gradient(circ, th, states[0], vh, thr)[0] + cm * fast_dot_gradient(circ, th, states[max_no], vh, thr)[0]).real
        out.append((f, g, max_no, w + 0.1 * (np.sqrt(abs(f)) - w)))
        w = out[-1][3]
        th = th - step * g + 0.01 * rng.standard_normal(th.size)
    return out


def _prep32(n):
    qc = _Circ(n, phase=0.0)
    for q in range(n):
        qc.add("h", [q])
    for q in range(n - 1):
        qc.add("cx", [q, q + 1])
    qc.add("cx", [3, 9]).add("cp", [20, 11], [0.8])
    for q in range(n):
        qc.add("ry", [q], [0.1 * (q % 7) - 0.3])
    return qc


def test_beyond_dense_reach_matches_the_transfer_matrix_reference(monkeypatch):
    from aqc_research_amd import mps_engine
    from aqc_research_amd.model_sp_lhs.objective_base import MpsStateHandler
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter

    n = 32
    monkeypatch.delenv("AQC_MPS_METHOD", raising=False)
    rng = np.random.default_rng(32)
    qc = _prep32(n)
    circ = _trotter(n, 1)
    th = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    target = _target(circ, th + 0.03 * rng.standard_normal(th.size), MpsStateHandler(n, 1, qc).device_state(5))
    ref = _surrogate_reference(circ, target, ref_prep_states(qc, n), th.copy(), 3, 0.05, np.random.default_rng(2))
    runs = {}
    for route in ("lanes", "single"):
        monkeypatch.setattr(mps_engine, "LOCKSTEP_MAX_BOND", 0 if route == "single" else 32)
        user = dict(num_qubits=n, max_flips=1, state_prep_func=lambda _n: qc, enable_optim_stats=False, verbose=0, maxiter=5)
        o = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
        o.set_target(target)
        assert o._native_mps and isinstance(o._state_handler, MpsStateHandler)
        runs[route] = _run(o, th.copy(), 3, 0.05, np.random.default_rng(2))
        assert o._lk_live == (route == "lanes")
    assert ref[0][0] < 0.9   # the prepared states overlap the target: the values are not trivially 1 and 0
    _assert_same(ref, runs["lanes"], 1e-10)
    _assert_same(ref, runs["single"], 1e-10)
    _assert_same(runs["lanes"], runs["single"], 1e-12)


def test_front_door_general_preparation_at_32_qubits():
    from aqc_research_amd.model_sp_lhs.objective_base import MpsStateHandler
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter
    from aqc_research_amd.optimizer import AqcOptimizer

    n = 32
    rng = np.random.default_rng(320)
    qc = _prep32(n)
    circ = _trotter(n, 1)
    th_true = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    target = _target(circ, th_true, MpsStateHandler(n, 1, qc).device_state(0))
    user = dict(num_qubits=n, max_flips=1, state_prep_func=lambda _n: qc, enable_optim_stats=False, verbose=0, maxiter=6, trunc_thr=1e-12)
    objv = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)   # NotImplementedError before MpsStateHandler
    objv.set_target(target)
    th0 = th_true + 0.03 * rng.standard_normal(th_true.size)
    f0 = objv.objective(th0)
    res = AqcOptimizer(optimizer_name="lbfgs", maxiter=6).optimize(objv, circ, th0)
    assert objv._native_mps and objv._lk_live and f0 > 1e-3
    assert res["cost"] < 0.5 * f0
    bad = _Circ(n).add("h", [0]).add("ccx", [0, 1, 2])
    with pytest.raises(NotImplementedError, match="'ccx'"):
        SpSurrogateObjectiveFastMpsTrotter(user_parameters=dict(user, state_prep_func=lambda _n: bad), circ=circ)


def test_preparation_beyond_the_lanes_runs_on_the_single_lane_engine(monkeypatch):
    from aqc_research_amd.model_sp_lhs.objective_base import MpsStateHandler
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter

    n = 12
    rng = np.random.default_rng(12)
    qc = _Circ(n, phase=0.2)
    for q in range(n // 2):   # six Bell pairs across the middle: bond 64 there
        qc.add("h", [q]).add("cx", [q, q + n // 2])
    for q in range(n):
        qc.add("ry", [q], [float(rng.uniform(-1, 1))])
    circ = _trotter(n, 1)
    th = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    h = MpsStateHandler(n, 1, qc)
    assert h.max_bond == 64
    target = _target(circ, th + 0.05 * rng.standard_normal(th.size), h.device_state(2))
    runs = {}
    for route in ("dense", "mps"):
        monkeypatch.setenv("AQC_MPS_METHOD", route)
        user = dict(num_qubits=n, max_flips=1, state_prep_func=lambda _n: qc, enable_optim_stats=False, verbose=0, maxiter=5, trunc_thr=1e-16)
        o = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
        o.set_target(target)
        runs[route] = _run(o, th.copy(), 2, 0.05, np.random.default_rng(3))
        if route == "mps":
            assert o._native_mps and o._lk_refused and not o._lk_live
    _assert_same(runs["dense"], runs["mps"], 1e-11)
