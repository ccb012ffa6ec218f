"""GPU: pair density matrices of DeviceMPS states (aqc_research_amd/mps_observables.py, csrc/aqc_mps_obs.hip) against the dense statement
(tests/obs_ref.py on mps_to_vector of the state), against the NumPy statement of the MPS formulas (tests/mps_obs_ref.py) beyond dense
reach, and against properties that need no reference; the derived figures against observables.py; the driver's option.

Bond profiles (n = 13 unless said): A reaches the fused cap with bonds that are no multiples of 4 or 16 and rectangular sites, B are
product states (n = 2 has no chain step at all), C has a bond of 1 inside, D lies beyond the fused cap (the rule picks gemm), F is
oracle.random_mps(13, 8).  The tolerance is the project's TOL = 1e-10 for normalised states; the tests print what they observe and
DESIGN.md 6p records it."""
import functools

import numpy as np
import pytest

from tests import mps_obs_ref, obs_ref, xxz_ref
from tests.helpers import TOL

pytestmark = pytest.mark.gpu

PROFILES = {
    "A": (mps_obs_ref.PROFILE_A, 601), "B2": (mps_obs_ref.profile_b(2), 602), "B4": (mps_obs_ref.profile_b(4), 603),
    "B13": (mps_obs_ref.profile_b(13), 604), "C": (mps_obs_ref.PROFILE_C, 605), "D": (mps_obs_ref.PROFILE_D, 606),
}
NAMES = sorted(PROFILES) + ["F"]
FUSED_NAMES = [k for k in NAMES if k != "D"]


def _maxdiff(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(QiskitMPS tuple, dense vector, the dense statement's matrices of all pairs): computed once, never changed."""
    from aqc_research_amd.mps_operations import mps_to_vector

    if name == "F":
        from oracle.aqc_oracle import random_mps

        mps = random_mps(13, 8, np.random.default_rng(607))
    else:
        mps = mps_obs_ref.hand_made(*PROFILES[name])
    psi = mps_to_vector(mps)
    n = len(mps[0])
    want = obs_ref.pair_rdms(psi, obs_ref.all_pairs(n))
    for arr in (psi, want):
        arr.setflags(write=False)
    return mps, psi, want


def _device(name):
    from aqc_research_amd.mps_engine import DeviceMPS

    return DeviceMPS.from_qiskit(_case(name)[0])


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


@pytest.mark.parametrize("method", (None, "fused", "gemm"))
@pytest.mark.parametrize("name", NAMES)
def test_all_pairs_match_the_dense_statement(name, method):
    from aqc_research_amd.mps_observables import pair_density_matrices, route

    _, psi, want = _case(name)
    m = _device(name)
    try:
        assert route(m.bond_dims) == ("gemm" if name == "D" else "fused")
        if name == "D" and method == "fused":
            with pytest.raises(ValueError):
                pair_density_matrices(m, method="fused")
            return
        before = _flat(m.to_qiskit())
        got = pair_density_matrices(m, method=method)
        assert got.shape == want.shape and got.dtype == np.complex128
        err = _maxdiff(got, want)
        # properties that need no reference
        assert np.array_equal(got, got.conj().transpose(0, 2, 1))
        assert np.all(got.imag[:, np.arange(4), np.arange(4)] == 0.0)
        tr_err = float(np.max(np.abs(np.trace(got, axis1=1, axis2=2) - m.dot(m))))
        print(f"profile {name}, method {method}: max |rho - statement| = {err:.3g}, max |tr rho - <psi|psi>| = {tr_err:.3g}")
        assert err <= TOL, (name, method, err)
        assert tr_err <= TOL, (name, method, tr_err)
        assert np.array_equal(_flat(m.to_qiskit()), before)
    finally:
        m.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_state_scaled_by_three_gives_nine_rho(name):
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import pair_density_matrices

    gam, lam = _case(name)[0]
    scaled = ([(3.0 * gam[0][0], 3.0 * gam[0][1])] + list(gam[1:]), lam)
    for method in ((None, "gemm") if name == "D" else (None, "fused", "gemm")):
        one, three = pair_density_matrices(_case(name)[0], method=method), pair_density_matrices(scaled, method=method)
        err = _maxdiff(three, 9.0 * one)
        print(f"profile {name}, method {method}: max |rho(3 psi) - 9 rho(psi)| = {err:.3g}")
        assert err <= 9 * TOL, (name, method, err)
    m = DeviceMPS.from_qiskit(scaled)
    try:
        assert abs(m.dot(m) - 9.0) <= 9 * TOL
    finally:
        m.close()


@pytest.mark.parametrize("name", FUSED_NAMES)
def test_the_two_routes_agree(name):
    from aqc_research_amd.mps_observables import pair_density_matrices

    m = _device(name)
    try:
        fused, gemm = pair_density_matrices(m, method="fused"), pair_density_matrices(m, method="gemm")
    finally:
        m.close()
    diff = _maxdiff(fused, gemm)
    print(f"profile {name}: max |fused - gemm| = {diff:.3g}")
    assert diff <= 2 * TOL   # each within TOL of the statement
    assert np.array_equal(pair_density_matrices(_case(name)[0]), fused)   # the rule's choice, and a tuple uploaded for the call


@pytest.mark.parametrize("method", (None, "gemm"))
def test_lanes_subsets_orders_and_duplicates_are_bit_for_bit(method):
    from aqc_research_amd.mps_observables import pair_density_matrices

    states = [_device(k) for k in ("A", "B13", "F")]
    try:
        n = 13
        pairs = obs_ref.all_pairs(n)
        got = pair_density_matrices(states, method=method)
        assert got.shape == (3, len(pairs), 4, 4)
        for lane, m in enumerate(states):
            assert np.array_equal(pair_density_matrices(m, method=method), got[lane]), lane
        assert np.array_equal(pair_density_matrices(states, method=method), got)
        pick = [3, 17, 18, 40, 77]                                         # a subset of the pairs: other chains, shorter walks
        sub = pair_density_matrices(states, [pairs[k] for k in pick], method=method)
        assert np.array_equal(sub, got[:, pick])
        swapped = pair_density_matrices(states, [(j, i) for i, j in pairs], method=method)
        swap = [0, 2, 1, 3]
        assert np.array_equal(swapped, got[..., swap, :][..., :, swap])
        mixed = [(12, 0), (0, 12), (5, 6), (0, 12), (6, 5), (5, 6)]          # both orders and repeats in one list
        dup = pair_density_matrices(states, mixed, method=method)
        assert np.array_equal(dup[:, 1], dup[:, 3]) and np.array_equal(dup[:, 2], dup[:, 5])
        assert np.array_equal(dup[:, 1], got[:, pairs.index((0, 12))]) and np.array_equal(dup[:, 2], got[:, pairs.index((5, 6))])
        assert np.array_equal(dup[:, 0], dup[:, 1][..., swap, :][..., :, swap]) and np.array_equal(dup[:, 4], dup[:, 2][..., swap, :][..., :, swap])
        if method is None:   # A, B13 and F all go the fused way; D beside them goes its own
            d = _device("D")
            try:
                four = pair_density_matrices(states + [d])
                assert np.array_equal(four[:3], got) and np.array_equal(four[3], pair_density_matrices(d, method="gemm"))
            finally:
                d.close()
    finally:
        for m in states:
            m.close()


@pytest.mark.parametrize("name", ("A", "F"))
def test_derived_figures_match_observables_on_the_dense_state(name):
    from aqc_research_amd import mps_observables as mo
    from aqc_research_amd import observables as ob

    mps, psi, _ = _case(name)
    psi = np.array(psi)
    n = 13
    m = _device(name)
    try:
        worst = 0.0
        for axis in "xyz":
            got = mo.magnetisation(m, axis)
            assert got.shape == (n,)
            worst = max(worst, _maxdiff(got, ob.magnetisation(psi, axis)))
        for letters, connected in (("zz", False), ("xy", False), ("zz", True), ("xy", True)):
            got = mo.correlation_matrix(m, letters, connected)
            assert got.shape == (n, n)
            worst = max(worst, _maxdiff(got, ob.correlation_matrix(psi, letters, connected)))
        for delta in (1.0, -0.7):
            bonds = mo.bond_energies(m, delta)
            assert bonds.shape == (n - 1,)
            worst = max(worst, _maxdiff(bonds, ob.bond_energies(psi, delta)))
            energy = float(np.vdot(psi, xxz_ref.mul_vec(psi, delta)).real)
            # n - 1 bonds, each an operator of norm <= 1/2 + |delta|/4 on a matrix within TOL
            assert abs(bonds.sum() - energy) <= (n - 1) * TOL, (name, delta)
        print(f"profile {name}: derived figures, max difference from observables.py = {worst:.3g}")
        assert worst <= TOL
        both = mo.magnetisation([m, mps], "z")
        assert both.shape == (2, n) and np.array_equal(both[0], both[1])
        one = mo.reduced_density_matrix(m, (4,))
        assert one.shape == (2, 2) and _maxdiff(one, obs_ref.rdm(psi, (4,))) <= TOL
        assert _maxdiff(mo.reduced_density_matrix(m, (12,)), obs_ref.rdm(psi, (12,))) <= TOL
        assert _maxdiff(mo.reduced_density_matrix([m, m], (7, 2)), np.stack([obs_ref.rdm(psi, (7, 2))] * 2)) <= TOL
    finally:
        m.close()


def _trotter(n, layers=3, evol_time=0.8):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index

    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)
    th = init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=evol_time, delta=1.0)
    return circ, th, neel_state_index(n)


@pytest.mark.parametrize("engine", ("single", "lockstep"))
def test_engine_made_states(engine):
    """The Neel state at n = 12 under a second-order Trotter ansatz: exact against the dense statement, truncated against the statement of
    its own exported tensors -- together they pin the reading of the engine's tensor layout (Schmidt values folded into the sites)."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import pair_density_matrices
    from aqc_research_amd.mps_operations import mps_to_vector

    n = 12
    circ, th, neel = _trotter(n)
    pairs = obs_ref.all_pairs(n)
    basis = me.DeviceMPS.basis_state(n, neel)

    def make(thr, max_bond=0):
        if engine == "single":
            return me.v_mul_mps(circ, th, basis, trunc_thr=thr, max_bond=max_bond, method="single")
        lanes = me.LockstepLanes(n, 1)
        try:
            lanes.set_targets(basis)
            lanes.apply_circuit(circ, th[None, :], trunc_thr=thr, max_bond=max_bond)
            return lanes.export(0)
        finally:
            lanes.close()

    exact, cut = make(1e-16), make(1e-3)
    try:
        for method in (None, "gemm"):
            err = _maxdiff(pair_density_matrices(exact, method=method), obs_ref.pair_rdms(mps_to_vector(exact.to_qiskit()), pairs))
            got = pair_density_matrices(cut, method=method)
            err_cut = _maxdiff(got, mps_obs_ref.pair_rdms(cut.to_qiskit(), pairs))
            tr = float(np.max(np.abs(np.trace(got, axis1=1, axis2=2) - cut.dot(cut))))
            print(f"{engine}, method {method}: exact (bonds <= {exact.bond_dims.max()}) {err:.3g}; truncated (bonds <= {cut.bond_dims.max()}) "
                  f"{err_cut:.3g}, trace {tr:.3g}")
            assert err <= TOL and err_cut <= TOL and tr <= TOL
        assert cut.bond_dims.max() < exact.bond_dims.max()
    finally:
        for m in (exact, cut, basis):
            m.close()


def test_forty_qubits():
    """Beyond dense reach: n = 40, engine-made with max_bond = 16, against the NumPy statement of the MPS formulas."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import pair_density_matrices

    n = 40
    circ, th, neel = _trotter(n, layers=6, evol_time=2.4)
    basis = me.DeviceMPS.basis_state(n, neel)
    m = me.v_mul_mps(circ, th, basis, trunc_thr=1e-14, max_bond=16)
    try:
        assert m.bond_dims.max() == 16   # the cap binds
        pairs = [(q, q + 1) for q in range(n - 1)] + [(0, 39), (39, 0), (3, 21), (17, 38), (20, 22), (1, 39), (0, 2)]
        want = mps_obs_ref.pair_rdms(m.to_qiskit(), pairs)
        norm = m.dot(m)
        for method in (None, "fused", "gemm"):
            got = pair_density_matrices(m, pairs, method=method)
            err = _maxdiff(got, want)
            tr = float(np.max(np.abs(np.trace(got, axis1=1, axis2=2) - norm)))
            print(f"n = {n}, bonds <= {m.bond_dims.max()}, method {method}: max |rho - statement| = {err:.3g}, trace {tr:.3g}")
            assert err <= TOL and tr <= TOL
            assert np.array_equal(got, got.conj().transpose(0, 2, 1))
    finally:
        m.close()
        basis.close()


def test_abi_refusals_and_a_correct_call_afterwards():
    from ctypes import POINTER, c_int32, c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import pair_density_matrices

    L = _lib.lib()
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))   # noqa: E731
    a, d, one, five = _device("C"), _device("D"), DeviceMPS.basis_state(1), DeviceMPS.basis_state(5)
    try:
        out = np.zeros((2, 2, 4, 4), dtype=np.complex128)
        good = np.array([0, 1, 3, 2], dtype=np.int32)
        hs = (c_void_p * 2)(a.handle, a.handle)

        def call(states, nstates, npairs, pairs, method=0, dst=out):
            return L.aqc_mps_obs_pairs(states, nstates, npairs, None if pairs is None else i32(pairs), method, None if dst is None else _lib.dptr(dst))

        assert call(None, 2, 2, good) == 1 and call(hs, 2, 2, None) == 1 and call(hs, 2, 2, good, dst=None) == 1   # null pointers
        assert call((c_void_p * 2)(a.handle, None), 2, 2, good) == 1
        assert call(hs, 0, 2, good) == 1 and call(hs, 2, 0, good) == 1
        assert call((c_void_p * 1)(one.handle), 1, 1, good) == 1                                     # n < 2
        assert call(hs, 2, 1, np.array([0, 4], dtype=np.int32)) == 1 and call(hs, 2, 1, np.array([-1, 2], dtype=np.int32)) == 1
        assert call(hs, 2, 1, np.array([2, 2], dtype=np.int32)) == 1
        assert call((c_void_p * 2)(a.handle, five.handle), 2, 2, good) == 1                          # different n
        assert call(hs, 2, 2, good, method=3) == 1
        assert call((c_void_p * 1)(d.handle), 1, 1, good, method=1) == 1 and b"fused" in L.aqc_last_error()
        live = live_buffers()
        assert call(hs, 2, 2, good) == 0
        assert _maxdiff(out[1], obs_ref.pair_rdms(np.array(_case("C")[1]), [(0, 1), (3, 2)])) <= TOL
        assert live_buffers() == live
        with pytest.raises(ValueError):
            pair_density_matrices(a, [(0, 4)])
    finally:
        for m in (a, d, one, five):
            m.close()


def test_driver_records_observables_from_mps_states(monkeypatch):
    from aqc_research_amd import observables as ob
    from aqc_research_amd.model_sp_lhs import time_evol as te
    from aqc_research_amd.mps_operations import mps_to_vector

    kw = dict(num_horizons=1, num_layers_inc=1, maxiter=3, fidelity_thr=0.9, objective="sur_fast_mps_trotter")
    dense = te.run_simulation(te.UserOptions(observables=True, num_qubits=6, **kw))[0]["observables"]
    mps = te.run_simulation(te.UserOptions(observables="mps", num_qubits=6, **kw))[0]["observables"]
    assert sorted(mps) == sorted(dense) == ["bond_energies", "bond_energies_gt", "magnetisation", "magnetisation_gt"]
    for key in dense:
        assert mps[key].shape == dense[key].shape
        err = _maxdiff(mps[key], dense[key])
        print(f"n = 6, {key}: |mps - dense| = {err:.3g}")
        assert err <= TOL, (key, err)
    with pytest.raises(ValueError):
        te.UserOptions(observables="mps", objective="sur_max")
    # beyond dense reach the states come from the native engine as plain tuples
    n = 4
    monkeypatch.setattr(te, "_DENSE_MAX_QUBITS", 3)
    opts = te.UserOptions(observables="mps", num_qubits=n, **kw)
    rec = te.run_simulation(opts)[0]
    got = rec["observables"]
    gt = te.generate_target(opts, 0).t1_gt
    assert isinstance(gt, tuple) and not hasattr(gt, "dense_state")
    psi = mps_to_vector(gt)
    assert _maxdiff(got["magnetisation_gt"], ob.magnetisation(psi)) <= TOL
    assert _maxdiff(got["bond_energies_gt"], ob.bond_energies(psi, opts.delta)) <= TOL
    from aqc_research_amd.model_sp_lhs.trotter import trotter_ansatz
    from aqc_research_amd.mps_operations import no_truncation_threshold

    a1 = mps_to_vector(te._evolved_state(opts, trotter_ansatz(n, rec["num_layers"], opts.second_order_trotter), rec["thetas"], no_truncation_threshold()))
    assert _maxdiff(got["magnetisation"], ob.magnetisation(a1)) <= TOL and _maxdiff(got["bond_energies"], ob.bond_energies(a1, opts.delta)) <= TOL
    with pytest.raises(ValueError):   # what the dense option refuses stays refused
        te.generate_target(te.UserOptions(observables=True, num_qubits=n, **kw), 0)


def test_chains_walked_in_several_groups():
    """Bonds of 512: the gemm route's scratch of a chain is 9 x 512^2 complex numbers (36 MiB), so the 256 MiB of a group hold 7 of the
    10 chains and the walk is made twice.  No reference is formed at this size: a call with one pair has one chain and one group, and a
    pair's matrix must not depend on what else is in the call -- bit for bit -- nor its trace on anything but <psi|psi>."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import pair_density_matrices, route

    dims = [1, 8, 64, 512, 512, 512, 300, 512, 512, 64, 8, 1]
    n = len(dims) - 1
    m = DeviceMPS.from_qiskit(mps_obs_ref.hand_made(dims, 608))
    try:
        assert route(m.bond_dims) == "gemm"
        pairs = [(q, q + 1) for q in range(n - 1)] + [(0, 10), (2, 7), (3, 9), (7, 3), (8, 10)]
        got = pair_density_matrices(m, pairs)
        tr = float(np.max(np.abs(np.trace(got, axis1=1, axis2=2) - m.dot(m))))
        print(f"bonds <= 512, two groups of chains: max |tr rho - <psi|psi>| = {tr:.3g}")
        assert tr <= TOL
        assert np.array_equal(got, got.conj().transpose(0, 2, 1))
        for k in (0, 6, 7, 9, 10, 11, 12, 13, 14):   # chains of the first group, of the second, and pairs that cross many sites
            assert np.array_equal(pair_density_matrices(m, [pairs[k]])[0], got[k]), pairs[k]
        swap = [0, 2, 1, 3]
        assert np.array_equal(got[13], pair_density_matrices(m, [(3, 7)])[0][swap, :][:, swap])
    finally:
        m.close()
