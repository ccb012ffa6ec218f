"""CPU-only: the NumPy statement of reduced density matrices (tests/obs_ref.py) against <psi|O|psi> from dense Kronecker products, and
the host-only algebra of aqc_research_amd/observables.py (Pauli strings, argument checks) against the statement."""
import itertools

import numpy as np
import pytest

from tests import obs_ref, xxz_ref

TOL = 1e-13   # sums of at most 64 products of amplitudes of a normalised state


@pytest.mark.parametrize("n", range(2, 7))
def test_statement_matches_dense_expectations(n):
    psi = xxz_ref.random_states(n, 1, 300 + n)[0]
    worst = 0.0
    for i, j in itertools.permutations(range(n), 2):
        rho = obs_ref.rdm(psi, (i, j))
        assert abs(np.trace(rho) - 1) <= TOL and np.max(np.abs(rho - rho.conj().T)) <= TOL
        for a, b in itertools.product("ixyz", repeat=2):
            want = obs_ref.dense_expectation(psi, {i: a, j: b})
            worst = max(worst, abs(obs_ref.expectation(rho, a + b) - want))
    for q in range(n):
        for a in "xyz":
            worst = max(worst, abs(obs_ref.expectation(obs_ref.rdm(psi, (q,)), a) - obs_ref.dense_expectation(psi, {q: a})))
    assert worst <= TOL, worst


@pytest.mark.parametrize("n", (4, 5, 6))
def test_statement_four_site_string(n):
    psi = xxz_ref.random_states(n, 1, 400 + n)[0]
    qubits = (n - 1, 0, 2, 1)
    rho = obs_ref.rdm(psi, qubits)
    want = obs_ref.dense_expectation(psi, dict(zip(qubits, "xyzx")))
    assert abs(obs_ref.expectation(rho, "xyzx") - want) <= TOL
    # a three-qubit matrix is the partial trace of it over the last listed qubit (the highest index bit)
    part = rho.reshape(2, 8, 2, 8).trace(axis1=0, axis2=2)
    assert np.max(np.abs(part - obs_ref.rdm(psi, qubits[:3]))) <= TOL


@pytest.mark.parametrize("n", range(2, 7))
def test_single_qubit_matrix_is_the_same_from_every_pair(n):
    psi = xxz_ref.random_states(n, 1, 500 + n)[0]
    for q in range(n):
        want = obs_ref.rdm(psi, (q,))
        for other in range(n):
            if other == q:
                continue
            first = obs_ref.rdm(psi, (q, other)).reshape(2, 2, 2, 2).trace(axis1=0, axis2=2)    # row index = q + 2 other
            second = obs_ref.rdm(psi, (other, q)).reshape(2, 2, 2, 2).trace(axis1=1, axis2=3)
            assert np.max(np.abs(first - want)) <= TOL and np.max(np.abs(second - want)) <= TOL


def test_pair_order_is_a_transposition_of_the_index_bits():
    psi = xxz_ref.random_states(5, 1, 77)[0]
    swap = [0, 2, 1, 3]
    a, b = obs_ref.rdm(psi, (1, 4)), obs_ref.rdm(psi, (4, 1))
    assert np.array_equal(a[np.ix_(swap, swap)], b)


def test_module_algebra_matches_statement():
    from aqc_research_amd import observables as obs

    psi = xxz_ref.random_states(6, 2, 78)
    for letters in ("x", "zz", "xy", "yi", "xyz", "xyzx"):
        assert np.array_equal(obs.pauli_matrix(letters), obs_ref.pauli_on_rdm(letters))
        qubits = (5, 0, 3, 2)[: len(letters)]
        rho = np.stack([obs_ref.rdm(s, qubits) for s in psi])
        got = obs.pauli_expectation(rho, letters.upper())
        assert got.shape == (2,)
        for lane in range(2):
            assert abs(got[lane] - obs_ref.expectation(rho[lane], letters)) <= TOL
        assert isinstance(obs.pauli_expectation(rho[0], letters), float)
    with pytest.raises(ValueError):
        obs.pauli_expectation(np.eye(4) / 4, "xq")
    with pytest.raises(ValueError):
        obs.pauli_expectation(np.eye(4) / 4, "x")
    with pytest.raises(ValueError):
        obs.pauli_expectation(np.eye(4) / 4, "")


def test_argument_checks_need_no_device():
    from aqc_research_amd import observables as obs

    good = np.zeros(8, dtype=np.complex128)
    good[0] = 1
    with pytest.raises(TypeError):
        obs.pair_density_matrices(good.astype(np.complex64))
    with pytest.raises(TypeError):
        obs.pair_density_matrices(np.zeros((8, 2), dtype=np.complex128).T)
    with pytest.raises(ValueError):
        obs.pair_density_matrices(np.zeros(12, dtype=np.complex128))
    with pytest.raises(ValueError):
        obs.pair_density_matrices(good, [(1, 1)])
    with pytest.raises(ValueError):
        obs.pair_density_matrices(good, [(0, 3)])
    with pytest.raises(ValueError):
        obs.pair_density_matrices(good, [])
    with pytest.raises(ValueError):
        obs.pair_density_matrices(good, [(0, 1, 2)])
    with pytest.raises(ValueError):
        obs.reduced_density_matrix(np.zeros(64, dtype=np.complex128), (0, 1, 2, 3, 4))
    with pytest.raises(ValueError):
        obs.reduced_density_matrix(good, (0, 1, 2, 2))
    with pytest.raises(ValueError):
        obs.magnetisation(good, "q")
    with pytest.raises(ValueError):
        obs.correlation_matrix(good, "z")
    with pytest.raises(ValueError):
        obs.bond_energies(good, float("nan"))
