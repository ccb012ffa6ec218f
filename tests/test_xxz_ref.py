"""CPU-only: the NumPy statement of exact XXZ evolution (tests/xxz_ref.py) against the reference's own make_hamiltonian /
exact_evolution outputs (tests/golden/xxz.npz) and against scipy's expm; the host route of trotter.exact_evolution; the driver's
``ground_truth`` option; the ABI table."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import expm

from tests import xxz_ref
from tests.helpers import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION_TOL, AMP_TOL = 1e-14, 1e-13
DELTAS = (1.0, 0.5, -0.7, 0.0, 2.5)
TIMES = (0.3, 1.2, 9.6, -1.2)


@pytest.fixture(scope="module")
def golden():
    return load("xxz.npz")


def _maxdiff(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def test_fixture_covers_the_stated_cases(golden):
    names = [str(k) for k in golden["names"]]
    assert sorted(names) == sorted(f"n{n}_d{d}" for n in (2, 3, 5) for d in (1.0, 0.4))
    assert [float(t) for t in golden["times"]] == [0.7, 2.4]


def test_statement_matches_reference_outputs(golden):
    for key in (str(k) for k in golden["names"]):
        n, delta = int(golden[f"{key}/n"]), float(golden[f"{key}/delta"])
        h = golden[f"{key}/h"]
        assert _maxdiff(xxz_ref.dense_hamiltonian(n, delta), h) <= ACTION_TOL, key
        for tag in ("neel", "rand"):
            psi = golden[f"{key}/{tag}"]
            assert _maxdiff(xxz_ref.mul_vec(psi, delta), h @ psi) <= ACTION_TOL, (key, tag)
            for t in (float(t) for t in golden["times"]):
                err = _maxdiff(xxz_ref.evolve(psi, delta, t), golden[f"{key}/{tag}_t{t}"])
                assert err <= AMP_TOL, (key, tag, t, err)
    assert np.argmax(np.abs(golden["n5_d1.0/neel"])) == xxz_ref.neel_index(5)


@pytest.mark.parametrize("n", (2, 3, 4, 6, 8))
def test_statement_matches_dense_h_and_expm(n):
    psi = xxz_ref.random_states(n, 1, 40 + n)[0]
    worst_action = worst_amp = worst_norm = 0.0
    for delta in DELTAS:
        h = xxz_ref.dense_hamiltonian(n, delta)
        assert _maxdiff(h, h.conj().T) == 0.0 and _maxdiff(h.imag, 0.0) == 0.0      # real and symmetric
        assert np.linalg.norm(h, 2) <= xxz_ref.radius(n, delta) * (1 + 1e-12)
        worst_action = max(worst_action, _maxdiff(xxz_ref.mul_vec(psi, delta), h @ psi))
        for t in TIMES:
            got = xxz_ref.evolve(psi, delta, t)
            worst_amp = max(worst_amp, _maxdiff(got, expm(-1j * t * h) @ psi))
            worst_norm = max(worst_norm, abs(np.linalg.norm(got) - 1.0))
    print(f"n = {n}: action {worst_action:.3g}, amplitudes {worst_amp:.3g}, norm {worst_norm:.3g}")
    assert worst_action <= ACTION_TOL
    assert worst_amp <= AMP_TOL
    assert worst_norm <= AMP_TOL


def test_statement_edge_times():
    psi = xxz_ref.random_states(4, 1, 7)[0]
    assert np.array_equal(xxz_ref.evolve(psi, 1.0, 0.0), psi)
    assert xxz_ref.series_length(0.0) == 20
    back = xxz_ref.evolve(xxz_ref.evolve(psi, 0.5, 1.2), 0.5, -1.2)
    assert _maxdiff(back, psi) <= AMP_TOL


@pytest.mark.parametrize("n", (2, 5, 9))
def test_lane_forms_of_the_statement_agree(n):
    """The slice form of the action and the lane-wise series, which the GPU tests use at their larger sizes, against the plain ones."""
    states = xxz_ref.random_states(n, 4, 900 + n)
    times = (0.0, 0.3, -1.2, 9.6)
    for delta in (1.0, -0.7, 0.0, 2.5):
        assert _maxdiff(xxz_ref.mul_vec_slices(states, delta), xxz_ref.mul_vec(states, delta)) <= ACTION_TOL
        assert _maxdiff(xxz_ref.mul_vec_slices(states[1], delta), xxz_ref.mul_vec(states[1], delta)) <= ACTION_TOL
        each = np.stack([xxz_ref.evolve(states[l], delta, t) for l, t in enumerate(times)])
        assert _maxdiff(xxz_ref.evolve_lanes(states, delta, times), each) <= AMP_TOL
        shared = np.stack([xxz_ref.evolve(states[2], delta, t) for t in times])
        assert _maxdiff(xxz_ref.evolve_lanes(states[2], delta, times), shared) <= AMP_TOL


def test_exact_evolution_dense_route_reproduces_reference(golden):
    """trotter.exact_evolution with a dense ndarray Hamiltonian: the reference's own route, on the host, no GPU."""
    from aqc_research_amd.model_sp_lhs import trotter

    for key in (str(k) for k in golden["names"]):
        n, delta = int(golden[f"{key}/n"]), float(golden[f"{key}/delta"])
        ham = trotter.XXZHamiltonian(n, delta)
        assert (ham.num_qubits, ham.delta) == (n, delta)
        h = ham.matrix()
        assert _maxdiff(h, golden[f"{key}/h"]) <= ACTION_TOL
        for t in (float(t) for t in golden["times"]):
            for tag in ("neel", "rand"):
                got = trotter.exact_evolution(h, golden[f"{key}/{tag}"], t)
                assert _maxdiff(got, golden[f"{key}/{tag}_t{t}"]) <= AMP_TOL, (key, tag, t)
            by_index = trotter.exact_evolution(h, trotter.neel_state_index(n), t)
            by_circuit = trotter.exact_evolution(h, trotter.neel_init_state(n), t)
            assert _maxdiff(by_index, golden[f"{key}/neel_t{t}"]) <= AMP_TOL
            assert np.array_equal(by_index, by_circuit)


def test_exact_evolution_argument_errors():
    from aqc_research_amd.model_sp_lhs import trotter

    h = trotter.make_hamiltonian(3, 1.0)
    with pytest.raises(ValueError):
        trotter.exact_evolution(h, np.zeros(4, dtype=np.complex128), 1.0)
    with pytest.raises(ValueError):
        trotter.exact_evolution(h, 8, 1.0)
    with pytest.raises(ValueError):
        trotter.exact_evolution(h[:, :4], 0, 1.0)
    with pytest.raises(ValueError):
        trotter.exact_evolution(h, 0, float("nan"))
    with pytest.raises(TypeError):
        trotter.exact_evolution("xxz", 0, 1.0)
    for bad in ((1, 1.0), (31, 1.0), (4, float("inf"))):
        with pytest.raises(ValueError):
            trotter.XXZHamiltonian(*bad)


def test_user_options_ground_truth():
    from aqc_research_amd.model_sp_lhs.time_evol import UserOptions, generate_target

    assert UserOptions().ground_truth == "trotter"
    assert UserOptions(ground_truth="exact").ground_truth == "exact"
    for bad in ("Exact", "expm", None, 1):
        with pytest.raises(ValueError):
            UserOptions(ground_truth=bad)
    # an MPS objective beyond dense reach has no dense state to hold the exact one: refused before anything touches a device
    with pytest.raises(ValueError):
        generate_target(UserOptions(ground_truth="exact", objective="sur_fast_mps_trotter", num_qubits=26), 0)


def test_python_argument_errors_need_no_device():
    from aqc_research_amd import xxz

    good = np.zeros(8, dtype=np.complex128)
    with pytest.raises(TypeError):
        xxz.xxz_mul_vec(good.astype(np.complex64), 1.0)
    with pytest.raises(TypeError):
        xxz.xxz_evolve(np.zeros((2, 8, 1), dtype=np.complex128), 1.0, 1.0)
    with pytest.raises(TypeError):
        xxz.xxz_energy(np.zeros((8, 2), dtype=np.complex128).T, 1.0)
    with pytest.raises(ValueError):
        xxz.xxz_mul_vec(np.zeros(2, dtype=np.complex128), 1.0)          # n = 1
    with pytest.raises(ValueError):
        xxz.xxz_mul_vec(np.zeros(12, dtype=np.complex128), 1.0)
    with pytest.raises(ValueError):
        xxz.xxz_evolve(good, float("nan"), 1.0)
    with pytest.raises(ValueError):
        xxz.xxz_evolve(good, 1.0, float("inf"))
    with pytest.raises(ValueError):
        xxz.xxz_evolve(np.zeros((3, 8), dtype=np.complex128), 1.0, [0.1, 0.2])
    with pytest.raises(ValueError):
        xxz.xxz_evolve(good, 1.0, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        xxz.xxz_evolve(good, 1.0, [])
    assert xxz.spectral_radius(5, -2.0) == xxz_ref.radius(5, -2.0) == 4.0
    with pytest.raises(ValueError):
        xxz.spectral_radius(1, 1.0)


def test_abi_names_declared():
    from aqc_research_amd import _lib

    header = open(os.path.join(ROOT, "include", "aqc_hip.h")).read()
    for name in ("aqc_xxz_mul_vec", "aqc_xxz_energy", "aqc_xxz_evolve"):
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint " + name + r"\s*\(", header), name
