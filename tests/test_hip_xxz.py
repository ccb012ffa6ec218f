"""GPU: the matrix-free XXZ Hamiltonian and the Chebyshev series of exp(-iHt) (aqc_research_amd/xxz.py, csrc/aqc_xxz.hip) against
the NumPy statement (tests/xxz_ref.py), against expm where a matrix fits, and against properties no size limits; the Trotter
states of the package against the exact ones; the driver's exact ground truth.

Sizes: a tiled kernel resolves bonds inside a tile, across two neighbouring tiles and between distant tiles; n = 2 .. 16 reaches
every one of those whatever the tile is (below a tile, exactly a tile, one straddling bond, the first high bonds)."""
import functools

import numpy as np
import pytest
from scipy.linalg import expm

from tests import xxz_ref
from tests.helpers import TOL

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-12
LANE_TIMES = (0.0, 0.3, 1.2, -1.2, 9.6)


def _maxdiff(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


@functools.lru_cache(maxsize=None)
def _states(n, lanes):
    return xxz_ref.random_states(n, lanes, 7000 + n)


def _neel(n):
    v = np.zeros(2**n, dtype=np.complex128)
    v[xxz_ref.neel_index(n)] = 1
    return v


@pytest.mark.parametrize("n", range(2, 17))
def test_mul_vec_matches_statement(n):
    """|H psi| terms: at most n + 1 products of size <= max(1/2, |delta| (n - 1) / 4) on a normalised state: rounding near 5e-14."""
    from aqc_research_amd.xxz import xxz_mul_vec

    states = _states(n, 3)
    before = states.copy()
    for delta in (1.0, -0.7, 0.0):
        got = xxz_mul_vec(states, delta)
        assert got.shape == states.shape and got.dtype == np.complex128
        err = _maxdiff(got, xxz_ref.mul_vec(states, delta))
        print(f"n = {n}, delta = {delta}: {err:.3g}")
        assert err <= STATE_TOL, (n, delta, err)
        for lane in range(3):
            assert np.array_equal(xxz_mul_vec(states[lane], delta), got[lane]), (n, delta, lane)
    assert np.array_equal(states, before)


@pytest.mark.parametrize("delta", (1.0, 2.5))
@pytest.mark.parametrize("n", (3, 8, 11, 12, 13, 16))
def test_evolve_matches_statement(n, delta):
    from aqc_research_amd.xxz import spectral_radius, xxz_evolve

    states = _states(n, len(LANE_TIMES))
    before = states.copy()
    k_ref = np.array([xxz_ref.series_length(xxz_ref.radius(n, delta) * t) for t in LANE_TIMES])
    for label, src in (("shared", states[0]), ("lanes", states)):
        got, info = xxz_evolve(src, delta, np.array(LANE_TIMES), details=True)
        assert got.shape == (len(LANE_TIMES), 2**n)
        assert info["terms"].dtype == np.int32 and np.array_equal(info["terms"], k_ref), (info["terms"], k_ref)
        assert info["radius"] == spectral_radius(n, delta) == xxz_ref.radius(n, delta)
        err = _maxdiff(got, xxz_ref.evolve_lanes(src, delta, LANE_TIMES))
        print(f"n = {n}, delta = {delta}, {label}: {err:.3g}, terms {info['terms'].tolist()}")
        assert err <= STATE_TOL, (n, delta, label, err)
        assert np.array_equal(got[0], np.broadcast_to(src, got.shape)[0])          # t = 0: a copy of the input
        if n <= 8:
            h = xxz_ref.dense_hamiltonian(n, delta)
            ref = np.stack([expm(-1j * t * h) @ np.broadcast_to(src, got.shape)[l] for l, t in enumerate(LANE_TIMES)])
            assert _maxdiff(got, ref) <= TOL
    assert np.array_equal(states, before)
    # a scalar time: one state -> one state; a stack -> the same time on every lane
    one = xxz_evolve(states[1], delta, 1.2)
    assert one.shape == (2**n,) and _maxdiff(one, xxz_ref.evolve_lanes(states[1], delta, [1.2])[0]) <= STATE_TOL
    same = xxz_evolve(states[:2], delta, 1.2)
    assert same.shape == (2, 2**n) and np.array_equal(same[1], one)


def test_properties_at_20_qubits():
    from aqc_research_amd.xxz import xxz_energy, xxz_evolve

    n, delta = 20, 1.0
    ini = _neel(n)
    index = np.arange(2**n, dtype=np.uint64)
    weight = np.zeros(2**n, dtype=np.int64)
    for q in range(n):
        weight += ((index >> np.uint64(q)) & np.uint64(1)).astype(np.int64)
    outside = weight != n // 2                                # the Neel state has n / 2 qubits up
    a = xxz_evolve(ini, delta, 0.8)
    assert np.all(a[outside] == 0.0)                          # H moves amplitude inside a magnetisation sector only: zeros stay zero
    assert np.count_nonzero(a[~outside]) > 1000
    assert abs(np.linalg.norm(a) - 1.0) <= STATE_TOL
    b = xxz_evolve(a, delta, 0.8)
    c = xxz_evolve(ini, delta, 1.6)
    assert np.all(c[outside] == 0.0)
    assert abs(np.linalg.norm(c) - 1.0) <= STATE_TOL
    assert _maxdiff(b, c) <= STATE_TOL
    back = xxz_evolve(c, delta, -1.6)
    assert _maxdiff(back, ini) <= STATE_TOL
    e0, e1 = xxz_energy(ini, delta), xxz_energy(c, delta)
    assert isinstance(e0, float) and e0 == delta * (n - 1) / 4      # every bond of the Neel state is anti-aligned
    assert abs(e1 - e0) <= STATE_TOL


def test_energy_matches_mul_vec_and_repeats():
    from aqc_research_amd.xxz import xxz_energy, xxz_mul_vec

    n = 13
    states = _states(n, 3)
    for delta in (1.0, -0.7):
        e = xxz_energy(states, delta)
        assert e.shape == (3,) and e.dtype == np.float64
        h = xxz_mul_vec(states, delta)
        for lane in range(3):
            assert abs(e[lane] - np.vdot(states[lane], h[lane]).real) <= STATE_TOL
            assert xxz_energy(states[lane], delta) == e[lane]
        assert np.array_equal(xxz_energy(states, delta), e)          # fixed-order sums: the same bits
    small = _states(4, 2)
    ref = [np.vdot(v, xxz_ref.dense_hamiltonian(4, 2.5) @ v).real for v in small]
    assert _maxdiff(xxz_energy(small, 2.5), ref) <= STATE_TOL


@pytest.mark.parametrize("n,t,delta", [(13, 1.2, 1.0), (12, 2.4, 0.5)])
def test_trotter_converges_to_exact(n, t, delta):
    """Second-order Trotter: the error of the state (global phase included) falls by 4 per doubling of the steps."""
    from aqc_research_amd.model_sp_lhs.time_evol import fidelity
    from aqc_research_amd.model_sp_lhs.trotter import XXZHamiltonian, exact_evolution, neel_init_state, trotter_state

    exact = exact_evolution(XXZHamiltonian(n, delta), neel_init_state(n), t)
    errs, last = [], None
    for steps in (4, 8, 16):
        last = trotter_state(n, evol_time=t, num_steps=steps, delta=delta, second_order=True, with_global_phase=True)
        errs.append(float(np.linalg.norm(last - exact)))
    factors = [errs[0] / errs[1], errs[1] / errs[2]]
    fid = fidelity(last, exact)
    print(f"n = {n}, t = {t}, delta = {delta}: errors {errs}, factors {factors}, fidelity {fid}")
    assert all(3.5 <= f <= 4.5 for f in factors), factors
    assert fid > 0.99999


def test_generate_target_with_exact_ground_truth():
    from aqc_research_amd.model_sp_lhs.time_evol import UserOptions, fidelity, generate_target
    from aqc_research_amd.model_sp_lhs.trotter import XXZHamiltonian, exact_evolution, neel_init_state, neel_state_index
    from aqc_research_amd.mps_operations import DenseBackedMPS
    from aqc_research_amd.xxz import xxz_evolve

    n = 12
    default = generate_target(UserOptions(num_qubits=n), 0)
    exact = generate_target(UserOptions(num_qubits=n, ground_truth="exact"), 0)
    t = exact.evol_time
    assert t == 1.2
    assert np.array_equal(exact.t1_gt, xxz_evolve(_neel(n), 1.0, t))
    assert np.array_equal(exact.t1, default.t1)
    assert not np.array_equal(exact.t1_gt, default.t1_gt)
    assert 0.9 < fidelity(exact.t1, exact.t1_gt) < 1.0
    assert 0.9 < fidelity(default.t1_gt, exact.t1_gt) <= 1.0 + 1e-12
    mps = generate_target(UserOptions(num_qubits=n, ground_truth="exact", objective="sur_fast_mps_trotter"), 0)
    assert isinstance(mps.t1_gt, DenseBackedMPS) and isinstance(mps.t1, DenseBackedMPS)
    assert np.array_equal(mps.t1_gt.dense_state, exact.t1_gt)
    ham = XXZHamiltonian(n, 1.0)
    by_circuit, by_index = exact_evolution(ham, neel_init_state(n), t), exact_evolution(ham, neel_state_index(n), t)
    assert np.array_equal(by_circuit, by_index) and np.array_equal(by_index, exact.t1_gt)
    assert np.array_equal(exact_evolution(ham, _neel(n), t), by_index)


def test_errors_and_buffer_lifetime():
    from ctypes import POINTER, c_int32

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.xxz import xxz_energy, xxz_evolve, xxz_mul_vec

    good = _states(5, 3)
    xxz_mul_vec(good, 1.0)                                     # the library is loaded and the device initialised
    before = live_buffers()
    with pytest.raises(ValueError):
        xxz_mul_vec(np.zeros(2, dtype=np.complex128), 1.0)     # n = 1
    with pytest.raises(ValueError):
        xxz_evolve(np.zeros(24, dtype=np.complex128), 1.0, 0.5)
    with pytest.raises(TypeError):
        xxz_energy(good.astype(np.complex64), 1.0)
    with pytest.raises(TypeError):
        xxz_evolve(good[:, ::2], 1.0, 0.5)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            xxz_evolve(good, 1.0, bad)
        with pytest.raises(ValueError):
            xxz_evolve(good, bad, 0.5)
        with pytest.raises(ValueError):
            xxz_mul_vec(good, bad)
        with pytest.raises(ValueError):
            xxz_energy(good, bad)
    with pytest.raises(ValueError):
        xxz_evolve(good, 1.0, [0.1, 0.2])                      # three lanes, two times
    with pytest.raises(ValueError):
        xxz_evolve(good, 1.0, np.zeros((3, 1)))
    # the C entry points check for themselves
    L = _lib.lib()
    src, dst = good.copy(), np.empty_like(good)
    times, terms = np.array([0.1, 0.2, 0.3]), np.zeros(3, dtype=np.int32)
    pt = terms.ctypes.data_as(POINTER(c_int32))
    d = _lib.dptr
    assert L.aqc_xxz_mul_vec(0, 1, 3, 1.0, d(src), d(dst)) != 0 and b"shape" in L.aqc_last_error()
    assert L.aqc_xxz_mul_vec(0, 31, 1, 1.0, d(src), d(dst)) != 0
    assert L.aqc_xxz_mul_vec(0, 5, 0, 1.0, d(src), d(dst)) != 0
    assert L.aqc_xxz_mul_vec(0, 30, 4, 1.0, d(src), d(dst)) != 0          # lanes << n beyond the build's limit
    assert L.aqc_xxz_mul_vec(0, 5, 3, float("nan"), d(src), d(dst)) != 0
    assert L.aqc_xxz_mul_vec(-1, 5, 3, 1.0, d(src), d(dst)) != 0
    assert L.aqc_xxz_mul_vec(L.aqc_device_count(), 5, 3, 1.0, d(src), d(dst)) != 0
    assert L.aqc_xxz_mul_vec(0, 5, 3, 1.0, None, d(dst)) != 0
    assert L.aqc_xxz_energy(0, 5, 3, 1.0, d(src), None) != 0
    assert L.aqc_xxz_evolve(0, 5, 3, 0, 1.0, None, d(src), d(dst), pt) != 0
    times[1] = float("inf")
    assert L.aqc_xxz_evolve(0, 5, 3, 0, 1.0, d(times), d(src), d(dst), pt) != 0 and b"finite" in L.aqc_last_error()
    times[1] = 1e300
    assert L.aqc_xxz_evolve(0, 5, 3, 0, 1.0, d(times), d(src), d(dst), pt) != 0 and b"terms" in L.aqc_last_error()
    times[1] = 0.2
    assert L.aqc_xxz_evolve(0, 5, 3, 0, 1.0, d(times), d(src), d(dst), None) == 0      # terms_out may be NULL
    assert L.aqc_xxz_evolve(0, 5, 3, 0, 1.0, d(times), d(src), d(src), pt) == 0        # dst may be src
    assert _maxdiff(src, dst) == 0.0 and np.all(terms >= 20)
    ref = xxz_ref.evolve_lanes(good, 1.0, times)
    assert _maxdiff(dst, ref) <= STATE_TOL
    assert live_buffers() == before
