"""CPU: the NumPy statement of measuring an MPS (tests/mps_sample_ref.py) against the dense vector -- amplitudes, the sampled
distribution, exact zeros -- and the margin condition that tests/test_hip_mps_sampling.py relies on, for its exact cases."""
import numpy as np
import pytest

from tests import mps_obs_ref, mps_sample_ref as ref


@pytest.mark.parametrize("name", ("A", "B2", "B13", "C", "D"))
def test_amplitudes_of_the_sampled_bits_are_entries_of_the_dense_vector(name):
    mps = ref.case(name)
    psi = mps_obs_ref.dense(mps)
    bits, amps, _ = ref.sample(mps, 300, seed=ref.PHILOX_SEED)
    assert bits.dtype == np.uint8 and bits.shape == (300, len(mps[0])) and set(np.unique(bits)) <= {0, 1}
    err = float(np.max(np.abs(amps - psi[ref.indices(bits)])))
    print(f"profile {name}: max |amplitude - dense| = {err:.3g}")
    # n products of at most max(dims) terms each, partial products of magnitude <= the norm: the worst case of plain rounding
    tol = len(mps[0]) * max(ref.CASES[name][0]) * np.finfo(np.float64).eps * ref.NORM
    assert err <= tol
    assert float(np.max(np.abs(ref.amplitudes(mps, bits) - amps))) <= tol
    assert abs(np.vdot(psi, psi).real - mps_obs_ref.norm2(mps)) <= 1e-12


def test_the_rule_samples_the_distribution_of_the_state():
    """n = 6: every one of the 64 frequencies within 5 binomial standard deviations of |psi|^2 / N (observed: the largest deviation is
    3.07 sigma)."""
    mps = mps_obs_ref.hand_made([1, 2, 4, 8, 4, 2, 1], 5)
    shots = 200_000
    bits, _, _ = ref.sample(mps, shots, seed=7)
    psi = mps_obs_ref.dense(mps)
    p = np.abs(psi) ** 2 / np.vdot(psi, psi).real
    freq = np.bincount(ref.indices(bits), minlength=64) / shots
    sigma = np.sqrt(p * (1.0 - p) / shots)
    worst = float(np.max(np.abs(freq - p) / sigma))
    print(f"largest deviation: {worst:.3g} sigma")
    assert worst <= 5.0


def test_branches_of_zero_weight_are_never_taken():
    n, k = 13, 0b1011001110001
    one = np.ones((1, 1), dtype=np.complex128)
    basis = ([((1.0 - ((k >> q) & 1)) * one, float((k >> q) & 1) * one) for q in range(n)], [np.ones(1) for _ in range(n - 1)])
    bits, amps, _ = ref.sample(basis, 200, seed=3)
    assert np.all(ref.indices(bits) == k) and np.all(amps == 1.0)
    # a product state: qubits 0, 3, 4 fixed to 1, 0, 1, the others in superposition
    rng = np.random.default_rng(8)
    gam = []
    for q in range(7):
        a, b = rng.standard_normal(2) + 1j * rng.standard_normal(2)
        if q in (0, 4):
            a = 0.0
        if q == 3:
            b = 0.0
        gam.append((a * one, b * one))
    product = (gam, [np.ones(1) for _ in range(6)])
    bits, amps, _ = ref.sample(product, 2000, seed=4)
    assert np.all(bits[:, 0] == 1) and np.all(bits[:, 3] == 0) and np.all(bits[:, 4] == 1)
    assert np.all(np.abs(amps) > 0.0)
    assert len(np.unique(ref.indices(bits))) == 16   # all 2^4 strings of the free qubits occur in 2000 shots


# (case, lanes the GPU test samples it on); smallest margins observed over shots 0 .. 4095 with Philox seed 2024:
# A 1.6e-5 (lane 1: 2.8e-5, lane 2: 7.1e-6), C 1.3e-4, D 3.0e-5, B13 1.1e-5, N40 5.8e-7, B2 3.0e-5
@pytest.mark.parametrize("name,lanes", (("A", (0, 1, 2)), ("C", (0,)), ("D", (0, 1)), ("B13", (0,)), ("N40", (0,)), ("B2", (0,))))
def test_no_shot_of_the_gpu_cases_is_near_a_threshold(name, lanes):
    mps = ref.case(name)
    for lane in lanes:
        _, _, margin = ref.sample(mps, 4096, seed=ref.PHILOX_SEED, lane=lane)
        print(f"profile {name}, lane {lane}: smallest margin {margin.min():.3g}")
        assert margin.min() >= ref.MARGIN, (name, lane, int(np.argmin(margin)))


def test_uniforms_depend_on_shot_and_lane_numbers_only():
    a = ref.uniforms(5, 1, range(10), 7)
    assert np.array_equal(a[3:6], ref.uniforms(5, 1, [3, 4, 5], 7))
    assert not np.array_equal(a, ref.uniforms(5, 2, range(10), 7)) and not np.array_equal(a, ref.uniforms(6, 1, range(10), 7))
    assert np.array_equal(ref.uniforms(5, 1, [4], 11)[0, :7], a[4])   # a longer register continues the same stream
