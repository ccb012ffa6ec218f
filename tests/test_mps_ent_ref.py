"""CPU: the NumPy statement of the Schmidt spectra (tests/mps_ent_ref.py) against SVDs of the dense vector, why the statement is a QR
chain and not the eigenvalues of L_q R_q, the entropies on analytic inputs, and the rank rule of the ABI against the statement of the
truncation reference (tests/mps_trunc_ref.decide).

Profiles as in tests/test_hip_mps_pauli.py; "pad" has a bond of 8 over a cut of rank 4, so exact zeros are among the wanted values (as
in A, whose bonds exceed the rank of its cuts).  The bound is TOL x |psi|: a singular value moves by at most the norm of a
perturbation, and |psi| is the Frobenius norm of every cut's matrix."""
import functools

import numpy as np
import pytest

from tests import mps_ent_ref, mps_obs_ref, mps_trunc_ref
from tests.helpers import TOL

PROFILES = {"A": (mps_obs_ref.PROFILE_A, 801), "B2": (mps_obs_ref.profile_b(2), 802), "B13": (mps_obs_ref.profile_b(13), 803),
            "C": (mps_obs_ref.PROFILE_C, 804)}
NAMES = sorted(PROFILES) + ["F", "pad"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(QiskitMPS tuple, bond dimensions, dense vector, Schmidt values by dense SVDs): computed once, never changed."""
    if name == "F":
        from oracle.aqc_oracle import random_mps

        mps = random_mps(13, 8, np.random.default_rng(807))
    elif name == "pad":
        mps = mps_ent_ref.pad_case()
    else:
        mps = mps_obs_ref.hand_made(*PROFILES[name])
    dims = [1] + [int(np.asarray(g0).shape[1]) for g0, _ in mps[0]]
    psi = mps_obs_ref.dense(mps)
    want = mps_ent_ref.schmidt_dense(psi, dims)
    for arr in (psi, want):
        arr.setflags(write=False)
    return mps, dims, psi, want


@pytest.mark.parametrize("name", NAMES)
def test_the_statement_matches_dense_svds(name):
    mps, dims, psi, want = case(name)
    got = mps_ent_ref.schmidt(mps)
    norm = float(np.linalg.norm(psi))
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    print(f"profile {name}: max |QR chain - dense SVD| = {err:.3g} (|psi| = {norm:.3g})")
    assert got.shape == want.shape == (len(dims) - 2, max(dims[1:-1] + [1]))
    assert err <= TOL * norm
    assert np.all(np.diff(got, axis=1) <= 0.0)
    assert np.allclose((got ** 2).sum(axis=1), norm ** 2, rtol=1e-12, atol=0.0)
    for q in range(1, len(dims) - 1):
        assert np.all(got[q - 1, dims[q]:] == 0.0)


def test_pad_has_a_rank_deficient_bond():
    _, dims, psi, want = case("pad")
    assert dims[4] == 8 and np.all(want[3, 4:] <= 1e-15 * want[3, 0]) and want[3, 3] > 1e-3 * want[3, 0]
    got = mps_ent_ref.schmidt(case("pad")[0])
    assert np.all(got[3, 4:] <= TOL * float(np.linalg.norm(psi)))


def test_the_squared_method_misses_the_tolerance():
    """Why the rule is a QR chain: eigenvalues of L_q R_q carry an error of about sqrt(eps) s_max where a value is (next to) zero."""
    mps, _, psi, want = case("A")
    norm = float(np.linalg.norm(psi))
    squares = float(np.max(np.abs(mps_ent_ref.schmidt_by_squares(mps) - want)))
    chain = float(np.max(np.abs(mps_ent_ref.schmidt(mps) - want)))
    print(f"profile A: QR chain {chain:.3g}, eig(L R) {squares:.3g} from the dense SVD")
    assert chain <= TOL * norm < squares


def test_the_factors_square_to_the_environments():
    mps, dims, psi, _ = case("A")
    ts = mps_obs_ref.site_tensors(mps)
    c, d = mps_ent_ref.factors(ts)
    left, right = mps_obs_ref.left_environments(ts), mps_obs_ref.right_environments(ts)
    norm2 = float(np.linalg.norm(psi)) ** 2
    for q in range(len(dims)):
        assert c[q].shape == d[q].shape == (dims[q], dims[q])
        assert np.max(np.abs(c[q].conj().T @ c[q] - left[q])) <= TOL * norm2
        assert np.max(np.abs((d[q].conj().T @ d[q]).conj() - right[q])) <= TOL * norm2
        assert np.all(np.tril(c[q], -1) == 0.0) and np.all(c[q][min(2 * dims[max(q - 1, 0)], dims[q]):] == 0.0)


def test_householder_r_of_the_statement():
    rng = np.random.default_rng(3)
    for rows, cols in ((2, 2), (10, 7), (128, 64), (2, 5), (1, 3)):
        m = rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols))
        m[:, cols // 2] = 0.0
        r = mps_ent_ref.householder_r(m)
        assert r.shape == (cols, cols) and np.all(np.tril(r, -1) == 0.0) and np.all(r[min(rows, cols):] == 0.0)
        assert np.max(np.abs(r.conj().T @ r - m.conj().T @ m)) <= 64 * np.finfo(float).eps * np.linalg.norm(m) ** 2
    assert np.all(mps_ent_ref.householder_r(np.zeros((6, 3))) == 0.0)


def test_nested_pairs_have_the_prescribed_spectrum():
    mps, vals = mps_ent_ref.nested_pairs((0.1, 0.01, 0.001, 0.7))
    psi = mps_obs_ref.dense(mps)
    assert abs(np.linalg.norm(psi) - 1.0) <= 1e-14 and vals.size == 16
    s = np.linalg.svd(psi.reshape(16, 16), compute_uv=False)
    assert np.max(np.abs(s - vals)) <= 1e-15
    assert np.max(np.abs(mps_ent_ref.schmidt(mps)[3] - vals)) <= 1e-15


def test_entropies_on_analytic_inputs():
    from aqc_research_amd.mps_observables import entropies_of

    bell = np.array([1.0, 1.0]) / np.sqrt(2.0)
    product = np.array([3.0, 0.0, 0.0])
    p = np.array([0.9, 0.1, 0.0])
    for alpha in (0.0, 0.5, 1.0, 2.0, 7.5, np.inf):
        assert abs(entropies_of(bell, alpha) - np.log(2.0)) <= 1e-15, alpha
        assert abs(entropies_of(5.0 * bell, alpha) - np.log(2.0)) <= 1e-15      # nothing is assumed normalised
        assert entropies_of(product, alpha) == 0.0, alpha
    s = np.sqrt(p)
    assert abs(entropies_of(s, 1.0) - (-(0.9 * np.log(0.9) + 0.1 * np.log(0.1)))) <= 1e-15
    assert abs(entropies_of(s, 2.0) - (-np.log(0.9 ** 2 + 0.1 ** 2))) <= 1e-15
    assert abs(entropies_of(s, 0.5) - 2.0 * np.log(np.sqrt(0.9) + np.sqrt(0.1))) <= 1e-15
    assert abs(entropies_of(s, np.inf) - (-np.log(0.9))) <= 1e-15 and abs(entropies_of(s, 0.0) - np.log(2.0)) <= 1e-15
    both = entropies_of(np.stack([s, np.array([1.0, 1.0, 0.0])]), 1.0)          # the last axis is the spectrum
    assert both.shape == (2,) and abs(both[1] - np.log(2.0)) <= 1e-15
    assert np.isnan(entropies_of(np.array([np.nan, np.nan]), 1.0)) and np.isnan(entropies_of(np.array([np.nan, 1.0]), 2.0))
    assert entropies_of(np.zeros((0, 1))).shape == (0,)


def test_rank_rule_of_the_abi_against_the_truncation_reference():
    from aqc_research_amd.mps_observables import rank_rule

    rng = np.random.default_rng(41)
    taken = 0
    for _ in range(2000):
        if taken == 200:
            break
        size = int(rng.integers(1, 40))
        s = np.sort(np.abs(rng.standard_normal(size)) * 10.0 ** rng.uniform(-9, 0, size))[::-1].copy()
        if rng.random() < 0.3:
            s[size // 2:] *= 1e-16                                             # values under the floor
        thr = 0.0 if rng.random() < 0.25 else float(10.0 ** rng.uniform(-14, -1))
        cap = 0 if rng.random() < 0.5 else int(rng.integers(1, 40))
        if not s[0] > 0.0:
            continue
        d = mps_trunc_ref.decide(s, thr, cap)
        try:
            mps_trunc_ref.check_margins([d])
        except AssertionError:
            continue
        taken += 1
        rank, dropped = rank_rule(s, thr, cap)
        assert rank == d.k, (s, thr, cap)
        above_floor = max(j + 1 for j, v in enumerate(s) if v > mps_trunc_ref.FLOOR * s[0])
        assert dropped == mps_trunc_ref._final_rank(s, above_floor, thr, cap)[1]
    assert taken == 200
