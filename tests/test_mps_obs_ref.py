"""CPU: the NumPy statement of the pair density matrices of an MPS (tests/mps_obs_ref.py) against the dense statement
(tests/obs_ref.rdm) on hand-made states, every pair in both orders.  The bound is that of two references against each other: an entry
is a sum of at most 2^11 products of amplitudes of a normalised state on the dense side and a chain of at most 13 products of
matrices of norm <= 1 on the other; 1e-13 leaves two orders of magnitude over the 1.5e-15 observed."""
import numpy as np
import pytest

from tests import mps_obs_ref, obs_ref

REF_TOL = 1e-13

CASES = {
    "A": (mps_obs_ref.PROFILE_A, 501),
    "B2": (mps_obs_ref.profile_b(2), 502),
    "B4": (mps_obs_ref.profile_b(4), 503),
    "B13": (mps_obs_ref.profile_b(13), 504),
    "C": (mps_obs_ref.PROFILE_C, 505),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_statement_matches_the_dense_one(name):
    dims, seed = CASES[name]
    mps = mps_obs_ref.hand_made(dims, seed)
    n = len(dims) - 1
    psi = mps_obs_ref.dense(mps)
    assert abs(np.vdot(psi, psi).real - 1.0) <= 1e-13 and abs(mps_obs_ref.norm2(mps) - 1.0) <= 1e-13
    pairs = obs_ref.all_pairs(n)
    pairs = pairs + [(j, i) for i, j in pairs]
    got = mps_obs_ref.pair_rdms(mps, pairs)
    err = float(np.max(np.abs(got - obs_ref.pair_rdms(psi, pairs))))
    print(f"profile {name}: max |MPS statement - dense statement| = {err:.3g}")
    assert err <= REF_TOL, (name, err)


def test_scaled_state_is_not_normalised_away():
    mps = mps_obs_ref.hand_made(mps_obs_ref.PROFILE_C, 7, norm=3.0)
    got = mps_obs_ref.pair_rdms(mps, [(0, 3)])[0]
    assert abs(np.trace(got).real - 9.0) <= 1e-13 and abs(mps_obs_ref.norm2(mps) - 9.0) <= 1e-13
