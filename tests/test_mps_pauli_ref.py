"""CPU: the two NumPy statements of <phi|P|psi> (tests/mps_pauli_ref.py) against each other -- the transfer-matrix walk and the dense
vector with bit flips and signs -- at the project's TOL = 1e-10 x |phi| |psi| (|<phi|P|psi>| <= |phi| |psi|), on hand-made states and
the oracle's random MPS, phi = psi and phi != psi; conjugate symmetry; the XXZ bond terms against the dense statement's bond energies."""
import functools

import numpy as np
import pytest

from tests import mps_obs_ref, mps_pauli_ref, obs_ref
from tests.helpers import TOL

BONDS_16 = [1, 2, 4, 8, 16, 16, 16, 13, 16, 16, 8, 4, 2, 1]


@functools.lru_cache(maxsize=None)
def _state(name):
    if name == "C":
        return mps_obs_ref.hand_made(mps_obs_ref.PROFILE_C, 701)
    if name == "F":
        from oracle.aqc_oracle import random_mps

        return random_mps(13, 8, np.random.default_rng(702))
    return mps_obs_ref.hand_made(BONDS_16, 703, norm=1.5)


CASES = {"C": ("C", "C"), "F": ("F", "F"), "H16": ("H16", "H16"), "H16xF": ("H16", "F")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_two_statements_agree(name):
    bra, ket = (_state(k) for k in CASES[name])
    n = len(ket[0])
    strings = mps_pauli_ref.ref_strings(n, 710 + n)
    scale = np.sqrt(mps_obs_ref.norm2(bra) * mps_obs_ref.norm2(ket))
    walk, dense = mps_pauli_ref.by_transfer(bra, ket, strings), mps_pauli_ref.by_dense(bra, ket, strings)
    err = float(np.max(np.abs(walk - dense)))
    print(f"case {name}: max |walk - dense| = {err:.3g} (|phi| |psi| = {scale:.3g})")
    assert err <= TOL * scale
    assert float(np.max(np.abs(dense))) <= scale * (1 + 1e-12)
    # <phi|P|psi> = conj <psi|P|phi>
    back = mps_pauli_ref.by_transfer(ket, bra, strings)
    assert float(np.max(np.abs(walk - back.conj()))) <= TOL * scale
    if CASES[name][0] == CASES[name][1]:
        assert float(np.max(np.abs(walk.imag))) <= TOL * scale
        assert abs(walk[0] - mps_obs_ref.norm2(ket)) <= TOL * scale   # the identity string
    # all-Y on a product of |0>s has the phase i^n: <1..1|Y..Y|0..0> = i^n
    zeros = ([(np.ones((1, 1)), np.zeros((1, 1)))] * n, [np.ones(1)] * (n - 1))
    ones = ([(np.zeros((1, 1)), np.ones((1, 1)))] * n, [np.ones(1)] * (n - 1))
    ally = np.full((1, n), 2, dtype=np.uint8)
    assert abs(mps_pauli_ref.by_transfer(ones, zeros, ally)[0] - 1j ** n) <= 1e-15
    assert abs(mps_pauli_ref.by_dense(ones, zeros, ally)[0] - 1j ** n) <= 1e-15


@pytest.mark.parametrize("name", ("C", "F"))
@pytest.mark.parametrize("delta", (1.0, -0.7))
def test_xxz_bond_terms_are_the_bond_energies(name, delta):
    mps = _state(name)
    n = len(mps[0])
    psi = mps_obs_ref.dense(mps)
    terms = mps_pauli_ref.xxz_terms(n, delta)
    vals = mps_pauli_ref.by_transfer(mps, mps, [s for _, s in terms])
    got = (np.array([w for w, _ in terms]) * vals.real).reshape(n - 1, 3).sum(axis=1)
    want = np.array([-0.25 * (obs_ref.expectation(r, "xx") + obs_ref.expectation(r, "yy") + delta * obs_ref.expectation(r, "zz"))
                     for r in (obs_ref.rdm(psi, (q, q + 1)) for q in range(n - 1))])
    err = float(np.max(np.abs(got - want)))
    print(f"case {name}, delta {delta}: max |bond terms - bond energies| = {err:.3g}")
    assert err <= TOL * mps_obs_ref.norm2(mps)
