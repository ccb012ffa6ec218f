"""CPU: the NumPy statement of operator matrix elements between MPS states (tests/mps_melem_ref.py) against
conj(dense phi) . dense(O) . dense psi, within 1e-12 of scale = |phi| |O|_2 |psi| (the CPU bound of the operator sums; rounding of a
few hundred fp64 operations per element is about 1e-15), on the jobs that the GPU tests share; and the list of entries that the library's rule header gives (aqc_mps_melem_entries, host only)
against the statement's."""
import numpy as np
import pytest

from tests import mps_melem_ref as ref
from tests import mps_obs_ref, mps_opsum_ref

CPU_TOL = 1e-12


@pytest.mark.parametrize("name", ref.CASES)
def test_statement_against_dense(name):
    bra, op, ket = ref.case(name)
    want, scale = ref.dense_value(bra, op, ket)
    got = ref.value(bra, op, ket)
    print(f"{name}: |statement - dense| / scale = {abs(got - want) / scale:.3g}, |value| / scale = {abs(want) / scale:.3g}")
    assert scale > 0.0 and abs(got - want) <= CPU_TOL * scale


def test_expectation_and_hermitian_symmetry():
    psi, phi = mps_obs_ref.hand_made(ref.KET6, 41), mps_obs_ref.hand_made(ref.BRA6, 42)
    h = mps_opsum_ref.xxz(6, ref.DELTA)
    e, scale = ref.dense_value(psi, h, psi)
    assert abs(ref.value(psi, h, psi) - e) <= CPU_TOL * scale and abs(e.imag) <= CPU_TOL * scale
    a, b = ref.value(phi, h, psi), ref.value(psi, h, phi)
    assert abs(a - np.conj(b)) <= CPU_TOL * ref.dense_value(phi, h, psi)[1]


@pytest.mark.parametrize("name", ["xxz6", "inner1", "cap64", "identity6"])
def test_skipping_zeros_changes_no_finite_result(name):
    """With the zeros of W multiplied through instead of skipped, every sum gains terms that are exact zeros: the same number."""
    bra, op, ket = ref.case(name)
    sites = [ref.IDENTITY_SITE] * len(ket[0]) if op is None else op
    skipped = sum(len(ref.entries(w, skip=False)) - len(ref.entries(w)) for w in sites)
    assert (skipped > 0) == (name != "inner1")            # a random operator has no zero to skip
    assert ref.value(bra, op, ket, skip=True) == ref.value(bra, op, ket, skip=False)


def test_a_zero_of_the_operator_never_meets_the_states():
    """What skipping is for besides speed: a NaN in a tensor entry that only zeros of W would read leaves the value finite."""
    n = 3
    p0 = np.diag([1.0, 0.0]).astype(np.complex128).reshape(1, 1, 2, 2)       # |0><0| on qubit 1: T_1[1] is never read
    op = [ref.IDENTITY_SITE, p0, ref.IDENTITY_SITE]
    bra, ket = mps_obs_ref.hand_made([1, 2, 2, 1], 43), mps_obs_ref.hand_made([1, 2, 2, 1], 44)
    want = ref.value(bra, op, ket)
    gam = [tuple(g.copy() for g in site) for site in ket[0]]
    gam[1][1][:] = np.nan
    assert len(gam) == n and ref.value(bra, op, (gam, ket[1])) == want
    assert not np.isfinite(ref.value(bra, op, (gam, ket[1]), skip=False))


def _library_entries(w):
    """(rows of a, s', b, s, first; masks) of one operator site from the library's rule header (aqc_mps_melem_entries, host only)."""
    from aqc_research_amd import _lib
    from aqc_research_amd._lib import dptr, iptr

    dl, dr = (1, 1) if w is None else w.shape[:2]
    out, mask = np.zeros((4 * dl * dr, 5), dtype=np.int32), np.zeros(dr, dtype=np.int32)
    count = _lib.lib().aqc_mps_melem_entries(dl, dr, None if w is None else dptr(np.ascontiguousarray(w, dtype=np.complex128)), iptr(out), iptr(mask))
    assert 0 <= count <= out.shape[0]
    return out[:count], mask


def test_the_library_lists_the_entries_of_the_statement():
    """The list that both device routes walk (csrc/aqc_mps_melem_rule.h) against ``entries`` here: the same entries in the same
    order, the first entry of every G marked, the masks those of the G that the statement forms."""
    rng = np.random.default_rng(51)
    sparse = rng.standard_normal((3, 4, 2, 2)) + 1j * rng.standard_normal((3, 4, 2, 2))
    sparse[rng.random((3, 4, 2, 2)) < 0.6] = 0.0
    sparse[0, 1, 1, 0], sparse[2, 3, 0, 1], sparse[1, 0, 0, 0] = np.nan, -0.0, complex(-0.0, 5e-324)
    sites = [None, sparse] + [np.asarray(w) for w in mps_opsum_ref.xxz(6, ref.DELTA)[:3]] + list(mps_opsum_ref.random_mpo([1, 2, 1, 3], 52))
    for w in sites:
        got, mask = _library_entries(w)
        want = ref.entries(ref.IDENTITY_SITE if w is None else w)
        assert [tuple(r[:4]) for r in got.tolist()] == [e[:4] for e in want]
        seen = set()
        for a, sp, b, s, first in got.tolist():
            assert first == ((b, s) not in seen)
            seen.add((b, s))
        assert mask.tolist() == [sum(1 << s for s in range(2) if (b, s) in seen) for b in range(mask.size)]
    assert len(_library_entries(np.asarray(mps_opsum_ref.xxz(6, ref.DELTA)[2]))[0]) == 16      # of 100: what makes an XXZ site cheap


def test_entries_order_and_identity():
    w = np.zeros((2, 3, 2, 2), dtype=np.complex128)
    w[0, 0, 0, 0], w[0, 0, 0, 1], w[1, 0, 0, 0], w[0, 2, 1, 1], w[1, 1, 0, 1] = 1.0, -2j, 3.0, np.nan, -0.0
    got = [(a, sp, b, s) for a, sp, b, s, _ in ref.entries(w)]
    assert got == [(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 2, 1), (1, 0, 0, 0)]
    assert len(ref.entries(w, skip=False)) == 24
    assert [(a, sp, b, s) for a, sp, b, s, _ in ref.entries(ref.IDENTITY_SITE)] == [(0, 0, 0, 0), (0, 1, 0, 1)]
