"""CPU: the NumPy statement of linear combinations of MPS states (tests/mps_combine_ref.py) against sum_k c_k dense(psi_k), and, with
truncation, against the dense walk of tests/test_mps_compress_ref.py on that sum.

Errors are bounded relative to scale = sum_k |c_k| |psi_k| (1e-12 scale: a few hundred roundings of the products of a state of at most
9 sites); every decision must pass mps_trunc_ref.check_margins, so that the ranks are those of the sum and not of its rounding.  The
thresholds and caps of the truncated cases are picked on the direct-sum tuple (mps_compress_ref.pick) and held to a relative gap of
MIN_GAP next to every cut, as the compression tests hold theirs."""
import numpy as np
import pytest

from tests import mps_combine_ref, mps_compress_ref, mps_obs_ref, mps_trunc_ref
from tests.test_mps_compress_ref import MIN_GAP, dense_walk, normalised


@pytest.mark.parametrize("name", mps_combine_ref.CASES)
def test_the_statement_is_the_dense_sum(name):
    from aqc_research_amd.mps_engine import is_canonical

    states, coeffs, want_bonds = mps_combine_ref.case(name)
    n = len(states[0][0])
    total = mps_combine_ref.direct_sum(states, coeffs)
    want, scale = mps_combine_ref.dense_sum(states, coeffs)
    summed = [1] + [g0.shape[1] for g0, _ in total[0]]
    assert summed[n] == 1 and all(summed[q] == sum(s[0][q][0].shape[0] for s in states) for q in range(1, n))
    assert float(np.linalg.norm(mps_obs_ref.dense(total) - want)) <= 1e-12 * scale          # the direct sum itself
    ref = mps_combine_ref.combine(states, coeffs)
    err = float(np.linalg.norm(ref.to_vector() - want))
    margins = mps_trunc_ref.check_margins(ref.decisions)
    print(f"case {name}: summed bonds {summed} -> {ref.bond_dims.tolist()}, |statement - dense sum| = {err:.3g} (scale {scale:.3g}), margins {margins}")
    assert err <= 1e-12 * scale
    assert ref.bond_dims.tolist() == want_bonds
    assert abs(ref.discarded) <= 1e-24 * scale ** 2
    if n > 1:
        assert is_canonical(normalised(ref.to_qiskit(), float(np.linalg.norm(want))))


def test_the_cap_case_sums_to_the_cap():
    states, coeffs, _ = mps_combine_ref.case("cap64")
    total = mps_combine_ref.direct_sum(states, coeffs)
    assert max(g0.shape[1] for g0, _ in total[0]) == 64


def test_a_state_listed_twice_is_one_object():
    for name in ("twice", "half", "nearly"):
        states, _, _ = mps_combine_ref.case(name)
        assert states[0] is states[1]


def test_the_w_state():
    states, coeffs, _ = mps_combine_ref.case("w8")
    vec = mps_combine_ref.combine(states, coeffs).to_vector()
    want = np.zeros(256)
    want[[1 << q for q in range(8)]] = 1.0 / np.sqrt(8.0)
    assert float(np.max(np.abs(vec - want))) <= 1e-12


@pytest.mark.parametrize("as_cap", (False, True), ids=("trunc_thr", "max_bond"))
@pytest.mark.parametrize("name", mps_combine_ref.TRUNCATED)
def test_truncation_matches_the_dense_walk(name, as_cap):
    states, coeffs, exact = mps_combine_ref.case(name)
    n = len(states[0][0])
    want, scale = mps_combine_ref.dense_sum(states, coeffs)
    thr, cap, ref, gap = mps_combine_ref.truncation(name, as_cap)
    mps_trunc_ref.check_margins(ref.decisions)
    vec, ranks, dropped, lams, decisions, spectra = dense_walk(want, n, thr, cap)
    mps_trunc_ref.check_margins(decisions)
    print(f"case {name}, trunc_thr {thr:g}, max_bond {cap}: bonds {exact} -> {ref.bond_dims.tolist()}, smallest gap {gap}, discarded {ref.discarded:.3g}")
    assert gap is not None and gap >= MIN_GAP
    dense_gaps = mps_compress_ref.gaps(decisions, spectra)
    assert dense_gaps and min(dense_gaps) >= MIN_GAP
    assert np.any(ref.bond_dims < np.array(exact))
    assert ref.bond_dims[1:n].tolist() == ranks
    bound = 1e-12 * scale / gap
    err = float(np.linalg.norm(ref.to_vector() - vec))
    print(f"    |statement - dense walk| = {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    assert abs(ref.discarded - sum(dropped)) <= 1e-12 * scale ** 2
    for a, b in zip(ref.lam, lams):
        assert np.max(np.abs(a - b)) <= bound


def test_bad_arguments():
    states, coeffs, _ = mps_combine_ref.case("n3")
    with pytest.raises(ValueError):
        mps_combine_ref.direct_sum(states, coeffs[:1])
    with pytest.raises(ValueError):
        mps_combine_ref.direct_sum(states + [mps_combine_ref.case("n2")[0][0]], coeffs + [1.0])
