"""CPU: the NumPy statement of operator sums on MPS states (tests/mps_opsum_ref.py) against sum_t c_t dense(O_t) dense(psi_t), and, with
truncation, against the dense walk of tests/test_mps_compress_ref.py on that sum; the operators that ``mps_engine.MPO`` builds against
their Kronecker products.

Errors are bounded relative to scale = sum_t |c_t| |O_t|_2 |psi_t| (1e-12 scale, the bound of tests/test_mps_combine_ref.py: a few
hundred roundings of the products of a state of at most 9 sites); every decision must pass mps_trunc_ref.check_margins, so that the
ranks are those of the sum and not of its rounding.  The thresholds and caps of the truncated cases are picked on the direct-sum tuple
(mps_compress_ref.pick), thresholds in units of the squared norm of the untruncated result, and held to a relative gap of MIN_GAP next
to every cut, as the compression tests hold theirs."""
import numpy as np
import pytest

from tests import mps_compress_ref, mps_obs_ref, mps_opsum_ref, mps_trunc_ref
from tests.test_mps_compress_ref import MIN_GAP, dense_walk, normalised

_I = np.eye(2, dtype=np.complex128)
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.diag([1.0, -1.0]).astype(np.complex128)
_LETTER = {"I": _I, "X": _X, "Y": _Y, "Z": _Z}


def _kron(factors):
    """factors[q] on qubit q, qubit q being index bit q: the last factor is the leftmost of the Kronecker product."""
    m = np.ones((1, 1), dtype=np.complex128)
    for f in factors:
        m = np.kron(f, m)
    return m


def _string(s):
    return _kron([_LETTER[ch] for ch in s])


@pytest.mark.parametrize("name", mps_opsum_ref.CASES)
def test_the_statement_is_the_dense_result(name):
    from aqc_research_amd.mps_engine import is_canonical

    terms = mps_opsum_ref.case(name)
    n = len(terms[0][2][0])
    total = mps_opsum_ref.opsum(terms)
    want, scale = mps_opsum_ref.dense_sum(terms)
    summed = mps_opsum_ref.product_bonds(terms)
    if n > 1:   # the product bonds D_q chi_q of every term, summed
        for q in range(1, n):
            assert summed[q] == sum((1 if op is None else op[q].shape[0]) * state[0][q][0].shape[0] for _, op, state in terms)
    assert summed[0] == summed[n] == 1
    assert float(np.linalg.norm(mps_obs_ref.dense(total) - want)) <= 1e-12 * scale          # the direct sum of the products itself
    ref = mps_opsum_ref.statement(terms)
    err = float(np.linalg.norm(ref.to_vector() - want))
    margins = mps_trunc_ref.check_margins(ref.decisions)
    print(f"case {name}: summed product bonds {summed} -> {ref.bond_dims.tolist()}, |statement - dense result| = {err:.3g} (scale {scale:.3g}), margins {margins}")
    assert err <= 1e-12 * scale
    assert abs(ref.discarded) <= 1e-24 * scale ** 2
    if n > 1:
        assert is_canonical(normalised(ref.to_qiskit(), float(np.linalg.norm(want))))


def test_the_shapes_of_the_cases():
    assert mps_opsum_ref.product_bonds(mps_opsum_ref.case("random")) == [1, 4, 9, 20, 9, 4, 1]
    assert mps_opsum_ref.statement(mps_opsum_ref.case("random")).bond_dims.tolist() == [1, 2, 4, 8, 4, 2, 1]
    assert mps_opsum_ref.product_bonds(mps_opsum_ref.case("residual")) == [1, 14, 22, 37, 22, 14, 1]      # 5 x P5 + P5 + P7
    assert max(mps_opsum_ref.product_bonds(mps_opsum_ref.case("cap64"))) == 64
    assert max(mps_opsum_ref.product_bonds(mps_opsum_ref.case("beyond"))) == 65
    assert mps_opsum_ref.case("n3")[0][1][1].shape[1] == 1 and mps_opsum_ref.case("n3")[0][1][0].shape[1] == 2   # D_2 = 1 inside
    terms = mps_opsum_ref.case("residual")
    assert terms[0][2] is terms[1][2]                                                     # the same state object twice
    assert all(f in mps_opsum_ref.CASES for f in mps_opsum_ref.FUSED + mps_opsum_ref.TRUNCATED)


def test_the_projector_on_the_w_state():
    terms = mps_opsum_ref.case("wproj")
    vec = mps_opsum_ref.statement(terms).to_vector()
    want = np.zeros(256)
    want[1 << 2] = 1.0 / np.sqrt(8.0)
    assert float(np.max(np.abs(vec - want))) <= 1e-12
    gone = [(1.0, mps_opsum_ref.projector(8, (1, 5)), terms[0][2])]                       # two qubits up: the W state has none
    assert float(np.linalg.norm(mps_opsum_ref.dense_sum(gone)[0])) == 0.0
    with pytest.raises(ValueError):
        mps_opsum_ref.statement(gone)


@pytest.mark.parametrize("as_cap", (False, True), ids=("trunc_thr", "max_bond"))
@pytest.mark.parametrize("name", mps_opsum_ref.TRUNCATED)
def test_truncation_matches_the_dense_walk(name, as_cap):
    terms = mps_opsum_ref.case(name)
    n = len(terms[0][2][0])
    want, scale = mps_opsum_ref.dense_sum(terms)
    exact = mps_opsum_ref.statement(terms).bond_dims
    thr, cap, ref, gap = mps_opsum_ref.truncation(name, as_cap)
    mps_trunc_ref.check_margins(ref.decisions)
    vec, ranks, dropped, lams, decisions, spectra = dense_walk(want, n, thr, cap)
    mps_trunc_ref.check_margins(decisions)
    print(f"case {name}, trunc_thr {thr:g}, max_bond {cap}: bonds {exact.tolist()} -> {ref.bond_dims.tolist()}, smallest gap {gap}, discarded {ref.discarded:.3g}")
    assert gap is not None and gap >= MIN_GAP
    dense_gaps = mps_compress_ref.gaps(decisions, spectra)
    assert dense_gaps and min(dense_gaps) >= MIN_GAP
    assert np.any(ref.bond_dims < exact) and int(ref.bond_dims.max()) > 1 and ref.discarded > 0.0   # it drops something and keeps a bond
    assert ref.bond_dims[1:n].tolist() == ranks
    bound = 1e-12 * scale / gap
    err = float(np.linalg.norm(ref.to_vector() - vec))
    print(f"    |statement - dense walk| = {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    assert abs(ref.discarded - sum(dropped)) <= 1e-12 * scale ** 2
    for a, b in zip(ref.lam, lams):
        assert np.max(np.abs(a - b)) <= bound


def test_the_xxz_automaton_is_the_hamiltonian():
    from aqc_research_amd.mps_engine import MPO

    n, delta = 6, 0.7
    h = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for i in range(n - 1):
        pair = lambda p: _kron([p if q in (i, i + 1) else _I for q in range(n)])   # noqa: E731
        h += -0.25 * (pair(_X) + pair(_Y) + delta * pair(_Z))
    op = MPO.xxz(n, delta)
    assert op.bond_dims.tolist() == [1, 5, 5, 5, 5, 5, 1] and op.num_qubits == n
    assert np.array_equal(op.to_dense(), h)                                               # exactly
    assert np.array_equal(mps_opsum_ref.dense_op(op.sites), h)
    assert np.array_equal(MPO.xxz(2, delta).to_dense(), -0.25 * (np.kron(_X, _X) + np.kron(_Y, _Y) + delta * np.kron(_Z, _Z)))
    assert np.array_equal(MPO.xxz(1, delta).to_dense(), np.zeros((2, 2)))


def test_pauli_sums_and_product_operators():
    from aqc_research_amd.mps_engine import MPO

    terms = [(0.5, "XIZYII"), (1.0j, "ZZIIII"), (-2.0, "IIIIIY"), (0.25 - 0.5j, "YXYXZI")]
    op = MPO.from_pauli_sum(terms)
    assert op.bond_dims.tolist() == [1, 4, 4, 4, 4, 4, 1]                                 # D = the number of terms: nothing is compressed
    assert np.array_equal(op.to_dense(), sum(w * _string(s) for w, s in terms))
    one = MPO.from_pauli_string("XIZYII", 0.5)
    assert one.bond_dims.tolist() == [1] * 7 and np.array_equal(one.to_dense(), 0.5 * _string("XIZYII"))
    sparse = MPO.from_pauli_sum([(1.5, ("ZZ", (1, 4))), (-1.0, ("X", (0,)))], num_qubits=5)
    assert np.array_equal(sparse.to_dense(), 1.5 * _string("IZIIZ") - _string("XIIII"))
    letters = np.array([[1, 0, 3], [0, 2, 2]], dtype=np.uint8)
    assert np.array_equal(MPO.from_pauli_sum([(1.0, letters[0]), (2.0, letters[1])]).to_dense(), _string("XIZ") + 2.0 * _string("IYY"))
    assert np.array_equal(MPO.from_pauli_sum([(2.0, "X"), (1.0j, "Z")]).to_dense(), 2.0 * _X + 1.0j * _Z)   # one qubit: D = 1
    assert np.array_equal(MPO.identity(4).to_dense(), np.eye(16))
    rng = np.random.default_rng(821)
    mats = [rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2)) for _ in range(4)]
    assert np.allclose(MPO.product_operator(mats).to_dense(), _kron(mats), rtol=0, atol=1e-13)   # (products of four roundings each)
    random = mps_opsum_ref.random_mpo(mps_opsum_ref.MPO_BONDS, 822)
    assert np.allclose(MPO(random).to_dense(), mps_opsum_ref.dense_op(random), rtol=0, atol=1e-13)


def test_bad_arguments():
    terms = mps_opsum_ref.case("n3")
    with pytest.raises(ValueError):
        mps_opsum_ref.opsum([])
    with pytest.raises(ValueError):
        mps_opsum_ref.product(mps_opsum_ref.random_mpo([1, 2, 1], 1), terms[0][2])        # an operator on 2 qubits, a state of 3
    with pytest.raises(ValueError):
        mps_opsum_ref.opsum(terms + [(1.0, None, mps_opsum_ref.case("n2")[0][2])])
