"""GPU: matrix elements of operators between MPS states (aqc_research_amd/mps_observables.py: operator_elements, operator_matrix,
expectations, variance_by_walk; kernels: csrc/aqc_mps_melem.hip) on both routes against the NumPy statement (tests/mps_melem_ref.py),
against each other, against what the project already computes (overlaps, energy, pauli_strings, apply_operator, variance) and against
properties that need no reference.

The shapes are the smallest at which the walk can still go wrong: one and two qubits, rectangular sites with no bond a multiple of 4,
an operator with and without zeros and with a bond of 1 inside, a bond of exactly 64 against 65 and an operator bond of exactly 32
against 33 (the caps of the fused route), and 40 qubits beyond dense reach.  The tolerance is the project's TOL = 1e-10 times
scale = |phi| |O|_2 |psi|; the tests print what they observe and DESIGN.md 6ze records it."""
import functools
from ctypes import POINTER, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from tests import mps_melem_ref as ref
from tests import mps_obs_ref, mps_opsum_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes

pytestmark = pytest.mark.gpu


def _mpo(op):
    from aqc_research_amd.mps_engine import MPO

    return None if op is None else MPO(op)


@functools.lru_cache(maxsize=None)
def _want(name):
    """(statement, scale) of a shared case: computed once."""
    bra, op, ket = ref.case(name)
    scale = ref.dense_value(bra, op, ket)[1]
    return ref.value(bra, op, ket), scale


def _routes(name):
    return (None, "fused", "gemm") if name in ref.FUSED else (None, "gemm")


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


@pytest.mark.parametrize("name", ref.CASES)
def test_values_match_the_statement_on_both_routes(name):
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import melem_route, operator_elements

    bra, sites, ket = ref.case(name)
    op = _mpo(sites)
    want, scale = _want(name)
    b, k = DeviceMPS.from_qiskit(bra, assume_canonical=True), DeviceMPS.from_qiskit(ket, assume_canonical=True)
    try:
        assert melem_route(b.bond_dims, k.bond_dims, None if op is None else op.bond_dims) == ("fused" if name in ref.FUSED else "gemm")
        before = _flat(b.to_qiskit()), _flat(k.to_qiskit())
        got = {}
        for method in _routes(name):
            got[method] = operator_elements([(b, op, k)], method=method)
            assert got[method].shape == (1,) and got[method].dtype == np.complex128
            err = abs(got[method][0] - want) / scale
            print(f"{name}, method {method}: |value - statement| / scale = {err:.3g}, |value| / scale = {abs(want) / scale:.3g}")
            assert err <= TOL, (name, method, err)
        if "fused" in got:
            assert abs(got["fused"][0] - got["gemm"][0]) <= TOL * scale
            assert np.array_equal(got[None], got["fused"])
        else:
            assert np.array_equal(got[None], got["gemm"])
            with pytest.raises(ValueError, match="fused.*job 0"):
                operator_elements([(b, op, k)], method="fused")
        assert np.array_equal(_flat(b.to_qiskit()), before[0]) and np.array_equal(_flat(k.to_qiskit()), before[1])
        if sites is not None:
            assert all(np.array_equal(w, s) for w, s in zip(op.sites, sites))
        tuples = operator_elements([(bra, op, ket)])          # QiskitMPS tuples are uploaded for the call: the same bits
        assert np.array_equal(tuples, got[None])
    finally:
        b.close()
        k.close()


_B40 = [1, 2, 4, 8] + [16] * 33 + [8, 4, 2, 1]
_TERMS40 = [(0.7, ("XX", (3, 4))), (-1.3, ("YZY", (10, 20, 30))), (0.4, ("Z", (39,)))]


@pytest.mark.parametrize("method", (None, "fused", "gemm"))
def test_forty_qubits_match_the_pauli_strings(method):
    """Beyond dense reach: a 3-string Pauli sum (D = 3) on bonds of 16 against sum_k w_k <phi|P_k|psi> of pauli_strings, as an
    expectation value and between two states; scale = sum_k |w_k| |phi| |psi|."""
    from aqc_research_amd.mps_engine import MPO, DeviceMPS
    from aqc_research_amd.mps_observables import expectations, operator_elements, pauli_strings

    psi, phi = (DeviceMPS.from_qiskit(mps_obs_ref.hand_made(_B40, seed), assume_canonical=True) for seed in (931, 932))
    try:
        op = MPO.from_pauli_sum(_TERMS40, num_qubits=40)
        assert op.bond_dims.max() == 3
        w = np.array([t[0] for t in _TERMS40])
        strings = [t[1] for t in _TERMS40]
        scale = float(np.abs(w).sum())          # hand_made states have norm 1
        want_e = (pauli_strings(psi, strings) * w).sum()
        want_x = (pauli_strings(psi, strings, bras=phi) * w).sum()
        got_e = expectations(psi, [op], method=method)[0]
        got_x = operator_elements([(phi, op, psi)], method=method)[0]
        print(f"n = 40, method {method}: expectation off by {abs(got_e - want_e) / scale:.3g}, bra != ket off by {abs(got_x - want_x) / scale:.3g} of scale")
        assert abs(got_e - want_e) <= TOL * scale and abs(got_x - want_x) <= TOL * scale
        assert abs(want_e) > 1e-6 * scale       # (the comparison is not between two zeros)
    finally:
        psi.close()
        phi.close()


def test_agreement_with_what_already_exists():
    from aqc_research_amd.mps_engine import MPO, DeviceMPS, apply_operator
    from aqc_research_amd.mps_observables import energy, expectations, operator_elements, operator_matrix, overlaps, variance, variance_by_walk

    hm = mps_obs_ref.hand_made
    dims = [1, 2, 4, 7, 4, 2, 1]
    tup = [hm(dims, 941), hm(ref.BRA6, 942)]
    psi, phi = (DeviceMPS.from_qiskit(t, assume_canonical=True) for t in tup)
    made = []
    try:
        h = MPO.xxz(6, ref.DELTA)
        hnorm = float(np.linalg.norm(h.to_dense(), 2))
        for method in (None, "fused", "gemm"):
            # identity jobs against overlaps
            gram = operator_matrix(None, [psi, phi], method=method)
            assert np.abs(gram - overlaps([psi, phi], [psi, phi])).max() <= TOL
            # a Pauli sum against energy
            terms = [(0.5, "XXIIII"), (-0.25, "IZZIII"), (1.5, "IIIYIY")]
            e = expectations(psi, [MPO.from_pauli_sum(terms)], method=method)
            assert e.shape == (1,) and abs(e[0].real - energy(psi, terms)) <= TOL * 2.25 and abs(e[0].imag) <= TOL * 2.25
            # H in a basis of two states against overlaps with H psi_j, nothing truncated
            hm_ = operator_matrix(h, [psi, phi], method=method)
            images = apply_operator(h, [psi, phi], 0.0)
            made += images
            want = overlaps([psi, phi], images)
            print(f"method {method}: max |operator_matrix - overlaps with H psi| = {np.abs(hm_ - want).max():.3g}")
            assert hm_.shape == (2, 2) and np.abs(hm_ - want).max() <= TOL * hnorm
            assert np.abs(hm_ - hm_.conj().T).max() <= TOL * hnorm           # H is Hermitian
            rect = operator_matrix(h, [psi], [phi, psi, phi], method=method)
            assert rect.shape == (3, 1) and np.array_equal(rect[:, 0], [hm_[1, 0], hm_[0, 0], hm_[1, 0]])
            # the variance against the route through H psi
            v = variance_by_walk([psi, phi], h, method=method)
            assert v.shape == (2,) and np.abs(v - variance([psi, phi], h)).max() <= TOL * hnorm ** 2
            assert abs(variance_by_walk(psi, h, method=method) - v[0]) == 0.0
            # scaling: 3 phi and 2 psi give 6 x
            big = operator_elements([(hm(ref.BRA6, 942, 3.0), h, hm(dims, 941, 2.0))], method=method)[0]
            assert abs(big - 6.0 * hm_[1, 0]) <= TOL * 6.0 * hnorm
            # the forward of the class
            assert psi.operator_elements(h, method=method) == hm_[0, 0]
            assert np.array_equal(psi.operator_elements(h, [phi, psi], method=method), hm_[::-1, 0])
    finally:
        for m in made + [psi, phi]:
            m.close()


def test_variance_of_a_pauli_string_on_a_basis_state_is_zero():
    from aqc_research_amd.mps_engine import MPO, DeviceMPS
    from aqc_research_amd.mps_observables import expectations, variance_by_walk

    zz = MPO.from_pauli_string(("ZZ", (7, 8)), num_qubits=10)
    m = DeviceMPS.basis_state(10, 0b0110010001)          # qubits 7 and 8 are |1>: an eigenstate of Z_7 Z_8
    try:
        for method in (None, "fused", "gemm"):
            assert abs(variance_by_walk(m, zz, method=method)) <= TOL
            assert abs(abs(expectations(m, [zz], method=method)[0]) - 1.0) <= TOL
    finally:
        m.close()


def _op_array(sites):
    return np.concatenate([np.asarray(w, dtype=np.complex128).ravel() for w in sites])


def _op_from(flat, bonds):
    from aqc_research_amd.mps_engine import MPO

    out, at = [], 0
    for q in range(len(bonds) - 1):
        size = 4 * bonds[q] * bonds[q + 1]
        out.append(flat[at:at + size].reshape(bonds[q], bonds[q + 1], 2, 2))
        at += size
    return MPO(out)


def _nan_state(state):
    gam, lam = state
    return [(np.full_like(g0, np.nan), np.full_like(g1, np.nan)) for g0, g1 in gam], lam


_LANE_BONDS = {"fused": ([1, 2, 3, 5, 3, 2, 1], [1, 2, 4, 7, 4, 2, 1]), "gemm": ([1, 2, 4, 65, 4, 2, 1], [1, 2, 4, 7, 4, 2, 1])}


@pytest.mark.parametrize("method", ("fused", "gemm"))
def test_jobs_hold_the_lane_contract(method):
    """Four jobs as lanes, each with a bra, a ket and an operator of its own, probes (0, 3).  F: the other lanes get other states and
    operators; N: they get NaN tensors and NaN operator entries, and the probes' bits do not move."""
    from aqc_research_amd.mps_observables import operator_elements

    hm = mps_obs_ref.hand_made
    bd, kd = _LANE_BONDS[method]
    obonds = mps_opsum_ref.MPO_BONDS
    bras, kets = [hm(bd, 951 + l) for l in range(4)], [hm(kd, 961 + l) for l in range(4)]
    ops = np.stack([_op_array(mps_opsum_ref.random_mpo(obonds, 971 + l)) for l in range(4)])
    donors = ([hm(bd, 955 + l) for l in range(4)], [hm(kd, 965 + l) for l in range(4)],
              np.stack([_op_array(mps_opsum_ref.random_mpo(obonds, 975 + l)) for l in range(4)]))

    def run(inputs):
        b, k, o = inputs
        return operator_elements([(b[l], _op_from(o[l], obonds), k[l]) for l in range(4)], method=None if method == "gemm" else method)

    def poison(inputs, lanes):
        b, k, o = inputs
        for l in lanes:
            b[l], k[l] = _nan_state(b[l]), _nan_state(k[l])
        o[lanes] = np.nan
        return b, k, o

    def reference(inputs, lane):
        b, k, o = inputs
        return ref.value(b[lane], list(_op_from(o[lane], obonds).sites), k[lane])

    scale = max(np.linalg.norm(mps_opsum_ref.dense_op(list(_op_from(ops[l], obonds).sites)), 2) for l in (0, 3))   # the states have norm 1
    base = check_lanes(run, (bras, kets, ops), probes=(0, 3), other=donors, poison=poison, reference=reference, reference_lanes=(0, 3),
                       tol=TOL * float(scale))
    poisoned = poison((list(bras), list(kets), ops.copy()), [1, 2])
    got = run(poisoned)
    assert np.all(np.isnan(got[1:3])) and np.array_equal(got[[0, 3]], base["out"][[0, 3]])


def test_a_mixed_call_equals_its_one_job_calls_bit_for_bit():
    """A call that repeats a job, mixes fused and gemm jobs and, with the scratch budget lowered, runs its fused jobs in several groups
    and its gemm jobs in several groups: every value is that of the one-job call."""
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import MPO, DeviceMPS
    from aqc_research_amd.mps_observables import operator_elements

    hm = mps_obs_ref.hand_made
    small = [DeviceMPS.from_qiskit(hm(ref.KET6, 981 + l), assume_canonical=True) for l in range(3)]
    wide = [DeviceMPS.from_qiskit(hm([1, 2, 4, 65, 4, 2, 1], 985 + l), assume_canonical=True) for l in range(2)]
    try:
        h, r = MPO.xxz(6, ref.DELTA), _mpo(mps_opsum_ref.random_mpo(mps_opsum_ref.MPO_BONDS, 989))
        jobs = [(small[0], h, small[1]), (wide[0], h, small[0]), (small[2], r, small[2]), (small[0], h, small[1]), (wide[1], h, small[0]),
                (small[1], None, small[2]), (wide[0], h, small[0]), (wide[1], r, wide[0]), (small[2], r, small[0])]
        alone = np.array([operator_elements([j])[0] for j in jobs])
        assert np.all(np.isfinite(alone)) and alone[0] == alone[3] and alone[1] == alone[6] and len(set(alone.tolist())) == 7
        whole = operator_elements(jobs)
        assert np.array_equal(whole, alone)
        before = _lib.lib().aqc_mps_melem_budget(16 * 2 * 800)       # a fused job takes 2 * 245 + 280 numbers: two of the five a group
        try:
            assert np.array_equal(operator_elements(jobs), alone)
            assert np.array_equal(operator_elements(jobs, method="gemm"), np.array([operator_elements([j], method="gemm")[0] for j in jobs]))
        finally:
            _lib.lib().aqc_mps_melem_budget(before)
    finally:
        for m in small + wide:
            m.close()


def _abi(states, ops, job_bra, job_op, job_ket, method):
    """The ABI call on open DeviceMPS states, no check of the Python layer in between: (status, values)."""
    from aqc_research_amd import _lib
    from aqc_research_amd._lib import dptr, iptr
    from aqc_research_amd.mps_engine import _packed_ops

    n = states[0].num_qubits
    dims, off, data = _packed_ops(ops, n)
    jb, jo, jk = (np.array(a, dtype=np.int32) for a in (job_bra, job_op, job_ket))
    out = np.zeros(len(jb), dtype=np.complex128)
    handles = (c_void_p * len(states))(*[m.handle for m in states])
    rc = _lib.lib().aqc_mps_melem(handles, len(states), len(ops), iptr(dims) if ops else None, off.ctypes.data_as(POINTER(c_int64)) if ops else None,
                                  dptr(data) if ops else None, len(jb), iptr(jb), iptr(jo), iptr(jk), method, dptr(out))
    return rc, out


def test_refused_calls_and_nan_operators_return_their_buffers():
    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import MPO, DeviceMPS
    from aqc_research_amd.mps_observables import operator_elements

    hm = mps_obs_ref.hand_made
    a, b = (DeviceMPS.from_qiskit(hm(ref.KET6, 991 + l), assume_canonical=True) for l in range(2))
    wide = DeviceMPS.from_qiskit(hm([1, 2, 4, 65, 4, 2, 1], 993), assume_canonical=True)
    other = DeviceMPS.from_qiskit(hm([1, 2, 2, 1], 994), assume_canonical=True)
    try:
        h, fat = MPO.xxz(6, ref.DELTA), _mpo(mps_opsum_ref.random_mpo([1, 4, 33, 4, 4, 2, 1], 995))
        live = live_buffers()
        err = lambda: _lib.lib().aqc_last_error().decode()   # noqa: E731
        for states, ops, jb, jo, jk, method, words in (
                ([a, b], [h], [0, 2], [0, 0], [1, 1], 0, "job 1 names a state"), ([a, b], [h], [0, 0], [0, 0], [1, -1], 0, "job 1 names a state"),
                ([a, b], [h], [0], [1], [1], 0, "job 0 names an operator"), ([a, b], [h], [0], [-2], [1], 0, "job 0 names an operator"),
                ([a, b], [h], [0], [0], [1], 3, "unknown method"), ([a, other], [h], [0], [0], [0], 0, "differ in size"),
                ([a, wide], [h], [0, 1], [0, 0], [0, 0], 1, "job 1"), ([a, b], [h, fat], [0, 0, 1], [0, -1, 1], [1, 1, 1], 1, "job 2")):
            rc, _ = _abi(states, ops, jb, jo, jk, method)
            assert rc != 0 and words in err(), (words, err())
            assert live_buffers() == live
        rc, _ = _abi([a, wide], [h], [0, 1], [0, 0], [0, 0], 1)
        assert rc != 0 and "fused" in err() and "65" in err()
        rc, _ = _abi([a, b], [h, fat], [0], [1], [1], 1)
        assert rc != 0 and "operator bond" in err() and "33" in err()
        # a NaN operator entry spoils its own jobs only
        sick = [np.array(w) for w in h.sites]
        sick[3][0, 1, 0, 1] = np.nan
        sick = MPO(sick)
        jobs = [(a, h, b), (a, sick, b), (b, None, a), (wide, sick, a), (wide, h, a)]
        clean = operator_elements([jobs[0], jobs[2], jobs[4]])
        for method in (None, "gemm"):
            got = operator_elements(jobs, method=method)
            assert not np.isfinite(got[1]) and not np.isfinite(got[3]) and np.all(np.isfinite(got[[0, 2, 4]]))
            assert np.array_equal(got[[0, 2, 4]], clean if method is None else operator_elements([jobs[0], jobs[2], jobs[4]], method="gemm"))
            assert live_buffers() == live
    finally:
        for m in (a, b, wide, other):
            m.close()
