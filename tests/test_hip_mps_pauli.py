"""GPU: Pauli strings between DeviceMPS states (aqc_research_amd/mps_observables.py: pauli_strings, overlaps, energy; kernels:
csrc/aqc_mps_pauli.hip) against the dense statement (tests/mps_pauli_ref.by_dense), against the NumPy walk (by_transfer) beyond dense
reach, against what the project already computes (magnetisation, correlation_matrix, bond_energies, dot, dot_ops) and against
properties that need no reference.

Bond profiles are those of tests/test_hip_mps_observables.py (n = 13 unless said): A reaches the fused cap with bonds that are no
multiples of 4 or 16 and rectangular sites, B are product states, C has a bond of 1 inside, D lies beyond the fused cap (the rule picks
gemm), F is oracle.random_mps(13, 8), Q1 is one qubit.  The tolerance is the project's TOL = 1e-10 x |phi| |psi|, since
|<phi|P|psi>| <= |phi| |psi|; the tests print what they observe and DESIGN.md 6r records it."""
import functools

import numpy as np
import pytest

from tests import mps_obs_ref, mps_pauli_ref
from tests.helpers import TOL

pytestmark = pytest.mark.gpu

PROFILES = {
    "A": (mps_obs_ref.PROFILE_A, 801), "B2": (mps_obs_ref.profile_b(2), 802), "B13": (mps_obs_ref.profile_b(13), 803),
    "C": (mps_obs_ref.PROFILE_C, 804), "D": (mps_obs_ref.PROFILE_D, 805), "Q1": ([1, 1], 806),
}
NAMES = sorted(PROFILES) + ["F"]
FUSED_NAMES = [k for k in NAMES if k != "D"]
PAULI2 = {1: mps_pauli_ref.PAULI[1], 2: mps_pauli_ref.PAULI[2], 3: mps_pauli_ref.PAULI[3]}


def _methods(*names):
    return (None, "gemm") if "D" in names else (None, "fused", "gemm")


def _maxdiff(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(QiskitMPS tuple, dense vector, test strings, <psi|P|psi> of the dense statement): computed once, never changed."""
    if name == "F":
        from oracle.aqc_oracle import random_mps

        mps = random_mps(13, 8, np.random.default_rng(807))
    else:
        mps = mps_obs_ref.hand_made(*PROFILES[name])
    psi = mps_obs_ref.dense(mps)
    n = len(mps[0])
    strings = mps_pauli_ref.ref_strings(n, 810 + n)
    if name == "A":   # more workgroups than compute units
        strings = np.concatenate([strings, np.random.default_rng(811).integers(0, 4, size=(300, n)).astype(np.uint8)])
    want = mps_pauli_ref.by_dense(mps, mps, strings, psi, psi)
    for arr in (psi, strings, want):
        arr.setflags(write=False)
    return mps, psi, strings, want


@functools.lru_cache(maxsize=None)
def _cross(bra, ket):
    """<bra|P|ket> of the dense statement for the ket's strings."""
    (bm, bpsi, _, _), (km, kpsi, strings, _) = _case(bra), _case(ket)
    want = mps_pauli_ref.by_dense(bm, km, strings, bpsi, kpsi)
    want.setflags(write=False)
    return want


def _device(name):
    from aqc_research_amd.mps_engine import DeviceMPS

    return DeviceMPS.from_qiskit(_case(name)[0])


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


@pytest.mark.parametrize("method", (None, "fused", "gemm"))
@pytest.mark.parametrize("name", NAMES)
def test_expectation_values_match_the_dense_statement(name, method):
    from aqc_research_amd.mps_observables import pauli_route, pauli_strings

    _, _, strings, want = _case(name)
    m = _device(name)
    try:
        assert pauli_route(None, m.bond_dims) == ("gemm" if name == "D" else "fused")
        if name == "D" and method == "fused":
            with pytest.raises(ValueError):
                pauli_strings(m, strings, method="fused")
            return
        before = _flat(m.to_qiskit())
        got = pauli_strings(m, strings, method=method)
        assert got.shape == want.shape and got.dtype == np.complex128
        err, imag = _maxdiff(got, want), float(np.max(np.abs(got.imag)))
        print(f"profile {name}, method {method}, {len(strings)} strings: max |<P> - statement| = {err:.3g}, max |Im| = {imag:.3g}")
        assert err <= TOL and imag <= TOL, (name, method, err, imag)
        assert np.array_equal(_flat(m.to_qiskit()), before)
    finally:
        m.close()


@pytest.mark.parametrize("bra,ket", (("A", "F"), ("F", "A"), ("D", "A")))
def test_bra_ket_values_match_the_dense_statement(bra, ket):
    from aqc_research_amd.mps_observables import pauli_route, pauli_strings

    strings, want = _case(ket)[2], _cross(bra, ket)
    b, k = _device(bra), _device(ket)
    try:
        assert pauli_route(b.bond_dims, k.bond_dims) == ("gemm" if "D" in (bra, ket) else "fused")
        before = _flat(b.to_qiskit()), _flat(k.to_qiskit())
        for method in _methods(bra, ket):
            got = pauli_strings(k, strings, bras=b, method=method)
            swapped = pauli_strings(b, strings, bras=k, method=method)
            err, sym = _maxdiff(got, want), _maxdiff(got, swapped.conj())
            print(f"<{bra}|P|{ket}>, method {method}: max |value - statement| = {err:.3g}, max |value - conj(swapped)| = {sym:.3g}")
            assert got.shape == want.shape and err <= TOL and _maxdiff(swapped, want.conj()) <= TOL and sym <= TOL
        if "D" in (bra, ket):
            with pytest.raises(ValueError):
                pauli_strings(k, strings, bras=b, method="fused")
        assert np.array_equal(_flat(b.to_qiskit()), before[0]) and np.array_equal(_flat(k.to_qiskit()), before[1])
    finally:
        b.close()
        k.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_state_as_its_own_bra_gives_the_expectation_values(name):
    from aqc_research_amd.mps_observables import pauli_strings

    strings = _case(name)[2]
    m = _device(name)
    try:
        for method in _methods(name):
            one, two = pauli_strings(m, strings, method=method), pauli_strings(m, strings, bras=m, method=method)
            diff = _maxdiff(one, two)
            print(f"profile {name}, method {method}: max |expectation mode - bra/ket mode| = {diff:.3g}")
            assert diff <= TOL
    finally:
        m.close()


@pytest.mark.parametrize("name", FUSED_NAMES)
def test_the_two_routes_agree(name):
    from aqc_research_amd.mps_observables import pauli_strings

    strings = _case(name)[2]
    m, f = _device(name), _device("F" if len(_case(name)[0][0]) == 13 else name)
    try:
        d1 = _maxdiff(pauli_strings(m, strings, method="fused"), pauli_strings(m, strings, method="gemm"))
        d2 = _maxdiff(pauli_strings(m, strings, bras=f, method="fused"), pauli_strings(m, strings, bras=f, method="gemm"))
        print(f"profile {name}: max |fused - gemm| = {d1:.3g} (expectation), {d2:.3g} (against a bra)")
        assert d1 <= TOL and d2 <= TOL
        assert np.array_equal(pauli_strings(_case(name)[0], strings), pauli_strings(m, strings, method="fused"))   # the rule's choice, a tuple
    finally:
        m.close()
        f.close()


def test_overlaps_against_dot():
    from aqc_research_amd.mps_observables import overlaps

    states = [_device(k) for k in ("A", "F", "B13", "D")]   # pairs with D go the gemm way, the others fused
    try:
        want = np.array([[a.dot(b) for b in states] for a in states])
        for method in (None, "gemm"):
            got = overlaps(states, states, method=method)
            err, herm = _maxdiff(got, want), _maxdiff(got, got.conj().T)
            print(f"4 x 4 overlaps, method {method}: max |overlap - dot| = {err:.3g}, max |G - G^H| = {herm:.3g}")
            assert got.shape == (4, 4) and err <= TOL and herm <= TOL
        rect = overlaps(states[:1], states[1:3])
        assert rect.shape == (1, 2) and _maxdiff(rect, want[:1, 1:3]) <= TOL
        assert np.array_equal(states[0].overlaps(states[1:3]), rect[0])
    finally:
        for m in states:
            m.close()


@pytest.mark.parametrize("name", ("A", "F"))
def test_agreement_with_the_pair_density_matrices_and_dot_ops(name):
    from aqc_research_amd import mps_observables as mo

    n = 13
    m, other = _device(name), _device("F" if name == "A" else "A")
    try:
        for method in (None, "gemm"):
            z = mo.pauli_strings(m, [("Z", (q,)) for q in range(n)], method=method)
            worst = _maxdiff(z.real, mo.magnetisation(m, "z"))
            for letters in ("zz", "xy"):
                pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
                vals = mo.pauli_strings(m, [(letters.upper(), p) for p in pairs], method=method)
                c = mo.correlation_matrix(m, letters)
                worst = max(worst, _maxdiff(vals.real, [c[i, j] for i, j in pairs]), float(np.max(np.abs(vals.imag))))
            for delta in (1.0, -0.7):
                e = mo.energy(m, mps_pauli_ref.xxz_terms(n, delta), method=method)
                assert np.shape(e) == ()
                worst = max(worst, abs(float(e) - float(mo.bond_energies(m, delta).sum())))
            strings = _case(name)[2][14:24]   # ten of the random strings
            got = m.pauli_strings(strings, bra=other, method=method)
            want = [other.dot_ops(m, [(q, PAULI2[int(s[q])]) for q in range(n) if s[q]]) for s in strings]
            worst = max(worst, _maxdiff(got, want))
            print(f"profile {name}, method {method}: max difference from magnetisation, correlation_matrix, bond_energies, dot_ops = {worst:.3g}")
            assert worst <= TOL
        both = mo.energy([m, _case(name)[0]], mps_pauli_ref.xxz_terms(n, 1.0))
        assert both.shape == (2,) and both[0] == both[1]
    finally:
        m.close()
        other.close()


@pytest.mark.parametrize("method", (None, "gemm"))
def test_strings_lanes_and_duplicates_are_bit_for_bit(method):
    from aqc_research_amd.mps_observables import pauli_strings

    states = [_device(k) for k in ("A", "B13", "F")]
    bras = [_device(k) for k in ("F", "A", "A")]
    try:
        strings = np.array(_case("A")[2][:50])
        strings[37] = strings[5]                                            # a string listed twice
        for kw in ({}, {"bras": bras}):
            got = pauli_strings(states, strings, method=method, **kw)
            assert got.shape == (3, 50)
            assert np.array_equal(got[:, 37], got[:, 5])
            for lane, m in enumerate(states):
                one = pauli_strings(m, strings, method=method, **({"bras": bras[lane]} if kw else {}))
                assert np.array_equal(one, got[lane]), lane
            m = states[0]
            lane_kw = {"bras": bras[0]} if kw else {}
            for s in range(50):
                assert np.array_equal(pauli_strings(m, strings[s:s + 1], method=method, **lane_kw)[0], got[0, s]), s
        if method is None:   # A, B13 and F go the fused way; D beside them goes its own
            d = _device("D")
            try:
                four = pauli_strings(states + [d], strings)
                assert np.array_equal(four[:3], pauli_strings(states, strings)) and np.array_equal(four[3], pauli_strings(d, strings, method="gemm"))
            finally:
                d.close()
    finally:
        for m in states + bras:
            m.close()


@pytest.mark.parametrize("name", ("A", "D", "F"))
def test_scaled_states_scale_the_values(name):
    from aqc_research_amd.mps_observables import pauli_strings

    def times(mps, f):
        gam, lam = mps
        return [(f * gam[0][0], f * gam[0][1])] + list(gam[1:]), lam

    mps, strings = _case(name)[0], _case(name)[2][:54]
    phi = _case("A" if name != "A" else "F")[0]
    for method in _methods(name):
        one, nine = pauli_strings(mps, strings, method=method), pauli_strings(times(mps, 3.0), strings, method=method)
        cross, six = pauli_strings(mps, strings, bras=phi, method=method), pauli_strings(times(mps, 2.0), strings, bras=times(phi, 3.0), method=method)
        e9, e6 = _maxdiff(nine, 9.0 * one), _maxdiff(six, 6.0 * cross)
        print(f"profile {name}, method {method}: max |<P>(3 psi) - 9 <P>(psi)| = {e9:.3g}, max |<3 phi|P|2 psi> - 6 <phi|P|psi>| = {e6:.3g}")
        assert e9 <= 9 * TOL and e6 <= 6 * TOL


def _trotter(n, layers=3, evol_time=0.8):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index

    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)
    th = init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=evol_time, delta=1.0)
    return circ, th, neel_state_index(n)


def test_forty_qubits():
    """Beyond dense reach: n = 40, engine-made with max_bond = 16, expectation mode and a bra / ket pair against the NumPy walk."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import pauli_strings

    n = 40
    basis = me.DeviceMPS.basis_state(n, _trotter(n)[2])
    made = []
    try:
        for evol_time in (2.4, 2.0):
            circ, th, _ = _trotter(n, layers=6, evol_time=evol_time)
            made.append(me.v_mul_mps(circ, th, basis, trunc_thr=1e-14, max_bond=16))
        psi, phi = made
        assert psi.bond_dims.max() == 16   # the cap binds
        strings = mps_pauli_ref.ref_strings(n, 850, random_count=20)
        qpsi, qphi = psi.to_qiskit(), phi.to_qiskit()
        scale = float(np.sqrt(abs(psi.dot(psi)) * abs(phi.dot(phi))))
        want, cross = mps_pauli_ref.by_transfer(qpsi, qpsi, strings), mps_pauli_ref.by_transfer(qphi, qpsi, strings)
        for method in (None, "fused", "gemm"):
            e1 = _maxdiff(pauli_strings(psi, strings, method=method), want)
            e2 = _maxdiff(pauli_strings(psi, strings, bras=phi, method=method), cross)
            print(f"n = {n}, bonds <= 16, method {method}: max |<P> - walk| = {e1:.3g}, max |<phi|P|psi> - walk| = {e2:.3g} "
                  f"(largest |<phi|P|psi>| = {np.max(np.abs(cross)):.3g})")
            assert e1 <= TOL * abs(psi.dot(psi)) and e2 <= TOL * scale
    finally:
        for m in made + [basis]:
            m.close()


def test_engine_made_states():
    """The Neel state at n = 12 under a second-order Trotter ansatz, exact, against the dense vector of the same state; and the basis
    state itself: Z strings are +-1 and X_q is 0, exactly."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import pauli_strings
    from aqc_research_amd.mps_operations import mps_to_vector

    n = 12
    circ, th, neel = _trotter(n)
    basis = me.DeviceMPS.basis_state(n, neel)
    exact = me.v_mul_mps(circ, th, basis, trunc_thr=1e-16, max_bond=0, method="single")
    try:
        strings = mps_pauli_ref.ref_strings(n, 860)
        q = exact.to_qiskit()
        vec = mps_to_vector(q)
        want = mps_pauli_ref.by_dense(q, q, strings, vec, vec)
        for method in (None, "gemm"):
            err = _maxdiff(pauli_strings(exact, strings, method=method), want)
            print(f"engine-made, n = {n}, bonds <= {exact.bond_dims.max()}, method {method}: max |<P> - dense| = {err:.3g}")
            assert err <= TOL
            zs = np.array([[3 * ((k >> q) & 1) for q in range(n)] for k in (0, 1, 5, 0xFFF, 0x0A5, 0x800)], dtype=np.uint8)
            signs = [(-1.0) ** bin(k & neel).count("1") for k in (0, 1, 5, 0xFFF, 0x0A5, 0x800)]
            assert np.array_equal(pauli_strings(basis, zs, method=method), np.array(signs, dtype=np.complex128))
            xs = pauli_strings(basis, [("X", (q,)) for q in range(n)] + [("Y", (q,)) for q in range(n)], method=method)
            assert np.array_equal(xs, np.zeros(2 * n, dtype=np.complex128))
    finally:
        for m in (exact, basis):
            m.close()


def test_abi_refusals_leave_no_buffers_and_a_correct_call_follows():
    from ctypes import POINTER, c_uint8, c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import pauli_strings

    L = _lib.lib()
    u8 = lambda a: a.ctypes.data_as(POINTER(c_uint8))   # noqa: E731
    a, d, five = _device("C"), _device("D"), DeviceMPS.basis_state(5)
    try:
        strings = np.array(_case("C")[2][:6])
        out = np.zeros((2, 6), dtype=np.complex128)
        hs = (c_void_p * 2)(a.handle, a.handle)

        def call(bras, kets, npairs, nstrings, s, method=0, dst=out):
            return L.aqc_mps_pauli(bras, kets, npairs, nstrings, None if s is None else u8(s), method, None if dst is None else _lib.dptr(dst))

        live = live_buffers()
        assert call(None, None, 2, 6, strings) == 1 and call(None, hs, 2, 6, None) == 1 and call(None, hs, 2, 6, strings, dst=None) == 1
        assert call(None, (c_void_p * 2)(a.handle, None), 2, 6, strings) == 1 and call((c_void_p * 2)(a.handle, None), hs, 2, 6, strings) == 1
        assert call(None, hs, 0, 6, strings) == 1 and call(None, hs, 2, 0, strings) == 1
        assert call(None, (c_void_p * 2)(a.handle, five.handle), 2, 6, strings) == 1 and b"differ" in L.aqc_last_error()
        assert call((c_void_p * 2)(a.handle, five.handle), hs, 2, 6, strings) == 1
        assert call(None, hs, 2, 6, strings, method=3) == 1
        bad = strings.copy()
        bad[2, 1] = 9
        assert call(None, hs, 2, 6, bad) == 1 and b"string 2, qubit 1" in L.aqc_last_error()
        dstrings = np.array(_case("D")[2][:6])
        assert call(None, (c_void_p * 1)(d.handle), 1, 6, dstrings, method=1) == 1 and b"fused" in L.aqc_last_error()
        assert call((c_void_p * 1)(d.handle), (c_void_p * 1)(d.handle), 1, 6, dstrings, method=1) == 1
        assert live_buffers() == live
        with pytest.raises(ValueError):
            pauli_strings(d, dstrings, method="fused")
        assert live_buffers() == live
        assert call(None, hs, 2, 6, strings) == 0
        assert _maxdiff(out[1], _case("C")[3][:6]) <= TOL and np.array_equal(out[0], out[1])
        assert call(hs, hs, 2, 6, strings, method=2) == 0 and _maxdiff(out[0], _case("C")[3][:6]) <= TOL
        assert _maxdiff(pauli_strings(d, dstrings), _case("D")[3][:6]) <= TOL
        assert live_buffers() == live
        closed = _device("C")
        closed.close()
        with pytest.raises(ValueError):
            pauli_strings(closed, strings)
    finally:
        for m in (a, d, five):
            m.close()


def test_jobs_walked_in_several_groups():
    """Bonds of 512: a job of the gemm route holds 3 x 512^2 complex numbers (12 MiB), so the 256 MiB of a group hold 21 of 30 strings
    and the walk is made twice.  No reference is formed at this size: a call with one string has one group, and a value must not depend
    on what else is in the call -- bit for bit -- nor the identity string on anything but <psi|psi>."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import pauli_route, pauli_strings

    dims = [1, 8, 64, 512, 512, 512, 300, 512, 512, 64, 8, 1]
    n = len(dims) - 1
    m = DeviceMPS.from_qiskit(mps_obs_ref.hand_made(dims, 870))
    try:
        assert pauli_route(None, m.bond_dims) == "gemm"
        strings = np.concatenate([np.zeros((1, n), dtype=np.uint8), np.random.default_rng(871).integers(0, 4, size=(29, n)).astype(np.uint8)])
        got = pauli_strings(m, strings)
        both = pauli_strings(m, strings, bras=m)
        norm = m.dot(m)
        print(f"bonds <= 512, two groups of jobs: |<I> - <psi|psi>| = {abs(got[0] - norm):.3g}, max |expectation - bra/ket| = {_maxdiff(got, both):.3g}")
        assert abs(got[0] - norm) <= TOL and abs(both[0] - norm) <= TOL and _maxdiff(got, both) <= TOL
        assert float(np.max(np.abs(got.imag))) <= TOL
        for k in (0, 5, 20, 21, 29):   # strings of the first group and of the second
            assert np.array_equal(pauli_strings(m, strings[k:k + 1])[0], got[k]), k
            assert np.array_equal(pauli_strings(m, strings[k:k + 1], bras=m)[0], both[k]), k
    finally:
        m.close()
