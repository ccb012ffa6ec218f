"""GPU: Schmidt spectra of DeviceMPS states (aqc_research_amd/mps_observables.py: schmidt_values, entanglement_entropies,
bond_dims_needed; kernels: csrc/aqc_mps_ent.hip) against SVDs of the dense vector (tests/mps_ent_ref.schmidt_dense), against the NumPy
QR chain (mps_ent_ref.schmidt) beyond dense reach, the two routes against each other, and properties that need no reference.

Bond profiles are those of tests/test_mps_ent_ref.py plus Q1 (one qubit: no cut) and D (beyond the fused cap: the rule picks
canonical).  The tolerance is the project's TOL = 1e-10 x |psi|: a singular value moves by at most the norm of a perturbation and
|psi| is the Frobenius norm of every cut.  The tests print what they observe and DESIGN.md 6u records it."""
import functools

import numpy as np
import pytest

from tests import mps_ent_ref, mps_obs_ref, mps_trunc_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes
from tests.test_mps_ent_ref import NAMES as CPU_NAMES
from tests.test_mps_ent_ref import case as _cpu_case

pytestmark = pytest.mark.gpu

NAMES = list(CPU_NAMES) + ["D", "Q1"]
EXTRA = {"D": (mps_obs_ref.PROFILE_D, 805), "Q1": ([1, 1], 806)}


def _maxdiff(a, b) -> float:
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


@functools.lru_cache(maxsize=None)
def _case(name):
    """(QiskitMPS tuple, bond dimensions, |psi|, Schmidt values by dense SVDs): computed once, never changed."""
    if name in EXTRA:
        mps = mps_obs_ref.hand_made(*EXTRA[name])
        dims = list(EXTRA[name][0])
        psi = mps_obs_ref.dense(mps)
        want = mps_ent_ref.schmidt_dense(psi, dims)
        want.setflags(write=False)
    else:
        mps, dims, psi, want = _cpu_case(name)
    return mps, dims, float(np.linalg.norm(psi)), want


def _device(name):
    from aqc_research_amd.mps_engine import DeviceMPS

    return DeviceMPS.from_qiskit(_case(name)[0])


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


@pytest.mark.parametrize("name", NAMES)
def test_values_match_the_dense_statement_on_both_routes(name):
    from aqc_research_amd.mps_observables import entanglement_route, schmidt_values

    _, dims, norm, want = _case(name)
    m = _device(name)
    try:
        assert entanglement_route(m.bond_dims) == ("canonical" if name == "D" else "fused")
        before = _flat(m.to_qiskit())
        got = {}
        for method in (None, "fused", "canonical"):
            if name == "D" and method == "fused":
                with pytest.raises(ValueError):
                    schmidt_values(m, method="fused")
                continue
            vals, info = schmidt_values(m, method=method, details=True)
            assert vals.shape == want.shape == (len(dims) - 2, max(dims[1:-1] + [1])) and vals.dtype == np.float64
            assert info["route"] == (method or ("canonical" if name == "D" else "fused")) and np.all(info["status"] == 0)
            assert info["sweeps"].shape == info["status"].shape == (len(dims) - 2,)
            err = _maxdiff(vals, want)
            print(f"profile {name}, method {method}: max |value - dense SVD| = {err:.3g} (|psi| = {norm:.3g}), "
                  f"sweeps {info['sweeps'].min() if vals.size else 0} - {info['sweeps'].max() if vals.size else 0}")
            assert err <= TOL * norm, (name, method, err)
            assert np.all(np.diff(vals, axis=1) <= 0.0)
            for q in range(1, len(dims) - 1):
                assert np.all(vals[q - 1, dims[q]:] == 0.0)
            got[method] = vals
        if "fused" in got:
            routes = _maxdiff(got["fused"], got["canonical"])
            print(f"profile {name}: max |fused - canonical| = {routes:.3g}")
            assert routes <= TOL * norm
            assert np.array_equal(got[None], got["fused"])
            assert np.array_equal(m.schmidt_values(), got["fused"]) and np.array_equal(schmidt_values(_case(name)[0]), got["fused"])   # a tuple
        assert np.array_equal(_flat(m.to_qiskit()), before)
    finally:
        m.close()


def test_a_prescribed_spectrum():
    """Nested pairs (k, 7 - k) in cos a_k |00> + sin a_k |11>: the middle cut's 16 values are products of cosines and sines, the
    smallest 1e-6 of the largest, and must be right to TOL absolute."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import schmidt_values

    mps, vals = mps_ent_ref.nested_pairs((0.1, 0.01, 0.001, 0.7))
    assert 0.5e-6 < vals[-1] / vals[0] < 2e-6
    m = DeviceMPS.from_qiskit(mps)
    try:
        for method in (None, "fused"):
            got = schmidt_values(m, method=method)
            err = _maxdiff(got[3], vals)
            print(f"nested pairs, method {method}: max |value - product| = {err:.3g}, smallest value {got[3, -1]:.6e} (wanted {vals[-1]:.6e})")
            assert got.shape == (7, 16) and err <= TOL
            assert _maxdiff(got, mps_ent_ref.schmidt(mps)) <= TOL
    finally:
        m.close()


def test_factors_square_to_the_environments():
    from aqc_research_amd.mps_observables import schmidt_factors, schmidt_values

    mps, dims, norm, want = _case("A")
    ts = mps_obs_ref.site_tensors(mps)
    left, right = mps_obs_ref.left_environments(ts), mps_obs_ref.right_environments(ts)
    m = _device("A")
    try:
        vals, c, d = schmidt_factors(m)
        assert np.array_equal(vals, schmidt_values(m, method="fused")) and len(c) == len(d) == len(dims) - 2
        worst_l = worst_r = 0.0
        for q in range(1, len(dims) - 1):
            cq, dq = c[q - 1], d[q - 1]
            assert cq.shape == dq.shape == (dims[q], dims[q]) and np.all(np.tril(cq, -1) == 0.0) and np.all(np.tril(dq, -1) == 0.0)
            worst_l = max(worst_l, _maxdiff(cq.conj().T @ cq, left[q]))
            worst_r = max(worst_r, _maxdiff((dq.conj().T @ dq).conj(), right[q]))
            assert _maxdiff(np.linalg.svd(cq @ dq.T, compute_uv=False), want[q - 1, :dims[q]]) <= TOL * norm
        print(f"profile A: max |C^H C - L| = {worst_l:.3g}, max |conj(D^H D) - R| = {worst_r:.3g}")
        assert worst_l <= TOL * norm ** 2 and worst_r <= TOL * norm ** 2
    finally:
        m.close()


def _times(mps, f):
    gam, lam = mps
    return [(f * gam[0][0], f * gam[0][1])] + list(gam[1:]), lam


@pytest.mark.parametrize("method", ("fused", "canonical"))
def test_scaled_states_scale_the_values(method):
    from aqc_research_amd.mps_observables import schmidt_values

    mps, _, norm, _ = _case("A")
    one, three = schmidt_values(mps, method=method), schmidt_values(_times(mps, 3.0), method=method)
    err = _maxdiff(three, 3.0 * one)
    print(f"profile A, method {method}: max |s(3 psi) - 3 s(psi)| = {err:.3g}")
    assert err <= 3 * TOL * norm


def test_a_change_of_gauge_keeps_the_values():
    """X and its inverse (a random 7 x 7 matrix, condition number 5) inserted on the bond of dimension 7 of A.  The factors of the new
    gauge are larger than the state, and what the product C_q D_q^T loses scales with them: the bound is TOL |C_q|_F |D_q|_F of the
    reference's factors, per cut."""
    from aqc_research_amd.mps_observables import schmidt_values

    mps, dims, norm, want = _case("A")
    bond = dims.index(7)
    rng = np.random.default_rng(830)
    u, _, vh = np.linalg.svd(rng.standard_normal((7, 7)) + 1j * rng.standard_normal((7, 7)))
    x = u @ np.diag(np.linspace(1.0, 5.0, 7)) @ vh
    xinv = vh.conj().T @ np.diag(1.0 / np.linspace(1.0, 5.0, 7)) @ u.conj().T
    assert np.linalg.cond(x) <= 10.0
    gam = list(mps[0])
    gam[bond - 1] = (gam[bond - 1][0] @ x, gam[bond - 1][1] @ x)
    gam[bond] = (xinv @ gam[bond][0], xinv @ gam[bond][1])
    gauged = (gam, mps[1])
    c, d = mps_ent_ref.factors(mps_obs_ref.site_tensors(gauged))
    got = schmidt_values(gauged, method="fused")
    worst = 0.0
    for q in range(1, len(dims) - 1):
        bound = TOL * float(np.linalg.norm(c[q]) * np.linalg.norm(d[q]))
        err = _maxdiff(got[q - 1], want[q - 1])
        worst = max(worst, err / bound)
        assert err <= bound, (q, err, bound)
    print(f"profile A with X, X^-1 on bond {bond}: largest error / bound = {worst:.3g}")


def test_engine_made_states():
    """A 2-layer second-order Trotter circuit on 12 qubits, exact, against SVDs of its dense vector; after canonicalize() the values are
    the state's own bond vectors."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import entanglement_entropies, entropies_of, schmidt_values
    from aqc_research_amd.mps_operations import mps_to_vector
    from tests.test_hip_mps_pauli import _trotter

    n = 12
    circ, th, neel = _trotter(n, layers=2)
    basis = me.DeviceMPS.basis_state(n, neel)
    exact = me.v_mul_mps(circ, th, basis, trunc_thr=1e-16, max_bond=0, method="single")
    try:
        dims = [int(v) for v in exact.bond_dims]
        want = mps_ent_ref.schmidt_dense(mps_to_vector(exact.to_qiskit()), dims)
        for method in (None, "canonical"):
            err = _maxdiff(schmidt_values(exact, method=method), want)
            print(f"engine-made, n = {n}, bonds <= {max(dims)}, method {method}: max |value - dense SVD| = {err:.3g}")
            assert err <= TOL
        vals = schmidt_values(exact)
        assert np.array_equal(entanglement_entropies(exact), entropies_of(vals)) and np.array_equal(exact.entropies(2.0), entropies_of(vals, 2.0))
        assert np.array_equal(schmidt_values(basis), np.ones((n - 1, 1)))   # a product state: one value of 1 at every cut, exactly
        canon = exact.clone().canonicalize()
        try:
            lam = canon.to_qiskit()[1]
            got = schmidt_values(canon)
            own = np.zeros_like(got)
            for q, v in enumerate(lam):
                own[q, :len(v)] = v
            err = _maxdiff(got, own)
            print(f"after canonicalize(): max |value - bond vector| = {err:.3g}")
            assert err <= TOL
        finally:
            canon.close()
    finally:
        for m in (exact, basis):
            m.close()


def test_forty_qubits():
    """Beyond dense reach: n = 40, engine-made with max_bond = 16, against the NumPy QR chain of the exported tensors."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import schmidt_values
    from tests.test_hip_mps_pauli import _trotter

    n = 40
    circ, th, neel = _trotter(n, layers=6, evol_time=2.4)
    basis = me.DeviceMPS.basis_state(n, neel)
    psi = me.v_mul_mps(circ, th, basis, trunc_thr=1e-14, max_bond=16)
    try:
        assert psi.bond_dims.max() == 16
        want = mps_ent_ref.schmidt(psi.to_qiskit())
        norm = float(np.sqrt(abs(psi.dot(psi))))
        for method in (None, "canonical"):
            err = _maxdiff(schmidt_values(psi, method=method), want)
            print(f"n = {n}, bonds <= 16, method {method}: max |value - QR chain| = {err:.3g} (|psi| = {norm:.6g})")
            assert err <= TOL * norm
    finally:
        for m in (psi, basis):
            m.close()


def test_bond_dims_needed_is_what_a_truncating_gate_leaves():
    """On a canonical clone the identity gate on (q, q + 1) with trunc_thr leaves bond q + 1 at the rank the rule gives of that cut's
    spectrum; the threshold is the first of a fixed list at which no decision sits where rounding could flip it."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import bond_dims_needed, schmidt_values
    from tests.test_hip_mps_pauli import _trotter

    n = 12
    circ, th, neel = _trotter(n, layers=2)
    basis = me.DeviceMPS.basis_state(n, neel)
    exact = me.v_mul_mps(circ, th, basis, trunc_thr=1e-16, max_bond=0, method="single")
    canon = exact.clone().canonicalize()
    eye4 = np.eye(4, dtype=np.complex128)
    try:
        vals, dims = schmidt_values(exact), exact.bond_dims
        thr = None
        for cand in (1e-6, 3e-6, 1e-7, 1e-5, 1e-8):
            decisions = [mps_trunc_ref.decide(vals[q - 1, :dims[q]], cand, 0) for q in range(1, n)]
            try:
                mps_trunc_ref.check_margins(decisions)
            except AssertionError:
                continue
            thr = cand
            break
        assert thr is not None
        ranks, dropped = bond_dims_needed(exact, thr)
        assert ranks.shape == dropped.shape == (n - 1,) and [d.k for d in decisions] == ranks.tolist()
        assert np.any(ranks < dims[1:n]) and np.all(dropped < thr)
        full, none = bond_dims_needed(exact)
        assert np.all(none == 0.0) and np.all(full <= dims[1:n])
        capped, _ = bond_dims_needed(exact, 0.0, 3)
        assert np.array_equal(capped, np.minimum(full, 3))
        left = []
        for q in range(n - 1):
            one = canon.clone()
            try:
                one.gate2(eye4, q, q + 1, thr)
                left.append(int(one.bond_dims[q + 1]))
                assert abs((one.discarded_weight - canon.discarded_weight) - dropped[q]) <= TOL
            finally:
                one.close()
        print(f"trunc_thr = {thr:g}: bonds {dims[1:n].tolist()} -> {ranks.tolist()}, dropped up to {dropped.max():.3g}")
        assert left == ranks.tolist()
    finally:
        for m in (canon, exact, basis):
            m.close()


_LANE_N = 7
_LANE_BONDS = {"A": [1, 2, 3, 7, 64, 37, 5, 1], "A2": [1, 2, 4, 13, 33, 64, 2, 1], "D": [1, 2, 4, 65, 96, 40, 2, 1], "D2": [1, 2, 3, 17, 65, 72, 2, 1]}


@functools.lru_cache(maxsize=None)
def _lane_mps(profile, seed):
    return mps_obs_ref.hand_made(_LANE_BONDS[profile], seed)


@pytest.mark.parametrize("method", ("fused", "canonical"))
def test_lanes_hold_the_lane_contract(method):
    """Four states, probes (0, 3).  F: neighbours with other bonds of the same route (and no larger ones, so the width K of the result
    stays); N: every neighbour state holds NaN tensors, its rows are NaN and the probes' bits do not move."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import entanglement_route, schmidt_values

    mine, theirs = ("A", "A2") if method == "fused" else ("D", "D2")
    made = []

    def device(profile, seed, nan=False):
        gam, lam = _lane_mps(profile, seed)
        if nan:
            gam = [(g0 * np.nan, g1 * np.nan) for g0, g1 in gam]
        made.append(DeviceMPS.from_qiskit((gam, lam), assume_canonical=True))
        return made[-1]

    try:
        states = [device(mine, 880 + l) for l in range(4)]
        poison = [device(mine, 880 + l, nan=True) for l in range(4)]
        assert all(entanglement_route(m.bond_dims) == method for m in states)
        dims = _LANE_BONDS[mine]
        check_lanes(lambda s: schmidt_values(s), states, probes=(0, 3), tol=TOL, other=[device(theirs, 890 + l) for l in range(4)], poison=poison,
                    reference=lambda s, l: mps_ent_ref.schmidt_dense(mps_obs_ref.dense(_lane_mps(mine, 880 + l)), dims), reference_lanes=(0, 3))
        vals, info = schmidt_values([states[0], poison[1], poison[2], states[3]], details=True)
        assert np.all(np.isnan(vals[1:3])) and np.all(np.isfinite(vals[[0, 3]])) and np.all(info["status"][1:3] == 2) and np.all(info["status"][[0, 3]] == 0)
        twice = schmidt_values([states[0], states[1], states[0]])
        assert np.array_equal(twice[0], twice[2]) and np.array_equal(twice[0], schmidt_values(states[0]))
    finally:
        for m in made:
            m.close()


def test_more_matrices_than_a_launch_of_sixty_four():
    """40 states of profile C in one call: 120 cuts.  Every lane has the bits of its own one-state call."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import schmidt_values

    tuples = [mps_obs_ref.hand_made(mps_obs_ref.PROFILE_C, 900 + l) for l in range(40)]
    made = [DeviceMPS.from_qiskit(t, assume_canonical=True) for t in tuples]
    try:
        got = schmidt_values(made)
        assert got.shape == (40, 3, 3)
        worst = 0.0
        for l in (0, 1, 17, 38, 39):
            assert np.array_equal(schmidt_values(made[l]), got[l]), l
        for l, t in enumerate(tuples):
            worst = max(worst, _maxdiff(got[l], mps_ent_ref.schmidt_dense(mps_obs_ref.dense(t), mps_obs_ref.PROFILE_C)))
        print(f"40 states of profile C: max |value - dense SVD| = {worst:.3g}")
        assert worst <= TOL
    finally:
        for m in made:
            m.close()


def test_refusals_leave_no_buffers_and_a_correct_call_follows():
    from ctypes import c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import schmidt_factors, schmidt_values

    L = _lib.lib()
    a, d, five = _device("C"), _device("D"), DeviceMPS.basis_state(5)
    try:
        s = np.zeros((2, 3, 96))
        sweeps, status = np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32)
        hs = (c_void_p * 2)(a.handle, a.handle)

        def call(states, nstates, method=0, kmax=3, dst=s, factors=None):
            return L.aqc_mps_ent_schmidt(states, nstates, method, kmax, None if dst is None else _lib.dptr(dst), _lib.iptr(sweeps), _lib.iptr(status), factors)

        live = live_buffers()
        assert call(None, 2) == 1 and call(hs, 2, dst=None) == 1 and call(hs, 0) == 1 and call(hs, 2, method=3) == 1
        assert call((c_void_p * 2)(a.handle, None), 2) == 1
        assert call((c_void_p * 2)(a.handle, five.handle), 2) == 1 and b"differ" in L.aqc_last_error()            # mixed n
        assert call(hs, 2, kmax=2) == 1 and b"kmax" in L.aqc_last_error()
        assert call((c_void_p * 1)(d.handle), 1, method=1, kmax=96) == 1 and b"fused" in L.aqc_last_error()        # beyond the cap
        assert call((c_void_p * 1)(d.handle), 1, kmax=96, factors=_lib.dptr(np.zeros(1 << 16, np.complex128))) == 1
        assert live_buffers() == live
        with pytest.raises(ValueError):
            schmidt_values(d, method="fused")
        with pytest.raises(ValueError):
            schmidt_values(_case("D")[0], method="fused")     # a tuple: uploaded for the call, closed after the refusal
        with pytest.raises(ValueError):
            schmidt_factors(d)
        with pytest.raises(ValueError):
            schmidt_values([a, five])
        closed = _device("C")
        closed.close()
        with pytest.raises(ValueError):
            schmidt_values([a, closed])
        assert live_buffers() == live
        assert call(hs, 2, kmax=96) == 0
        want = _case("C")[3]
        assert _maxdiff(s[0, :, :3], want) <= TOL and np.array_equal(s[0], s[1]) and np.all(s[:, :, 3:] == 0.0) and np.all(status == 0)
        assert _maxdiff(schmidt_values(d), _case("D")[3]) <= TOL
        assert live_buffers() == live
    finally:
        for m in (a, d, five):
            m.close()
