"""GPU: measurement of DeviceMPS states (aqc_research_amd/mps_sampling.py, csrc/aqc_mps_sample.hip) against the NumPy statement of
the rule (tests/mps_sample_ref.py), against the dense vector where it can be formed, and against properties that need no reference.

Cases (tests/mps_sample_ref.CASES, hand_made states of norm 1.7): A reaches the fused cap with bonds that are no multiples of 4 or 16,
B2 / B13 are product states, C has a bond of 1 inside, D lies beyond the fused cap (the rule picks gemm, ``method="fused"`` raises), N40
is n = 40 with bonds of 16, beyond dense reach.  All samples use Philox seed 2024; 1000 shots are 15 full blocks of the fused kernel and
a tail of 40.

Bits are compared exactly on every shot whose reference margin is >= 1e-9 (ten times the project's TOL; fp64 differences observed in
this code base are ~1e-15); shots below may be left out, at most 1 % of a case.  tests/test_mps_sample_ref.py asserts that the
reference leaves out none of these cases' shots, so a test that skips many is failing.  The tests print what they observe and DESIGN.md
6q records it."""
import functools

import numpy as np
import pytest

from tests import mps_obs_ref, mps_sample_ref as ref
from tests.helpers import TOL

pytestmark = pytest.mark.gpu

SEED = ref.PHILOX_SEED
SHOTS = 1000
ROUTES = [(name, method) for name in ("A", "B2", "B13", "C", "N40") for method in ("fused", "gemm")] + [("D", "gemm")]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(QiskitMPS tuple, reference bits, amplitudes, margins of shots 0 .. 999 of lane 0): computed once, never changed."""
    mps = ref.case(name)
    bits, amps, margin = ref.sample(mps, SHOTS, seed=SEED)
    for arr in (bits, amps, margin):
        arr.setflags(write=False)
    return mps, bits, amps, margin


@functools.lru_cache(maxsize=None)
def _dense(name):
    from aqc_research_amd.mps_operations import mps_to_vector

    psi = mps_to_vector(_case(name)[0])
    psi.setflags(write=False)
    return psi


def _device(name):
    from aqc_research_amd.mps_engine import DeviceMPS

    return DeviceMPS.from_qiskit(_case(name)[0])


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


def _kept(margin, what):
    keep = margin >= ref.MARGIN
    assert np.count_nonzero(~keep) <= len(margin) // 100, (what, int(np.count_nonzero(~keep)))
    return keep


@pytest.mark.parametrize("name,method", ROUTES)
def test_bits_and_amplitudes_match_the_rule(name, method):
    from aqc_research_amd.mps_sampling import route, sample

    mps, want_bits, want_amps, margin = _case(name)
    n = len(mps[0])
    m = _device(name)
    try:
        assert route(m.bond_dims) == ("gemm" if name == "D" else "fused")
        if name == "D":
            with pytest.raises(ValueError):
                sample(m, SHOTS, seed=SEED, method="fused")
        before = _flat(m.to_qiskit())
        got = sample(m, SHOTS, seed=SEED, method=method, details=True)
        assert np.array_equal(_flat(m.to_qiskit()), before)
        by_rule = m.sample(SHOTS, seed=SEED)
    finally:
        m.close()
    bits, amps, prob, norm2 = got["bits"], got["amplitudes"], got["probabilities"], got["norm2"]
    assert bits.shape == (SHOTS, n) and bits.dtype == np.uint8 and amps.shape == (SHOTS,) and amps.dtype == np.complex128
    assert prob.shape == (SHOTS,) and isinstance(norm2, float)
    keep = _kept(margin, (name, method))
    assert np.array_equal(bits[keep], want_bits[keep]), (name, method, int(np.argmax(np.any(bits != want_bits, axis=1))))
    if method == ("gemm" if name == "D" else "fused"):
        assert np.array_equal(by_rule, bits)   # the rule's choice, through the DeviceMPS forward
    err = float(np.max(np.abs(amps[keep] - want_amps[keep])))
    err_norm = abs(norm2 - mps_obs_ref.norm2(mps))
    line = f"profile {name}, method {method}: {int(np.count_nonzero(~keep))} shots left out, max |amp - rule| = {err:.3g}, |norm2 - rule| = {err_norm:.3g}"
    assert err <= TOL * ref.NORM, line
    assert err_norm <= TOL * ref.NORM ** 2, line
    assert np.array_equal(prob, (amps.real ** 2 + amps.imag ** 2) / norm2)
    assert np.all(prob > 0.0) and np.all(prob <= 1.0 + TOL)
    distinct = np.unique(np.concatenate([bits, np.ascontiguousarray(prob).view(np.uint8).reshape(SHOTS, 8)], axis=1), axis=0)
    total = float(distinct[:, n:].copy().view(np.float64).sum())   # every distinct string once (equal strings have equal probabilities)
    assert len(distinct) == len(np.unique(bits, axis=0)) and total <= 1.0 + TOL, line
    if n <= 13:
        err_dense = float(np.max(np.abs(amps - _dense(name)[ref.indices(bits)])))
        line += f", max |amp - dense| = {err_dense:.3g}"
        assert err_dense <= TOL * ref.NORM, line
    print(line + f", the distinct strings carry {total:.4f} of the probability")


@pytest.mark.parametrize("method", ("fused", "gemm"))
def test_all_amplitudes_of_ten_qubits(method):
    """Odd bonds up to 32; 1024 strings are 16 workgroups of the fused kernel."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_operations import mps_to_vector
    from aqc_research_amd.mps_sampling import amplitudes

    n = 10
    mps = mps_obs_ref.hand_made([1, 2, 3, 5, 7, 13, 17, 32, 16, 4, 1], 21, norm=ref.NORM)
    every = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)
    m = DeviceMPS.from_qiskit(mps)
    try:
        before = _flat(m.to_qiskit())
        got = amplitudes(m, every, method=method)
        assert np.array_equal(m.amplitudes(every[37:300], method=method), got[37:300])   # rows do not depend on their neighbours
        assert np.array_equal(_flat(m.to_qiskit()), before)
    finally:
        m.close()
    err = float(np.max(np.abs(got - mps_to_vector(mps))))
    print(f"n = 10, method {method}: max |amplitudes - dense vector| = {err:.3g}")
    assert got.shape == (1 << n,) and err <= TOL * ref.NORM
    assert np.array_equal(amplitudes([mps, mps], every[:70], method=method), np.stack([got[:70]] * 2))   # tuples, lanes


def test_forty_qubits_amplitudes_of_the_sampled_strings():
    from aqc_research_amd.mps_sampling import amplitudes, sample

    mps, _, want_amps, margin = _case("N40")
    keep = _kept(margin, "N40")
    m = _device("N40")
    try:
        got = sample(m, SHOTS, seed=SEED, details=True)
        for method in ("fused", "gemm"):
            amps = amplitudes(m, got["bits"], method=method)
            err = float(np.max(np.abs(amps[keep] - want_amps[keep])))
            err_ref = float(np.max(np.abs(amps - ref.amplitudes(mps, got["bits"]))))
            # amplitudes of 40 qubits are tiny: also relative to the norm of the 1000 of them (40 products of 16 terms round to
            # 40 x 16 x 2^-52 = 1.4e-13 of the partial products at worst)
            rel = float(np.linalg.norm(amps - ref.amplitudes(mps, got["bits"])) / np.linalg.norm(amps))
            print(f"n = 40, method {method}: max |amplitudes - rule| = {max(err, err_ref):.3g}, relative to their norm {rel:.3g}")
            assert err <= TOL * ref.NORM and err_ref <= TOL * ref.NORM and rel <= TOL
            if method == "fused":
                assert np.array_equal(amps, got["amplitudes"])   # the same products as the sampling walk
    finally:
        m.close()


@pytest.mark.parametrize("name,method", (("A", "fused"), ("A", "gemm"), ("D", "gemm"), ("N40", "fused")))
def test_a_shot_depends_on_state_seed_lane_and_number_only(name, method):
    from aqc_research_amd.mps_sampling import sample

    mps = _case(name)[0]
    m = _device(name)
    try:
        before = _flat(m.to_qiskit())
        whole = sample(m, SHOTS, seed=SEED, method=method)
        halves = [sample(m, 500, seed=SEED, first_shot=f, method=method) for f in (0, 500)]
        assert np.array_equal(np.concatenate(halves), whole)
        assert np.array_equal(sample(m, 1, seed=SEED, first_shot=777, method=method)[0], whole[777])
        other = sample(m, SHOTS, seed=SEED + 1, method=method)
        assert other.shape == whole.shape and not np.array_equal(other, whole)
        three = sample([m, m, mps], SHOTS, seed=SEED, method=method, details=True)   # lanes 1 and 2 hold the same state
        assert three["bits"].shape == (3,) + whole.shape and three["norm2"].shape == (3,) and three["amplitudes"].shape == (3, SHOTS)
        assert np.array_equal(three["bits"][0], whole)
        assert not np.array_equal(three["bits"][1], whole) and not np.array_equal(three["bits"][2], whole)
        assert not np.array_equal(three["bits"][1], three["bits"][2])
        assert three["norm2"][0] == three["norm2"][1] == three["norm2"][2]
        if name == "A":   # the margins of lanes 1 and 2 are asserted for this case (tests/test_mps_sample_ref.py)
            for lane in (1, 2):
                want_bits, want_amps, margin = ref.sample(mps, SHOTS, seed=SEED, lane=lane)
                keep = _kept(margin, (name, lane))
                assert np.array_equal(three["bits"][lane][keep], want_bits[keep]), lane
                assert float(np.max(np.abs(three["amplitudes"][lane][keep] - want_amps[keep]))) <= TOL * ref.NORM
        assert np.array_equal(_flat(m.to_qiskit()), before)
    finally:
        m.close()


@pytest.mark.parametrize("name", ("A", "B2", "B13", "C", "N40"))
def test_the_two_routes_agree(name):
    """Identical bits on all shots (they are >= 1e-9 from every threshold), amplitudes within TOL x norm."""
    from aqc_research_amd.mps_sampling import sample

    m = _device(name)
    try:
        fused, gemm = (sample(m, SHOTS, seed=SEED, method=method, details=True) for method in ("fused", "gemm"))
    finally:
        m.close()
    diff = float(np.max(np.abs(fused["amplitudes"] - gemm["amplitudes"])))
    print(f"profile {name}: max |fused - gemm| amplitude = {diff:.3g}, norm2 {abs(fused['norm2'] - gemm['norm2']):.3g}")
    assert np.array_equal(fused["bits"], gemm["bits"])
    assert diff <= TOL * ref.NORM and abs(fused["norm2"] - gemm["norm2"]) <= TOL * ref.NORM ** 2


def test_mixed_routes_in_one_call():
    """A and D beside each other: each lane goes its own way by the rule and keeps its lane number."""
    from aqc_research_amd.mps_sampling import sample

    a, d = _device("A"), _device("D")
    try:
        both = sample([a, d, a], 200, seed=SEED)
        assert np.array_equal(both[0], _case("A")[1][:200])
        want_d, _, margin = ref.sample(_case("D")[0], 200, seed=SEED, lane=1)
        keep = _kept(margin, "D, lane 1")
        assert np.array_equal(both[1][keep], want_d[keep])
        assert np.array_equal(both[2], sample([a, a, a], 200, seed=SEED, method="fused")[2])
    finally:
        a.close()
        d.close()


def test_engine_made_states():
    """The Neel state at n = 12 under a second-order Trotter ansatz, exact and truncated at 1e-3: bits against the rule run on the
    state's own exported tensors."""
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index
    from aqc_research_amd.mps_sampling import sample

    n = 12
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 3), second_order=True)
    th = init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=0.8, delta=1.0)
    basis = me.DeviceMPS.basis_state(n, neel_state_index(n))
    exact = me.v_mul_mps(circ, th, basis, trunc_thr=1e-16, method="single")
    cut = me.v_mul_mps(circ, th, basis, trunc_thr=1e-3, method="single")
    try:
        assert cut.bond_dims.max() < exact.bond_dims.max()
        for label, m in (("exact", exact), ("truncated", cut)):
            tensors = m.to_qiskit()
            want_bits, want_amps, margin = ref.sample(tensors, SHOTS, seed=SEED)
            keep = _kept(margin, label)
            for method in ("fused", "gemm"):
                got = sample(m, SHOTS, seed=SEED, method=method, details=True)
                err = float(np.max(np.abs(got["amplitudes"][keep] - want_amps[keep])))
                print(f"{label} (bonds <= {m.bond_dims.max()}), method {method}: {int(np.count_nonzero(~keep))} shots left out, smallest margin "
                      f"{margin.min():.3g}, max |amp - rule| = {err:.3g}, norm2 {got['norm2']:.12f}")
                assert np.array_equal(got["bits"][keep], want_bits[keep]), (label, method)
                assert err <= TOL and abs(got["norm2"] - mps_obs_ref.norm2(tensors)) <= TOL
    finally:
        for m in (exact, cut, basis):
            m.close()


def test_a_basis_state_returns_its_own_bits():
    from aqc_research_amd.mps_engine import DeviceMPS

    n, k = 13, 0b1011001110001
    m = DeviceMPS.basis_state(n, k)
    try:
        for method in ("fused", "gemm"):
            got = m.sample(300, seed=SEED, method=method, details=True)
            assert np.all(ref.indices(got["bits"]) == k) and np.all(got["amplitudes"] == 1.0) and got["norm2"] == 1.0
            assert np.all(got["probabilities"] == 1.0)
            assert np.array_equal(m.amplitudes(got["bits"][:3] ^ np.uint8(1), method=method), np.zeros(3))
    finally:
        m.close()


def test_abi_refusals_and_a_correct_call_afterwards():
    from ctypes import POINTER, c_uint8, c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_sampling import amplitudes, sample

    L = _lib.lib()
    c, d, one, five = _device("C"), _device("D"), DeviceMPS.basis_state(1, 1), DeviceMPS.basis_state(5)
    try:
        n = 4
        bits = np.zeros((2, 8, n), dtype=np.uint8)
        amps = np.zeros((2, 8), dtype=np.complex128)
        u8 = lambda a: a.ctypes.data_as(POINTER(c_uint8))   # noqa: E731
        hs = (c_void_p * 2)(c.handle, c.handle)
        assert L.aqc_mps_sample((c_void_p * 2)(c.handle, None), 2, 8, 0, 1, 0, u8(bits), None, None) == 1
        assert L.aqc_mps_sample((c_void_p * 2)(c.handle, five.handle), 2, 8, 0, 1, 0, u8(bits), None, None) == 1 and b"differ" in L.aqc_last_error()
        assert L.aqc_mps_sample((c_void_p * 1)(d.handle), 1, 8, 0, 1, 1, u8(np.zeros((8, 13), np.uint8)), None, None) == 1 and b"fused" in L.aqc_last_error()
        bad = np.zeros((8, n), dtype=np.uint8)
        bad[5, 2] = 2
        assert L.aqc_mps_amplitudes(hs, 2, 8, u8(bad), 0, _lib.dptr(amps)) == 1 and b"bit string 5, qubit 2" in L.aqc_last_error()
        with pytest.raises(ValueError):
            amplitudes(c, np.zeros((3, 5), dtype=np.uint8))   # five bits for four qubits
        live = live_buffers()
        assert L.aqc_mps_sample(hs, 2, 8, 0, SEED, 0, u8(bits), _lib.dptr(amps), None) == 0
        assert np.array_equal(bits[0], _case("C")[1][:8])
        assert L.aqc_mps_amplitudes(hs, 2, 8, u8(bits[1]), 2, _lib.dptr(amps)) == 0
        assert float(np.max(np.abs(amps[0] - _dense("C")[ref.indices(bits[1])]))) <= TOL * ref.NORM
        assert live_buffers() == live
        got = sample(one, 5, seed=3, details=True)   # a one-qubit state is a legal MPS
        assert np.array_equal(got["bits"], np.ones((5, 1), dtype=np.uint8)) and np.all(got["amplitudes"] == 1.0)
        # a state of norm zero has no distribution: the call fails and names lane and shot
        gam, lam = _case("C")[0]
        dead = ([(0.0 * gam[0][0], 0.0 * gam[0][1])] + list(gam[1:]), lam)
        for method in ("fused", "gemm"):
            with pytest.raises(RuntimeError, match="lane 1, shot 40"):
                sample([_case("C")[0], dead], 3, seed=1, first_shot=40, method=method)
        assert live_buffers() == live
    finally:
        for m in (c, d, one, five):
            m.close()
