"""GPU: dense vectors into MPS states on the device (mps_engine.from_vectors, aqc_mps_from_vec; kernels csrc/aqc_mps_fromvec.hip) on both
routes, against the dense vector itself, the NumPy statement (tests/mps_fromvec_ref.py) and the host rule
(mps_operations.vector_to_canonical_mps).

Bounds: TOL x |psi| at trunc_thr = 0; with truncation TOL x |psi| / gap against the statement (the bound of tests/test_hip_mps_compress.py:
two SVDs of the same matrix that differ by rounding agree on the kept subspace to rounding / gap), the gap read from the reference's
decisions and held to >= MIN_GAP in tests/test_mps_fromvec_ref.py, where the threshold and the cap are chosen.  Bonds must be equal,
weights agree within TOL x |psi|^2.  The tests print what they observe; DESIGN.md 6y records it."""
import functools

import numpy as np
import pytest

from tests import mps_layers_ref, mps_obs_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes
from tests.test_mps_compress_ref import MIN_GAP, normalised
from tests.test_mps_fromvec_ref import basis, random_state, trotter_state, truncation

pytestmark = pytest.mark.gpu


def _vec(state):
    return mps_obs_ref.dense(state.to_qiskit())


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


def _close(states):
    for m in states:
        if m is not None:
            m.close()


@functools.lru_cache(maxsize=None)
def _wide_state(n):
    """The dense vector of a seeded hand-made MPS with bonds [1, 2, 4, 8, 16, 32, 32, ..., 32, 16, 8, 4, 2, 1], read-only."""
    dims = [min(2 ** q, 2 ** (n - q), 32) for q in range(n + 1)]
    psi = mps_obs_ref.dense(mps_obs_ref.hand_made(dims, 1500 + n, norm=1.5))
    psi.setflags(write=False)
    return dims, psi


@pytest.mark.parametrize("n", (2, 3))
def test_smallest_registers(n):
    from aqc_research_amd.mps_engine import DeviceMPS, from_vector_route

    psi = random_state(n, 30 + n, 1.7)
    keep = psi.copy()
    assert from_vector_route(n) == "fused"
    out, info = DeviceMPS.from_vector(psi, method="fused", details=True)
    try:
        err = float(np.linalg.norm(_vec(out) - psi))
        print(f"n = {n}: |dense(out) - psi| = {err:.3g} (|psi| = 1.7), bonds {info['bonds'].tolist()}, sweeps {info['sweeps'].tolist()}, parts {info['parts'].tolist()}")
        assert info["route"] == "fused" and info["status"] == 0 and info["failed_at"] == -1
        assert info["bonds"].tolist() == out.bond_dims.tolist() == [1] + [2] * (n - 1) + [1]
        assert info["parts"].tolist() == [1] * (n - 1)
        assert err <= TOL * 1.7 and abs(out.discarded_weight) <= TOL * 1.7 ** 2
        assert np.array_equal(psi, keep)
    finally:
        out.close()


@pytest.mark.parametrize("index", (0, 0b10110))
def test_basis_states_have_bonds_of_one(index):
    """Every cut is exactly rank-deficient: the 1e-14 floor sees it, which the squared route would not."""
    from aqc_research_amd.mps_engine import from_vectors

    psi = 2.0j * basis(5, index)
    out, info = from_vectors(psi, method="fused", details=True)
    try:
        assert info["bonds"].tolist() == [1] * 6 and info["status"] == 0
        assert np.max(np.abs(_vec(out) - psi)) <= TOL * 2.0 and np.all(np.abs(info["dropped"]) <= TOL * 4.0)
    finally:
        out.close()


def test_full_width_without_truncation():
    from aqc_research_amd.mps_engine import from_vectors, is_canonical

    n, norm = 11, 2.5
    psi = random_state(n, 411, norm)
    out, info = from_vectors(psi, details=True)
    try:
        natural = [min(2 ** q, 2 ** (n - q)) for q in range(n + 1)]
        err = float(np.linalg.norm(_vec(out) - psi))
        lam = out.to_qiskit()[1]
        lam_err = max(float(np.max(np.abs(lam[q - 1] - np.linalg.svd(psi.reshape(2 ** (n - q), 2 ** q), compute_uv=False)))) for q in range(1, n))
        print(f"n = {n}, random, no cap: |dense(out) - psi| = {err:.3g}, max |bond vector - dense SVD| = {lam_err:.3g} (|psi| = {norm}), "
              f"discarded {out.discarded_weight:.3g}, sweeps {info['sweeps'].tolist()}, parts {info['parts'].tolist()}")
        assert info["route"] == "fused" and info["status"] == 0
        assert out.bond_dims.tolist() == info["bonds"].tolist() == natural and max(natural) == 32
        assert err <= TOL * norm and lam_err <= TOL * norm
        assert is_canonical(normalised(out.to_qiskit(), norm))
        assert abs(out.discarded_weight) <= TOL * norm ** 2 and np.all(np.abs(info["dropped"]) <= TOL * norm ** 2)
    finally:
        out.close()


def test_several_partial_factors_at_64_columns():
    """n = 15 is the smallest register with more than one partial factor at a site of 64 columns (site 5: 512 rows, two parts of four
    blocks); at n = 14 that site has 256 rows, four blocks, one part."""
    from aqc_research_amd.mps_engine import from_vectors

    dims14, psi14 = _wide_state(14)
    out14, info14 = from_vectors(psi14, 0.0, 32, method="fused", details=True)
    _close([out14])
    assert not any(p > 1 and b == 32 for p, b in zip(info14["parts"], info14["bonds"][:-2]))
    n = 15
    dims, psi = _wide_state(n)
    norm = float(np.linalg.norm(psi))
    out, info = from_vectors(psi, 0.0, 32, method="fused", details=True)
    try:
        err = float(np.linalg.norm(_vec(out) - psi))
        print(f"n = {n}, hand-made bonds up to 32: |dense(out) - psi| = {err:.3g} (|psi| = {norm:.3g}), parts {info['parts'].tolist()}, "
              f"sweeps {info['sweeps'].tolist()}, discarded {out.discarded_weight:.3g}")
        assert info["status"] == 0
        assert any(p > 1 and b == 32 for p, b in zip(info["parts"], info["bonds"][:-2]))      # site q has 2 bonds[q] columns
        assert info["bonds"].tolist() == dims                                                   # the exact ranks
        assert err <= TOL * norm and abs(out.discarded_weight) <= TOL * norm ** 2
    finally:
        out.close()


@pytest.mark.parametrize("as_cap", (False, True), ids=("trunc_thr", "max_bond"))
def test_truncation_matches_the_statement_on_both_routes(as_cap):
    from aqc_research_amd.mps_engine import from_vectors

    psi = trotter_state()
    norm = float(np.linalg.norm(psi))
    thr, cap, ref, gap = truncation(as_cap)
    assert gap >= MIN_GAP
    bound = TOL * norm / gap
    want = ref.to_vector()
    want_dropped = np.array([d.total - d.kept for d in ref.decisions])
    made = {}
    try:
        for method in ("fused", "host"):
            out, info = from_vectors(psi, thr, cap, method=method, details=True)
            made[method] = out
            err = float(np.linalg.norm(_vec(out) - want))
            werr = float(np.max(np.abs(info["dropped"] - want_dropped)))
            print(f"Trotter n = 12, trunc_thr {thr:g}, max_bond {cap}, {method}: bonds -> {out.bond_dims.tolist()}, |out - statement| = {err:.3g} "
                  f"(bound {bound:.3g}), max |dropped - statement| = {werr:.3g}, sweeps {info['sweeps'].tolist()}")
            assert info["route"] == method and info["status"] == 0
            assert out.bond_dims.tolist() == info["bonds"].tolist() == ref.bond_dims.tolist()
            assert err <= bound
            assert werr <= TOL * norm ** 2 and abs(float(info["dropped"].sum()) - ref.discarded) <= TOL * norm ** 2
            for a, b in zip(out.to_qiskit()[1], ref.lam):
                assert np.max(np.abs(a - b)) <= bound
        assert abs(made["fused"].discarded_weight - ref.discarded) <= TOL * norm ** 2
        routes = float(np.linalg.norm(_vec(made["fused"]) - _vec(made["host"])))
        print(f"    |fused - host| = {routes:.3g}")
        assert routes <= bound
    finally:
        _close(made.values())


def test_chunks_give_the_bits_of_one_chunk():
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import from_vectors

    n = 8
    vecs = np.stack([random_state(n, 700 + l, 1.0 + l) for l in range(5)])
    whole, info = from_vectors(vecs, 1e-3, 6, method="fused", details=True)
    L = _lib.lib()
    L.aqc_mps_from_vec_budget(2 * 2 * 16 * 2 ** n)        # two lanes per chunk: 2 + 2 + 1
    try:
        chunked, info2 = from_vectors(vecs, 1e-3, 6, method="fused", details=True)
        L.aqc_mps_from_vec_budget(16 * 2 ** n)             # not even one lane: an error that names the size
        with pytest.raises(RuntimeError, match=str(2 * 16 * 2 ** n)):
            from_vectors(vecs, 1e-3, 6, method="fused")
    finally:
        L.aqc_mps_from_vec_budget(0)
    try:
        for key in ("bonds", "dropped", "sweeps", "status"):
            assert np.array_equal(info[key], info2[key]), key
        for a, b in zip(whole, chunked):
            assert np.array_equal(_flat(a.to_qiskit()), _flat(b.to_qiskit()))
        assert np.any(info["bonds"] < np.array([min(2 ** q, 2 ** (n - q)) for q in range(n + 1)]))
    finally:
        _close(list(whole) + list(chunked))


def test_lanes_hold_the_lane_contract():
    """Nine vectors of 8 qubits, probes (0, 4, 8).  N: every other lane is NaN, gets status 2 and no state; the probes' bits do not move."""
    from aqc_research_amd.mps_engine import from_vectors

    n, lanes, width = 8, 9, 16
    vecs = np.stack([random_state(n, 800 + l, 1.0 + 0.5 * l) for l in range(lanes)])
    other = np.stack([random_state(n, 850 + l, 2.0) for l in range(lanes)])
    keep = vecs.copy()
    seen = []

    def run(arr):
        before = arr.copy()
        states, info = from_vectors(arr, 1e-3, 6, details=True)
        assert np.array_equal(arr, before, equal_nan=True)          # the inputs stay bit for bit
        lam = np.full((lanes, n - 1, width), np.nan)
        dense = np.full((lanes, 2 ** n), np.nan, dtype=np.complex128)
        for l, m in enumerate(states):
            if m is None:
                continue
            lam[l] = 0.0
            for q, v in enumerate(m.to_qiskit()[1]):
                lam[l, q, :v.size] = v
            dense[l] = _vec(m)
            m.close()
        seen.append((info["status"].copy(), [m is None for m in states]))
        return {"lam": lam, "dense": dense, "bonds": info["bonds"], "dropped": info["dropped"]}

    base = check_lanes(run, vecs, checks="RPFN", other=other)
    assert np.all(base["bonds"][:, 1:-1] >= 1) and np.any(base["bonds"] == 6)
    status, missing = seen[-1]                                      # the N call: the last one
    assert status.tolist() == [0, 2, 2, 2, 0, 2, 2, 2, 0] and missing == [s != 0 for s in status]
    assert np.array_equal(vecs, keep)
    mixed = vecs.copy()
    mixed[3] = 0.0                                                  # a zero vector fails alone
    states, info = from_vectors(mixed, 1e-3, 6, details=True)
    try:
        assert info["status"].tolist() == [0, 0, 0, 2, 0, 0, 0, 0, 0] and states[3] is None and info["failed_at"][3] == 0
        assert info["bonds"][3].tolist() == [1] + [0] * n
        for l in (0, 8):
            assert np.array_equal(_vec(states[l]), base["dense"][l])
        with pytest.raises(RuntimeError, match="lane 3, site 0"):
            from_vectors(mixed, 1e-3, 6)
    finally:
        _close(states)


def test_converted_states_serve_the_other_calls():
    """The gauge is the engine's: Pauli strings and samples of a converted state, and its overlap with the host rule's state."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_operations import vector_to_canonical_mps

    n, norm = 9, 1.3
    v = random_state(n, 950, norm)
    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
    Z = np.diag([1.0, -1.0]).astype(np.complex128)
    strings = ["ZIIIIIIII", "XXIIIIIII", "IYIZIIIXI", "ZZZZZZZZZ", "IIIIIIIII"]
    want = []
    for s in strings:
        w = v
        for q, ch in enumerate(s):
            if ch != "I":
                w = mps_layers_ref.dense_gate1(w, n, {"X": X, "Y": Y, "Z": Z}[ch], q)
        want.append(np.vdot(v, w))
    m = DeviceMPS.from_vector(v, method="fused")
    host = DeviceMPS.from_qiskit(vector_to_canonical_mps(v, 0.0), assume_canonical=True)
    try:
        got = m.pauli_strings(strings)
        perr = float(np.max(np.abs(got - np.array(want))))
        shots = m.sample(64, seed=5, details=True)
        index = (shots["bits"].astype(np.int64) << np.arange(n)).sum(axis=1)
        aerr = float(np.max(np.abs(shots["amplitudes"] - v[index])))
        dot = m.dot(host)
        print(f"n = {n}: max |<P> - dense| = {perr:.3g}, max |sampled amplitude - psi| = {aerr:.3g}, |<from_vector|host rule> - |v|^2| = {abs(dot - norm ** 2):.3g}")
        assert perr <= TOL * norm ** 2 and aerr <= TOL * norm and abs(shots["norm2"] - norm ** 2) <= TOL * norm ** 2
        assert abs(dot - norm ** 2) <= TOL * norm ** 2
    finally:
        m.close()
        host.close()


def test_fused_beyond_the_route_is_refused():
    from aqc_research_amd.mps_engine import from_vector_route, from_vectors

    v = basis(12, 5)
    assert from_vector_route(12) == "host"
    with pytest.raises(ValueError):
        from_vectors(v, method="fused")
    out, info = from_vectors(v, details=True)           # the rule's own choice: the host route
    try:
        assert info["route"] == "host" and out.bond_dims.tolist() == [1] * 13
    finally:
        out.close()
