"""GPU: the truncated MPS arithmetic (trunc_thr > 0, max_bond > 0) of the single-lane engine and of the lockstep lanes against the
NumPy reference of the engine's stated rule (tests/mps_trunc_ref.py) -- not against Aer, whose truncation stays unpinned.

Only quantities that do not depend on the gauge are compared: every bond dimension (exactly), each bond's Schmidt values (sorted,
to 1e-12 of the largest), the discarded weight (1e-14 + 1e-9 d), the state (dense to TOL up to 16 qubits, else the overlaps
<ref|dev> and <dev|dev> by transfer matrices), objective values and gradients (1e-9).  Every case first asserts that the
reference met no decision within reach of rounding (mps_trunc_ref.check_margins), so a mismatch is a fault of the device code."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests import mps_trunc_ref as ref
from tests.helpers import TOL, canonical_mps, maxdiff

pytestmark = pytest.mark.gpu

ROUTES = ["single", "lockstep"]
GRAD_TOL = 1e-9
_SUMMARY: dict = {}   # route -> quantity -> largest difference met; "margins" -> smallest margin of each kind


def _note(route: str, key: str, value: float) -> None:
    d = _SUMMARY.setdefault(route, {})
    d[key] = max(d.get(key, 0.0), float(value))


def _margins(decisions, ties: bool = False) -> None:
    """Asserts the margins of the reference's decisions and keeps the smallest; ``ties``: a cap that cuts inside a degenerate
    cluster is expected (and its decision left out)."""
    if ties:
        decisions = [d for d in decisions if d.cap_margin is None or d.cap_margin >= ref.MIN_MARGIN]
    got = ref.check_margins(decisions)
    m = _SUMMARY.setdefault("margins", {})
    for k, v in got.items():
        m[k] = min(m.get(k, np.inf), v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for route, d in sorted(_SUMMARY.items()):
        print(f"\ntruncation parity [{route}]: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(d.items())))


@pytest.fixture(params=ROUTES)
def route(request, monkeypatch):
    monkeypatch.setenv("AQC_MPS_APPLY", request.param)
    return request.param


_LANES: dict = {}


def _lanes(n: int, lanes: int = 1):
    """One LockstepLanes per shape for the whole file."""
    from aqc_research_amd.mps_engine import LockstepLanes

    if (n, lanes) not in _LANES:
        _LANES[(n, lanes)] = LockstepLanes(n, lanes)
    return _LANES[(n, lanes)]


def _compare(route: str, dev, want: ref.RefMPS, state: bool = True) -> None:
    """Gauge-free comparison of a DeviceMPS with the reference."""
    got = ref.RefMPS.from_qiskit(dev.to_qiskit())
    assert list(dev.bond_dims) == list(want.bond_dims), f"bonds {list(dev.bond_dims)} != {list(want.bond_dims)}"
    _note(route, "bonds", 0)
    for q, (a, b) in enumerate(zip(got.lam, want.lam)):
        err = maxdiff(np.sort(a), np.sort(b))
        assert err <= 1e-12 * b.max(), f"Schmidt values of bond {q} differ by {err:.3g}"
        _note(route, "lambda/max", err / b.max())
    d = dev.discarded_weight
    assert abs(d - want.discarded) <= 1e-14 + 1e-9 * want.discarded, f"discarded {d!r} != {want.discarded!r}"
    _note(route, "discarded", abs(d - want.discarded))
    if not state:
        return
    if want.n <= 16:
        err = maxdiff(orc.mps_to_vector(dev.to_qiskit()), want.to_vector())
        assert err < TOL, f"state differs by {err:.3g}"
        _note(route, "state", err)
    else:
        rr = ref.dot(want, want)
        err = max(abs(ref.dot(want, got) - rr), abs(ref.dot(got, got) - rr))
        assert err < TOL, f"overlaps differ by {err:.3g}"
        _note(route, "overlap", err)


def _one_block(n: int, ent: str, c: int, t: int, angle: float = 0.0):
    """(circuit, thetas) whose only gate that is not the identity is the entangler on (c, t): how one 2-qubit gate runs on a lane."""
    from aqc_research_amd import ParametricCircuit

    circ = ParametricCircuit(n, ent, np.array([[c], [t]], dtype=np.int64))
    th = np.zeros(circ.num_thetas)
    if ent == "cp":
        th[-1] = angle
    return circ, th


def _gates_on_route(route, m_dev, n, pairs, thr, max_bond):
    """cx on every (ctrl, targ) of ``pairs``, truncating: gate by gate on a copy (single), or as a circuit of zero angles on a lane."""
    from aqc_research_amd import ParametricCircuit

    if route == "single":
        out = m_dev.clone()
        for c, t in pairs:
            out.gate2(ref.entangler("cx"), c, t, thr, max_bond)
        return out
    circ = ParametricCircuit(n, "cx", np.array(pairs, dtype=np.int64).T.copy())
    ls = _lanes(n)
    ls.set_targets(m_dev)
    ls.apply_circuit(circ, np.zeros((1, circ.num_thetas)), trunc_thr=thr, max_bond=max_bond)
    return ls.export(0)


def _gate_on_route(route, m_dev, n, ent, c, t, angle, thr, max_bond):
    if route == "single":
        return m_dev.clone().gate2(ref.entangler(ent, angle), c, t, thr, max_bond)
    circ, th = _one_block(n, ent, c, t, angle)
    ls = _lanes(n)
    ls.set_targets(m_dev)
    ls.apply_circuit(circ, th[None, :], trunc_thr=thr, max_bond=max_bond)
    return ls.export(0)


# ---- 1. one gate -----------------------------------------------------------------------------------------------------------

GATE_CASES = [   # (n, seed, ctrl, targ, entangler): both ends of the register (both Jacobi orientations), long range both ways
    (6, 11, 0, 1, "cx"), (7, 12, 1, 0, "cp"), (8, 13, 6, 7, "cz"), (8, 14, 7, 5, "cx"), (9, 15, 1, 6, "cp"), (10, 16, 8, 2, "cx"),
    (10, 17, 4, 5, "cz"),
]


@pytest.mark.parametrize("case", GATE_CASES, ids=[f"n{c[0]}-{c[2]}{c[3]}-{c[4]}" for c in GATE_CASES])
def test_one_gate_against_the_reference(route, case):
    """One truncated 2-qubit gate on a canonical state for thr in {1e-10, 1e-6, 1e-3, 0.5, 2.0} x max_bond in {0, 1, 2, 3, k - 1}."""
    from aqc_research_amd.mps_engine import DeviceMPS

    n, seed, c, t, ent = case
    rng = np.random.default_rng(seed)
    q_mps = canonical_mps(orc.rand_state(n, rng), 64)
    angle = float(rng.uniform(0.3, 2.8))
    m = DeviceMPS.from_qiskit(q_mps)
    exact = ref.RefMPS.from_qiskit(q_mps).gate2(ref.entangler(ent, angle), c, t)
    k = int(exact.bond_dims[min(c, t) + 1])
    for thr in (1e-10, 1e-6, 1e-3, 0.5, 2.0):
        for mb in sorted({0, 1, 2, 3, max(k - 1, 1)}):
            want = ref.RefMPS.from_qiskit(q_mps).gate2(ref.entangler(ent, angle), c, t, thr, mb)
            _margins(want.decisions)
            _compare(route, _gate_on_route(route, m, n, ent, c, t, angle, thr, mb), want)
    m.close()


def test_generic_two_qubit_unitary_against_the_reference():
    """A generic 4 x 4 unitary (single-lane engine: the lanes know only the ansatz entanglers), adjacent and long range."""
    from aqc_research_amd.mps_engine import DeviceMPS

    n = 8
    rng = np.random.default_rng(21)
    q_mps = canonical_mps(orc.rand_state(n, rng), 64)
    g4 = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]
    m = DeviceMPS.from_qiskit(q_mps)
    for c, t in ((3, 4), (0, 1), (7, 6), (6, 1), (2, 5)):
        for thr, mb in ((1e-6, 0), (1e-3, 3), (0.0, 2), (2.0, 0)):
            want = ref.RefMPS.from_qiskit(q_mps).gate2(g4, c, t, thr, mb)
            _margins(want.decisions)
            _compare("single", m.clone().gate2(g4, c, t, thr, mb), want)
    m.close()


# ---- 2. whole circuits -----------------------------------------------------------------------------------------------------

def _circuit(kind: str, n: int, rng, depth: int):
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz

    if kind == "trotter2":
        return TrotterAnsatz(n, orc.trotter_blocks(n, 1), second_order=True)
    blocks = np.stack([rng.permutation(n)[:2] for _ in range(depth)], axis=1).astype(np.int64)
    return ParametricCircuit(n, kind, blocks)


CIRCUIT_CASES = [("cx", 8, 31), ("cz", 9, 32), ("cp", 10, 33), ("trotter2", 8, 34)]


@pytest.mark.parametrize("kind,n,seed", CIRCUIT_CASES)
def test_whole_circuits_against_the_reference(route, kind, n, seed):
    """v_mul_mps / v_dagger_mul_mps with long-range blocks and a 2nd-order Trotter ansatz, thr x max_bond."""
    from aqc_research_amd import mps_engine as me

    rng = np.random.default_rng(seed)
    circ = _circuit(kind, n, rng, 14)
    th = orc.rand_thetas(circ.num_thetas, rng)
    q_mps = canonical_mps(orc.rand_state(n, rng), 4)
    m = me.DeviceMPS.from_qiskit(q_mps)
    for thr in (1e-10, 1e-6, 1e-3):
        for mb in (0, 4, 8):
            for inverse in (False, True):
                want = ref.apply_circuit(circ, th, ref.RefMPS.from_qiskit(q_mps), inverse, thr, mb)
                _margins(want.decisions)
                fn = me.v_dagger_mul_mps if inverse else me.v_mul_mps
                _compare(route, fn(circ, th, m, trunc_thr=thr, max_bond=mb, method=route), want)
    m.close()


def test_several_lanes_with_different_targets():
    """LockstepLanes.apply_circuit + export: three lanes, each with its own target and thetas."""
    from aqc_research_amd import mps_engine as me

    n, lanes = 9, 3
    rng = np.random.default_rng(41)
    circ = _circuit("cx", n, rng, 16)
    ths = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    q_mps = [canonical_mps(orc.rand_state(n, rng), 8) for _ in range(lanes)]
    devs = [me.DeviceMPS.from_qiskit(q) for q in q_mps]
    ls = _lanes(n, lanes).set_targets(devs)
    for thr, mb in ((1e-6, 0), (1e-3, 8), (1e-10, 4)):
        for inverse in (False, True):
            disc, bonds = ls.apply_circuit(circ, ths, inverse=inverse, trunc_thr=thr, max_bond=mb, details=True)
            for b in range(lanes):
                want = ref.apply_circuit(circ, ths[b], ref.RefMPS.from_qiskit(q_mps[b]), inverse, thr, mb)
                _margins(want.decisions)
                out = ls.export(b)
                _compare("lockstep", out, want)
                assert abs(disc[b] - want.discarded) <= 1e-14 + 1e-9 * want.discarded and bonds[b] == want.bond_dims.max()
                out.close()
    for d in devs:
        d.close()


# ---- 3. the gradient walk ----------------------------------------------------------------------------------------------------

GRAD_CASES = [("cx", 8, 51, None, True), ("cp", 9, 52, (3, 11), False), ("cz", 8, 53, (0, 7), True), ("trotter2", 8, 54, None, True)]


@pytest.mark.parametrize("kind,n,seed,br,front", GRAD_CASES)
def test_gradient_walk_against_the_reference(route, kind, n, seed, br, front):
    """fast_dot_gradient_mps (single, or one lockstep lane), LockstepLanes.evaluate and apply_vh(flips=True) + gradient, truncating."""
    from aqc_research_amd import mps_engine as me

    rng = np.random.default_rng(seed)
    circ = _circuit(kind, n, rng, 14)
    th = orc.rand_thetas(circ.num_thetas, rng)
    x_q = canonical_mps(orc.rand_state(n, rng), 2)
    y_q = canonical_mps(orc.rand_state(n, rng), 8)
    xm, ym = me.DeviceMPS.from_qiskit(x_q), me.DeviceMPS.from_qiskit(y_q)
    for thr, mb in ((1e-6, 0), (1e-3, 6), (1e-10, 4)):
        vh_ref = ref.apply_circuit(circ, th, ref.RefMPS.from_qiskit(y_q), True, thr, mb)
        g_ref, w, z = ref.fast_dot_gradient(circ, th, ref.RefMPS.from_qiskit(x_q), vh_ref, thr, mb, br, front)
        _margins(vh_ref.decisions + w.decisions + z.decisions)
        h_ref = ref.dot(ref.RefMPS.from_qiskit(x_q), vh_ref)
        # the walk from a given vh
        vh = me.v_dagger_mul_mps(circ, th, ym, trunc_thr=thr, max_bond=mb, method=route)
        _compare(route, vh, vh_ref)
        g = me.fast_dot_gradient_mps(circ, th, xm, vh, trunc_thr=thr, max_bond=mb, block_range=br, front_layer=front, method=route)
        assert maxdiff(g, g_ref) < GRAD_TOL
        _note(route, "gradient", maxdiff(g, g_ref))
        vh.close()
        if route != "lockstep":
            continue
        # the lanes' own evaluation: V^H, h and the walk in one call
        ls = _lanes(n).set_targets(ym).set_lhs(xm)
        h, gl, disc, bonds = ls.evaluate(circ, th[None, :], trunc_thr=thr, max_bond=mb, block_range=br, front_layer=front, details=True)
        assert abs(h[0] - h_ref) < GRAD_TOL and maxdiff(gl[0], g_ref) < GRAD_TOL
        assert abs(disc[0] - vh_ref.discarded) <= 1e-14 + 1e-9 * vh_ref.discarded and bonds[0] == vh_ref.bond_dims.max()
        _note(route, "h", abs(h[0] - h_ref))
        _note(route, "gradient", maxdiff(gl[0], g_ref))
        # the two phases: V^H with the flip amplitudes <X_q lhs|vh>, then the walk
        amps = ls.apply_vh(circ, th[None, :], trunc_thr=thr, max_bond=mb, flips=True)
        x_ref = ref.RefMPS.from_qiskit(x_q)
        want = [h_ref] + [ref.dot(x_ref, vh_ref, [(q, ref._X)]) for q in range(n)]
        assert maxdiff(amps[0], want) < GRAD_TOL
        _note(route, "amplitudes", maxdiff(amps[0], want))
        g2 = ls.gradient(circ, block_range=br, front_layer=front)
        assert maxdiff(g2[0], g_ref) < GRAD_TOL
    xm.close()
    ym.close()


# ---- 4. bond limits ----------------------------------------------------------------------------------------------------------

def test_lanes_at_their_bond_cap(route):
    """Bonds of exactly 32 (the lanes' kLaneCap: 64 columns, the whole LDS work matrix) on both routes."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    n = 10
    rng = np.random.default_rng(61)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", 54))
    th = orc.rand_thetas(circ.num_thetas, rng)
    zero = me.DeviceMPS.basis_state(n)
    for thr, mb in ((0.0, 0), (1e-13, 32), (1e-6, 31), (1e-10, 24)):
        want = ref.apply_circuit(circ, th, ref.RefMPS.basis_state(n), False, thr, mb)
        _margins(want.decisions)
        assert want.bond_dims.max() == (32 if mb in (0, 32) else mb) or thr >= 1e-6
        _compare(route, me.v_mul_mps(circ, th, zero, trunc_thr=thr, max_bond=mb, method=route), want)
    zero.close()


def test_single_lane_engine_at_bond_128():
    """n = 14 around the middle bond (128): the zgemm theta path (chi_m > 64) and the multi-launch Jacobi (2 chi > 64)."""
    from aqc_research_amd.mps_engine import DeviceMPS

    n = 14
    rng = np.random.default_rng(71)
    q_mps = canonical_mps(orc.rand_state(n, rng), 128)
    m = DeviceMPS.from_qiskit(q_mps)
    want = ref.RefMPS.from_qiskit(q_mps)
    g4 = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]
    for c, t, g in ((6, 7, g4), (7, 6, ref.entangler("cx")), (5, 8, ref.entangler("cp", 1.1)), (8, 7, g4)):
        want.gate2(g, c, t, 1e-10, 0)
        m.gate2(g, c, t, 1e-10, 0)
    _margins(want.decisions)
    assert want.bond_dims.max() == 128
    _compare("single", m, want)
    m.close()


# ---- 5. spectra where Jacobi gets hard -------------------------------------------------------------------------------------

def _bell_pairs(n):
    v = np.ones(1)
    for _ in range(n // 2):
        v = np.kron(np.array([1, 0, 0, 1]) / np.sqrt(2), v)
    return v.astype(complex)


def _graded(n, rng, values):
    """sum_j c_j |u_j>|v_j> across the middle cut, c graded down to next to the 1e-14 floor."""
    h = n // 2
    u = np.linalg.qr(rng.standard_normal((1 << h, 1 << h)) + 1j * rng.standard_normal((1 << h, 1 << h)))[0]
    w = np.linalg.qr(rng.standard_normal((1 << (n - h), 1 << (n - h))) + 1j * rng.standard_normal((1 << (n - h), 1 << (n - h))))[0]
    mat = sum(c * np.outer(w[:, j], u[:, j]) for j, c in enumerate(values))   # [high qubits][low qubits]
    return (mat / np.linalg.norm(mat)).reshape(-1)


SPECTRA = ["bell", "ghz", "basis", "graded"]


@pytest.mark.parametrize("spectrum", SPECTRA)
def test_hard_spectra_against_the_reference(route, spectrum):
    """Exactly degenerate Schmidt values kept whole (Bell pairs, GHZ), rank-1 two-site tensors (basis states), graded spectra that
    end next to the floor (T_q' = U S / lambda_{q-1} divides by them); a cap inside a degenerate cluster compares bonds, lambda
    and discarded weight only (the state is not unique there)."""
    from aqc_research_amd.mps_engine import DeviceMPS

    n = 8
    rng = np.random.default_rng(81)
    if spectrum == "bell":
        vec = _bell_pairs(n)
    elif spectrum == "ghz":
        vec = np.zeros(1 << n, complex)
        vec[0] = vec[-1] = 1 / np.sqrt(2)
    elif spectrum == "basis":
        vec = np.zeros(1 << n, complex)
        vec[0b10110010] = 1.0
    else:
        vec = _graded(n, rng, np.geomspace(1.0, 3e-13, 9))
    q_mps = canonical_mps(vec, 64)
    m = DeviceMPS.from_qiskit(q_mps)
    pairs = [(3, 4), (1, 2), (4, 6), (2, 1), (6, 3)]
    for thr, mb in ((0.0, 0), (1e-10, 0), (1e-3, 0), (0.0, 1), (1e-6, 2)):
        want = ref.RefMPS.from_qiskit(q_mps)
        for c, t in pairs:
            want.gate2(ref.entangler("cx"), c, t, thr, mb)
        if any(d.cap_margin is not None and d.cap_margin < ref.MIN_MARGIN for d in want.decisions):
            # a cap inside a degenerate cluster: one gate only, since the decisions after it depend on the gauge
            want = ref.RefMPS.from_qiskit(q_mps)
            want.gate2(ref.entangler("cx"), *pairs[0], thr, mb)
            _margins(want.decisions, ties=True)
            out = _gates_on_route(route, m, n, pairs[:1], thr, mb)
            _compare(route, out, want, state=False)
        else:
            _margins(want.decisions)
            out = _gates_on_route(route, m, n, pairs, thr, mb)
            _compare(route, out, want)
        out.close()
    m.close()


def test_the_floor_decides_at_a_graded_bond(route):
    """Schmidt values down to 1e-13 of the largest across the middle bond, split by an identity gate (cp at angle 0) that leaves
    the spectrum as it is: the rank floor alone decides that bond -- the 1e-13 value stays, the numerically zero ones go."""
    from aqc_research_amd.mps_engine import DeviceMPS

    n = 8
    rng = np.random.default_rng(82)
    q_mps = canonical_mps(_graded(n, rng, [1.0, 0.3, 1e-2, 1e-4, 1e-7, 1e-10, 1e-13]), 64)
    m = DeviceMPS.from_qiskit(q_mps)
    want = ref.RefMPS.from_qiskit(q_mps).gate2(ref.entangler("cp", 0.0), 3, 4)
    _margins(want.decisions)
    assert want.bond_dims[4] == 7
    _compare(route, _gate_on_route(route, m, n, "cp", 3, 4, 0.0, 0.0, 0), want)
    m.close()


# ---- 6. beyond dense reach ---------------------------------------------------------------------------------------------------

def test_32_qubit_trotter_walk_against_the_reference(route):
    """A 32-qubit 2nd-order Trotter circuit at thr = 1e-8 (bonds <= 32): V^H|target>, h and the gradient walk -- no dense vector
    exists anywhere; bonds, lambda, discarded weight, overlaps, h and gradient against the reference walk."""
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index

    n, thr = 32, 1e-8
    rng = np.random.default_rng(91)
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 1), second_order=True)
    th0 = init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=0.5, delta=1.0)
    th = th0 + 0.05 * orc.rand_thetas(circ.num_thetas, rng)
    neel = neel_state_index(n)
    basis = me.DeviceMPS.basis_state(n, neel)
    target_ref = ref.apply_circuit(circ, th0, ref.RefMPS.basis_state(n, neel), False, thr, 0)
    target = me.v_mul_mps(circ, th0, basis, trunc_thr=thr, method=route)
    _compare(route, target, target_ref)
    vh_ref = ref.apply_circuit(circ, th, target_ref.copy(), True, thr, 0)
    g_ref, w, z = ref.fast_dot_gradient(circ, th, ref.RefMPS.basis_state(n, neel), vh_ref, thr, 0)
    _margins(target_ref.decisions + vh_ref.decisions + w.decisions + z.decisions)
    assert vh_ref.bond_dims.max() <= 32 and vh_ref.discarded > 0
    h_ref = ref.dot(ref.RefMPS.basis_state(n, neel), vh_ref)
    vh = me.v_dagger_mul_mps(circ, th, target, trunc_thr=thr, method=route)
    _compare(route, vh, vh_ref)
    g = me.fast_dot_gradient_mps(circ, th, basis, vh, trunc_thr=thr, method=route)
    assert maxdiff(g, g_ref) < GRAD_TOL
    _note(route, "gradient", maxdiff(g, g_ref))
    if route == "lockstep":
        h, gl = _lanes(n).set_targets(target).set_lhs(basis).evaluate(circ, th[None, :], trunc_thr=thr)
        assert abs(h[0] - h_ref) < GRAD_TOL and maxdiff(gl[0], g_ref) < GRAD_TOL
        _note(route, "h", abs(h[0] - h_ref))
    for x in (vh, target, basis):
        x.close()


# ---- 7. canonicalisation on import -------------------------------------------------------------------------------------------

def test_import_canonicalises_like_the_reference(route):
    """from_qiskit(random_mps, trunc_thr=1e-6) canonicalises the non-canonical tensors (identity sweeps), then a truncated circuit."""
    from aqc_research_amd import mps_engine as me

    n = 9
    rng = np.random.default_rng(101)
    q_mps = orc.random_mps(n, 5, rng)
    assert not me.is_canonical(q_mps)
    m = me.DeviceMPS.from_qiskit(q_mps, trunc_thr=1e-6)
    want = ref.RefMPS.from_qiskit(q_mps).canonicalize()
    _margins(want.decisions)
    _compare("single", m, want)
    circ = _circuit("cz", n, rng, 12)
    th = orc.rand_thetas(circ.num_thetas, rng)
    for thr, mb in ((1e-6, 0), (1e-3, 6)):
        w = ref.apply_circuit(circ, th, want.copy(), True, thr, mb)
        _margins(w.decisions)
        _compare(route, me.v_dagger_mul_mps(circ, th, m, trunc_thr=thr, max_bond=mb, method=route), w)
    m.close()


# ---- 8. the front door at the reference's default threshold ------------------------------------------------------------------

def _times(q_mps, c: float):
    """c |q_mps> in canonical (Vidal) form: every Schmidt vector times c, the inner Gammas divided by c."""
    gam, lam = q_mps
    n = len(gam)
    gam = [(g0 / c, g1 / c) if 0 < q < n - 1 else (g0, g1) for q, (g0, g1) in enumerate(gam)]
    return gam, [c * v for v in lam]


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_front_door_on_the_engine_at_the_default_threshold(route, scale, monkeypatch):
    """mps_operations.v_dagger_mul_mps and mps_dot_objective.fast_dot_gradient with AQC_MPS_METHOD=mps at trunc_thr = 1e-6, also for an
    input of norm 2: the result's tensors describe a state of norm 2 (mps_dot(out, out) = 4)."""
    from aqc_research_amd import mps_dot_objective as mdo
    from aqc_research_amd import mps_operations as mo
    from aqc_research_amd.mps_engine import is_canonical

    monkeypatch.setenv("AQC_MPS_METHOD", "mps")
    n, thr = 10, 1e-6
    rng = np.random.default_rng(111)
    circ = _circuit("cx", n, rng, 16)
    th = orc.rand_thetas(circ.num_thetas, rng)
    q_mps = _times(canonical_mps(orc.rand_state(n, rng), 6), scale)
    x_q = canonical_mps(orc.rand_state(n, rng), 2)
    start = ref.RefMPS.from_qiskit(q_mps)
    if not is_canonical(q_mps):
        start.canonicalize()
    vh_ref = ref.apply_circuit(circ, th, start, True, thr, 0)
    out = mo.v_dagger_mul_mps(circ, th, q_mps, trunc_thr=thr)
    got = ref.RefMPS.from_qiskit(out)
    assert list(got.bond_dims) == list(vh_ref.bond_dims)
    assert maxdiff(orc.mps_to_vector(out), vh_ref.to_vector()) < TOL
    assert abs(mo.mps_dot(out, out) - scale ** 2) < 1e-9 and abs(ref.dot(vh_ref, vh_ref) - scale ** 2) < 1e-9
    _note(route, "state", maxdiff(orc.mps_to_vector(out), vh_ref.to_vector()))
    # the gradient on the tensors the front door handed out, imported (and canonicalised when they are not) as the engine does
    zr = ref.RefMPS.from_qiskit(out)
    if not is_canonical(out):
        zr.canonicalize()
    xr = ref.RefMPS.from_qiskit(x_q)
    if not is_canonical(x_q):
        xr.canonicalize()
    g_ref, w, z = ref.fast_dot_gradient(circ, th, xr, zr, thr, 0)
    _margins(vh_ref.decisions + zr.decisions + xr.decisions + w.decisions + z.decisions)
    g = mdo.fast_dot_gradient(circ, th, x_q, out, trunc_thr=thr)
    assert maxdiff(g, g_ref) < GRAD_TOL
    _note(route, "gradient", maxdiff(g, g_ref))


def test_front_door_dense_and_engine_agree_on_an_unnormalised_state(monkeypatch):
    """A norm-2 state through v_dagger_mul_mps(trunc_thr=1e-6) on the dense route (DenseBackedMPS, tensors by
    vector_to_canonical_mps) and on the engine: the same mps_dot(out, out) = 4 and the same dense vector."""
    from aqc_research_amd import mps_operations as mo

    n = 6
    rng = np.random.default_rng(121)
    circ = _circuit("cx", n, rng, 8)
    th = orc.rand_thetas(circ.num_thetas, rng)
    q_mps = _times(canonical_mps(orc.rand_state(n, rng), 8), 2.0)
    dense = orc.v_dagger_mul_vec(circ, th, orc.mps_to_vector(q_mps))
    outs = {}
    for method in ("dense", "mps"):
        monkeypatch.setenv("AQC_MPS_METHOD", method)
        out = mo.v_dagger_mul_mps(circ, th, q_mps, trunc_thr=1e-6)
        outs[method] = (mo.mps_dot(out, out), mo.mps_to_vector(out), orc.mps_dot(out, out))
    for method, (nn, vec, host_nn) in outs.items():
        assert abs(nn - 4.0) < 1e-9 and abs(host_nn - 4.0) < 1e-9, method
        assert maxdiff(vec, dense) < TOL, method
    assert maxdiff(outs["dense"][1], outs["mps"][1]) < TOL
