"""GPU: device-resident MPS engine (truncated 2-qubit gates by one-sided Jacobi SVD).  Exactness with
trunc_thr -> 0 against the dense oracle -- the level the reference's own MPS tests pin (test_mps.py:57-199,
test_mps_fast_dot_gradient.py:126-153) -- plus the truncation contract and a register beyond dense reach."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["single", "auto"])
def _apply_route(request, monkeypatch):
    """Every test of the engine runs twice: whole circuits (v_mul_mps / v_dagger_mul_mps) on the single-lane engine, and -- the default --
    layer by layer on one lockstep lane wherever bonds stay <= 32."""
    monkeypatch.setenv("AQC_MPS_APPLY", request.param)


@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (7, 3), (3, 7), (16, 16), (40, 64), (64, 40), (128, 128), (200, 72), (66, 300), (512, 512),
                                   (100, 513)])
def test_jacobi_svd(shape):
    """1..64: one workgroup in LDS; up to 512 rows: the persistent two-level kernel (also 72 = 9 blocks, an odd
    tournament, and 66 = a ragged last block); beyond: one launch per round."""
    from aqc_research_amd.mps_engine import svd

    rng = np.random.default_rng(sum(shape))
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if shape == (16, 16):
        a[:, 5] = a[:, 2] * (0.3 - 2j)        # rank deficient
        a[:, 9] = 0
    u, s, vh, sweeps = svd(a)
    k = min(shape)
    assert (sweeps > 0 or k == 1) and sweeps < 40 and np.all(np.diff(s) <= 1e-13)
    assert maxdiff(s, np.linalg.svd(a, compute_uv=False)) < 1e-11 * max(1.0, s[0])
    assert maxdiff((u * s) @ vh, a) < 1e-11 * max(1.0, s[0])
    good = s > 1e-12 * s[0]
    assert maxdiff(u[:, good].conj().T @ u[:, good], np.eye(int(good.sum()))) < 1e-11
    assert maxdiff(vh[good] @ vh[good].conj().T, np.eye(int(good.sum()))) < 1e-11


def test_blocked_jacobi_agrees_with_round_per_launch(monkeypatch):
    """The persistent two-level kernel and the plain one-launch-per-round tournament give the same decomposition."""
    from aqc_research_amd.mps_engine import svd

    rng = np.random.default_rng(9)
    a = rng.standard_normal((160, 96)) + 1j * rng.standard_normal((160, 96))
    u1, s1, vh1, _ = svd(a)
    monkeypatch.setenv("AQC_SVD_BLOCKED", "0")
    u0, s0, vh0, _ = svd(a)
    assert maxdiff(s0, s1) < 1e-12 * s0[0]
    assert maxdiff((u0 * s0) @ vh0, (u1 * s1) @ vh1) < 1e-11 * s0[0]


def _dense(mps):
    return orc.mps_to_vector(mps.to_qiskit())


def test_gates_exact_against_dense():
    from aqc_research_amd import gates
    from aqc_research_amd.mps_engine import DeviceMPS

    n, chi = 7, 4
    rng = np.random.default_rng(70)
    q_mps = orc.random_mps(n, chi, rng)
    ref = orc.mps_to_vector(q_mps)
    m = DeviceMPS.from_qiskit(q_mps)
    assert maxdiff(_dense(m), ref) < TOL                      # import / export round trip
    other = DeviceMPS.from_qiskit(orc.random_mps(n, 3, rng))
    assert abs(m.dot(other) - np.vdot(ref, _dense(other))) < TOL
    m.gate1(gates.ry_matrix(0.7), 3)
    orc.ry(ref, 1 << 3, 0.7)
    for c, t, ent in ((0, 1, "cx"), (2, 1, "cz"), (1, 5, "cp"), (6, 0, "cx"), (3, 4, "cp"), (5, 2, "cx")):
        g = gates.controlled({"cx": [[0, 1], [1, 0]], "cz": [[1, 0], [0, -1]], "cp": np.diag([1, np.exp(0.9j)])}[ent])
        m.gate2(g, c, t)
        orc._entangle(ref, 1 << c, 1 << t, ent, 0.9)
        assert maxdiff(_dense(m), ref) < TOL
    g4 = np.linalg.qr(rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4)))[0]   # generic 2-qubit unitary
    m.gate2(g4, 4, 1)
    v = ref.reshape([2] * n)                                   # axis n-1-q <-> qubit q
    v = np.moveaxis(v, (n - 1 - 4, n - 1 - 1), (0, 1)).reshape(4, -1)
    v = (g4 @ v).reshape([2, 2] + [2] * (n - 2))
    ref = np.moveaxis(v, (0, 1), (n - 1 - 4, n - 1 - 1)).reshape(-1)
    assert maxdiff(_dense(m), ref) < TOL
    assert m.discarded_weight < 1e-20
    c = m.clone()
    c.gate1(gates.rx_matrix(1.0), 0)
    assert maxdiff(_dense(m), ref) < TOL                      # clone is independent
    assert m.bond_dims.max() <= 2 ** (n // 2)


def test_dot_ops_with_generic_operators_against_dense():
    """<(prod G_i) a|b> with random complex 2x2 operators -- neither Hermitian nor unitary, so reading b through anything but G^H shows --
    on the first, a middle and the last site, then on two sites.  Bonds 4 against 3 at 5 qubits: the smallest shape at which all four bond
    dimensions of an inner site step differ."""
    from aqc_research_amd.mps_engine import DeviceMPS

    n = 5
    rng = np.random.default_rng(71)
    a, b = DeviceMPS.from_qiskit(orc.random_mps(n, 4, rng)), DeviceMPS.from_qiskit(orc.random_mps(n, 3, rng))
    va, vb = _dense(a), _dense(b)
    for qubits in ((0,), (2,), (4,), (1, 3)):
        ops = [(q, rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))) for q in qubits]
        ga = va.copy()
        for q, g in ops:
            orc.gate2x2(ga, 1 << q, g)
        assert abs(a.dot_ops(b, ops) - np.vdot(ga, vb)) < TOL, qubits


@pytest.mark.parametrize("kind", ["cx", "cz", "cp", "trotter2"])
def test_native_gradient_and_circuit_against_oracle(kind):
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz
    from aqc_research_amd import mps_engine as eng
    from aqc_research_amd.mps_engine import DeviceMPS, fast_dot_gradient_mps, v_dagger_mul_mps, v_mul_mps

    n = 6
    rng = np.random.default_rng(len(kind) * 13)
    if kind == "trotter2":
        a = orc.Ansatz(n, "cx", orc.trotter_blocks(n, 1), True, True)
        circ = TrotterAnsatz(n, a.blocks, second_order=True)
    else:
        blocks = np.stack([rng.permutation(n)[:2] for _ in range(9)], axis=1).astype(np.int64)
        a = orc.Ansatz(n, kind, blocks)
        circ = ParametricCircuit(n, kind, blocks)
    th = orc.rand_thetas(a.num_thetas, rng)
    x_q, y_q = orc.random_mps(n, 2, rng), orc.random_mps(n, 3, rng)
    x, y = orc.mps_to_vector(x_q), orc.mps_to_vector(y_q)
    xm, ym = DeviceMPS.from_qiskit(x_q), DeviceMPS.from_qiskit(y_q)
    assert maxdiff(_dense(v_mul_mps(circ, th, xm)), orc.v_mul_vec(a, th, x)) < 10 * TOL
    vhy = v_dagger_mul_mps(circ, th, ym)
    vhy_ref = orc.v_dagger_mul_vec(a, th, y)
    assert maxdiff(_dense(vhy), vhy_ref) < 10 * TOL
    g = fast_dot_gradient_mps(circ, th, xm, vhy)
    assert maxdiff(g, orc.grad_of_dot_product(a, th, x, vhy_ref)) < 100 * TOL
    br = (2, min(7, a.num_blocks))
    gp = fast_dot_gradient_mps(circ, th, xm, vhy, block_range=br, front_layer=False)
    assert maxdiff(gp, orc.grad_of_dot_product(a, th, x, vhy_ref, br, False)) < 100 * TOL
    # the C-side walk (one ABI call, cached environments) against the gate-per-call walk with full chains
    assert maxdiff(g, eng.fast_dot_gradient_mps_gatewise(circ, th, xm, vhy)) < TOL
    assert maxdiff(gp, eng.fast_dot_gradient_mps_gatewise(circ, th, xm, vhy, block_range=br, front_layer=False)) < TOL
    assert maxdiff(_dense(vhy), _dense(eng._apply_circuit_gatewise(circ, th, ym.clone(), True, 0.0, 0))) < TOL


@pytest.mark.parametrize("kind", ["cx", "cz", "cp", "trotter2"])
def test_gradient_walk_of_both_engines_against_the_gatewise_walk(kind):
    """The two executors of the one gradient-walk skeleton (csrc/aqc_mps_gradwalk.h) against the gate-per-call walk with full chains, on
    the smallest shapes with swap routing in both orientations ((0,3): control below, (4,1): control above), P11 records (cp), the
    Trotter decorations and a block range that leaves slots out.  What the walk does not record is exactly zero."""
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz
    from aqc_research_amd import mps_engine as eng
    from aqc_research_amd.mps_engine import DeviceMPS, fast_dot_gradient_mps, v_dagger_mul_mps

    n = 5
    rng = np.random.default_rng(500 + len(kind))
    if kind == "trotter2":
        a = orc.Ansatz(n, "cx", orc.trotter_blocks(n, 1), True, True)
        circ = TrotterAnsatz(n, a.blocks, second_order=True)
    else:
        blocks = np.array([[0, 4, 1, 2], [3, 1, 2, 4]], dtype=np.int64)
        a = orc.Ansatz(n, kind, blocks)
        circ = ParametricCircuit(n, kind, blocks)
    th = orc.rand_thetas(a.num_thetas, rng)
    xm = DeviceMPS.from_qiskit(orc.random_mps(n, 2, rng))
    vhy = v_dagger_mul_mps(circ, th, DeviceMPS.from_qiskit(orc.random_mps(n, 3, rng)))
    tpb = 5 if kind == "cp" else 4
    for kw in ({}, {"block_range": (1, 3), "front_layer": False}):
        ref = eng.fast_dot_gradient_mps_gatewise(circ, th, xm, vhy, **kw)
        unrecorded = np.zeros(a.num_thetas, dtype=bool)
        if kw:
            unrecorded[:3 * n] = True
            unrecorded[3 * n:3 * n + tpb] = True          # block 0
            unrecorded[3 * n + 3 * tpb:] = True          # blocks 3, 4, ...
        assert np.all(ref[~unrecorded] != 0) and np.all(ref[unrecorded] == 0)
        for method in ("single", "lockstep"):
            g = fast_dot_gradient_mps(circ, th, xm, vhy, trunc_thr=0, max_bond=0, method=method, **kw)
            assert maxdiff(g, ref) < TOL, (method, kw)
            assert np.all(g[unrecorded] == 0), (method, kw)


def test_truncation_contract_and_large_register():
    """trunc_thr > 0: bonds shrink, the norm is kept, the error is of the order of the discarded weight;
    and a 40-qubit register (2^40 amplitudes dense) runs with small bonds."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure
    from aqc_research_amd.mps_engine import DeviceMPS, fast_dot_gradient_mps, v_dagger_mul_mps, v_mul_mps

    n = 10
    rng = np.random.default_rng(3)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", 54))
    th = orc.rand_thetas(circ.num_thetas, rng)
    zero = DeviceMPS.basis_state(n)
    exact = v_mul_mps(circ, th, zero)
    cut = v_mul_mps(circ, th, zero, trunc_thr=1e-4)
    assert exact.bond_dims.max() == 32 and cut.bond_dims.max() < 32
    disc = cut.discarded_weight
    assert 0 < disc < 1e-2 and abs(cut.dot(cut) - 1) < 10 * disc
    assert 1 - abs(exact.dot(cut)) ** 2 < 10 * disc
    capped = v_mul_mps(circ, th, zero, max_bond=8)
    assert capped.bond_dims.max() == 8
    a = orc.as_ansatz(circ)
    assert maxdiff(_dense(exact), orc.v_mul_vec(a, th, np.eye(1 << n, 1, dtype=complex).ravel())) < 10 * TOL

    n = 40
    circ = ParametricCircuit(n, "cz", create_ansatz_structure(n, "spin", "full", n - 1))   # one brickwork layer
    th = 0.5 * orc.rand_thetas(circ.num_thetas, rng)
    zero = DeviceMPS.basis_state(n)
    target = v_mul_mps(circ, th + 0.05, zero, trunc_thr=1e-14)
    vh = v_dagger_mul_mps(circ, th, target, trunc_thr=1e-14)
    assert abs(vh.dot(vh) - 1) < 1e-9 and vh.bond_dims.max() <= 16
    g = fast_dot_gradient_mps(circ, th, zero, vh, trunc_thr=1e-14)
    for t in (1, 3 * n + 6, circ.num_thetas - 2):           # <V 0|target> against central differences
        e = np.zeros_like(th); e[t] = 1e-5
        f = [v_mul_mps(circ, th + s * e, zero, trunc_thr=1e-14).dot(target) for s in (+1, -1)]
        assert abs((f[0] - f[1]) / 2e-5 - g[t]) < 1e-7


def test_bond_256_at_16_qubits_matches_the_dense_route():
    """Config 3 at its largest bond (n = 16, 40 blocks, chi <= 256, trunc_thr = 1e-16): V^H|phi> and the
    gate-by-gate gradient on the engine equal the dense route to 1e-10.  2 chi = 512 > 64 columns takes the
    multi-launch Jacobi path.  The target is a canonical MPS, as Aer produces them; the discard rule is stated in the
    canonical gauge (sum of squared Schmidt values), so a non-canonical input (oracle random_mps) is outside the
    contract -- and Aer's own truncation arithmetic at trunc_thr = 1e-6 stays parity-unpinned."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure
    from aqc_research_amd.mps_engine import DeviceMPS, fast_dot_gradient_mps, v_dagger_mul_mps
    from oracle import aqc_ref as cref
    from tests.helpers import canonical_mps

    n = 16
    rng = np.random.default_rng(1)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", 40))
    th = orc.rand_thetas(circ.num_thetas, rng)
    raw = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    phi = canonical_mps(raw / np.linalg.norm(raw), 256)
    assert max(l.size for l in phi[1]) == 256
    dense = orc.mps_to_vector(phi)
    vh = v_dagger_mul_mps(circ, th, DeviceMPS.from_qiskit(phi), trunc_thr=1e-16)
    assert vh.bond_dims.max() == 256
    ref = cref.v_dagger_mul_vec(circ, th, dense)
    assert maxdiff(_dense(vh), ref) < TOL
    g = fast_dot_gradient_mps(circ, th, DeviceMPS.basis_state(n, 0), vh, trunc_thr=1e-16)
    x = np.zeros(1 << n, complex)
    x[0] = 1
    assert maxdiff(g, cref.grad_of_dot_product(circ, th, x, ref)) < TOL


def test_whole_circuit_calls_fail_loudly_on_bad_input():
    """aqc_mps_apply_circuit / aqc_mps_fast_dot_gradient validate the circuit description, the block range and the operands."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure
    from aqc_research_amd.mps_engine import DeviceMPS, fast_dot_gradient_mps, v_mul_mps

    circ = ParametricCircuit(5, "cx", create_ansatz_structure(5, "spin", "full", 6))
    th = np.zeros(circ.num_thetas)
    with pytest.raises(Exception, match="qubits"):
        v_mul_mps(circ, th, DeviceMPS.basis_state(6))
    with pytest.raises(ValueError, match="thetas"):
        v_mul_mps(circ, th[:-1], DeviceMPS.basis_state(5))
    with pytest.raises(Exception, match="size|qubits"):
        fast_dot_gradient_mps(circ, th, DeviceMPS.basis_state(5), DeviceMPS.basis_state(6))
    with pytest.raises(ValueError, match="block range"):
        fast_dot_gradient_mps(circ, th, DeviceMPS.basis_state(5), DeviceMPS.basis_state(5), block_range=(4, 9))
    # identity circuit (all angles zero, cx blocks): <V 0|0> = 1, and the operands are left intact
    a, b = DeviceMPS.basis_state(5), DeviceMPS.basis_state(5)
    g = fast_dot_gradient_mps(circ, th, a, b)
    assert g.shape == (circ.num_thetas,) and abs(a.dot(b) - 1) < 1e-14 and a.bond_dims.max() == 1


def test_reference_signature_functions_route_to_the_engine(monkeypatch):
    """fast_dot_gradient / v_dagger_mul_mps / cx_mul_mps with the reference signatures: the native engine
    (forced here on a small register) gives what the dense route gives."""
    from aqc_research_amd import TrotterAnsatz, mps_dot_objective as mdo, mps_operations as mpsop

    n = 6
    rng = np.random.default_rng(8)
    circ = TrotterAnsatz(n, orc.trotter_blocks(n, 1), second_order=False)
    th = orc.rand_thetas(circ.num_thetas, rng)
    x_q, y_q = orc.random_mps(n, 2, rng), orc.random_mps(n, 3, rng)
    res = {}
    for method in ("dense", "mps"):
        monkeypatch.setenv("AQC_MPS_METHOD", method)
        vh = mpsop.v_dagger_mul_mps(circ, th, y_q)
        res[method] = (orc.mps_to_vector(vh), mdo.fast_dot_gradient(circ, th, x_q, vh, block_range=(1, 9), front_layer=True))
    assert maxdiff(res["dense"][0], res["mps"][0]) < 10 * TOL and maxdiff(res["dense"][1], res["mps"][1]) < 100 * TOL
    a = orc.as_ansatz(circ)
    ref = orc.grad_of_dot_product(a, th, orc.mps_to_vector(x_q), orc.v_dagger_mul_vec(a, th, orc.mps_to_vector(y_q)), (1, 9), True)
    assert maxdiff(res["mps"][1], ref) < 100 * TOL
    out = mdo.cx_mul_mps(0.0, 4, 1, x_q, trunc_thr=1e-16)
    v = orc.mps_to_vector(x_q)
    orc.cx(v, 1 << 4, 1 << 1)
    assert maxdiff(orc.mps_to_vector(out), v) < TOL


def test_mps_objective_native_mode_matches_dense_mode(monkeypatch):
    """SpSurrogateObjectiveFastMpsTrotter on the MPS engine (what registers beyond ~24 qubits use) against the same
    objective on densified states, through an identical call sequence; then a 30-qubit smoke run."""
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter
    from aqc_research_amd.mps_engine import DeviceMPS, v_mul_mps

    n = 6
    rng = np.random.default_rng(21)
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 2), second_order=True)
    th = 0.6 * orc.rand_thetas(circ.num_thetas, rng)
    target = orc.random_mps(n, 4, rng)
    nrm = np.sqrt(abs(orc.mps_dot(target, target)))
    target = ([(g0 / nrm ** (1 / n), g1 / nrm ** (1 / n)) for g0, g1 in target[0]], target[1])
    seq = {}
    for method in ("dense", "mps"):
        monkeypatch.setenv("AQC_MPS_METHOD", method)
        user = dict(num_qubits=n, max_flips=1, enable_optim_stats=False, verbose=0, maxiter=5, trunc_thr=1e-16)
        o = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
        o.set_target(target)
        assert o._native_mps == (method == "mps")
        f0 = o.objective(th); g0 = o.gradient(th); f1 = o.objective(th + 0.02); g1 = o.gradient(th + 0.02)
        seq[method] = (f0, g0, f1, g1)
        assert bool(getattr(o, "_lk_live", False)) == (method == "mps")   # the engine route runs on two lockstep lanes
    for a, b in zip(seq["dense"], seq["mps"]):
        assert maxdiff(np.atleast_1d(a), np.atleast_1d(b)) < 1e-8
    # a register whose V^H|target> outgrows the lanes' bond (12 qubits, exact arithmetic, generic angles: bonds up to 64): the objective
    # notices on the first evaluation and stays on the single-lane engine
    n2 = 12
    circ2 = TrotterAnsatz(n2, make_trotter_like_circuit(n2, 4), second_order=True)
    th2 = orc.rand_thetas(circ2.num_thetas, rng)
    tgt2 = orc.random_mps(n2, 16, rng)
    seq2 = {}
    for method in ("dense", "mps"):
        monkeypatch.setenv("AQC_MPS_METHOD", method)
        user = dict(num_qubits=n2, max_flips=1, enable_optim_stats=False, verbose=0, maxiter=5, trunc_thr=1e-16)
        o = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ2)
        o.set_target(tgt2)
        seq2[method] = (o.objective(th2), o.gradient(th2))
        if method == "mps":
            assert o._native_mps and not o._lk_live and o._lk_refused
    nrm2 = abs(orc.mps_dot(tgt2, tgt2))
    for a, b in zip(seq2["dense"], seq2["mps"]):
        assert maxdiff(np.atleast_1d(a), np.atleast_1d(b)) < 1e-8 * max(1.0, nrm2)

    monkeypatch.setenv("AQC_MPS_METHOD", "auto")
    n = 30
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 1), second_order=False)
    th = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    tgt = v_mul_mps(circ, th + 0.02, DeviceMPS.basis_state(n), trunc_thr=1e-12).to_qiskit()
    user = dict(num_qubits=n, max_flips=1, enable_optim_stats=False, verbose=0, maxiter=5, trunc_thr=1e-12)
    o = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
    o.set_target(tgt)
    assert o._native_mps
    f = o.objective(th)
    g = o.gradient(th)
    assert 0.0 <= f < 0.5 and g.shape == (circ.num_thetas,) and np.isfinite(g).all() and np.linalg.norm(g) > 1e-3
    e = np.zeros_like(th); e[7] = 1e-5              # weight = 1, max_no = 0 at the start: f = 1 - |h0|^2
    o2 = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ); o2.set_target(tgt)
    fd = (o2.objective(th + e) - o2.objective(th - e)) / 2e-5
    assert abs(fd - g[7]) < 1e-5


def test_lbfgs_on_the_native_mps_objective_32_qubits():
    """A short L-BFGS run on a 32-qubit register (no dense state anywhere): the surrogate objective must go down
    from its perturbed start towards the planted optimum."""
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter
    from aqc_research_amd.mps_engine import DeviceMPS, v_mul_mps
    from aqc_research_amd.optimizer import AqcOptimizer

    n = 32
    rng = np.random.default_rng(32)
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 1), second_order=False)
    th_true = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    target = v_mul_mps(circ, th_true, DeviceMPS.basis_state(n), trunc_thr=1e-12).to_qiskit()
    user = dict(num_qubits=n, max_flips=1, enable_optim_stats=False, verbose=0, maxiter=6, trunc_thr=1e-12)
    objv = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
    objv.set_target(target)
    th0 = th_true + 0.03 * rng.standard_normal(th_true.size)
    f0 = objv.objective(th0)
    res = AqcOptimizer(optimizer_name="lbfgs", maxiter=6).optimize(objv, circ, th0)
    assert objv._native_mps and objv._lk_live and f0 > 1e-3
    assert res["cost"] < 0.2 * f0 and res["fidelity"] > 1 - 0.2 * f0


def test_100_qubit_register_with_neel_reference_state():
    """The reference advertises "up to 100 qubits" for its MPS route: objective + full gradient on 100 qubits from
    the Neel state (basis indices are Python integers there), checked against a central difference."""
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_fast_mps_trotter import SpSurrogateObjectiveFastMpsTrotter
    from aqc_research_amd.model_sp_lhs.trotter import neel_state_index
    from aqc_research_amd.mps_engine import DeviceMPS, v_mul_mps

    n = 100
    rng = np.random.default_rng(100)
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 1), second_order=False)
    neel = neel_state_index(n)
    th = 0.2 * orc.rand_thetas(circ.num_thetas, rng)
    target = v_mul_mps(circ, th + 0.01 * rng.standard_normal(th.size), DeviceMPS.basis_state(n, neel), trunc_thr=1e-12).to_qiskit()
    user = dict(num_qubits=n, max_flips=1, state_prep_func=lambda _n: neel, enable_optim_stats=False, verbose=0, maxiter=3, trunc_thr=1e-12)
    objv = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
    objv.set_target(target)
    assert objv._native_mps and objv.num_states == n + 1
    f = objv.objective(th)
    g = objv.gradient(th)
    assert 0 < f < 0.2 and g.shape == (circ.num_thetas,) and np.isfinite(g).all()
    t = 3 * n + 41
    e = np.zeros_like(th); e[t] = 1e-5
    probe = SpSurrogateObjectiveFastMpsTrotter(user_parameters=user, circ=circ)
    probe.set_target(target)
    assert abs((probe.objective(th + e) - probe.objective(th - e)) / 2e-5 - g[t]) < 1e-5
