"""GPU: gate layers on MPS states (mps_engine.apply_gates / v_mul_mps_many, aqc_mps_apply_gates; kernels csrc/aqc_mps_layers.hip) on both
routes, against the dense vector, the NumPy statement (tests/mps_layers_ref.py) and the engine's own gate1 / gate2 / v_mul_mps loop.

Bounds: TOL x |psi| at trunc_thr = 0; with truncation TOL x |psi| x s_max / gap against the statement (Wedin's bound on the kept
subspace), the gap read from the reference's decisions and held to >= 1e-3 there (tests/test_mps_layers_ref.py, where the thresholds
and caps are chosen too).  Ranks must be equal, weights agree within TOL.  The tests print what they observe; DESIGN.md 6x records it."""
import functools

import numpy as np
import pytest

from tests import mps_layers_ref, mps_obs_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes
from tests.test_mps_layers_ref import MIN_GAP, TROTTER_N, TRUNCATED, program, trotter, trotter_case, truncation, unitary

pytestmark = pytest.mark.gpu

ROUTES = ("fused", "gatewise")


def _flat(qiskit_mps):
    gam, lam = qiskit_mps
    return np.concatenate([np.concatenate([g0.ravel(), g1.ravel()]) for g0, g1 in gam] + [np.asarray(v, dtype=np.complex128) for v in lam])


def _vec(state):
    return mps_obs_ref.dense(state.to_qiskit())


def _loop(state, gates, thr=0.0, cap=0):
    """What apply_gates replaces, on the engine: gate1 / gate2 per op on a clone."""
    m = state.clone()
    for g, where in gates:
        if mps_layers_ref.is_pair(where):
            m.gate2(g, int(where[0]), int(where[1]), thr, cap)
        else:
            m.gate1(g, int(where))
    return m


def _full_bonds(n):
    return [min(2 ** q, 2 ** (n - q)) for q in range(n + 1)]


def _brickwork(n, seed, layers=2):
    rng = np.random.default_rng(seed)
    gates = [(unitary(rng, 2), q) for q in range(0, n, 2)]
    for layer in range(layers):
        gates += [(unitary(rng, 4), (q, q + 1) if (q + layer) % 3 else (q + 1, q)) for q in range(layer % 2, n - 1, 2)]
        gates += [(unitary(rng, 2), (3 * layer + 1) % n)]
    return gates


@functools.lru_cache(maxsize=None)
def _exact_case(name):
    """(number of qubits, start: an index of a basis state or a QiskitMPS tuple, canonicalise it first, gates)."""
    rng = np.random.default_rng(5)
    if name == "n1":
        return 1, 1, False, [(unitary(rng, 2), 0), (unitary(rng, 2), 0)]
    if name == "n2":
        return 2, 1, False, [(unitary(rng, 4), (0, 1))]
    if name == "n3":
        return 3, 0, False, [(unitary(rng, 4), (0, 1)), (unitary(rng, 4), (2, 1))]
    if name.startswith("brick"):   # brick6-zero, brick7-basis, brick6-random, ...
        n, start = int(name[5]), name.split("-")[1]
        gates = _brickwork(n, 30 + n)
        if start == "random":       # bonds at their bounds: theta is wide on the left half and tall on the right half
            return n, mps_obs_ref.hand_made(_full_bonds(n), 70 + n), True, gates
        return n, (0 if start == "zero" else 0b0101101 % 2 ** n), False, gates
    if name == "long-range":
        return 6, mps_obs_ref.hand_made([1, 2, 3, 3, 3, 2, 1], 81), False, program(6, 66)
    if name == "singles":
        return 5, mps_obs_ref.hand_made([1, 2, 3, 3, 2, 1], 82), False, [(unitary(rng, 2), q) for q in (0, 3, 3, 4, 0)]
    if name == "empty":
        return 4, mps_obs_ref.hand_made([1, 2, 3, 2, 1], 83), False, []
    raise KeyError(name)


EXACT = ["n1", "n2", "n3", "brick6-zero", "brick6-basis", "brick6-random", "brick7-zero", "brick7-basis", "brick7-random", "long-range", "singles", "empty"]


def _start(n, start, canonical):
    from aqc_research_amd.mps_engine import DeviceMPS

    if isinstance(start, int):
        return DeviceMPS.basis_state(n, start)
    m = DeviceMPS.from_qiskit(start, assume_canonical=True)
    return m.canonicalize() if canonical else m


@pytest.mark.parametrize("name", EXACT)
def test_exact_programs_on_both_routes(name):
    from aqc_research_amd.mps_engine import apply_gates, apply_route

    n, start, canonical, gates = _exact_case(name)
    m = _start(n, start, canonical)
    made = [m]
    try:
        psi = _vec(m)
        norm = float(np.linalg.norm(psi))
        want = mps_layers_ref.dense_program(psi, n, gates)
        before = _flat(m.to_qiskit())
        assert apply_route(m.bond_dims) == "fused"
        loop = _loop(m, gates)
        made.append(loop)
        loop_vec = _vec(loop)
        for method in (None,) + ROUTES:
            out, info = apply_gates(m, gates, method=method, details=True)
            made.append(out)
            vec = _vec(out)
            err, err_loop = float(np.linalg.norm(vec - want)), float(np.linalg.norm(vec - loop_vec))
            print(f"{name}, method {method}: |applied - dense| = {err:.3g}, |applied - gate loop| = {err_loop:.3g} (|psi| = {norm:.3g}), bonds {m.bond_dims.tolist()} -> "
                  f"{out.bond_dims.tolist()}, {info['layers']} layers, sweeps {info['sweeps'].tolist()}")
            assert info["route"] == (method or "fused") and info["status"] == 0
            assert err <= TOL * norm and err_loop <= TOL * norm
            assert out.bond_dims.tolist() == info["bonds"].tolist() == loop.bond_dims.tolist()
            assert abs(out.discarded_weight) <= TOL * norm ** 2 and abs(info["dropped"]) <= TOL * norm ** 2
            assert out.num_qubits == n and out.handle.value != m.handle.value
            assert np.array_equal(_flat(m.to_qiskit()), before)                       # the input, bit for bit
        again = m.applied(gates)
        made.append(again)
        assert np.array_equal(_flat(again.to_qiskit()), _flat(made[2].to_qiskit()))
        if not isinstance(start, int) and not canonical:
            from_tuple = apply_gates(start, gates)                                    # a tuple: uploaded for the call
            made.append(from_tuple)
            assert np.array_equal(_flat(from_tuple.to_qiskit()), _flat(made[2].to_qiskit()))
        if name == "empty":
            assert np.array_equal(_flat(made[2].to_qiskit()), before) and info["layers"] == 0
        if name.endswith("random"):
            assert m.bond_dims.tolist() == _full_bonds(n)
    finally:
        for x in made:
            x.close()


@pytest.mark.parametrize("bonds", ([1, 64, 64, 64, 1], [1, 40, 64, 40, 1]), ids=("64-64-64", "40-64-40"))
def test_at_the_cap(bonds):
    """A hand-made (not canonical) n = 4 state at the cap of the fused route: one gate on (1, 2) forms a theta of 128 x 128 (80 x 80: ragged
    against the 16-column blocks of the matrix cores) through the planes at their full size.  theta factorises through the middle bond of
    64 before the gate; the gate is a product u x v (operator Schmidt rank 1), so the rank stays at 64 = max_bond and nothing above the
    rank floor is cut: the result is the dense vector's.  (An entangling gate would raise the rank to 128 and max_bond = 64 would cut it,
    in a gauge where that is no small change of the state.)"""
    from aqc_research_amd.mps_engine import DeviceMPS, apply_gates, apply_route

    mps = mps_obs_ref.hand_made(bonds, 91)
    psi = mps_obs_ref.dense(mps)
    norm = float(np.linalg.norm(psi))
    rng = np.random.default_rng(92)
    gates = [(np.kron(unitary(rng, 2), unitary(rng, 2)), (1, 2))]
    want = mps_layers_ref.dense_program(psi, 4, gates)
    m = DeviceMPS.from_qiskit(mps, assume_canonical=True)
    made = [m]
    try:
        assert apply_route(m.bond_dims, 64) == "fused"
        for method in ROUTES:
            out, info = apply_gates(m, gates, 0.0, 64, method=method, details=True)
            made.append(out)
            err = float(np.linalg.norm(_vec(out) - want))
            print(f"bonds {bonds}, {method}: |applied - dense| = {err:.3g} (|psi| = {norm:.3g}), bonds -> {out.bond_dims.tolist()}, sweeps {info['sweeps'].tolist()}")
            assert info["status"] == 0 and err <= TOL * norm
            assert out.bond_dims[2] <= 64 and out.bond_dims[1] == bonds[1] and out.bond_dims[3] == bonds[3]
    finally:
        for x in made:
            x.close()


def test_beyond_the_cap_goes_gatewise():
    from aqc_research_amd.mps_engine import DeviceMPS, apply_gates, apply_route

    mps = mps_obs_ref.hand_made([1, 2, 65, 2, 1], 93)
    psi = mps_obs_ref.dense(mps)
    gates = [(unitary(np.random.default_rng(94), 4), (1, 2)), (unitary(np.random.default_rng(95), 2), 0)]
    want = mps_layers_ref.dense_program(psi, 4, gates)
    assert apply_route([1, 2, 65, 2, 1]) == "gatewise" and apply_route([1, 2, 64, 2, 1]) == "fused"
    assert apply_route([1] * 15) == "gatewise" and apply_route([1] * 15, 64) == "fused" and apply_route([1] * 15, 65) == "gatewise"
    m = DeviceMPS.from_qiskit(mps, assume_canonical=True)
    out = None
    try:
        with pytest.raises(ValueError):
            apply_gates(m, gates, method="fused")
        with pytest.raises(ValueError):
            apply_gates(mps, gates, method="fused")
        out, info = apply_gates(m, gates, details=True)
        err = float(np.linalg.norm(_vec(out) - want))
        print(f"input bond 65: route {info['route']}, |applied - dense| = {err:.3g}")
        assert info["route"] == "gatewise" and info["status"] == 0 and err <= TOL * np.linalg.norm(psi)
    finally:
        for x in (m, out):
            if x is not None:
                x.close()


@pytest.mark.parametrize("as_cap", TRUNCATED, ids=lambda c: "max_bond" if c else "trunc_thr")
def test_truncation_matches_the_statement_and_the_loop(as_cap):
    from aqc_research_amd import mps_engine as me

    thr, cap, ref, gap = truncation(as_cap)
    circ, th, neel, gates = trotter_case()
    assert gap >= MIN_GAP
    bound = TOL / gap
    want = ref.to_vector()
    basis = me.DeviceMPS.basis_state(TROTTER_N, neel)
    made = [basis]
    try:
        loop = me.v_mul_mps(circ, th, basis, trunc_thr=thr, max_bond=cap, method="single")
        made.append(loop)
        loop_vec = _vec(loop)
        for method in ROUTES:
            for call in ("apply_gates", "v_mul_mps_many"):
                if call == "apply_gates":
                    out, info = me.apply_gates(basis, gates, thr, cap, method=method, details=True)
                else:
                    out, info = me.v_mul_mps_many(circ, th, basis, thr, cap, method=method, details=True)
                made.append(out)
                vec = _vec(out)
                err, err_loop = float(np.linalg.norm(vec - want)), float(np.linalg.norm(vec - loop_vec))
                weight = out.discarded_weight
                print(f"Trotter n = {TROTTER_N}, trunc_thr {thr:g}, max_bond {cap}, {method}, {call}: bonds -> {out.bond_dims.tolist()}, |applied - statement| = {err:.3g}, "
                      f"|applied - v_mul_mps| = {err_loop:.3g} (bound {bound:.3g}), discarded {weight:.6g} (statement {ref.discarded:.6g}, loop {loop.discarded_weight:.6g}), "
                      f"sweeps min / median / max {int(info['sweeps'].min())} / {int(np.median(info['sweeps']))} / {int(info['sweeps'].max())}")
                assert info["status"] == 0
                assert out.bond_dims.tolist() == ref.bond_dims.tolist() == loop.bond_dims.tolist() == info["bonds"].tolist()
                assert abs(weight - ref.discarded) <= TOL and abs(weight - loop.discarded_weight) <= TOL and abs(info["dropped"] - ref.discarded) <= TOL
                assert err <= bound and err_loop <= bound
    finally:
        for x in made:
            x.close()


@pytest.mark.parametrize("inverse", (False, True), ids=("v", "v_dagger"))
def test_many_states_with_their_own_thetas(inverse):
    """n = 8, three states, per-state thetas with angles outside [-pi, pi], against v_mul_mps / v_dagger_mul_mps per state."""
    from aqc_research_amd import mps_engine as me

    n = 8
    circ, th, neel = trotter(n, layers=2)
    rng = np.random.default_rng(17)
    thetas = th[None, :] + rng.uniform(-9.0, 9.0, size=(3, th.size))
    assert np.any(np.abs(thetas) > np.pi)
    states = [me.DeviceMPS.basis_state(n, neel), me.DeviceMPS.basis_state(n, 5), me.DeviceMPS.from_qiskit(mps_obs_ref.hand_made([1, 2, 3, 4, 4, 3, 2, 2, 1], 18), assume_canonical=True)]
    many, one = (me.v_dagger_mul_mps_many, me.v_dagger_mul_mps) if inverse else (me.v_mul_mps_many, me.v_mul_mps)
    made = list(states)
    try:
        want = []
        for l, s in enumerate(states):
            made.append(one(circ, thetas[l], s, method="single"))
            want.append(_vec(made[-1]))
        for method in ROUTES:
            got = many(circ, thetas, states, method=method)
            made += got
            shared = many(circ, thetas[1], states, method=method)
            made += shared
            for l in range(3):
                norm = float(np.linalg.norm(want[l]))
                err = float(np.linalg.norm(_vec(got[l]) - want[l]))
                print(f"inverse {inverse}, {method}, state {l}: |many - one| = {err:.3g} (|psi| = {norm:.3g}), bonds {got[l].bond_dims.tolist()}")
                assert err <= TOL * norm and got[l].bond_dims.tolist() == made[3 + l].bond_dims.tolist()
            assert float(np.linalg.norm(_vec(shared[1]) - want[1])) <= TOL * np.linalg.norm(want[1])
        with pytest.raises(ValueError):
            many(circ, thetas[:2], states)
    finally:
        for x in made:
            x.close()


_LANE_BONDS = {"fused": [1, 2, 3, 7, 64, 37, 5, 1], "fused-other": [1, 2, 4, 13, 33, 64, 2, 1], "gatewise": [1, 2, 4, 65, 66, 40, 2, 1], "gatewise-other": [1, 2, 3, 17, 65, 34, 2, 1]}
_LANE_SIZE = 7 * 2 * 80 * 80   # room for every site of a lane state


def _lane_program():
    rng = np.random.default_rng(23)
    return [(unitary(rng, 2), 0), (unitary(rng, 4), (0, 1)), (unitary(rng, 4), (3, 2)), (unitary(rng, 4), (5, 6)), (unitary(rng, 2), 4), (unitary(rng, 4), (1, 2)), (unitary(rng, 4), (4, 5))]


def _lane_outputs(results, info):
    sites = np.zeros((len(results), _LANE_SIZE), dtype=np.complex128)
    for l, out in enumerate(results):
        if out is None:
            sites[l] = np.nan
            continue
        flat = _flat(out.to_qiskit())
        sites[l, :flat.size] = flat
        out.close()
    return {"state": sites, "bonds": info["bonds"], "dropped": info["dropped"], "status": info["status"]}


@pytest.mark.parametrize("method", ROUTES)
def test_lanes_hold_the_lane_contract(method):
    """Four states, probes (0, 3), at a threshold that cuts.  F: neighbours with other bonds of the same route; N: every neighbour holds
    NaN tensors, gets status 2 and no state, and the probes' bits do not move."""
    from aqc_research_amd.mps_engine import DeviceMPS, apply_gates, apply_route

    gates = _lane_program()
    made = []

    def device(profile, seed, nan=False):
        gam, lam = mps_obs_ref.hand_made(_LANE_BONDS[profile], seed)
        if nan:
            gam = [(g0 * np.nan, g1 * np.nan) for g0, g1 in gam]
        made.append(DeviceMPS.from_qiskit((gam, lam), assume_canonical=True))
        return made[-1]

    def run(states):
        results, info = apply_gates(states, gates, 1e-4, details=True)
        assert info["route"] == method
        return _lane_outputs(results, info)

    try:
        states = [device(method, 880 + l) for l in range(4)]
        poison = [device(method, 880 + l, nan=True) for l in range(4)]
        assert all(apply_route(m.bond_dims) == method for m in states)
        before = [_flat(m.to_qiskit()) for m in states]
        base = check_lanes(run, states, probes=(0, 3), other=[device(method + "-other", 890 + l) for l in range(4)], poison=poison, distinct=("state",))
        assert np.all(base["status"] == 0) and np.all(base["bonds"] >= 1)
        results, info = apply_gates([states[0], poison[1], poison[2], states[3], states[0]], gates, 1e-4, details=True)
        assert results[1] is None and results[2] is None and info["status"].tolist() == [0, 2, 2, 0, 0] and info["route"] == method
        assert np.all(info["bonds"][1:3] == 0) and info["failed_at"][1].tolist() == [0, 0]
        twice = _flat(results[4].to_qiskit())
        assert np.array_equal(twice, _flat(results[0].to_qiskit())) and results[4].handle.value != results[0].handle.value   # a state listed twice
        for l in (0, 3):
            assert np.array_equal(_flat(results[l].to_qiskit()), base["state"][l, :_flat(results[l].to_qiskit()).size])
        for l in (0, 3, 4):
            results[l].close()
        with pytest.raises(RuntimeError, match="lane 1, layer 0, site 0"):
            apply_gates([states[0], poison[1]], gates, 1e-4)
        assert all(np.array_equal(_flat(m.to_qiskit()), b) for m, b in zip(states, before))           # the inputs, bit for bit
    finally:
        for m in made:
            m.close()


def test_chunks_of_matrices_give_the_same_bits():
    """A layer's matrices (gates x states) go through the batched SVD in chunks that fit its budget.  With the budget lowered to 3 matrices
    and to 1 matrix per chunk, 9 lanes (per-state matrices: every listing a lane) keep the bits of their one-state calls."""
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import DeviceMPS, apply_gates

    L = _lib.lib()
    n, lanes = 6, 9
    rng = np.random.default_rng(29)
    gates = _brickwork(n, 31)
    per_lane = [[(np.stack([unitary(rng, g.shape[0]) for _ in range(lanes)]), where) if i % 2 else (g, where) for i, (g, where) in enumerate(gates)]][0]
    states = [DeviceMPS.from_qiskit(mps_obs_ref.hand_made(_full_bonds(n), 300 + l), assume_canonical=True) for l in range(lanes - 1)]
    states.append(states[2])   # a second listing, with other matrices: a lane of its own
    made = list(states[:-1])
    per_matrix = 16 * 5 * 16 * 16   # mps_layers_chunk at K = 8: five stores of 16 x 16 complex numbers
    try:
        whole, info = apply_gates(states, per_lane, 1e-3, details=True)
        made += whole
        assert info["route"] == "fused" and np.all(info["status"] == 0)
        ones = []
        for l in range(lanes):
            mine = [(g[l] if g.ndim == 3 else g, where) for g, where in per_lane]
            ones.append(apply_gates(states[l], mine, 1e-3))
            made.append(ones[-1])
            assert np.array_equal(_flat(ones[-1].to_qiskit()), _flat(whole[l].to_qiskit())), l
            assert ones[-1].discarded_weight == whole[l].discarded_weight
        assert not np.array_equal(_flat(whole[2].to_qiskit()), _flat(whole[8].to_qiskit()))
        default = L.aqc_mps_apply_svd_budget(3 * per_matrix + 7)
        assert default == 256 << 20
        for chunk in (3, 1):
            assert L.aqc_mps_apply_svd_budget(chunk * per_matrix + 7) > 0
            got, again = apply_gates(states, per_lane, 1e-3, details=True)
            made += got
            for key in ("bonds", "dropped", "sweeps", "status"):
                assert np.array_equal(info[key], again[key]), (chunk, key)
            for l in range(lanes):
                assert np.array_equal(_flat(got[l].to_qiskit()), _flat(whole[l].to_qiskit())), (chunk, l)
    finally:
        L.aqc_mps_apply_svd_budget(0)
        for x in made:
            x.close()
    assert L.aqc_mps_apply_svd_budget(0) == 256 << 20


def test_refusals_leave_no_buffers_and_a_correct_call_follows():
    from ctypes import c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS, apply_gates

    L = _lib.lib()
    mps = mps_obs_ref.hand_made([1, 2, 3, 2, 1], 41)
    a, wide, five = DeviceMPS.from_qiskit(mps, assume_canonical=True), DeviceMPS.from_qiskit(mps_obs_ref.hand_made([1, 2, 65, 2, 1], 42), assume_canonical=True), DeviceMPS.basis_state(5)
    g4, g2 = unitary(np.random.default_rng(43), 4), unitary(np.random.default_rng(44), 2)
    out_ok = None
    try:
        hs, out = (c_void_p * 2)(a.handle, a.handle), (c_void_p * 2)()
        qubits, kinds = np.array([[1, 2], [0, 0]], dtype=np.int32), np.array([2, 1], dtype=np.int32)
        mats = np.concatenate([g4.ravel(), g2.ravel()])
        ranks, sweeps, status, dropped = np.zeros((2, 5), np.int32), np.zeros((2, 1), np.int32), np.zeros((2, 3), np.int32), np.zeros(2)

        def call(states, nstates, thr=0.0, cap=0, method=0, dst=out, q=qubits, k=kinds, m=mats):
            return L.aqc_mps_apply_gates(states, nstates, 2, _lib.iptr(q), _lib.iptr(k), _lib.dptr(m), 0, thr, cap, method, dst, _lib.iptr(ranks), _lib.dptr(dropped),
                                         _lib.iptr(sweeps), _lib.iptr(status))

        live = live_buffers()
        assert call(None, 2) == 1 and call(hs, 2, dst=None) == 1 and call(hs, 0) == 1 and call(hs, 2, method=3) == 1
        assert call((c_void_p * 2)(a.handle, None), 2) == 1                                                        # a closed handle
        assert call((c_void_p * 2)(a.handle, five.handle), 2) == 1 and b"differ" in L.aqc_last_error()            # mixed n
        assert call((c_void_p * 1)(wide.handle), 1, method=1) == 1 and b"fused" in L.aqc_last_error()             # beyond the cap
        assert call(hs, 2, cap=-1) == 1 and b"max_bond" in L.aqc_last_error()
        assert call(hs, 2, thr=-1e-3) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert call(hs, 2, thr=float("nan")) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert call(hs, 2, q=np.array([[1, 4], [0, 0]], dtype=np.int32)) == 1 and b"out of range" in L.aqc_last_error()
        assert call(hs, 2, q=np.array([[1, 1], [0, 0]], dtype=np.int32)) == 1 and call(hs, 2, k=np.array([2, 3], dtype=np.int32)) == 1
        bad = mats.copy()
        bad[5] = np.nan
        assert call(hs, 2, m=bad) == 1 and b"not finite" in L.aqc_last_error()
        assert out[0] is None and out[1] is None and live_buffers() == live
        closed = DeviceMPS.from_qiskit(mps, assume_canonical=True)
        closed.close()
        gates = [(g4, (1, 2)), (g2, 0)]
        for refused in (lambda: apply_gates([a, five], gates), lambda: apply_gates([a, closed], gates), lambda: apply_gates(wide, gates, method="fused"),
                        lambda: apply_gates(a, gates, 0.0, -1), lambda: apply_gates(a, gates, -1e-3), lambda: apply_gates(a, gates, float("nan")),
                        lambda: apply_gates(a, gates, method="canonical"), lambda: apply_gates(a, [(g4, (1, 4))]), lambda: apply_gates(a, [(g4, 1)]),
                        lambda: apply_gates(a, [(g2 * np.nan, 1)]), lambda: apply_gates(a, [(np.stack([g2, g2]), 1)]), lambda: apply_gates([], gates)):
            with pytest.raises(ValueError):
                refused()
        assert live_buffers() == live
        out_ok = apply_gates(a, gates)
        want = mps_layers_ref.dense_program(mps_obs_ref.dense(mps), 4, gates)
        assert float(np.linalg.norm(_vec(out_ok) - want)) <= TOL * np.linalg.norm(want)
        out_ok.close()
        out_ok = None
        assert call(hs, 2) == 0 and out[0] and out[1] and out[0] != out[1] and status[:, 0].tolist() == [0, 0]
        assert ranks[0].tolist() == ranks[1].tolist() and ranks[0, 0] == 1 and ranks[0, 4] == 1
        for h in out:
            assert L.aqc_mps_destroy(c_void_p(h)) == 0
        assert live_buffers() == live
    finally:
        for m in (a, wide, five, out_ok):
            if m is not None:
                m.close()
