"""GPU: operator sums on MPS states on the device (mps_engine.operator_sums / apply_operator, aqc_mps_opsum; kernel
csrc/aqc_mps_opsum.hip, the sweep of compression) on both routes, against sum_t c_t dense(O_t) dense(psi_t) and the NumPy statement
(tests/mps_opsum_ref.py).

Cases of tests/mps_opsum_ref.py.  Bounds: TOL x scale at trunc_thr = 0, scale = sum_t |c_t| |O_t|_2 |psi_t|; with truncation
TOL x scale / gap against the statement, the relative gap read from the reference's decisions and held to >= 1e-3 there
(tests/test_mps_opsum_ref.py), as tests/test_hip_mps_combine.py bounds it.  Ranks must be equal, weights agree within TOL x scale^2.
The tests print what they observe; DESIGN.md records it."""
import functools

import numpy as np
import pytest

from tests import mps_combine_ref, mps_obs_ref, mps_opsum_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes
from tests.test_hip_mps_entanglement import _flat
from tests.test_mps_compress_ref import MIN_GAP, normalised

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dense(name):
    vec, scale = mps_opsum_ref.dense_sum(mps_opsum_ref.case(name))
    vec.setflags(write=False)
    return vec, scale


@functools.lru_cache(maxsize=None)
def _statement(name):
    return mps_opsum_ref.statement(mps_opsum_ref.case(name))


def _terms(terms, upload=True):
    """The terms of a reference case as ``operator_sums`` takes them: one MPO per distinct list of sites, one DeviceMPS (or the tuple
    itself) per distinct tuple.  Returns (terms, the DeviceMPS states made)."""
    from aqc_research_amd.mps_engine import MPO, DeviceMPS

    ops, states = {}, {}
    for _, op, state in terms:
        if op is not None and id(op) not in ops:
            ops[id(op)] = MPO(op)
        if id(state) not in states:
            states[id(state)] = DeviceMPS.from_qiskit(state, assume_canonical=True) if upload else state
    return [(c, None if op is None else ops[id(op)], states[id(s)]) for c, op, s in terms], (list(states.values()) if upload else [])


def _vec(state):
    return mps_obs_ref.dense(state.to_qiskit())


def _close(items):
    for x in items:
        if x is not None:
            x.close()


def _same(a, b):
    return np.array_equal(_flat(a.to_qiskit()), _flat(b.to_qiskit())) and a.discarded_weight == b.discarded_weight


@pytest.mark.parametrize("name", mps_opsum_ref.CASES)
def test_exact_results_on_both_routes(name):
    from aqc_research_amd.mps_engine import is_canonical, operator_sums, opsum_route

    case = mps_opsum_ref.case(name)
    n = len(case[0][2][0])
    want, scale = _dense(name)
    ref = _statement(name)
    rule = "fused" if name in mps_opsum_ref.FUSED else "canonical"
    terms, owned = _terms(case)
    made = {}
    try:
        assert opsum_route([t[2].bond_dims for t in terms], [None if t[1] is None else t[1].bond_dims for t in terms]) == rule
        before = [_flat(m.to_qiskit()) for m in owned]
        for method in (None, "fused", "canonical"):
            if method == "fused" and rule != "fused":
                with pytest.raises(ValueError, match="output 0"):
                    operator_sums([terms], method="fused")
                continue
            (out,), info = operator_sums([terms], method=method, details=True)
            made[method] = out
            assert info["route"] == [method or rule] and info["status"].tolist() == [0]
            assert info["ranks"].shape == info["dropped"].shape == info["sweeps"].shape == (1, n - 1)
            err = float(np.linalg.norm(_vec(out) - want))
            lam = out.to_qiskit()[1]
            lam_err = max([0.0] + [float(np.max(np.abs(a - b))) if a.shape == b.shape else np.inf for a, b in zip(lam, ref.lam)])
            print(f"case {name}, method {method}: |result - dense result| = {err:.3g}, max |bond vector - statement| = {lam_err:.3g} (scale {scale:.3g}), "
                  f"product bonds {mps_opsum_ref.product_bonds(case)} -> {out.bond_dims.tolist()}, sweeps {info['sweeps'].tolist()}")
            assert out.bond_dims.tolist() == ref.bond_dims.tolist() and out.bond_dims[1:n].tolist() == info["ranks"][0].tolist()
            assert err <= TOL * scale and lam_err <= TOL * scale
            if n > 1:
                assert is_canonical(normalised(out.to_qiskit(), float(np.linalg.norm(want))))
            assert abs(out.discarded_weight) <= TOL * scale ** 2 and np.all(np.abs(info["dropped"]) <= TOL * scale ** 2)
            assert [np.array_equal(_flat(m.to_qiskit()), b) for m, b in zip(owned, before)] == [True] * len(owned)   # the inputs, bit for bit
        if rule == "fused":
            routes = float(np.linalg.norm(_vec(made["fused"]) - _vec(made["canonical"])))
            print(f"case {name}: |fused - canonical| = {routes:.3g}")
            assert routes <= TOL * scale
        assert _same(made[None], made[rule])
        made["tuples"] = operator_sums([_terms(case, upload=False)[0]])[0]                 # tuples: uploaded for the call
        assert _same(made["tuples"], made[rule])
    finally:
        _close(list(made.values()) + owned)


@pytest.mark.parametrize("as_cap", (False, True), ids=("trunc_thr", "max_bond"))
@pytest.mark.parametrize("name", mps_opsum_ref.TRUNCATED)
def test_truncation_matches_the_statement(name, as_cap):
    from aqc_research_amd.mps_engine import operator_sums

    case = mps_opsum_ref.case(name)
    n = len(case[0][2][0])
    _, scale = _dense(name)
    thr, cap, ref, gap = mps_opsum_ref.truncation(name, as_cap)
    assert gap is not None and gap >= MIN_GAP
    bound = TOL * scale / gap
    want = ref.to_vector()
    terms, owned = _terms(case)
    made = []
    try:
        for method in ("fused", "canonical"):
            (out,), info = operator_sums([terms], thr, cap, method=method, details=True)
            made.append(out)
            err = float(np.linalg.norm(_vec(out) - want))
            weight = out.discarded_weight
            got = np.array([d.total - d.kept for d in ref.decisions])
            print(f"case {name}, trunc_thr {thr:g}, max_bond {cap}, {method}: bonds -> {out.bond_dims.tolist()}, |result - statement| = {err:.3g} "
                  f"(bound {bound:.3g}), discarded {weight:.6g} (statement {ref.discarded:.6g})")
            assert info["status"].tolist() == [0]
            assert out.bond_dims.tolist() == ref.bond_dims.tolist() and info["ranks"][0].tolist() == ref.bond_dims[1:n].tolist()
            assert abs(weight - ref.discarded) <= TOL * scale ** 2 and abs(float(info["dropped"].sum()) - weight) <= TOL * scale ** 2
            assert np.max(np.abs(info["dropped"][0] - got), initial=0.0) <= TOL * scale ** 2
            assert err <= bound
            lam = out.to_qiskit()[1]
            assert max(float(np.max(np.abs(a - b))) for a, b in zip(lam, ref.lam)) <= bound
    finally:
        _close(made + owned)


def test_both_routes_in_one_call():
    """A product bond of exactly 64 goes fused, 65 canonical; together in one call they have the bits of their own calls."""
    from aqc_research_amd.mps_engine import operator_sums

    at_cap, owned_a = _terms(mps_opsum_ref.case("cap64"))
    beyond, owned_b = _terms(mps_opsum_ref.case("beyond"))
    made = []
    try:
        alone = operator_sums([at_cap]) + operator_sums([beyond])
        made += alone
        both, info = operator_sums([at_cap, beyond], details=True)
        made += both
        assert info["route"] == ["fused", "canonical"] and info["status"].tolist() == [0, 0]
        assert _same(both[0], alone[0]) and _same(both[1], alone[1])
        with pytest.raises(ValueError, match="output 1"):
            operator_sums([at_cap, beyond], method="fused")
    finally:
        _close(made + owned_a + owned_b)


_ROWS = np.array([[0.0, 0.0, 1.3 - 0.2j],
                  [0.7, 0.0, -0.4j],
                  [0.5j, -0.9, 0.0],
                  [0.6, 0.2 + 0.7j, -1.1],
                  [0.7, 0.0, -0.4j]])


def _pool():
    """(operator sites, states): outputs are rows[0] H psi + rows[1] psi + rows[2] R phi."""
    hm = mps_obs_ref.hand_made
    return [mps_opsum_ref.xxz(6, 0.4), mps_opsum_ref.random_mpo([1, 2, 3, 2, 2, 2, 1], 831)], [hm(mps_opsum_ref.P5, 832), hm(mps_opsum_ref.P7, 833)]


def _row_terms(row, ops, states):
    return [(row[0], ops[0], states[0]), (row[1], None, states[0]), (row[2], ops[1], states[1])]


def test_identity_terms_are_linear_combinations():
    """Only identity terms: bit for bit the states of linear_combinations on the same terms, on both routes."""
    from aqc_research_amd.mps_engine import DeviceMPS, linear_combinations, operator_sums

    made, owned = [], []
    try:
        for name, method in (("three", "fused"), ("three", "canonical"), ("cap64", None), ("n1", None), ("n2", None)):
            states, coeffs, _ = mps_combine_ref.case(name)
            dev = {id(s): None for s in states}
            for s in states:
                if dev[id(s)] is None:
                    dev[id(s)] = DeviceMPS.from_qiskit(s, assume_canonical=True)
            owned += list(dev.values())
            listed = [dev[id(s)] for s in states]
            thr = mps_combine_ref.truncation(name, False)[0] if name == "three" else 0.0
            want, winfo = linear_combinations(listed, coeffs, thr, method=method, details=True)
            (got,), ginfo = operator_sums([[(c, None, s) for c, s in zip(coeffs, listed)]], thr, method=method, details=True)
            made += [want, got]
            assert _same(got, want), (name, method)
            for key in ("ranks", "dropped", "sweeps", "status"):
                assert np.array_equal(np.atleast_1d(winfo[key]), ginfo[key][0] if key != "status" else ginfo[key]), (name, key)
        wide = [mps_obs_ref.hand_made([1, 2, 4, 33, 40, 8, 2, 1], 834 + k) for k in range(2)]
        want, winfo = linear_combinations(wide, [0.6, -0.8j], 1e-4, details=True)
        (got,), ginfo = operator_sums([[(0.6, None, wide[0]), (-0.8j, None, wide[1])]], 1e-4, details=True)
        made += [want, got]
        assert winfo["route"] == "canonical" and ginfo["route"] == ["canonical"] and _same(got, want)
    finally:
        _close(made + owned)


def test_many_outputs_in_one_call():
    """Five outputs of one to three terms with operators, a repeated row among them: every output has the bits of its one-output call,
    also when the sweep runs in chunks of 3 and of 1 outputs; tuples and DeviceMPS inputs give the same bits."""
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import MPO, DeviceMPS, operator_sums

    L = _lib.lib()
    op_sites, tuples = _pool()
    ops = [MPO(s) for s in op_sites]
    dev = [DeviceMPS.from_qiskit(s, assume_canonical=True) for s in tuples]
    outputs = [_row_terms(row, ops, dev) for row in _ROWS]
    made = []
    per_output = 8 * 16 * 44 * 44   # mps_compress_chunk at K = 25 + 5 + 14, the largest summed product bond of the call
    try:
        whole, info = operator_sums(outputs, 1e-3, details=True)
        made += whole
        assert len(whole) == 5 and info["status"].tolist() == [0] * 5 and info["route"] == ["fused"] * 5
        assert _same(whole[4], whole[1]) and whole[4].handle.value != whole[1].handle.value
        from_tuples = operator_sums([_row_terms(row, ops, tuples) for row in _ROWS], 1e-3)
        made += from_tuples
        for j in range(5):
            one, one_info = operator_sums([outputs[j]], 1e-3, details=True)
            made += one
            ref_terms = [(c, None if op is None else list(op.sites), tuples[dev.index(s)]) for c, op, s in outputs[j] if c != 0]
            want, scale = mps_opsum_ref.dense_sum(ref_terms)
            exact = operator_sums([outputs[j]])
            made += exact
            err = float(np.linalg.norm(_vec(exact[0]) - want))
            print(f"output {j}: |result - dense result| = {err:.3g} (scale {scale:.3g})")
            assert err <= TOL * scale
            assert _same(one[0], whole[j]) and _same(from_tuples[j], whole[j]), j
            assert np.array_equal(one_info["ranks"][0], info["ranks"][j]) and np.array_equal(one_info["dropped"][0], info["dropped"][j])
        default = L.aqc_mps_opsum_svd_budget(3 * per_output + 7)
        assert default == 256 << 20
        for chunk in (3, 1):
            assert L.aqc_mps_opsum_svd_budget(chunk * per_output + 7) > 0
            got, again = operator_sums(outputs, 1e-3, details=True)
            made += got
            for key in ("ranks", "dropped", "sweeps", "status"):
                assert np.array_equal(info[key], again[key]), (chunk, key)
            for j in range(5):
                assert _same(got[j], whole[j]), (chunk, j)
    finally:
        L.aqc_mps_opsum_svd_budget(0)
        _close(made + dev)
    assert L.aqc_mps_opsum_svd_budget(0) == 256 << 20


_WIDE = [1, 2, 4, 13, 8, 4, 2, 1]   # times the XXZ Hamiltonian's 5: a product bond of 65, beyond the fused cap
_LANE_SIZE = 7 * 2 * 64 * 64


@pytest.mark.parametrize("method", ("fused", "canonical"))
def test_outputs_hold_the_lane_contract(method):
    """Four outputs as lanes, each c_0 H psi_l + c_1 psi_l with a state and a coefficient row of its own, probes (0, 3), at a threshold
    that cuts.  F: the other lanes get other states and coefficients; N: they get NaN coefficients, their outputs get status 2 and no
    state, and the probes' bits do not move."""
    from aqc_research_amd.mps_engine import MPO, operator_sums

    hm = mps_obs_ref.hand_made
    dims = mps_opsum_ref.P5 if method == "fused" else _WIDE
    h = MPO.xxz(len(dims) - 1, 0.6)
    states = [hm(dims, 841 + l) for l in range(4)]
    donors = [hm(dims, 851 + l) for l in range(4)]
    rng = np.random.default_rng(846)
    rows = rng.standard_normal((4, 2)) + 1j * rng.standard_normal((4, 2))
    other = rng.standard_normal((4, 2)) + 1j * rng.standard_normal((4, 2))

    def run(inputs):
        lanes, coeffs = inputs
        results, info = operator_sums([[(coeffs[l, 0], h, lanes[l]), (coeffs[l, 1], None, lanes[l])] for l in range(4)], 1e-4, details=True)
        assert info["route"] == [method] * 4
        sites = np.zeros((4, _LANE_SIZE), dtype=np.complex128)
        for l, out in enumerate(results):
            if out is None:
                sites[l] = np.nan
                continue
            flat = _flat(out.to_qiskit())
            sites[l, :flat.size] = flat
            out.close()
        return {"state": sites, "ranks": info["ranks"], "dropped": info["dropped"], "status": info["status"]}

    def poison(inputs, lanes):
        kept, coeffs = inputs
        coeffs[lanes] = np.nan
        return kept, coeffs

    base = check_lanes(run, (states, rows), probes=(0, 3), other=(donors, other), poison=poison, distinct=("state",))
    assert np.all(base["status"] == 0) and np.all(base["ranks"] >= 1)
    poisoned = rows.copy()
    poisoned[1:3] = np.nan
    got = run((states, poisoned))
    assert got["status"].tolist() == [0, 2, 2, 0] and np.all(got["ranks"][1:3] == 0) and np.all(np.isnan(got["state"][1:3]))
    assert np.array_equal(got["state"][[0, 3]], base["state"][[0, 3]])


def test_failed_outputs_fail_alone():
    """A NaN coefficient, a NaN operator entry and a state that the operator annihilates (|1><1| on a qubit that is |0>: a site of exact
    zeros): status 2 and None for that output only, and the buffers of the call are returned."""
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import MPO, DeviceMPS, operator_sums

    w = DeviceMPS.from_qiskit(mps_opsum_ref.w_state(8), assume_canonical=True)
    down = DeviceMPS.basis_state(8, 0b00010001)                  # qubit 2 is |0>
    keep = MPO(mps_opsum_ref.projector(8, (2,)))
    sick = [s.copy() for s in mps_opsum_ref.projector(8, (2,))]
    sick[4][0, 0, 1, 0] = np.nan
    sick = MPO(sick)
    made = []
    try:
        live = live_buffers()
        alone = operator_sums([[(1.0, keep, w)]])
        made += alone
        outputs = [[(1.0, keep, w)], [(float("nan"), keep, w)], [(1.0, sick, w)], [(1.0, keep, down)], [(1.0, keep, w), (2.0, keep, down)], [(1.0, keep, w)]]
        for method in (None, "canonical"):
            results, info = operator_sums(outputs, method=method, details=True)
            made += results
            assert info["status"].tolist() == [0, 2, 2, 2, 0, 0] and [r is None for r in results] == [False, True, True, True, False, False]
            assert np.all(info["ranks"][1:4] == 0)
            if method is None:
                assert _same(results[0], alone[0]) and _same(results[5], alone[0])
            vec = results[4].to_vector()                          # the annihilated term adds a block of zeros
            assert abs(vec[4] - 1.0 / np.sqrt(8.0)) <= TOL and abs(float(np.linalg.norm(vec)) - 1.0 / np.sqrt(8.0)) <= TOL
        with pytest.raises(RuntimeError, match="output 3, cut 1"):
            operator_sums(outputs[:1] + outputs[4:] + [outputs[3]])
        _close(made)
        made = []
        assert live_buffers() == live
    finally:
        _close(made + [w, down])


def test_xxz_on_ten_qubits_matches_the_dense_kernel():
    from aqc_research_amd.mps_engine import MPO, apply_operator, from_vectors, to_vectors
    from aqc_research_amd.xxz import xxz_mul_vec

    n, delta = 10, 0.45
    rng = np.random.default_rng(861)
    v = rng.standard_normal((3, 1 << n)) + 1j * rng.standard_normal((3, 1 << n))
    v /= np.linalg.norm(v, axis=1)[:, None]
    h = MPO.xxz(n, delta)
    states = from_vectors(v)
    made = []
    try:
        images, info = apply_operator(h, states, details=True)
        made += images
        got = to_vectors(images)
        want = xxz_mul_vec(v, delta)
        scale = float(np.linalg.norm(h.to_dense(), 2))
        err = float(np.max(np.linalg.norm(got - want, axis=1)))
        print(f"XXZ on {n} qubits, random vectors: routes {info['route']}, max |H psi (MPS) - H psi (dense kernel)| = {err:.3g} (scale {scale:.3g})")
        assert info["status"].tolist() == [0, 0, 0] and err <= TOL * scale
        one, one_info = states[1].applied_operator(h, details=True)
        made.append(one)
        assert _same(one, images[1]) and one_info["route"] == info["route"][1] and one_info["ranks"].shape == (n - 1,)
        made.append(apply_operator(h, states[1]))
        assert _same(made[-1], images[1])
    finally:
        _close(made + states)


def test_forty_qubits():
    """Beyond dense reach: n = 40, two hand-made states of bond 16 and a 3-string Pauli sum (product bonds 48): <phi|O psi> by overlaps
    equals sum_k w_k <phi|P_k|psi> by pauli_strings; the variance of a ZZ string on a basis state is 0."""
    from aqc_research_amd.mps_engine import MPO, DeviceMPS, apply_operator
    from aqc_research_amd.mps_observables import overlaps, pauli_strings, variance

    n = 40
    dims = [min(2 ** q, 2 ** (n - q), 16) for q in range(n + 1)]
    psi, phi = (DeviceMPS.from_qiskit(mps_obs_ref.hand_made(dims, 871 + k), assume_canonical=True) for k in range(2))
    strings = [("XZ", (3, 17)), ("YY", (20, 21)), ("ZXZ", (0, 19, 39))]
    weights = np.array([0.8 - 0.3j, -0.5, 0.6j])
    op = MPO.from_pauli_sum(list(zip(weights, strings)), num_qubits=n)
    basis = DeviceMPS.basis_state(n, (1 << 7) | (1 << 30))
    out = None
    try:
        out, info = apply_operator(op, psi, details=True)
        got = overlaps([phi, psi], [out])[:, 0]
        want = np.array([pauli_strings(psi, strings, bras=phi) @ weights, pauli_strings(psi, strings) @ weights])
        scale = float(np.abs(weights).sum())                     # the states have norm 1, a string 2-norm 1
        err = float(np.max(np.abs(got - want)))
        print(f"n = {n}, bond 16, 3 strings: route {info['route']}, bonds up to {int(out.bond_dims.max())}, max |<phi|O psi> - sum_k w_k <phi|P_k|psi>| = {err:.3g}")
        assert op.bond_dims.max() == 3 and info["route"] == "fused" and info["status"] == 0 and int(out.bond_dims.max()) <= 48
        assert err <= TOL * scale
        zz = MPO.from_pauli_string(("ZZ", (7, 8)), num_qubits=n)
        var = variance(basis, zz)
        both = variance([basis, psi], zz)
        print(f"variance of Z_7 Z_8: basis state {var:.3g}, random state {both[1]:.6g}")
        assert abs(var) <= TOL and both[0] == var and 0.0 < both[1] <= 1.0 + TOL
        assert abs(both[1] - (1.0 - pauli_strings(psi, [("ZZ", (7, 8))])[0].real ** 2)) <= TOL   # (ZZ)^2 = 1
    finally:
        _close([psi, phi, basis, out])


def test_refusals_leave_no_buffers_and_a_correct_call_follows():
    from ctypes import POINTER, c_int64, c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import MPO, DeviceMPS, operator_sums

    L = _lib.lib()
    case = mps_opsum_ref.case("n3")
    terms, owned = _terms(case)
    wide = DeviceMPS.from_qiskit(mps_obs_ref.hand_made([1, 2, 33, 1], 881), assume_canonical=True)
    five = DeviceMPS.basis_state(5)
    owned += [wide, five]
    op = terms[0][1]
    made = []
    try:
        hs, out = (c_void_p * 2)(terms[0][2].handle, terms[1][2].handle), (c_void_p * 2)()
        off, st, ops_of = np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([0, 0, -1], np.int32)
        cf = np.array([0.0, 0.9, 0.6, 0.0, -1.0, 0.0])
        od = np.ascontiguousarray(op.bond_dims.reshape(1, 4))
        oo = np.array([[0, 8, 16, 20]], np.int64)
        data = np.ascontiguousarray(np.concatenate([w.ravel() for w in op.sites]))
        ranks, sweeps, status, dropped = np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32), np.zeros(2, np.int32), np.zeros((2, 2))

        def call(states=hs, nstates=2, nops=1, op_dims=od, op_off=oo, op_data=data, nout=2, term_off=off, term_state=st, term_op=ops_of, coeffs=cf,
                 thr=0.0, cap=0, method=0, dst=out):
            ip = lambda a: None if a is None else _lib.iptr(a)   # noqa: E731
            dp = lambda a: None if a is None else _lib.dptr(a)   # noqa: E731
            return L.aqc_mps_opsum(states, nstates, nops, ip(op_dims), None if op_off is None else op_off.ctypes.data_as(POINTER(c_int64)), dp(op_data), nout,
                                   ip(term_off), ip(term_state), ip(term_op), dp(coeffs), thr, cap, method, dst, _lib.iptr(ranks), _lib.dptr(dropped),
                                   _lib.iptr(sweeps), _lib.iptr(status))

        live = live_buffers()
        assert call(states=None) == 1 and call(dst=None) == 1 and call(term_off=None) == 1 and call(term_state=None) == 1 and call(term_op=None) == 1
        assert call(coeffs=None) == 1 and call(op_dims=None) == 1 and call(op_off=None) == 1 and call(op_data=None) == 1
        assert call(nout=0) == 1 and call(nstates=0) == 1 and call(method=3) == 1 and call(nops=-1) == 1
        assert call(states=(c_void_p * 2)(terms[0][2].handle, None)) == 1
        assert call(states=(c_void_p * 2)(terms[0][2].handle, five.handle)) == 1 and b"differ" in L.aqc_last_error()       # mixed n
        assert call(term_off=np.array([1, 2, 3], np.int32)) == 1 and b"term_off" in L.aqc_last_error()
        assert call(term_off=np.array([0, 0, 3], np.int32)) == 1 and b"at least one term" in L.aqc_last_error()               # an empty output
        assert call(term_state=np.array([0, 2, 1], np.int32)) == 1 and b"state outside" in L.aqc_last_error()
        assert call(term_op=np.array([0, 1, -1], np.int32)) == 1 and b"operator outside" in L.aqc_last_error()
        assert call(term_op=np.array([0, -2, -1], np.int32)) == 1 and b"operator outside" in L.aqc_last_error()
        assert call(nops=0) == 1 and b"operator outside" in L.aqc_last_error()
        assert call(op_dims=np.array([[1, 2, 1, 2]], np.int32)) == 1 and b"operator 0" in L.aqc_last_error()                  # dims not of n = 3
        assert call(op_dims=np.array([[1, 2, 2, 1]], np.int32)) == 1 and b"packed layout" in L.aqc_last_error()
        assert call(op_off=np.array([[-1, 7, 15, 19]], np.int64)) == 1 and b"packed layout" in L.aqc_last_error()
        wide_op = MPO(mps_opsum_ref.random_mpo([1, 2, 2, 1], 882))
        wd, wdata = np.ascontiguousarray(wide_op.bond_dims.reshape(1, 4)), np.ascontiguousarray(np.concatenate([w.ravel() for w in wide_op.sites]))
        assert call(states=(c_void_p * 2)(wide.handle, wide.handle), op_dims=wd, op_off=np.array([[0, 8, 24, 32]], np.int64), op_data=wdata, method=1) == 1
        assert b"fused" in L.aqc_last_error()                                                                                # 66 + 66: beyond the cap
        assert call(cap=-1) == 1 and b"max_bond" in L.aqc_last_error()
        assert call(thr=-1e-3) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert call(thr=float("nan")) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert out[0] is None and out[1] is None and live_buffers() == live
        closed = DeviceMPS.basis_state(3)
        closed.close()
        h5 = MPO.xxz(5, 0.5)
        for bad in (lambda: operator_sums([[(1.0, op, terms[0][2]), (1.0, None, five)]]), lambda: operator_sums([[(1.0, op, closed)]]),
                    lambda: operator_sums([[(1.0, h5, terms[0][2])]]), lambda: operator_sums([[(1.0, wide_op, wide)]], method="fused"),
                    lambda: operator_sums([terms], 0.0, -1), lambda: operator_sums([terms], -1e-3), lambda: operator_sums([[(0.0, op, terms[0][2])]]),
                    lambda: operator_sums([terms], method="gemm"), lambda: operator_sums([terms, []])):
            with pytest.raises(ValueError):
                bad()
        assert live_buffers() == live
        with pytest.raises(RuntimeError, match="output 0"):
            operator_sums([[(float("nan"), op, terms[0][2])]])
        assert live_buffers() == live
        (ok,) = operator_sums([terms])
        made.append(ok)
        want, scale = _dense("n3")
        assert float(np.linalg.norm(_vec(ok) - want)) <= TOL * scale and ok.bond_dims.tolist() == _statement("n3").bond_dims.tolist()
        ok.close()
        assert call() == 0 and out[0] and out[1] and out[0] != out[1] and status.tolist() == [0, 0]
        first = [(0.9j, case[0][1], case[0][2]), (0.6, case[0][1], case[1][2])]
        assert ranks[0].tolist() == mps_opsum_ref.statement(first).bond_dims[1:3].tolist()
        assert ranks[1].tolist() == [1, 2]                                                      # - psi_1 alone: its own bonds
        plain = (c_void_p * 2)()                                                                # no operators at all: the op arrays may be null
        assert call(nops=0, op_dims=None, op_off=None, op_data=None, term_op=np.array([-1, -1, -1], np.int32), dst=plain) == 0 and plain[0] and plain[1]
        for h in list(out) + list(plain):
            assert L.aqc_mps_destroy(c_void_p(h)) == 0
        assert live_buffers() == live
    finally:
        _close(owned)
